"""GPU: the marginal-likelihood gradient operator  g_p = 1/2 sum_ij (Kinv_ij - alpha_i alpha_j) dK_ij/dtheta_p  (csrc/gp_nll.hip) at operand
level: each of its three kernel forms against the extended-precision truth of tests/gp_truth.py (`nll_grad_truth`) on the float64 operands
the kernel itself received, entry by entry:  r = |got - truth| / (2^-53 S) <= C,  S = 1/2 sum_ij (|Kinv_ij| + |alpha_i alpha_j|) |dK_ij/dtheta_p|.
The project's bound on the whole chain, 1e-7 max(1, |g|max) per tensor, is relative to the largest entry; this one holds every entry to
its own term sum.  Entries without a non-zero term (the slots of an absent degree; the lengthscale entry at N = 1) must be exactly 0.0.

  C = 16 x r_orc rounded up to a power of two = 64; r_orc = 2.445: a float64 torch evaluation of the same formula on the same operands,
  worst over every case here (tests/test_gp_truth_cpu.py; at (N, D, degree) = (7, 7, 2), below 0.35 from N = 65 on).

`mcp_nll_grad` (nll_grad_row in nll_grad_kernel + nll_colsum_kernel) directly: N below the segment count of stage 2, every NPpad boundary
(D = 7 | 8, 15 | 16, 31 | 32) at N = 257, the 256-stride of stage 1 and the tails of the column sum's four-way unroll at D = 6, the limit
N = 4096; at (65, 8, 2) a row pitch ldk = N + 3 with NaN in the padding, `kern->scal` with the by-value lambda, noise and mean poisoned, and
a non-symmetric W with alpha = 0 through nll.cov_weighted_grad.

`mcp_nll_epoch` through nll.BatchedFit (one epoch, lr = 0), both gradient forms, the form asserted from `mcp_nll_epoch_plan`: the truth is
formed from what the epoch itself left in its workspace at the plan's offsets (Kinv, alpha, 1 / l, lambda, the polynomial weights), and holds
g_log_ls, g_log_lambda, g_mpk1, g_mpk2 to r <= C; a shared lengthscale to C + D (D - 1 more additions of the D entries, each within its own
S); g_sigma_n_log to C + 4 (the exp and two products on top of 1/2 tr Wm); g_mean to C against -sum(alpha), S = sum |alpha|.  At the shapes
of the row-per-workgroup form (`nll_grad_batch_kernel`, which no other test launches) the whole chain is also held to the project's
tolerances against orc.marginal_nll + autograd, and three GPs in one fit to the same GPs fitted alone (1e-9).

Kernels' worst r (one MI355X; profiles/NOTES.md part S).  No kernel needed a change; with many terms every form sits at r < 1/2, as the
float64 floor does -- the sums cancel to 1e-9 .. 1e-2 of S, so these are entries the per-tensor bound could not see:
      form / shape class                                            worst r
      mcp_nll_grad   N < segments (1, 3, 7)                         1.02  (7, 7, 2)
      mcp_nll_grad   NPpad boundaries, N = 257                      0.26  (D = 31)
      mcp_nll_grad   D = 6, N = 255 .. 1153                         0.25  (N = 255, degree 0)
      mcp_nll_grad   N = 4096                                       0.06
      mcp_nll_grad   (65, 8, 2): ldk, scal, non-symmetric W         0.19
      mcp_nll_epoch  LDS rows (nll_grad_rows_kernel)                0.16  (g_mean, (129, 6, 2)); g_sigma_n_log 0.47
      mcp_nll_epoch  row per workgroup (nll_grad_batch_kernel)      0.14  (g_mean, (530, 32, 2)); g_sigma_n_log 0.51
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gp_truth as gt

pytestmark = pytest.mark.gpu
CB = gt.C["nll_grad"]
ID3 = lambda c: "N%d-D%d-deg%d" % tuple(c[:3])


# ----------------------------------------------------------------------------------------------------------------------------------
# mcp_nll_grad directly
# ----------------------------------------------------------------------------------------------------------------------------------
def _nll_grad(op, W, alpha, ldk=None, scal=False):
    """mcp_nll_grad on the float64 operands of ``op`` with the matrix W [N, N] and alpha [N]: the gradient vector [4D + 3] (numpy)."""
    from gpu_helpers import G
    from mc_pilco_amd import hipabi as abi

    N, D, deg = op["X"].shape[0], op["D"], op["deg"]
    ldk = N if ldk is None else ldk
    Wp = np.full((N, ldk), np.nan)
    Wp[:, :N] = W
    keep = dict(X=G(op["X"]), W=G(Wp), alpha=G(alpha), inv_ls=G(op["inv_ls"]))
    k = abi.Kernel()
    k.D, k.poly_deg = D, deg
    k.lam, k.sigma_n2, k.mean = op["lam"], 0.01, 0.0
    k.inv_ls = keep["inv_ls"].data_ptr()
    for name in ("w1", "w20", "w21"):
        if op[name] is not None:
            keep[name] = G(op[name])
            setattr(k, name, keep[name].data_ptr())
    if scal:  # the device triple overrides the by-value fields: poison those
        keep["scal"] = G([op["lam"], 0.01, 0.0])
        k.scal = keep["scal"].data_ptr()
        k.lam = k.sigma_n2 = k.mean = float("nan")
    nbytes = abi.lib().mcp_nll_workspace_bytes(N, D)
    assert nbytes == 8 * N * (4 * D + 3)
    ws = torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device=keep["X"].device)
    g = torch.full((4 * D + 3,), float("nan"), dtype=torch.float64, device=keep["X"].device)
    abi.check(abi.lib().mcp_nll_grad(C.byref(k), N, abi.ptr(keep["X"]), abi.ptr(keep["W"]), ldk, abi.ptr(keep["alpha"]), abi.ptr(g), abi.ptr(ws), nbytes,
                                     abi.stream()), "mcp_nll_grad")
    return g.cpu().numpy()


def _hold(tag, got, truth, S, live, bound=CB):
    """Every live entry within ``bound``, every other entry exactly 0.0."""
    assert got.shape == live.shape and np.all(np.isfinite(got)), tag
    r = gt.r_entries(got, truth, S, live)
    print("NLLGRAD %s: worst r %.2f at live entry %d of %d (bound %g)" % (tag, r.max(), int(r.argmax()), r.size, bound))
    assert np.all(got[~live] == 0.0), (tag, got[~live])
    assert np.all(r <= bound), (tag, np.flatnonzero(r > bound), r.max())
    return float(r.max())


@pytest.mark.parametrize("case", gt.GRAD_SMALL_CASES + gt.GRAD_NPPAD_CASES + gt.GRAD_STRIDE_CASES + [gt.GRAD_LIMIT_CASE], ids=ID3)
def test_nll_grad_against_the_truth(case):
    op = gt.nll_grad_case(*case)
    got = _nll_grad(op, op["W"], op["alpha"])
    _hold("mcp_nll_grad N=%d D=%d deg=%d" % case, got, *gt.nll_grad_case_truth(case), gt.nll_grad_live(*case))


@pytest.mark.parametrize("variant", ["ldk", "scal"])
def test_nll_grad_with_a_row_pitch_and_with_device_scalars(variant):
    """ldk = N + 3 with NaN in the padding (a read past column N poisons the sums); kern->scal set, the by-value lambda, noise and mean NaN."""
    case = gt.GRAD_VARIANT_CASE
    op = gt.nll_grad_case(*case)
    got = _nll_grad(op, op["W"], op["alpha"], ldk=case[0] + 3 if variant == "ldk" else None, scal=variant == "scal")
    _hold("mcp_nll_grad (65, 8, 2) %s" % variant, got, *gt.nll_grad_case_truth(case), gt.nll_grad_live(*case))


def test_cov_weighted_grad_with_a_matrix_that_is_not_symmetric():
    """nll.cov_weighted_grad: sum_ij Wm_ij dK_ij/dtheta through mcp_nll_grad with 2 Wm for Kinv and alpha = 0.  Wm is any matrix: a kernel
    that read W_ji for W_ij, or only one triangle, gives the truth of another matrix (asserted to lie far outside the bound)."""
    import types

    from gpu_helpers import G, dev
    from mc_pilco_amd import nll, ops

    N, D, deg = case = gt.GRAD_VARIANT_CASE
    op = gt.nll_grad_case(*case)
    rs = np.random.RandomState(77)
    Wm = rs.randn(N, N)
    sp = ops.KernelSpec(torch.as_tensor(op["ls"]), op["lam"], 0.01, 0.0, *[torch.as_tensor(op[k]) for k in ("w1", "w20", "w21")])
    got = nll.cov_weighted_grad(types.SimpleNamespace(device=dev()), G(op["X"]), G(Wm), spec=sp).cpu().numpy()
    inv_ls = sp._device_operands(dev())["inv_ls"].cpu().numpy()  # (the operand the kernel read: 1 / l formed by the host layer)
    args = lambda W: (op["X"], 2.0 * W, np.zeros(N), inv_ls, op["lam"], op["w1"], op["w20"], op["w21"], deg)
    truth, S = gt.nll_grad_truth(*args(Wm))
    live = gt.nll_grad_live(*case)
    _hold("cov_weighted_grad (65, 8, 2) non-symmetric W", got, truth, S, live)
    # dK is symmetric, so W and W^T give the same sums: the matrix that tells a triangle-only kernel apart is the lower triangle doubled
    tri = np.tril(Wm, -1) * 2.0 + np.diag(np.diag(Wm))
    off = np.ones(4 * D + 3, dtype=bool)
    off[D + 1] = False  # (the trace sees the diagonal only)
    assert gt.r_entries(gt.backend().down(gt.nll_grad_truth(*args(tri))[0]), truth, S, off).min() > 100.0 * CB


# ----------------------------------------------------------------------------------------------------------------------------------
# mcp_nll_epoch: both gradient forms, the truth formed from the epoch's own operands
# ----------------------------------------------------------------------------------------------------------------------------------
MEAN = 0.1


def _plan(G, N, D):
    from mc_pilco_amd import hipabi as abi

    p = abi.NllPlan()
    assert abi.lib().mcp_nll_epoch_plan(G, N, D, C.byref(p)) == 0
    return p


def _gp(D, deg, ls, pw, ard=True, **kw):
    from test_gpu_gp_operators import _make_gp

    return _make_gp(D, deg, ls, pw, ard=ard, mean_init=np.array([MEAN]), flg_train_mean=True, **kw)


def _epoch(gps, X, Ys):
    """One BatchedFit epoch at lr = 0 over ``gps``: (the fit, per GP (loss, {parameter name: gradient}))."""
    from test_gpu_dropin import T
    from test_gpu_gp_operators import quiet
    from mc_pilco_amd import nll

    fit = nll.BatchedFit(gps, T(X), [T(Y) for Y in Ys], [1.0] * len(gps), [torch.optim.Adam(gp.parameters(), lr=0.0) for gp in gps], 1, 10 ** 9)
    assert fit.eligible, "the batched epoch must cover this case"
    with quiet():
        fit.run()
    assert int(fit.status.item()) == 0
    return fit, [(float(fit.loss[i]), {n: p.grad.detach().cpu().numpy().reshape(-1).copy() for n, p in gp.named_parameters() if p.grad is not None})
                 for i, gp in enumerate(gps)]


def _one_gp_route(gp, X, Y):
    from test_gpu_dropin import T
    from mc_pilco_amd import nll

    loss = float(nll.nll_loss_and_grad(gp, T(X), T(Y)))
    nll.check_status(gp)
    out = (loss, {n: p.grad.detach().cpu().numpy().reshape(-1).copy() for n, p in gp.named_parameters() if p.grad is not None})
    for p in gp.parameters():
        p.grad = None
    return out


def _epoch_operands(fit, plan, g, X, deg):
    """What epoch ``fit`` made for GP g, read from its workspace at the plan's offsets: the operands of the gradient stage."""
    N, D = X.shape
    ws = fit.ws.cpu().numpy()
    assert ws.size * 8 >= plan.total * 8 == fit.nbytes
    base = ws[plan.first_gp + g * plan.per_gp:plan.first_gp + (g + 1) * plan.per_gp]
    take = lambda off, n: base[off:off + n].copy()
    scal = take(plan.scal, 3)
    return dict(X=X, W=take(plan.Kinv, N * N).reshape(N, N), alpha=take(plan.alpha, N), inv_ls=take(plan.inv_ls, D), lam=float(scal[0]),
                w1=take(plan.w1, D + 1) if deg >= 1 else None, w20=take(plan.w20, D) if deg >= 2 else None,
                w21=take(plan.w21, D) if deg >= 2 else None, deg=deg)


def _hold_epoch(tag, gp, grads, op, ard):
    """The epoch's gradients of one GP against the truth on its own operands ``op``."""
    be = gt.backend()
    N, D = op["X"].shape
    deg = op["deg"]
    truth, S = gt.nll_grad_truth(*gt.nll_grad_args(op))
    rbf = gp if deg == 0 else gp.gp_list[0]
    by = {n.split(".")[-1]: [] for n in grads}
    for n, v in grads.items():
        by[n.split(".")[-1]].append(v)
    assert set(by) == {"log_lengthscales_par", "log_lambda_par", "sigma_n_log", "mean_par"} | ({"Sigma_pos_par"} if deg else set())
    one = np.ones(1, dtype=bool)
    worst = 0.0
    if ard:
        worst = max(worst, _hold(tag + " g_log_ls", by["log_lengthscales_par"][0], truth[:D], S[:D], np.ones(D, dtype=bool)))
    else:  # the D entries added up by one thread in order: D - 1 more roundings, each of a partial sum within the sum of the S
        assert rbf.log_lengthscales_par.numel() == 1
        worst = max(worst, _hold(tag + " g_log_ls (shared)", by["log_lengthscales_par"][0], truth[:D].sum(keepdims=True), S[:D].sum(keepdims=True), one,
                                 CB + D))
    worst = max(worst, _hold(tag + " g_log_lambda", by["log_lambda_par"][0], truth[D:D + 1], S[D:D + 1], one))
    # g_sigma_n_log = (1/2 tr Wm) * 2 * exp(2 sigma_n_log): truth and S scaled in the back end, sigma_n_log taken exactly
    fac = 2 * be.exp(2 * be.up(rbf.sigma_n_log.detach().cpu().numpy().astype(np.float64).reshape(-1)))
    worst = max(worst, _hold(tag + " g_sigma_n_log", by["sigma_n_log"][0], truth[D + 1:D + 2] * fac, S[D + 1:D + 2] * fac, one, CB + 4))
    a = be.up(op["alpha"])
    worst = max(worst, _hold(tag + " g_mean", by["mean_par"][0], -a.sum(keepdims=True), abs(a).sum(keepdims=True), one))
    if deg >= 1:
        worst = max(worst, _hold(tag + " g_mpk1", by["Sigma_pos_par"][0], truth[D + 2:2 * D + 3], S[D + 2:2 * D + 3], np.ones(D + 1, dtype=bool)))
    if deg >= 2:
        worst = max(worst, _hold(tag + " g_mpk2", by["Sigma_pos_par"][1], truth[2 * D + 3:], S[2 * D + 3:], np.ones(2 * D, dtype=bool)))
    print("NLLGRAD %s: worst r of the epoch's gradients %.2f" % (tag, worst))


def _oracle(X, Y, D, ls, pw, ard=True, sigma_n=0.1, lam=1.3):
    from test_gpu_gp_operators import Tt, _oracle_nll
    from helpers import hyper

    if lam == 1.3:
        return _oracle_nll(X, Y, D, ls, pw, ard=ard, mean=MEAN, sigma_n=sigma_n)
    h = hyper(ls, sigma_n, lam, pw)  # (_oracle_nll fixes lambda = 1.3: the GPs of the batch have their own)
    h.mean = Tt([MEAN])
    prm = [h.log_sigma_n, h.log_ls, h.log_lambda, h.mean] + list(h.poly_log_par or [])
    for q in prm:
        q.requires_grad_(True)
    from oracle import mcpilco_oracle as orc

    loss = orc.marginal_nll(h, Tt(X), Tt(Y))
    loss.backward()
    want = {"sigma_n_log": h.log_sigma_n.grad, "log_lengthscales_par": h.log_ls.grad, "log_lambda_par": h.log_lambda.grad, "mean_par": h.mean.grad}
    return float(loss.detach()), {k: v.numpy().reshape(-1) for k, v in want.items()}, [q.grad.numpy().reshape(-1) for q in (h.poly_log_par or [])]


EXPECT = ("sigma_n_log", "log_lengthscales_par", "log_lambda_par", "mean_par")


@pytest.mark.parametrize("case", gt.EPOCH_ROWS_CASES, ids=ID3)
def test_epoch_gradient_in_its_lds_rows_form_against_the_truth(case):
    from mc_pilco_amd import hipabi as abi

    N, D, deg = case
    X, Y, ls = gt.nll_data(N, D)
    gp = _gp(D, deg, ls, gt.nll_poly_weights(D, deg))
    plan = _plan(1, N, D)
    assert plan.grad_form == abi.NLL_GRAD_ROWS and plan.rows_per_wg == (N + 127) // 128
    fit, res = _epoch([gp], X, [Y])
    _hold_epoch("rows N=%d D=%d deg=%d" % case, gp, res[0][1], _epoch_operands(fit, plan, 0, X, deg), True)


@pytest.mark.parametrize("case", gt.EPOCH_FALLBACK_CASES, ids=lambda c: ID3(c) + ("" if c[3] else "-shared"))
def test_epoch_gradient_in_its_row_per_workgroup_form_against_the_truth(case):
    """nll_grad_batch_kernel: the operand-level truth, and the whole chain (both routes) against orc.marginal_nll + autograd at the
    project's tolerances -- loss rel 1e-9, gradient entries 1e-7 max(1, |g|max)."""
    from test_gpu_gp_operators import _against_oracle
    from mc_pilco_amd import hipabi as abi

    N, D, deg, ard = case
    X, Y, ls = gt.nll_data(N, D)
    pw = gt.nll_poly_weights(D, deg)
    gp = _gp(D, deg, ls, pw, ard=ard)
    plan = _plan(1, N, D)
    assert plan.grad_form == abi.NLL_GRAD_ROW_PER_WG and plan.slab_rows == N
    one = _one_gp_route(gp, X, Y)
    fit, res = _epoch([gp], X, [Y])
    tag = "fallback N=%d D=%d deg=%d%s" % (N, D, deg, "" if ard else " shared")
    _hold_epoch(tag, gp, res[0][1], _epoch_operands(fit, plan, 0, X, deg), ard)
    _against_oracle(tag, (one, res[0]), _oracle(X, Y, D, ls, pw, ard=ard), EXPECT + (("Sigma_pos_par",) if deg else ()))


BATCH_G = 3


def _batch_hyper(g):
    N, D, deg = gt.EPOCH_BATCH_CASE
    X = gt.nll_data(N, D)[0]
    rs = np.random.RandomState(1900 + g)
    Y = (np.sin((1.0 + 0.2 * g) * X[:, 0] + X[:, 1 + g]) + 0.1 * rs.randn(N)).reshape(-1, 1)
    return X, Y, np.sqrt(D) * rs.uniform(0.8, 1.6, D), gt.nll_poly_weights(D, deg, seed=g), 0.05 + 0.02 * g, 0.8 + 0.1 * g


def _batch_gp(g):
    N, D, deg = gt.EPOCH_BATCH_CASE
    _, _, ls, pw, sn, lam = _batch_hyper(g)
    return _gp(D, deg, ls, pw, sigma_n_init=sn * np.ones(1), lambda_init=np.array([lam]))


@functools.lru_cache(maxsize=None)
def _batch_together():
    """The three GPs in ONE fit: (per GP: the GP object, (loss, gradients), the operands the epoch made for it)."""
    from mc_pilco_amd import hipabi as abi

    N, D, deg = gt.EPOCH_BATCH_CASE
    gps = [_batch_gp(g) for g in range(BATCH_G)]
    plan = _plan(BATCH_G, N, D)
    assert plan.grad_form == abi.NLL_GRAD_ROW_PER_WG
    fit, res = _epoch(gps, _batch_hyper(0)[0], [_batch_hyper(g)[1] for g in range(BATCH_G)])
    return [(gps[g], res[g], _epoch_operands(fit, plan, g, _batch_hyper(0)[0], deg)) for g in range(BATCH_G)]


@pytest.mark.parametrize("g", range(BATCH_G))
def test_epoch_row_per_workgroup_form_with_three_gps_in_one_fit(g):
    """blockIdx.y = the GP: each GP of the batch against the truth on its own operands, against the same GP fitted alone (1e-9) and
    against the oracle at the project's tolerances."""
    from test_gpu_gp_operators import _against_oracle

    N, D, deg = gt.EPOCH_BATCH_CASE
    gp, (lt, gt_), op = _batch_together()[g]
    X, Y, ls, pw, sn, lam = _batch_hyper(g)
    tag = "fallback G=3 gp %d N=%d D=%d deg=%d" % (g, N, D, deg)
    assert abs(op["lam"] - lam) < 1e-14 * lam  # (block g holds GP g's hyper-parameters)
    _hold_epoch(tag, gp, gt_, op, True)
    solo = _batch_gp(g)
    one = _one_gp_route(solo, X, Y)
    _, alone = _epoch([solo], X, [Y])
    la, ga = alone[0]
    assert abs(lt - la) < 1e-9 * abs(la)
    assert set(gt_) == set(ga) and len(ga) == 5
    for n in ga:
        assert float(np.abs(gt_[n] - ga[n]).max()) < 1e-9 * max(1.0, float(np.abs(ga[n]).max())), n
    _against_oracle(tag, (one, (lt, gt_)), _oracle(X, Y, D, ls, pw, sigma_n=sn, lam=lam), EXPECT + ("Sigma_pos_par",))
