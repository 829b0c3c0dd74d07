"""GPU: the GP operators no rollout test reaches, at the shapes where their kernels take another path.

POSTERIOR (`mcp_posterior_fwd` / `mcp_posterior_bwd`: `posterior_fwd_kernel<P>`, `gp_jac<2>`, `phase_k<P,false,2>`, `phase_j<P,false,2>`)
against the extended-precision truth of tests/gp_truth.py: degree 0 / 1 / 2 x forced P = 1 / 2 / 4 x the shapes of gp_truth.SHAPES (every
Npad edge, M mod P != 0, the 15 / 16 boundary of phase J, D = 1 and D = 32), a prior mean, and both branches of the automatic dispatch.
Every case goes through `ops.posterior` + backward (`gZ = g_mu Jmu + g_var Jvar`) and through `mcp_posterior_fwd_ex` directly (Jmu, Jvar,
the status word, what ran).  Bounds: the project's rel 1e-10 on mu / var, and r = |got - truth| / (2^-53 S) <= C per quantity.

  C = 16 x r_orc rounded up to a power of two; r_orc = the float64 CPU oracle's worst r over the same cases (tests/test_gp_truth_cpu.py):
      quantity   r_orc    C     kernels' worst r (one MI355X, all 86 cases x P; profiles/NOTES.md part I)
      mu         1.889    32    5.16   (N = 1, D = 1, degree 2)
      var        1.145    32    1.29   (N = 1, D = 1, degree 1)
      Jmu        1.899    32    5.99   (N = 1, D = 1, degree 2)
      Jvar       1.799    32    11.79  (N = 1, D = 1, degree 2)
      A G A      8.986    256   7.49   (N = 300)
  Against the project's own statement: mu rel 8.9e-14, var abs 1.1e-12 at worst (N = 300), bound 1e-10.  No forced P fell back, D = 32 included.
  gZ: fma(g_mu, Jmu, g_var Jvar) adds two roundings of its own terms to the Jacobians' errors: r <= max(C_Jmu, C_Jvar) + 2 with
  S = |g_mu| S_Jmu + |g_var| S_Jvar (bound 34; measured 4.42).

TRAINING EPOCH (`mcp_nll_epoch` through nll.BatchedFit, and the one-GP route `nll.nll_loss_and_grad`) against orc.marginal_nll + autograd
in float64 on the CPU, at the project's tolerances (tests/test_gpu_realsize_r5.py): loss rel 1e-9, gradient entries 1e-7 max(1, |g|max):
non-ARD, a trained prior mean, frozen parameters (NULL gradient pointers), sigma_n_num, y_scale, N at the tile edges of the epoch's
kernels and at both limits, D = 1 and D = 32, and G = MCP_MAX_GP GPs in one fit (each equal to the same GP fitted alone to 1e-9).
BatchedFit is eligible for every one of these cases.  Measured: loss rel <= 4.6e-14, gradient entries <= 4.0e-11 (N = 1152).

SMALL OPERATORS: `ops.sym_sandwich` against the truth A G A (r <= C, non-symmetric G), `ops.cov_build` / `ops.cov_diag` rectangular at
37 x 53, D = 1 / 32, degree 2 against the oracle at the per-op rel 1e-12.
"""
import contextlib
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

import gp_truth as gt
from oracle import mcpilco_oracle as orc

pytestmark = pytest.mark.gpu
quiet = lambda: contextlib.redirect_stdout(io.StringIO())
Tt = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
QUANT = ("mu", "var", "Jmu", "Jvar")


# ----------------------------------------------------------------------------------------------------------------------------------
# posterior
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _packed(case):
    from gpu_helpers import G
    from mc_pilco_amd import ops

    op = gt.posterior_case(*case)
    sp = ops.KernelSpec(op["ls"], op["lam"], 0.01, op["mean"], op["w1"], op["w20"], op["w21"])
    return ops.PackedGP(sp, G(op["X"]), G(op["alpha"]), G(op["Kinv"])), G(op["Z"])


def _fwd_ex(gp, Z):
    """mcp_posterior_fwd_ex as the library exports it: (mu, var, Jmu, Jvar, status word, particles per workgroup that ran)."""
    from mc_pilco_amd import hipabi as abi

    M, D = Z.shape
    mu, var = torch.empty(M, dtype=Z.dtype, device=Z.device), torch.empty(M, dtype=Z.dtype, device=Z.device)
    Jm, Jv = torch.empty(M, D, dtype=Z.dtype, device=Z.device), torch.empty(M, D, dtype=Z.dtype, device=Z.device)
    status = torch.zeros(1, dtype=torch.int32, device=Z.device)
    g = gp.to_c()
    abi.check(abi.lib().mcp_posterior_fwd_ex(C.byref(g), M, abi.ptr(Z), abi.ptr(mu), abi.ptr(var), abi.ptr(Jm), abi.ptr(Jv), abi.ptr(status),
                                             abi.stream(), C.byref(abi.DISPATCH)), "mcp_posterior_fwd_ex")
    return mu, var, Jm, Jv, int(status.item()), abi.lib().mcp_debug_last_particles_per_wg()


def _check_posterior(case, code, expect_ran):
    from gpu_helpers import G, forced_variant
    from mc_pilco_amd import hipabi as abi
    from mc_pilco_amd import ops

    N, D, M, deg, mean = case
    gp, Z = _packed(case)
    tr = gt.posterior_case_truth(case)
    be = gt.backend()
    rs = np.random.RandomState(M + 31 * code)
    g_mu = rs.uniform(0.5, 1.5, M) * rs.choice([-1.0, 1.0], M)
    g_var = rs.uniform(0.5, 1.5, M) * rs.choice([-1.0, 1.0], M)
    with forced_variant(code):
        mu, var, Jm, Jv, status, ran = _fwd_ex(gp, Z)
        Zg = Z.clone().requires_grad_(True)
        st2 = torch.zeros(1, dtype=torch.int32, device=Z.device)
        mu2, var2 = ops.posterior(gp, Zg, status=st2)
        ran2 = abi.lib().mcp_debug_last_particles_per_wg()
        torch.autograd.backward([mu2, var2], [G(g_mu).reshape(-1, 1), G(g_var)])
    # what ran: a forced P may give way to a smaller one only where its operands do not fit the LDS -- never at D <= 8
    assert ran == ran2 and ran in (1, 2, 4)
    if expect_ran is not None:
        assert ran == expect_ran, "P = %d ran, %d expected" % (ran, expect_ran)
    else:
        assert ran <= code
    assert status == 0 and int(st2.item()) == 0
    assert mu2.shape == (M, 1) and torch.equal(mu2.detach().reshape(-1), mu) and torch.equal(var2.detach(), var)
    got = dict(mu=mu, var=var, Jmu=Jm, Jvar=Jv)
    r = {q: gt.r_of(got[q], *tr[q]) for q in QUANT}
    t_gz = be.up(g_mu)[:, None] * tr["Jmu"][0] + be.up(g_var)[:, None] * tr["Jvar"][0]
    s_gz = abs(be.up(g_mu))[:, None] * tr["Jmu"][1] + abs(be.up(g_var))[:, None] * tr["Jvar"][1]
    r["gZ"] = gt.r_of(Zg.grad, t_gz, s_gz)
    t_mu, t_var = be.down(tr["mu"][0]), be.down(tr["var"][0])
    e_mu = float(np.abs(mu.cpu().numpy() - t_mu).max() / np.abs(t_mu).max())
    e_var = float(np.abs(var.cpu().numpy() - t_var).max())
    kzz = float(be.down(tr["kzz"][0]).max())  # (the `diag` of the parity tests' normalisation)
    print("POSTERIOR N=%d D=%d M=%d deg=%d mean=%g code=%d ran=%d : r mu %.2f var %.2f Jmu %.2f Jvar %.2f gZ %.2f | mu rel %.1e var abs %.1e"
          % (N, D, M, deg, mean, code, ran, r["mu"], r["var"], r["Jmu"], r["Jvar"], r["gZ"], e_mu, e_var))
    assert e_mu < 1e-10
    assert e_var < 1e-10 * max(1.0, kzz)
    for q in QUANT:
        assert r[q] <= gt.C[q], (q, r[q])
    assert r["gZ"] <= max(gt.C["Jmu"], gt.C["Jvar"]) + 2.0, r["gZ"]


@pytest.mark.parametrize("P", [1, 2, 4])
@pytest.mark.parametrize("case", gt.POSTERIOR_CASES + [gt.MEAN_CASE], ids=lambda c: "N%d-D%d-M%d-deg%d-m%g" % c)
def test_posterior_and_input_jacobians_against_the_truth(case, P):
    """Forced P: at D <= 8 the forced kernel must be the one that ran (each of P = 1, 2, 4 for every degree and shape); wider inputs may
    fall back to fewer particles per workgroup where the LDS does not hold the operands -- recorded in the printed line, never skipped."""
    _check_posterior(case, P, P if case[1] <= 8 else None)


@pytest.mark.parametrize("case,ran", list(zip(gt.AUTO_CASES, (2, 4))), ids=["M300", "M1030"])
def test_posterior_automatic_dispatch_branches(case, ran):
    """`pick_particles_per_wg`: 257..1024 test points run two per workgroup (every 400-particle swarm), more than 1024 four."""
    _check_posterior(case, 0, ran)


# ----------------------------------------------------------------------------------------------------------------------------------
# training epoch
# ----------------------------------------------------------------------------------------------------------------------------------
def _make_gp(D, deg, ls, pw, ard=True, **rbf_kw):
    from test_gpu_dropin import mpk_dict, rbf_dict
    from mc_pilco_amd.gpr_lib.GP_prior import GP_prior as GP
    from mc_pilco_amd.gpr_lib.GP_prior import Sparse_GP, Stationary_GP

    rbf = dict(rbf_dict(D, ls if ard else np.asarray(ls)[:1], 0.1), flg_train_lambda=True, lambda_init=np.array([1.3]))
    rbf.update(rbf_kw)
    with quiet():
        if deg == 0:
            return Stationary_GP.RBF(**rbf)
        return GP.Sum_Independent_GP(Stationary_GP.RBF(**rbf), Sparse_GP.get_Volterra_MPK_GP(**mpk_dict(D, deg, pw)))


def _oracle_nll(X, Y, D, ls, pw, ard=True, mean=0.0, sigma_n_num=0.0, sigma_n=0.1):
    """(loss, {short parameter name: gradient}, [gradients of the polynomial parameters]) of orc.marginal_nll + autograd."""
    from helpers import hyper

    h = hyper(ls, sigma_n, 1.3, pw)
    ls_leaf = h.log_ls
    if not ard:  # one shared lengthscale: the gradient lands on the scalar
        ls_leaf = torch.log(Tt([np.asarray(ls)[0]]))
        ls_leaf.requires_grad_(True)
        h.log_ls = ls_leaf.expand(D)
    h.mean = Tt([mean])
    h.sigma_n_num = float(sigma_n_num)
    prm = [h.log_sigma_n, ls_leaf, h.log_lambda, h.mean] + list(h.poly_log_par or [])
    for q in prm:
        q.requires_grad_(True)
    loss = orc.marginal_nll(h, Tt(X), Tt(Y))
    loss.backward()
    want = {"sigma_n_log": h.log_sigma_n.grad, "log_lengthscales_par": ls_leaf.grad, "log_lambda_par": h.log_lambda.grad, "mean_par": h.mean.grad}
    return float(loss.detach()), {k: v.numpy().reshape(-1) for k, v in want.items()}, [q.grad.numpy().reshape(-1) for q in (h.poly_log_par or [])]


def _routes(gps, X, Ys, y_scales):
    """Per GP: ((loss, grads) of nll_loss_and_grad on Y * y_scale, (loss, grads) of ONE BatchedFit over all of them, lr = 0)."""
    from test_gpu_dropin import T
    from mc_pilco_amd import nll

    Xd = T(X)
    one = []
    for gp, Y, s in zip(gps, Ys, y_scales):
        loss = float(nll.nll_loss_and_grad(gp, Xd, T(Y * s)))
        nll.check_status(gp)
        one.append((loss, {n: p.grad.detach().cpu().numpy().reshape(-1).copy() for n, p in gp.named_parameters() if p.grad is not None}))
        for p in gp.parameters():
            p.grad = None
    fit = nll.BatchedFit(gps, Xd, [T(Y) for Y in Ys], list(y_scales), [torch.optim.Adam(gp.parameters(), lr=0.0) for gp in gps], 1, 10 ** 9)
    assert fit.eligible, "the batched epoch must cover this case"
    with quiet():
        fit.run()
    bat = [(float(fit.loss[i]), {n: p.grad.detach().cpu().numpy().reshape(-1).copy() for n, p in gp.named_parameters() if p.grad is not None})
           for i, gp in enumerate(gps)]
    return list(zip(one, bat))


def _against_oracle(tag, routes, oracle, expect):
    """The project's tolerances: loss rel 1e-9, every gradient entry 1e-7 max(1, |g|max).  ``expect``: the short names that must have been
    compared (so that a gradient that silently went missing fails)."""
    oloss, want, wpoly = oracle
    for which, (loss, grads) in zip(("nll_loss_and_grad", "mcp_nll_epoch"), routes):
        e_loss = abs(loss - oloss) / abs(oloss)
        seen, npoly, worst = set(), 0, 0.0
        for n, g in grads.items():
            short = n.split(".")[-1]
            if short == "Sigma_pos_par":
                ref = wpoly[npoly]
                npoly += 1
            else:
                ref = want[short]
            err = float(np.abs(g - ref).max()) / max(1.0, float(np.abs(ref).max()))
            worst = max(worst, err)
            assert g.shape == ref.shape and err < 1e-7, (tag, which, n, err)
            seen.add(short)
        print("NLL %s %s: loss rel %.2e, worst gradient error %.2e, checked %s" % (tag, which, e_loss, worst, sorted(seen)))
        assert e_loss < 1e-9, (tag, which, e_loss)
        assert seen == set(expect) and npoly == len(wpoly), (tag, which, seen)


BASE = ("sigma_n_log", "log_lengthscales_par", "log_lambda_par")


def _one_case(tag, N, D, deg, ard=True, y_scale=1.0, mean=0.0, sigma_n_num=0.0, expect=BASE, **rbf_kw):
    X, Y, ls = gt.nll_data(N, D)
    pw = gt.nll_poly_weights(D, deg)
    if sigma_n_num:
        rbf_kw["sigma_n_num"] = sigma_n_num
    gp = _make_gp(D, deg, ls, pw, ard=ard, **rbf_kw)
    if y_scale == 1.0:
        from test_gpu_dropin import T
        from test_gpu_realsize_r5 import _run_both_routes

        routes = _run_both_routes(gp, T(X), T(Y))
    else:
        routes = _routes([gp], X, [Y], [y_scale])[0]
    oracle = _oracle_nll(X, Y * y_scale, D, ls, pw, ard=ard, mean=mean, sigma_n_num=sigma_n_num)
    _against_oracle(tag, routes, oracle, tuple(expect) + (("Sigma_pos_par",) if deg else ()))
    return gp, routes


@pytest.mark.parametrize("deg", [0, 2])
def test_training_epoch_with_one_shared_lengthscale(deg):
    """(a) ard == 0: `exp(-log_ls[0])` for every dimension in nll_prep_kernel, the sum over D in nll_finish_kernel."""
    gp, _ = _one_case("non-ARD deg %d" % deg, 129, 6, deg, ard=False)
    rbf = gp if deg == 0 else gp.gp_list[0]
    assert rbf.log_lengthscales_par.numel() == 1 and not rbf.flg_ARD


def test_training_epoch_with_a_trained_prior_mean():
    """(b) g_mean = -sum(alpha) with a non-zero mean."""
    _one_case("mean 0.4", 129, 6, 0, mean=0.4, expect=BASE + ("mean_par",), mean_init=np.array([0.4]), flg_train_mean=True)


def test_training_epoch_with_frozen_parameters():
    """(c) NULL gradient pointers: frozen lengthscales and frozen sigma_n keep .grad None, the other gradients are those of the
    all-trainable run (bit for bit: the same kernels on the same numbers)."""
    _, full = _one_case("all trainable", 129, 6, 2)
    gp, part = _one_case("frozen ls, sigma_n", 129, 6, 2, expect=("log_lambda_par",), flg_train_lengthscales=False, flg_train_sigma_n=False)
    rbf = gp.gp_list[0]
    assert rbf.log_lengthscales_par.grad is None and rbf.sigma_n_log.grad is None
    for (l0, g0), (l1, g1) in zip(full, part):
        assert l0 == l1
        assert set(g1) < set(g0)
        for n in g1:
            assert np.array_equal(g0[n], g1[n]), n


def test_training_epoch_with_a_numerical_noise_floor():
    """(d) sigma_n_num2 != 0: the noise is exp(sigma_n_log)^2 + sigma_n_num^2, d/d sigma_n_log sees the first term only."""
    _one_case("sigma_n_num 0.05", 129, 6, 0, sigma_n_num=0.05)


def test_training_epoch_with_scaled_targets():
    """(e) y_scale = 2.5 through BatchedFit's y_scales (what flg_norm / norm_list feed): the epoch of Y with the scale is the one-GP route
    and the oracle on 2.5 Y."""
    _one_case("y_scale 2.5", 129, 6, 0, y_scale=2.5)


@pytest.mark.parametrize("N", [17, 31, 33, 128, 129, 256, 257, 1152])
def test_training_epoch_at_the_tile_edges(N):
    """(f) N = 17 (just above the lower limit), 31 / 33, 128 / 129 (nll_grad_rows_per_wg = ceil(N / 128)), 256 / 257 (the 256-column Gram tile of
    cov_build_batch_kernel), 1152 (the upper limit)."""
    _one_case("N %d" % N, N, 6, 0)


@pytest.mark.parametrize("D,deg", [(1, 0), (32, 1)])
def test_training_epoch_at_the_dimension_limits(D, deg):
    """(g) D = 1 (one lengthscale: the reference's flg_ARD is False there) and D = MCP_MAX_GPDIM with the linear term."""
    _one_case("D %d deg %d" % (D, deg), 129, D, deg, ard=D > 1)


def test_training_epoch_with_eight_gps_in_one_fit():
    """(h) G = MCP_MAX_GP: eight GPs with their own hyper-parameters and targets in one BatchedFit; each equals the same GP fitted alone to 1e-9
    (the bound of test_training_epoch_kernels_match_the_single_gp_path_at_large_n) and the oracle at the project's tolerances."""
    from helpers import hyper
    from mc_pilco_amd import hipabi

    Gn, N, D = hipabi.MAX_GP, 129, 6
    X = gt.nll_data(N, D)[0]
    Ys, lss = [], []
    for g in range(Gn):
        rs = np.random.RandomState(900 + g)
        Ys.append((np.sin((1.0 + 0.2 * g) * X[:, 0] + X[:, 1 + g % 5]) + 0.1 * rs.randn(N)).reshape(-1, 1))
        lss.append(np.sqrt(D) * rs.uniform(0.8, 1.6, D))
    make = lambda: [_make_gp(D, 0, lss[g], None, sigma_n_init=(0.05 + 0.02 * g) * np.ones(1), lambda_init=np.array([0.8 + 0.1 * g])) for g in range(Gn)]
    together = _routes(make(), X, Ys, [1.0] * Gn)
    alone = [_routes([gp], X, [Ys[g]], [1.0])[0] for g, gp in enumerate(make())]
    for g in range(Gn):
        (lt, gt_), (la, ga) = together[g][1], alone[g][1]
        assert abs(lt - la) < 1e-9 * abs(la), g
        assert set(gt_) == set(ga) and len(ga) == 3
        for n in ga:
            assert float(np.abs(gt_[n] - ga[n]).max()) < 1e-9 * max(1.0, float(np.abs(ga[n]).max())), (g, n)
        h = hyper(lss[g], 0.05 + 0.02 * g, 0.8 + 0.1 * g)
        prm = [h.log_sigma_n, h.log_ls, h.log_lambda]
        for q in prm:
            q.requires_grad_(True)
        ol = orc.marginal_nll(h, Tt(X), Tt(Ys[g]))
        ol.backward()
        want = {"sigma_n_log": h.log_sigma_n.grad, "log_lengthscales_par": h.log_ls.grad, "log_lambda_par": h.log_lambda.grad}
        _against_oracle("G=8 gp %d" % g, together[g], (float(ol.detach()), {k: v.numpy().reshape(-1) for k, v in want.items()}, []), BASE)


# ----------------------------------------------------------------------------------------------------------------------------------
# small operators
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", gt.SANDWICH_SIZES)
def test_sym_sandwich_against_the_truth(N):
    """`mcp_sym_sandwich` (MFMA GEMM) at one row, around the 16- and 64-wide tiles, 129 and 300, with a G that is NOT symmetric (A G A != A G^T A)."""
    from gpu_helpers import G
    from mc_pilco_amd import ops

    A, Gm = gt.sandwich_case(N)
    tr, S = gt.sandwich_case_truth(N)
    out = ops.sym_sandwich(G(A), G(Gm))
    r = gt.r_of(out, tr, S)
    if N in (17, 65):
        r_t = gt.r_of(out, *gt.sandwich_truth(A, Gm.t().contiguous()))
        assert r_t > 100.0 * gt.C["sandwich"]  # (the cases would tell a transposed G apart)
    print("SANDWICH N=%d: r %.2f (C %g)" % (N, r, gt.C["sandwich"]))
    assert r <= gt.C["sandwich"]


@pytest.mark.parametrize("D", [1, 32])
def test_rectangular_gram_and_diagonal_at_the_dimension_limits(D):
    """`mcp_cov_build` with N1 != N2, neither a multiple of 16 (37 x 53), and `mcp_cov_diag` on the same inputs, degree 2, D = 1 and
    D = MCP_MAX_GPDIM, with and without the noise flag, against the oracle at the per-op rel 1e-12."""
    from gpu_helpers import G, spec_from
    from helpers import hyper
    from test_gpu_parity import relerr
    from mc_pilco_amd import ops

    rs = np.random.RandomState(40 + D)
    X1, X2 = rs.uniform(-1.0, 1.0, (37, D)), rs.uniform(-1.0, 1.0, (53, D))
    ls = np.sqrt(D) * rs.uniform(0.8, 1.6, D)
    pw = gt.nll_poly_weights(D, 2)
    sp, h = spec_from(ls, 0.1, 1.3, pw), hyper(ls, 0.1, 1.3, pw)
    assert relerr(ops.cov_build(sp, G(X1), G(X2)), orc.gp_cov(h, Tt(X1), Tt(X2))) < 1e-12
    assert relerr(ops.cov_build(sp, G(X2), G(X1)), orc.gp_cov(h, Tt(X2), Tt(X1))) < 1e-12
    assert relerr(ops.cov_build(sp, G(X1), None, noise=True), orc.gp_cov(h, Tt(X1), None, noise=True)) < 1e-12
    for X in (X1, X2):
        assert relerr(ops.cov_diag(sp, G(X)), orc.gp_diag(h, Tt(X))) < 1e-12
        assert relerr(ops.cov_diag(sp, G(X), noise=True), orc.gp_diag(h, Tt(X)) + 0.1 ** 2) < 1e-12
