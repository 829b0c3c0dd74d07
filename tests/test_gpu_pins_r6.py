"""Round 6: three parity pins at exactly the launches the measured lines run (VERDICT r5 "next round" item 3).

  (a) ONE policy-gradient step at the headline launch -- c1: N = 300, M = 400, T = 150, recorded process noise and dropout masks -- on the
      automatic dispatch (`rollout_fwd_lat_kernel<4, 3, 0, false>` + `rollout_bwd_lat_kernel<2, false>`) against orc.policy_grad_step
      (MC_PILCO.py:615-674 + :522);
  (b) `sod_select_multi_kernel` on the UR5 pretrain shape (N = 600, D = 24, SE + polynomial(1), a threshold that rejects a quarter of the
      rows) against the REFERENCE's get_SOD index list (GP_prior.py:232-257; tests/golden/make_golden_r6.py);
  (c) `GP_prior.forward` as an autograd graph (`_ForwardFunction`, GP_prior.py:91-115) at N = 300 against the reference's own autograd
      under a criterion that touches all four outputs.

Tolerances (fp64) are written at each assertion.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
quiet = lambda: contextlib.redirect_stdout(io.StringIO())


# ----------------------------------------------------------------------------------------------------------------------------------
# (a) the headline launch
# ----------------------------------------------------------------------------------------------------------------------------------
def _oracle_on_reordered_training_set(o, key):
    """The SAME model with its training points in another order (X, alpha, rows / columns of Kinv permuted: an identical posterior whose
    N-long sums run in another order), the same x0 / eps / masks: how far the reference's own arithmetic is from itself over this horizon --
    the yardstick for a comparison of two implementations on a rollout that amplifies rounding differences."""
    import test_gpu_realsize as rs
    from oracle import mcpilco_oracle as orc

    name, M, Tn, _ = rs._real(key)
    pb, c = o["problem"], o["problem"]["cfg"]
    Tt = rs.Tt
    hyp = [orc.GPHyper(torch.log(Tt(c["lengthscales"])), torch.log(Tt([c["lam"]])), torch.log(Tt([c["sigma_n"]]))) for _ in range(c["G"])]
    g = torch.Generator().manual_seed(99)
    caches = []
    for ch in o["caches"]:
        pm = torch.randperm(ch.X.shape[0], generator=g)
        caches.append(orc.GPCache(ch.X[pm].contiguous(), ch.alpha[pm].contiguous(), ch.Kinv[pm][:, pm].contiguous(), ch.mX[pm].contiguous(), None))
    m = orc.SpeedModel(hyp, caches, c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    pi = pb["policy"]
    pp = orc.PolicyPar(torch.log(Tt(pi["lengthscales"])).reshape(1, -1), Tt(pi["centers"]), Tt(pi["weight"]), c["u_max"], pb["policy_kind"],
                       **pb["policy_extra"])
    cost_fn = lambda st: orc.cart_pole_cost(st, Tt(c["cost_target"]), Tt(c["cost_ls"]), c["cost_angle_index"], c["cost_pos_index"])
    with rs.one_cpu_thread():
        oc, os_, og, ost, oin = orc.policy_grad_step(m, pp, o["x0"], Tn, cost_fn, o["p"], o["eps"], o["masks"])
    return dict(cost=float(oc), grads=og, states=ost, inputs=oin)


def test_policy_gradient_step_at_the_exact_headline_launch_against_the_oracle():
    """BASELINE.json configs[1] as bench.py launches it: 100 clusters of 4 particles x 2 GPs = 200 workgroups of the lean forward kernel over
    150 time steps, the lean backward sweep behind it -- against the CPU oracle on the same x0, eps and masks and the oracle's own Kinv / alpha.

    Tolerances.  Cost rel 1e-9, std abs 1e-7.  States / inputs / gradients: SURVEY 8c's 1e-6 holds at M = 32 (test_gpu_realsize.py); over 400
    swinging cart-poles and 150 steps the WORST particle amplifies rounding differences further (measured round 6: states 1.9e-6, inputs 2.7e-6,
    gradients rel 2.3e-6, with the cost at 1.2e-11: a handful of trajectories, not a bias).  So the bound is tied to what the reference's own
    arithmetic does on this rollout: the oracle against ITSELF with the training set reordered (`_oracle_on_reordered_training_set`) -- the HIP
    path must stay within 4 x that distance (or 1e-6, whichever is larger), and within 1e-5 absolutely.  Both distances are printed."""
    import test_gpu_realsize as rs
    from gpu_helpers import dev
    from mc_pilco_amd import hipabi, ops

    rs.REAL.setdefault("se300_headline", ("c1", 400, 150))
    o = rs.oracle_answer("se300_headline")
    w = rs.hip_workload_on_oracle_operands("se300_headline")
    assert (w.M, w.T, w.model.gps[0].N, w.policy.B) == (400, 150, 300, 200)
    nz = ops.NoiseSpec(eps=o["eps"].to(dev()).contiguous(), masks=o["masks"].to(torch.uint8).to(dev()).contiguous())
    for q in w.params:
        q.grad = None
    st, inp, status = ops.rollout(w.model, w.policy, nz, o["x0"].to(dev()), w.T, o["p"])
    c, s = ops.expected_cost(w.cost, st)
    c.backward()
    L = hipabi.lib()
    assert L.mcp_debug_last_fwd_lean() == 1 and L.mcp_debug_last_particles_per_wg() == 4 and L.mcp_debug_last_gp_sharded() == 1
    assert L.mcp_debug_last_bwd_lean() == 1
    assert int(status.item()) == 0
    keys = ["log_ls", "centers", "weight"]
    grel = lambda a, b: max(float((a[k].reshape(b[k].shape) - b[k]).abs().max()) / float(b[k].abs().max()) for k in keys)
    hip_g = {k: q.grad.cpu() for q, k in zip(w.params, keys)}
    es = float((st.detach().cpu() - o["states"]).abs().max())
    eu = float((inp.detach().cpu() - o["inputs"]).abs().max())
    ec = abs(float(c.detach()) - o["cost"]) / abs(o["cost"])
    eg = grel(hip_g, o["grads"])
    r = _oracle_on_reordered_training_set(o, "se300_headline")
    rs_, ru = float((r["states"] - o["states"]).abs().max()), float((r["inputs"] - o["inputs"]).abs().max())
    rc, rg = abs(r["cost"] - o["cost"]) / abs(o["cost"]), grel(r["grads"], o["grads"])
    # where along the horizon the distance is made: the largest state error up to step 50 / 100 / 150
    upto = lambda a, b, t: float((a[:t] - b[:t]).abs().max())
    sh = st.detach().cpu()
    print("headline launch (M=400, T=150, N=300)  HIP vs oracle: states %.2e inputs %.2e cost rel %.2e std abs %.2e grad rel %.2e"
          % (es, eu, ec, abs(float(s) - o["std"]), eg))
    print("                     oracle vs oracle (training set reordered): states %.2e inputs %.2e cost rel %.2e grad rel %.2e" % (rs_, ru, rc, rg))
    print("                     state distance up to step 50 / 100 / 150: HIP %.1e / %.1e / %.1e, reordered oracle %.1e / %.1e / %.1e"
          % (upto(sh, o["states"], 50), upto(sh, o["states"], 100), es, upto(r["states"], o["states"], 50), upto(r["states"], o["states"], 100), rs_))
    assert ec < 1e-9 and abs(float(s) - o["std"]) < 1e-7
    assert upto(sh, o["states"], 50) < 1e-7  # (before the amplification sets in the two paths sit at the N = 300 contractions' rounding)
    assert es < min(1e-5, max(1e-6, 4.0 * rs_)) and eu < min(1e-5, max(1e-6, 4.0 * ru))
    assert eg < min(1e-5, max(1e-6, 4.0 * rg))


# ----------------------------------------------------------------------------------------------------------------------------------
# (b) subset-of-data selection across workgroups on the UR5 pretrain shape
# ----------------------------------------------------------------------------------------------------------------------------------
def test_sod_across_workgroups_on_the_ur5_pretrain_shape_vs_reference(golden):
    """N = 600 candidates in 10 workgroups, D = 24, SE + polynomial(1): the reference's refactor-from-scratch list, exact -- on the
    multi-workgroup kernel (the product's choice at this size) and on the one-workgroup kernel."""
    from gpu_helpers import G, spec_from
    from mc_pilco_amd import hipabi, ops

    fx = golden("sod_ur5_n600")
    sp = spec_from(fx["lengthscales"], float(fx["sigma_n"]), 1.0, [fx["poly_w1"]])
    X = G(fx["X"])
    assert tuple(X.shape) == (600, 24)
    assert hipabi.lib().mcp_sod_workspace_bytes(600) > 8 * (600 * 600 + 2 * 600)  # (room for the exchange: the multi-workgroup form runs)
    want = [int(i) for i in fx["idx"]]
    got = ops.sod_select(sp, X, float(fx["thr"]))
    print("sod_ur5_n600: kept %d of 600 (%.0f %% rejected), smallest margin |sqrt(var) - thr| of the reference's run %.3e (thr %.4g)"
          % (len(got), 100.0 * (600 - len(want)) / 600.0, float(fx["min_margin"]), float(fx["thr"])))
    assert 0.10 * 600 < 600 - len(want) < 0.45 * 600
    assert got == want
    assert ops.sod_select(sp, X, float(fx["thr"]), one_workgroup=True) == want


# ----------------------------------------------------------------------------------------------------------------------------------
# (c) the differentiable forward at N = 300
# ----------------------------------------------------------------------------------------------------------------------------------
class _OtherCriterion(torch.nn.modules.loss._Loss):
    """The formula of tests/golden/make_golden_r6.py: OtherCriterion."""

    def forward(self, out, Y):
        m_X, K, Kinv, logdet = out
        r = Y - m_X
        n = Y.shape[0]
        return (0.5 * (r.t() @ Kinv @ r) + 0.3 * logdet + 1e-3 * torch.trace(K) + 0.05 * (Kinv * Kinv).sum() / n).reshape(())


@pytest.mark.parametrize("name,deg", [("fwd_autograd_se_n300", 0), ("fwd_autograd_se_poly2_n300", 2)])
def test_forward_autograd_gradient_at_n300_vs_reference(golden, name, deg):
    """`_ForwardFunction` (Gram -> `chol_left_mfma_kernel` -> U^-1 -> K^-1; backward Wm = G_K - Kinv G_Kinv Kinv + g_logdet Kinv on the library's
    own MFMA GEMM, then `mcp_nll_grad`) against the reference's autograd through torch.cholesky / torch.inverse at N = 300: loss rel 1e-9,
    every gradient 1e-7 max(1, |g|_max) (cond(K) ~ 1e5 at sigma_n = 0.1)."""
    from test_gpu_dropin import T, mpk_dict, rbf_dict
    from mc_pilco_amd.gpr_lib.GP_prior import GP_prior as GP
    from mc_pilco_amd.gpr_lib.GP_prior import Sparse_GP, Stationary_GP

    fx = golden(name)
    assert fx["X"].shape == (300, 6)
    rbf = dict(rbf_dict(6, fx["lengthscales"], float(fx["sigma_n"])), flg_train_lambda=True)
    with quiet():
        if deg == 0:
            gp = Stationary_GP.RBF(**rbf)
        else:
            pw = [fx["poly_w%d" % k] for k in range(1, deg + 1)]
            gp = GP.Sum_Independent_GP(Stationary_GP.RBF(**rbf), Sparse_GP.get_Volterra_MPK_GP(**mpk_dict(6, deg, pw)))
    loss = _OtherCriterion()(gp(T(fx["X"])), T(fx["Y"]))
    loss.backward()
    ref_loss = float(np.asarray(fx["loss"]).reshape(-1)[0])
    names = [str(n) for n in fx["names"]]
    pars = dict(gp.named_parameters())
    worst = 0.0
    for n in names:
        ref = fx["grad__" + n].reshape(-1)
        got = pars[n].grad.detach().cpu().numpy().reshape(-1)
        worst = max(worst, float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max())))
    print("%s: loss rel %.2e, worst gradient error %.2e over %d tensors" % (name, abs(float(loss.detach()) - ref_loss) / abs(ref_loss), worst, len(names)))
    assert len(names) == 3 + deg
    assert abs(float(loss.detach()) - ref_loss) < 1e-9 * abs(ref_loss)
    assert worst < 1e-7


# ----------------------------------------------------------------------------------------------------------------------------------
# a plain Linear_GP (alone and inside a sum) on the differentiable forward
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,in_sum", [(True, False), (False, False), (True, True)])
def test_linear_gp_forward_and_gradients(offset, in_sum):
    """a default `Linear_GP` (sigma_n_log and Sigma_pos_par trainable; Sparse_GP.py:295-490), alone or as a child of
    `Sum_Independent_GP`, goes through `GP_prior.forward`'s autograd route and `get_alpha`: (K, K^-1, logdet) against torch ops on the same
    formula rel 1e-10 / 1e-8, the gradient of a criterion of all outputs w.r.t. every hyper-parameter against torch autograd rel 1e-7."""
    from gpu_helpers import dev
    from test_gpu_dropin import T, rbf_dict
    from mc_pilco_amd.gpr_lib.GP_prior import GP_prior as GP
    from mc_pilco_amd.gpr_lib.GP_prior import Sparse_GP, Stationary_GP
    from mc_pilco_amd.gpr_lib.Utils import Parameters_covariance_functions as PCF

    rs = np.random.RandomState(5 + int(offset) + 2 * int(in_sum))
    N, D = 90, 5
    X = T(rs.uniform(-1.0, 1.0, size=(N, D)))
    Y = T(rs.randn(N, 1))
    nf = D + 1 if offset else D
    w0 = 0.2 + rs.rand(nf)
    with quiet():
        lin = Sparse_GP.Linear_GP(active_dims=np.arange(D), sigma_n_init=None if in_sum else 0.3 * np.ones(1), Sigma_function=PCF.diagonal_covariance,
                                  Sigma_f_additional_par_list=[nf, True], Sigma_pos_par_init=w0, flg_offset=offset, dtype=torch.float64, device=dev())
        gp = GP.Sum_Independent_GP(Stationary_GP.RBF(**dict(rbf_dict(D, 1.0 + rs.rand(D), 0.3), flg_train_lambda=True)), lin) if in_sum else lin

    def crit(K, Kinv, logdet, r):
        return (0.5 * (r.t() @ Kinv @ r) + 0.3 * logdet + 1e-3 * torch.trace(K) + 0.05 * (Kinv * Kinv).sum() / N).reshape(())

    mX, K, Kinv, logdet = gp(X)
    loss = crit(K, Kinv, logdet, Y - mX)
    loss.backward()
    # the same kernel by torch ops on the live parameters (a second graph)
    pars = [q for q in gp.parameters() if q.requires_grad]
    got = [q.grad.detach().clone() for q in pars]
    for q in pars:
        q.grad = None
    phi = torch.cat([X, torch.ones(N, 1, dtype=torch.float64, device=dev())], 1) if offset else X
    Kt = phi @ torch.diag(torch.exp(lin.Sigma_pos_par) ** 2) @ phi.t()
    if in_sum:
        rbf = gp.gp_list[0]
        d = (X.unsqueeze(1) - X.unsqueeze(0)) / torch.exp(rbf.log_lengthscales_par).reshape(1, 1, -1)
        Kt = Kt + torch.exp(rbf.log_lambda_par) * torch.exp(-(d * d).sum(-1)) + torch.exp(rbf.sigma_n_log) ** 2 * torch.eye(N, dtype=torch.float64, device=dev())
    else:
        Kt = Kt + torch.exp(lin.sigma_n_log) ** 2 * torch.eye(N, dtype=torch.float64, device=dev())
    U = torch.linalg.cholesky(Kt).mH
    Ui = torch.inverse(U)
    Kinv_t = Ui @ Ui.t()
    logdet_t = 2.0 * torch.sum(torch.log(torch.diag(U)))
    loss_t = crit(Kt, Kinv_t, logdet_t, Y - mX.detach())
    want = torch.autograd.grad(loss_t, pars)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert rel(K.detach(), Kt.detach()) < 1e-12 and rel(Kinv.detach(), Kinv_t.detach()) < 1e-8 and abs(float(logdet) - float(logdet_t)) < 1e-10 * abs(float(logdet_t))
    assert abs(float(loss.detach()) - float(loss_t.detach())) < 1e-9 * abs(float(loss_t.detach()))
    assert len(pars) >= (4 if in_sum else 2)
    for g, w in zip(got, want):
        assert float((g - w).abs().max()) < 1e-7 * max(1.0, float(w.abs().max()))
    alpha, _, _ = gp.get_alpha(X, Y)  # (the call ADVICE r5 saw raise AttributeError)
    assert rel(alpha.detach(), (Kinv_t @ (Y - mX.detach())).detach()) < 1e-7
    # an in-place parameter change between forward and backward is refused, as torch's version check would in the reference
    out = gp(X)
    with torch.no_grad():
        lin.Sigma_pos_par.add_(0.01)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out[3].backward()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["masks", "philox"])
def test_pipelined_backward_sweep_of_the_wide_class(mode):
    """Round 6: one particle per workgroup on the wide classes (the UR5 launch script's M = 200) -- `rollout_bwd_kernel<24, 6, 512, 2, 1>` with a wave
    more than the basis functions need runs the chain of step t on wave 0 BESIDE the adjoint-independent half of the RBF stage (exp, Philox, distances)
    and prepares the features of step t - 1 beside the other half (`BwdArgs.pipe`).  Same arithmetic per basis function and per chain lane; the partial
    feature adjoints are summed over other groups of 64 basis functions, so the gradients agree with the sequential form to rounding (1e-12 relative)
    and, with recorded masks, with the oracle (1e-9, as the sequential form does)."""
    import torch
    from gpu_helpers import dev
    from mc_pilco_amd import hipabi, ops
    from test_gpu_realsize import oracle_answer, hip_workload_on_oracle_operands

    o = oracle_answer("ur5_400")
    w = hip_workload_on_oracle_operands("ur5_400")
    if mode == "masks":
        nz = ops.NoiseSpec(eps=o["eps"].to(dev()).contiguous(), masks=o["masks"].to(torch.uint8).to(dev()).contiguous())
    else:
        nz = ops.NoiseSpec(seed=11, call=2)
    L = hipabi.lib()
    out = {}
    try:
        L.mcp_debug_set_bwd_particles(1)
        for pipe in (1, 0, 1):
            L.mcp_debug_set_bwd_pipe(pipe)
            for q in w.params:
                q.grad = None
            st, inp, status = ops.rollout(w.model, w.policy, nz, o["x0"].to(dev()), w.T, o["p"])
            c, _ = ops.expected_cost(w.cost, st)
            c.backward()
            assert int(status.item()) == 0
            assert L.mcp_debug_last_bwd_pipe() == pipe and not L.mcp_debug_last_bwd_lean()
            g = [q.grad.clone() for q in w.params]
            if pipe in out:
                assert all(torch.equal(a, b) for a, b in zip(out[pipe], g))  # bitwise reproducible
            out[pipe] = g
    finally:
        L.mcp_debug_set_bwd_particles(0)
        L.mcp_debug_set_bwd_pipe(-1)
    for a, b, k in zip(out[1], out[0], ["log_ls", "centers", "weight"]):
        rel = float((a - b).abs().max() / b.abs().max())
        print("pipelined vs sequential sweep (%s) %s: rel %.2e" % (mode, k, rel))
        assert rel < 1e-12, k
        assert float(b.abs().max()) > 0.0
    if mode == "masks":
        for q, k in zip(out[1], ["log_ls", "centers", "weight"]):
            g = o["grads"][k]
            assert float((q.cpu().reshape(g.shape) - g).abs().max()) < 1e-9 * float(g.abs().max()), k
