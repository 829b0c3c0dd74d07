"""GPU: trajectory optimisation on the GP model -- mcp_linearize and mcp_lqr_pass through ops.linearize / ops.lqr_pass, the driver
policy_learning/ilqr.py and TV_linear_controller.from_lqr -- against the truth of tests/lqr_models.py (pinned on the CPU by
tests/test_lqr_truth_cpu.py).

Bounds.  Linearisation: GRAD_TOL of tests/test_gpu_tvl_rollout.py, 1e-9 relative to the largest entry (the same record, composed the way
the sweep that test bounds composes it); against ops.model_step's backward on the same row 1e-12 relative.  Pass: per case and output
(gain, kff, dv) max(1e-12, 64 d_ref) relative to the output's largest entry, d_ref the difference between the recursion in float64 and in
long double on that case (the truth's own rounding measures the case's conditioning; 64 allows for another order of the sums over
T <= 12 rows); the truth is given the KERNEL's A and B, so only the recursion's arithmetic differs.  The same bound holds the longest
horizon, T = MCP_LQR_MAX_T = 2048 (arm2, reg 1e-3, cond(Quu) <= 5.9), where an MI355X measured gain / kff / dv 9.3e-16 / 1.3e-15 / 7.0e-16
against the float64 recursion at d_ref 9.3e-16 / 1.5e-15 / 1.1e-15: the kernel is inside 64 d_ref there as at T = 12 (the regularised
recursion contracts, its rounding does not grow with the horizon), so no second float64 truth was needed."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
import layout_models
import lqr_models as lm
import pd_models
from gpu_helpers import DT, G, dev, relmax

pytestmark = pytest.mark.gpu
GRAD_TOL, STEP_TOL = 1e-9, 1e-12
CASES = [(s, d, N, T, M) for (s, d, N) in lm.MODELS for (T, M) in lm.SIZES]
cid = lambda c: "-".join(str(v) for v in c)


def pair(shape, N, deg):
    """A shape of pd_models or a layout of tests/layout_models.py."""
    models = layout_models if shape in layout_models.LAYOUTS else pd_models
    return clf.pair(models.build_pair, shape, N, deg, N + deg, None, pd_models.family(shape) == "delta")


def bound(d):
    return max(1e-12, 64.0 * d)


@functools.lru_cache(maxsize=None)
def record(shape, deg, N, T, M, sample, u_max=1.0):
    """The operands of a case and its record on the device: (c, oracle model, packed model, operands, states, jac)."""
    from mc_pilco_amd import ops

    c, m, pm = pair(shape, N, deg)
    um = list(u_max) if isinstance(u_max, tuple) else u_max
    o = lm.operands(c, T, M, 100 * T + M, um)
    x0, a, u, du, eps, target = o
    nz = ops.NoiseSpec(eps=G(eps)) if sample else None
    states, jac, status = ops.rollout_open_record(pm, G(x0), G(u[:T - 1]), noise=nz, particle_pred=sample)
    assert int(status.item()) == 0
    return c, m, pm, o, states, jac


# ---- 1. linearisation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [False, True], ids=["mean", "sampled"])
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_linearisation_against_autograd(case, sample):
    from mc_pilco_amd import ops

    shape, deg, N, T, M = case
    c, m, pm, (x0, a, u, du, eps, target), states, jac = record(shape, deg, N, T, M, sample)
    torch.set_num_threads(1)
    st_o = lm.oracle_rollout(shape, m, x0, u[:T - 1], eps, sample)
    assert float((states.cpu() - st_o).abs().max()) < 1e-9
    At, Bt = lm.autograd_AB(shape, m, st_o, u, eps, sample)
    A, B = ops.linearize(pm, states, jac)
    As, Bs = ops.linearize(pm, states, jac, du_da=G(du))
    ea, eb, ebs = relmax(A, At), relmax(B, Bt), relmax(Bs, Bt * du[:T - 1].unsqueeze(2))
    print("%s %s: A %.3e B %.3e B scaled %.3e" % (cid(case), "sampled" if sample else "mean", ea, eb, ebs))
    assert tuple(A.shape) == (T - 1, M, c["S"], c["S"]) and tuple(B.shape) == (T - 1, M, c["S"], c["U"])
    assert max(ea, eb, ebs) < GRAD_TOL and torch.equal(As, A)
    # each output alone
    A1, none = ops.linearize(pm, states, jac, du_da=G(du), want=(True, False))
    none2, B1 = ops.linearize(pm, states, jac, du_da=G(du), want=(False, True))
    assert none is None and none2 is None and torch.equal(A1, A) and torch.equal(B1, Bs)
    # g^T A, g^T B against the backward of one fused model step on the same row
    gen = torch.Generator().manual_seed(5)
    g = G(torch.randn(M, c["S"], dtype=DT, generator=gen))
    for t in sorted({0, T - 2}):
        xg, ug = states[t].clone().requires_grad_(True), G(u[t]).requires_grad_(True)
        nz = ops.NoiseSpec(eps=G(eps[t])) if sample else None
        nxt, status = ops.model_step(pm, xg, ug, t, noise=nz, particle_pred=sample)
        (g * nxt).sum().backward()
        ga, gb = torch.einsum("mr,mrc->mc", g, A[t]), torch.einsum("mr,mrk->mk", g, B[t])
        ex, eu = relmax(ga, xg.grad), relmax(gb, ug.grad)
        print("   row %d against model_step's backward: g^T A %.3e g^T B %.3e" % (t, ex, eu))
        assert int(status.item()) == 0 and torch.equal(nxt.detach(), states[t + 1]) and max(ex, eu) < STEP_TOL


# ---- 2. the pass ---------------------------------------------------------------------------------------------------------------------------
def cost_rows(c, T, states, a, target, u_max=1.0, r=1.0):
    from mc_pilco_amd.policy_learning.ilqr import Quadratic_tracking_cost

    cost = Quadratic_tracking_cost(target, torch.ones(c["S"], dtype=DT), input_lengthscales=[r] * c["U"])
    return cost.expansion(states, G(a), u_max, True)


def truth_of_the_pass(A, B, rows, reg):
    """riccati_truth and riccati_truth_ld per trajectory on the kernel's A, B: (gain [M,T,U,S], kff [M,T,U], dv [M,2]) twice, and the largest
    cond(Quu) of the case."""
    n = lambda v: v.detach().cpu().numpy()
    A, B, (lx, lu, hxx, huu) = n(A), n(B), [n(v) for v in rows]
    f64, ld, cond = [], [], 0.0
    for m in range(lx.shape[1]):
        args = (A[:, m], B[:, m], lx[:, m], lu[:, m], hxx[:, m], huu[:, m], reg)
        f64.append(lm.riccati_truth(*args))
        ld.append(lm.riccati_truth_ld(*args))
        cond = max(cond, f64[-1][3])
    stack = lambda res: [np.stack([r[i] for r in res]) for i in range(3)]
    return stack(f64), stack(ld), cond


def check_pass(what, got, f64, ld, cond):
    d = lm.d_ref(f64, ld)
    errs = [float(np.abs(g.detach().cpu().numpy() - t).max() / np.abs(t).max()) for g, t in zip(got, f64)]
    errs_ld = [float(np.abs(g.detach().cpu().numpy().astype(np.longdouble) - t).max() / np.abs(t).max()) for g, t in zip(got, ld)]
    print("%s: cond(Quu) <= %.2e | gain / kff / dv: d_ref %.2e %.2e %.2e, kernel vs float64 truth %.2e %.2e %.2e, vs long double %.2e %.2e %.2e"
          % ((what, cond) + tuple(d) + tuple(errs) + tuple(errs_ld)))
    assert cond <= 1e4  # (of the truth: the cost rows keep every Quu well conditioned)
    for e, dr in zip(errs, d):
        assert e <= bound(dr)


PASS_CASES = [c + (reg, 1.0) for c in CASES for reg in (0.0, 1e-3)] + [("arm2", 0, 37, 12, 5, 1e-3, (0.4, 1.7)), ("ur5", 1, 48, 3, 17, 0.0, (0.5, 0.7, 0.9, 1.1, 1.3, 1.5)),
                                                                           # every compiled limit of the model at once (G D = 256 = the pass's threads: the whole
                                                                           # workgroup prefetches jac), a bound per input
                                                                           ("limits", 0, 37, 3, 17, 0.0, (0.5, 0.6, 0.7, 0.8, 0.9, 1.1, 1.3, 1.5))]


@pytest.mark.parametrize("case", PASS_CASES, ids=cid)
def test_pass_against_the_recursion(case):
    from mc_pilco_amd import ops

    shape, deg, N, T, M, reg, u_max = case
    c, m, pm, (x0, a, u, du, eps, target), states, jac = record(shape, deg, N, T, M, False, u_max)
    um = list(u_max) if isinstance(u_max, tuple) else u_max
    J, lx, lu, hxx, huu, s = cost_rows(c, T, states, a, target, um)
    assert float((s.cpu() - du).abs().max()) < 1e-15
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    got = ops.lqr_pass(pm, states, jac, lx, lu, hxx, huu, reg=reg, du_da=s, status=status)
    assert int(status.item()) == 0 and tuple(got[0].shape) == (M, T, c["U"], c["S"]) and tuple(got[1].shape) == (M, T, c["U"]) and tuple(got[2].shape) == (M, 2)
    assert float(got[0][:, T - 1].abs().max()) == 0.0  # the last row has no gain
    A, B = ops.linearize(pm, states, jac, du_da=s)
    f64, ld, cond = truth_of_the_pass(A, B, (lx, lu, hxx, huu), reg)
    check_pass(cid(case), got, f64, ld, cond)
    assert bool((got[2][:, 0] < 0).all()) and bool((got[2][:, 1] > 0).all())


def test_pass_without_du_da_reads_ones():
    from mc_pilco_amd import ops

    c, m, pm, (x0, a, u, du, eps, target), states, jac = record("arm2", 0, 37, 12, 5, False)
    J, lx, lu, hxx, huu, s = cost_rows(c, 12, states, a, target)
    assert all(torch.equal(p, q) for p, q in zip(ops.lqr_pass(pm, states, jac, lx, lu, hxx, huu, reg=1e-3),
                                                 ops.lqr_pass(pm, states, jac, lx, lu, hxx, huu, reg=1e-3, du_da=torch.ones_like(s))))


# ---- 2b. the size limits: the longest horizon, the grid stride of the linearisation ------------------------------------------------------------
LONG = ("arm2", 0, 37)


def test_the_longest_horizon():
    """T = MCP_LQR_MAX_T = 2048 (dvt in dynamic LDS at its largest), M = 2, reg = 1e-3, mean record: status 0, every output finite, the pass
    against the recursion on the kernel's own A, B within bound(d_ref) -- d_ref at this length is the reference's own measure of the
    conditioning, printed beside the kernel's error --, and trajectory 0 carries the bits of an M = 1 launch."""
    from mc_pilco_amd import hipabi, ops

    T, M, reg = hipabi.LQR_MAX_T, 2, 1e-3
    assert T == 2048
    c, m, pm, (x0, a, u, du, eps, target), states, jac = record(*LONG, T, M, False)
    J, lx, lu, hxx, huu, s = cost_rows(c, T, states, a, target)
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    got = ops.lqr_pass(pm, states, jac, lx, lu, hxx, huu, reg=reg, du_da=s, status=status)
    assert int(status.item()) == 0 and bool(torch.isfinite(states).all()) and all(bool(torch.isfinite(v).all()) for v in got)
    A, B = ops.linearize(pm, states, jac, du_da=s)
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(B).all())
    torch.set_num_threads(1)
    f64, ld, cond = truth_of_the_pass(A, B, (lx, lu, hxx, huu), reg)
    check_pass("T %d M %d reg %g" % (T, M, reg), got, f64, ld, cond)
    one = ops.lqr_pass(pm, *[v[:, :1].contiguous() for v in (states, jac, lx, lu, hxx, huu)], reg=reg, du_da=s[:, :1].contiguous())
    assert all(torch.equal(p[0], q[0]) for p, q in zip(one, got))


def test_the_grid_stride_of_the_linearisation():
    """T = 2048, M = 33: (T - 1) M = 67 551 elements' worth of rows, above the 65 536 blocks of one pass over the grid.  The launch over the
    whole record equals, bit for bit, its launches over the slices [:, 0:16], [:, 16:32], [:, 32:33], each below that limit -- with and
    without du_da, and with one output alone."""
    from mc_pilco_amd import hipabi, ops

    T, M = hipabi.LQR_MAX_T, 33
    assert (T - 1) * M > 65536 > (T - 1) * 16
    c, m, pm, (x0, a, u, du, eps, target), states, jac = record(*LONG, T, M, False)
    dg = G(du)
    assert bool(torch.isfinite(states).all()) and bool(torch.isfinite(jac).all())
    cut = lambda v, sl: None if v is None else v[:, sl].contiguous()
    for d in (None, dg):
        for want in ((True, True), (True, False), (False, True)):
            whole = ops.linearize(pm, states, jac, du_da=d, want=want)
            parts = [ops.linearize(pm, cut(states, sl), cut(jac, sl), du_da=cut(d, sl), want=want) for sl in (slice(0, 16), slice(16, 32), slice(32, 33))]
            for i, out in enumerate(whole):
                assert (out is None) == (not want[i])
                if out is not None:
                    assert bool(torch.isfinite(out).all()) and torch.equal(out, torch.cat([p[i] for p in parts], 1))
    A, B = ops.linearize(pm, states, jac)
    assert float(A.abs().max()) > 0 and float(B[T - 2, M - 1].abs().max()) > 0  # (the last element of the last row was written)


# ---- 3. independence and reproducibility -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", lm.MODELS, ids=cid)
def test_bits_do_not_depend_on_the_run_or_on_the_launch(model):
    from mc_pilco_amd import ops

    shape, deg, N = model
    T, M = 3, 17
    c, m, pm, (x0, a, u, du, eps, target), states, jac = record(shape, deg, N, T, M, False)
    J, lx, lu, hxx, huu, s = cost_rows(c, T, states, a, target)
    run = lambda sl: ops.lqr_pass(pm, *[v[:, sl].contiguous() for v in (states, jac, lx, lu, hxx, huu)], reg=1e-3, du_da=s[:, sl].contiguous())
    whole, again = run(slice(0, M)), run(slice(0, M))
    assert all(torch.equal(p, q) for p, q in zip(whole, again)) and bool(torch.isfinite(whole[0]).all())
    for i in (0, 7, 16):
        one = run(slice(i, i + 1))
        assert all(torch.equal(p[0], q[i]) for p, q in zip(one, whole))
    lin = lambda sl: ops.linearize(pm, states[:, sl].contiguous(), jac[:, sl].contiguous(), du_da=s[:, sl].contiguous())
    (A, B), (A7, B7) = lin(slice(0, M)), lin(slice(7, 8))
    assert torch.equal(A[:, 7:8], A7) and torch.equal(B[:, 7:8], B7)


# ---- 4. status ---------------------------------------------------------------------------------------------------------------------------------
def test_status_and_the_failed_trajectory():
    """A negative huu in one row of one trajectory (reg = 0) raises MCP_STATUS_NOT_SPD alone, a NaN in lx MCP_STATUS_NAN alone; that
    trajectory's outputs are all NaN and the other four carry the bits of the clean launch.  (The kernel takes its documented branch.)"""
    from mc_pilco_amd import hipabi, ops

    T, M = 12, 5
    c, m, pm, (x0, a, u, du, eps, target), states, jac = record("arm2", 0, 37, T, M, False)
    J, lx, lu, hxx, huu, s = cost_rows(c, T, states, a, target)

    def run(lx_, huu_):
        status = torch.zeros(1, dtype=torch.int32, device=dev())
        return ops.lqr_pass(pm, states, jac, lx_, lu, hxx, huu_, reg=0.0, du_da=s, status=status), int(status.item())

    clean, word = run(lx, huu)
    assert word == 0 and all(bool(torch.isfinite(v).all()) for v in clean)
    for row, traj, bit in ((3, 2, hipabi.STATUS_NOT_SPD), (T - 1, 4, hipabi.STATUS_NOT_SPD), (5, 1, hipabi.STATUS_NAN), (T - 1, 0, hipabi.STATUS_NAN),
                           (0, 3, hipabi.STATUS_NAN)):
        lx_, huu_ = lx.clone(), huu.clone()
        if bit == hipabi.STATUS_NOT_SPD:
            huu_[row, traj, 0] = -50.0
        else:
            lx_[row, traj, 1] = float("nan")
        got, word = run(lx_, huu_)
        assert word == bit, (row, traj, word)
        for g, cl in zip(got, clean):
            assert bool(torch.isnan(g[traj]).all())
            keep = [i for i in range(M) if i != traj]
            assert torch.equal(g[keep], cl[keep])


# ---- 5. the driver -----------------------------------------------------------------------------------------------------------------------------
def _driver_case():
    from mc_pilco_amd.policy_learning.ilqr import Quadratic_tracking_cost

    T = 12
    c, m, pm = pair("arm2", 37, 0)
    x0, _, _, target = pd_models.inputs_for(c, 1, T, 3)[:4]
    cost = Quadratic_tracking_cost(target[:T], torch.ones(4, dtype=DT), input_lengthscales=[2.0, 2.0])
    return c, m, pm, T, x0[0], torch.zeros(T, 2, dtype=DT), cost


def test_zero_iterations_is_one_pass_about_the_rollout():
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning.ilqr import ilqr

    c, m, pm, T, x0, a0, cost = _driver_case()
    ctrl, info = ilqr(pm, x0, a0, cost, iterations=0)
    a = G(a0)
    states, jac, _ = ops.rollout_open_record(pm, G(x0.reshape(1, -1)), torch.tanh(a)[:T - 1].reshape(T - 1, 1, 2).contiguous())
    J, lx, lu, hxx, huu, s = cost.expansion(states, a.reshape(T, 1, 2), 1.0, True)
    gain, kff, dv = ops.lqr_pass(pm, states, jac, lx, lu, hxx, huu, reg=1e-6, du_da=s)
    assert torch.equal(ctrl.gain.detach(), gain[0]) and torch.equal(ctrl.ff.detach(), a) and torch.equal(info["kff"], kff[0])
    assert torch.equal(ctrl.target_traj, states[:, 0]) and info["status"] == [0] and info["alpha"] == [] and len(info["cost"]) == 1
    assert ctrl.gain.requires_grad and ctrl.ff.requires_grad and ctrl.flg_time_varying_gains and ctrl.flg_squash


def test_five_iterations():
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning.ilqr import ilqr

    c, m, pm, T, x0, a0, cost = _driver_case()
    torch.set_num_threads(1)
    first, info0 = ilqr(pm, x0, a0, cost, iterations=0)
    ctrl, info = ilqr(pm, x0, a0, cost, iterations=5)
    J, al = info["cost"], info["alpha"]
    print("ilqr cost per pass:", J, "alpha:", al, "reg:", info["reg"], "status:", info["status"])
    assert len(al) >= 1 and al[0] > 0 and len(J) == len(al) + 1 and all(w == 0 for w in info["status"])
    assert all(b < a for a, b, step in zip(J, J[1:], al) if step > 0) and all(b == a for a, b, step in zip(J, J[1:], al) if step == 0)
    # the first pass against the loop on the oracle
    truth = lm.ilqr_truth("arm2", m, x0, a0, cost, iterations=1)
    ops_ = truth["operands"][0]
    d = lm.d_ref(lm.riccati_truth(*ops_), lm.riccati_truth_ld(*ops_))
    tg, tk, _ = truth["passes"][0]
    eg = float(np.abs(first.gain.detach().cpu().numpy() - tg).max() / np.abs(tg).max())
    ek = float(np.abs(info0["kff"].cpu().numpy() - tk).max() / np.abs(tk).max())
    print("first pass against ilqr_truth: gain %.3e (bound %.3e) kff %.3e (bound %.3e); truth cost %s alpha %s"
          % (eg, bound(d[0]), ek, bound(d[1]), truth["cost"], truth["alpha"]))
    assert eg <= bound(d[0]) and ek <= bound(d[1])
    assert abs(J[0] - truth["cost"][0]) < 1e-9 * abs(J[0]) and al[0] == truth["alpha"][0]
    # the controller reproduces its own nominal: the error is zero along it, so a = ff
    with torch.no_grad():
        st, inp, status = ops.rollout_tvl(pm, ctrl.packed(), None, G(x0.reshape(1, -1)), T, particle_pred=False)
    es, ei = float((st[:, 0] - info["states"]).abs().max()), float((inp[:, 0] - info["inputs"]).abs().max())
    print("the controller's rollout against the final nominal: states %.3e inputs %.3e" % (es, ei))
    assert int(status.item()) == 0 and es <= 1e-13 and ei <= 1e-13
    assert torch.equal(ctrl.target_traj, info["states"]) and torch.equal(ctrl.ff.detach(), info["a"])


ARM_TARGET = lambda T: 0.3 * np.sin(0.3 * np.arange(T + 2).reshape(-1, 1) + np.array([0.0, 1.0, 2.0, 3.0]).reshape(1, -1))


def test_from_lqr_and_the_class_path():
    """from_lqr on a packed model and on a Model_learning; the controller is fusable, and one step of MC_PILCO with it (the pattern of
    tests/test_gpu_tvl_rollout.py::test_class_path) leaves finite gradients on gain and ff and a status of 0."""
    from mc_pilco_amd.policy_learning import Policy
    from mc_pilco_amd.policy_learning.ilqr import Quadratic_tracking_cost

    c, m, pm, T, x0, a0, cost = _driver_case()
    pol = Policy.TV_linear_controller.from_lqr(pm, x0, a0, cost, iterations=2, flg_train_gains=False)
    assert isinstance(pol, Policy.TV_linear_controller) and pol.fusable(pm, T) and not pol.gain.requires_grad and pol.ff.requires_grad
    with pytest.raises(ValueError):
        Policy.TV_linear_controller.from_lqr(pm, x0, a0, cost, flg_time_varying_gains=False)

    T = 8
    par = dict(state_dim=4, input_dim=2, gain=torch.zeros(T, 2, 4, dtype=DT), ff=torch.zeros(T, 2, dtype=DT), target_traj=G(ARM_TARGET(T)),
               flg_squash=True, u_max=1.5, dtype=DT, device=dev())
    obj = clf.arm_object(Policy.TV_linear_controller, par)
    cost8 = Quadratic_tracking_cost(ARM_TARGET(T), [0.5, 0.5, 2.0, 2.0], input_lengthscales=[3.0, 3.0])
    with contextlib.redirect_stdout(io.StringIO()):
        pol = Policy.TV_linear_controller.from_lqr(obj.model_learning, [0.1, -0.1, 0.0, 0.05], torch.zeros(T, 2, dtype=DT), cost8, iterations=3, u_max=1.5)
    assert pol.fusable(obj.model_learning.packed(), T) and pol.u_max == 1.5
    obj.control_policy = pol
    torch.manual_seed(5)
    with clf.normal_draws_on_the_cpu():
        st, inp = obj.apply_policy(**clf.sim_args(16, T))
    assert obj.last_feedback_fused is True and int(obj.last_status.item()) == 0
    loss, _ = obj.cost_function(st, inp, 0)
    loss.backward()
    for q in (pol.gain, pol.ff):
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0
