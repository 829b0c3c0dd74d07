"""GPU: the fused closed loop under the time-varying linear feedback law (mcp_rollout_tvl + mcp_rollout_tvl_bwd, ops.rollout_tvl with an
ops.PackedTVL, MC_PILCO / MC_PILCO4PMS.apply_policy with a TV_linear_controller, and the policy under particle sharding) against torch
autograd through the oracle's step with the law -- and for the measured form the measurement -- written out (tests/tvl_models.tvl_truth,
pinned on the CPU by tests/test_tvl_cpu.py, which also asserts on the truth alone that every sampled case keeps its variances positive
and that a wrong row index shows), and the bitwise contracts it shares with mcp_rollout_pd and the open-loop kernels.

Bounds: those of tests/test_gpu_pd_rollout.py and tests/test_gpu_pd_meas.py, unchanged -- states (and measured states)
1e-9 absolute, inputs 2e-9 absolute, gradients 1e-9 relative to the gradient's largest magnitude; the gain's gradient is compared as the
whole [T, U, S] tensor, so a row the sweep drops, misplaces or leaves unwritten fails at once."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
import pd_models
import tvl_models as tm
from closed_loop_family import Family, controller
from closed_loop_family import meas_spec as spec
from gpu_helpers import DT, G, dev, relmax
from pd_meas_models import meas_model, pos_noise_for
from rank_harness import rank_group, run_ranks

pytestmark = pytest.mark.gpu
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9
TOLS = (STATE_TOL, INPUT_TOL, GRAD_TOL)

TVL = Family("rollout_tvl", lambda pol: [pol.gain] + ([pol.ff] if pol.ff is not None else []),
             lambda e: "g_gain %.3e" % e[0] + ("" if len(e) < 2 else " g_ff %.3e" % e[1]), pd_models, lambda N, deg: N + deg)


def pair(shape, N, deg):
    """TVL.pair with the sampling time a measurement model needs on the delta-state layout too (the true form never reads it)."""
    return TVL.pair(shape, N, deg, None, measured=True)


def tv_controller(c, gain, ff, target, u_max=1.0, squash=True, trainable=True):
    from mc_pilco_amd.policy_learning import Policy

    return Policy.TV_linear_controller(state_dim=c["S"], input_dim=c["U"], gain=gain, ff=ff, target_traj=G(target), flg_time_varying_gains=gain.dim() == 3,
                                       flg_train_gains=trainable, flg_train_feedforward=trainable, flg_squash=squash, u_max=u_max, dtype=DT, device=dev())


def truth_of(t):
    return clf.Truth(t.states, t.inputs, t.meas, [t.g_gain] + ([t.g_ff] if t.g_ff is not None else []), t.g_x0, t.vmin)


# ---- 1. parity with the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tm.CASES, ids=tm.case_id)
def test_parity_with_the_truth(case):
    mode, shape, deg, N, T, M, variant, opt = case
    sample = mode == "sampled"
    c, m, pmod = pair(shape, N, deg)
    torch.set_num_threads(1)
    x0, gain, ff, target, eps, w, wu, kw = tm.case_operands(case, c)
    ms = meas_model(shape, variant) if variant else None
    pn = pos_noise_for(T, M, len(ms["pos"]), tm.case_seed(T, M)) if variant else None
    truth = tm.tvl_truth(shape, m, x0, gain, ff, target, eps, w, wu, sample, ms=ms, pos_noise=pn, **kw)
    if sample and T > 1:
        assert truth.vmin > 0.0  # the oracle alone keeps every step's variance positive on this seed
    pol = tv_controller(c, gain, ff, target, **kw)
    got = TVL.run(pmod, pol, x0, T, clf.noise_buffer(eps) if sample else None, w, wu, sample, meas=spec(ms, pn))
    clf.check_against(TVL, tm.case_id(case), truth_of(truth), got, TOLS)
    assert all(tuple(g.shape) == tuple(q.shape) for g, q in zip(got.grads, TVL.params(pol)))
    if opt.get("no_g_inputs"):  # row T - 1 feeds nothing but the inputs: exact zeros, written (not left over)
        assert not opt.get("shared") and all(float(g[T - 1].abs().max()) == 0.0 for g in got.grads)
        assert all(float(g[T - 2].abs().max()) > 0.0 for g in got.grads)


def test_rows_beyond_the_horizon_get_zero_gradient():
    """gain, ff and the target longer than T (and of different lengths): the first T rows are those of the exact-length policy bit for bit,
    the rows beyond are exact zeros."""
    c, m, pmod = pair("arm2", 37, 1)
    M, T = 17, 6
    x0, kp, kd, target, eps, w, wu, gain, ff = tm.tvl_inputs(c, M, T, 9)
    exact = TVL.run(pmod, tv_controller(c, gain, ff, target[:T]), x0, T, clf.noise_buffer(eps), w, wu, True)
    longer = TVL.run(pmod, tv_controller(c, torch.cat([gain, gain[:3] + 1.0]), torch.cat([ff, ff[:1] - 2.0]), target), x0, T, clf.noise_buffer(eps), w, wu, True)
    assert torch.equal(exact.states, longer.states) and torch.equal(exact.inputs, longer.inputs) and torch.equal(exact.g_x0, longer.g_x0)
    for a, b in zip(exact.grads, longer.grads):
        assert torch.equal(a, b[:T]) and float(b[T:].abs().max()) == 0.0 and b.shape[0] > T


# ---- 2. bit identities -------------------------------------------------------------------------------------------------------------------
def _family_case(measured, M, T, seed, N=37, deg=1, shape="arm2"):
    c, m, pmod = pair(shape, N, deg)
    x0, kp, kd, target, eps, w, wu, gain, ff = tm.tvl_inputs(c, M, T, seed)
    ms = meas_model(shape) if measured else None
    pn = pos_noise_for(T, M, len(ms["pos"]), seed=seed) if measured else None
    return c, m, pmod, x0, (gain, ff, target), (kp, kd), eps, w, wu, ms, pn


@pytest.mark.parametrize("measured", [False, True])
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_plain_launch_recording_launch_and_open_loop_launch_carry_the_same_bits(noise, measured):
    c, m, pmod, x0, law, _, eps, w, wu, ms, pn = _family_case(measured, 17, 6, 21)
    pol = tv_controller(c, *law)
    meas = (lambda: spec(ms, None if noise == "philox" else pn)) if measured else None
    clf.three_way_bit_identity(TVL, pmod, pol, x0, eps, 6, noise, meas=meas, sweep=(w, wu))


def test_the_ur5_shape_carries_the_same_bits():
    """D = 24, U = 6, S = 12: the widest row of the law (U S + U + S = 90 doubles), the measured form with six pairs."""
    c, m, pmod, x0, law, _, eps, w, wu, ms, pn = _family_case(True, 5, 4, 33, N=48, deg=1, shape="ur5")
    pol = tv_controller(c, *law)
    clf.three_way_bit_identity(TVL, pmod, pol, x0, eps, 4, "eps", sweep=(w, wu))
    sp = lambda: spec(ms, pn)
    s1, s2 = sp(), sp()
    with torch.no_grad():
        st, inp, _ = TVL.op(pmod, pol.packed(), clf.noise_buffer(eps), G(x0), 4, particle_pred=True, meas=s1)
    sr, ir, _ = TVL.op(pmod, pol.packed(), clf.noise_buffer(eps), G(x0), 4, particle_pred=True, meas=s2)
    assert sr.requires_grad and torch.equal(sr.detach(), st) and torch.equal(ir.detach(), inp) and torch.equal(s1.measured, s2.measured)


def _rung(N, deg, measured):
    c, m, pmod, x0, law, _, eps, w, wu, ms, pn = _family_case(measured, 5, 3, 305, N, deg)
    torch.set_num_threads(1)
    truth = tm.tvl_truth("arm2", m, x0, *law, eps, w, wu, True, ms=ms, pos_noise=pn)
    assert truth.vmin > 0.0
    return c, pmod, law, x0, eps, 3, w, wu, truth, ((lambda: spec(ms, pn)) if measured else None)


@pytest.mark.parametrize("measured", [False, True])
def test_the_four_trajectory_rung_of_the_recording_form(measured):
    """Sampled, degree 0, N = 640, M = 5, T = 3 on arm2: the recording launch runs 4 trajectories per workgroup.  Status 0; states, inputs
    (and measurements) carry the bits of the launch without a record, whose states carry the bits of the open-loop launch on its inputs;
    everything against the truth."""
    c, pmod, law, x0, eps, T, w, wu, truth, meas = _rung(640, 0, measured)
    clf.rung_of_the_recording_form(TVL, "rung N 640", pmod, tv_controller(c, *law), x0, eps, T, w, wu, truth_of(truth), TOLS, meas)


@pytest.mark.parametrize("measured", [False, True])
def test_the_four_trajectory_tile_without_a_record(measured):
    """Sampled, N = 1200 (the k panel of 16 trajectories does not fit), nothing requires grad: status 0, the states carry the bits of the
    open-loop launch on the inputs; states, inputs (and measurements) against the truth."""
    c, pmod, law, x0, eps, T, w, wu, truth, meas = _rung(1200, 0 if measured else 2, measured)
    clf.four_trajectory_tile_without_a_record(TVL, "rung N 1200", pmod, tv_controller(c, *law, trainable=False), x0, eps, T, truth_of(truth), TOLS, meas)


def raw_run(pmod, pk, tensors, ms, nz, x0, T, w, wu, sample=True):
    """One recording launch and one sweep through mcp_rollout_tvl / mcp_rollout_tvl_bwd: (states, inputs, meas, g_part, g_x0)."""
    from mc_pilco_amd import hipabi as abi

    M, S, U = x0.shape[0], pmod.S, pmod.U
    x = G(x0)
    st, inp = torch.empty(T, M, S, dtype=DT, device=dev()), torch.empty(T, M, U, dtype=DT, device=dev())
    jac = torch.empty(max(T - 1, 1), M, pmod.G, pmod.D, dtype=DT, device=dev())
    ym = torch.zeros(T, M, S, dtype=DT, device=dev())
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    gp = torch.full(((M + 15) // 16, T, U, S + 1), float("nan"), dtype=DT, device=dev())  # (every entry must be written)
    gx = torch.empty(M, S, dtype=DT, device=dev())
    pc, nc = pk.to_c(*tensors), nz.to_c()
    mc = None
    if ms is not None:
        mc = abi.Meas()
        ms.fill(mc, T, M, ym)
    ref = lambda s: None if s is None else C.byref(s)
    gs, gi = G(w), G(wu)  # (named: the buffers must outlive the launches that read them)
    lib = abi.lib()
    abi.check(lib.mcp_rollout_tvl(C.byref(pmod.c), C.byref(pc), ref(mc), C.byref(nc), M, T, int(sample), abi.ptr(x), abi.ptr(st), abi.ptr(inp),
                                  abi.ptr(jac), None, None, abi.ptr(status), abi.stream()), "mcp_rollout_tvl")
    abi.check(lib.mcp_rollout_tvl_bwd(C.byref(pmod.c), C.byref(pc), ref(mc), M, T, abi.ptr(st), abi.ptr(inp), abi.ptr(jac), abi.ptr(gs), abi.ptr(gi),
                                      abi.ptr(gp), abi.ptr(gx), abi.stream()), "mcp_rollout_tvl_bwd")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return st, inp, ym, gp, gx


@pytest.mark.parametrize("measured", [False, True])
def test_run_to_run_and_shard_invariance(measured):
    """Two runs of launch and sweep give the same bits; rows [a, b) launched with particle_offset = a (a 16 + 1 split, Philox) give the bits
    of one launch over all rows: states, inputs, measurements, g_x0 rows and -- a slab depends on its own trajectories alone -- the slab of
    g_part each part owns.  Every entry of g_part is written (the buffer starts as NaN) and is finite."""
    from mc_pilco_amd import ops

    c, m, pmod, x0, law, _, eps, w, wu, ms, pn = _family_case(measured, 17, 6, 9, deg=0)
    pk = tv_controller(c, *law).packed()
    tensors = (G(law[0]), G(law[1]))

    def run(a, b):
        return raw_run(pmod, pk, tensors, spec(ms), ops.NoiseSpec(seed=4, call=2, particle_offset=a), x0[a:b], 6, w[:, a:b], wu[:, a:b])

    whole, again = run(0, 17), run(0, 17)
    assert all(torch.equal(p, q) for p, q in zip(whole, again))
    assert bool(torch.isfinite(whole[3]).all()) and all(float(whole[3][i].abs().amax((1, 2)).min()) > 0 for i in (0, 1))
    for i, (a, b) in enumerate(((0, 16), (16, 17))):
        part = run(a, b)
        for j in (0, 1, 2):
            assert torch.equal(part[j], whole[j][:, a:b])
        assert tuple(part[3].shape) == (1, 6, 2, 5) and torch.equal(part[3][0], whole[3][i]) and torch.equal(part[4], whole[4][a:b])


def test_either_output_of_the_sweep_may_be_left_out():
    """g_part NULL and g_x0 NULL in turn through ops (only one of x0 / the parameters requires grad): the other output carries the same bits."""
    c, m, pmod, x0, law, _, eps, w, wu, ms, pn = _family_case(False, 17, 6, 9)
    full = TVL.run(pmod, tv_controller(c, *law), x0, 6, clf.noise_buffer(eps), w, wu, True)
    no_x0 = TVL.run(pmod, tv_controller(c, *law), x0, 6, clf.noise_buffer(eps), w, wu, True, x0_grad=False)
    assert no_x0.g_x0 is None and all(torch.equal(a, b) for a, b in zip(no_x0.grads, full.grads))
    frozen = TVL.run(pmod, tv_controller(c, *law, trainable=False), x0, 6, clf.noise_buffer(eps), w, wu, True)
    assert frozen.grads == [None, None] and torch.equal(frozen.g_x0, full.g_x0)
    from mc_pilco_amd.policy_learning import Policy

    pol = tv_controller(c, *law)
    pol.gain.requires_grad_(False)  # flg_train_gains = False: only the feedforward is trained
    ff_only = TVL.run(pmod, pol, x0, 6, clf.noise_buffer(eps), w, wu, True)
    assert ff_only.grads[0] is None and torch.equal(ff_only.grads[1], full.grads[1])
    assert isinstance(pol, Policy.TV_linear_controller)


# ---- 3. the PD special case ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measured", [False, True])
def test_pd_gains_against_the_pd_launch(measured):
    """from_pd gains against ops.rollout_pd on the same Philox stream, to the parity bounds (not bitwise: the dense dot adds its terms in
    another order).  The dense sweep leaves at the kp / kd entries, summed over the rows, 1 / (2 sqrt_k) of the PD sweep's gradient -- to
    1e-9 relative, entry by entry."""
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import Policy

    c, m, pmod, x0, law, (kp, kd), eps, w, wu, ms, pn = _family_case(measured, 17, 6, 9, deg=2)
    pd_pol = controller(c, kp, kd, law[2])
    nz = lambda: ops.NoiseSpec(seed=4, call=2)
    pd = clf.PD.run(pmod, pd_pol, x0, 6, nz(), w, wu, True, meas=spec(ms))
    pol = Policy.TV_linear_controller.from_pd(pd_pol, 6)
    assert pol.fusable(pmod, 6) and torch.equal(pol.gain.detach().cpu(), tm.from_pd(kp, kd, c["S"], 6))
    got = TVL.run(pmod, pol, x0, 6, nz(), w, wu, True, meas=spec(ms))
    es, ei = float((got.states - pd.states).abs().max()), float((got.inputs - pd.inputs).abs().max())
    k, h = torch.arange(c["U"]), c["S"] // 2
    gkp, gkd = 2 * G(kp) * got.grads[0][:, k, k].sum(0), 2 * G(kd) * got.grads[0][:, k, h + k].sum(0)
    eg = [float(((a - b).abs() / b.abs()).max()) for a, b in ((gkp, pd.grads[0]), (gkd, pd.grads[1]))]
    print("from_pd vs rollout_pd: states %.3e inputs %.3e g_kp %.3e g_kd %.3e g_x0 %.3e" % (es, ei, eg[0], eg[1], relmax(got.g_x0, pd.g_x0)))
    assert got.status == 0 and es < STATE_TOL and ei < INPUT_TOL and max(eg) < 1e-9 and relmax(got.g_x0, pd.g_x0) < GRAD_TOL
    assert (not measured) or float((got.meas - pd.meas).abs().max()) < STATE_TOL


# ---- 4. Philox mode: central differences of the op ---------------------------------------------------------------------------------------------
def test_philox_mode_against_central_differences():
    """Step 1e-6, bound 1e-5 relative with floor 1e-3, as tests/test_gpu_pd_rollout.py has it, on its case (arm2, N = 37, degree 2, M = 3,
    T = 6): three gain entries and two feedforward entries in different rows, and an entry of x0."""
    c, m, pmod = pair("arm2", 37, 2)
    M, T = 3, 6
    x0, kp, kd, target, _, w, wu, gain, ff = tm.tvl_inputs(c, M, T, 41)
    policy_of = lambda ts, trainable: tv_controller(c, ts[0], ts[1], target, trainable=trainable)
    US = c["U"] * c["S"]
    checks = [("gain[0,0,1]", 0, 1), ("gain[2,1,3]", 0, 2 * US + 7), ("gain[5,0,2]", 0, 5 * US + 2), ("ff[1,0]", 1, 2), ("ff[4,1]", 1, 9),
              ("x0[2,1]", 2, 2 * c["S"] + 1)]
    clf.central_differences(TVL, pmod, policy_of, [gain, ff], x0, w, wu, T, checks, step=1e-6, bound=(1e-5, 1e-3))


# ---- 5. status ------------------------------------------------------------------------------------------------------------------------------
def test_status_word():
    """clf.status_word; a NaN gain entry and a NaN feedforward entry reach the inputs and raise STATUS_NAN."""
    from mc_pilco_amd import hipabi

    c, m, pmod, x0, (gain, ff, target), _, eps, w, wu, ms, pn = _family_case(False, 5, 4, 31, deg=0)
    T = 4
    good = tv_controller(c, gain, ff, target, trainable=False).packed()
    bad = x0.clone()
    bad[3, 1] = float("nan")
    zero = tv_controller(c, gain, torch.zeros_like(ff), torch.zeros(4, 4, dtype=DT), trainable=False).packed()  # target 0, x = 0, ff = 0: u = 0 exactly
    clf.status_word(TVL, pmod, c, good, (good, bad), zero, x0, eps, T)
    nan_gain, nan_ff = gain.clone(), ff.clone()
    nan_gain[2, 1, 3] = float("nan")
    nan_ff[3, 0] = float("nan")
    for pol in (tv_controller(c, nan_gain, ff, target, trainable=False), tv_controller(c, gain, nan_ff, target, trainable=False)):
        st, inp, status = TVL.op(pmod, pol.packed(), None, G(x0), T, particle_pred=False)
        assert int(status.item()) & hipabi.STATUS_NAN and bool(torch.isnan(inp).any())


# ---- 6. class path ---------------------------------------------------------------------------------------------------------------------------
ARM_TARGET = lambda T: 0.3 * np.sin(0.3 * np.arange(T + 2).reshape(-1, 1) + np.array([0.0, 1.0, 2.0, 3.0]).reshape(1, -1))


def _arm_law(T):
    gen = torch.Generator().manual_seed(12)
    gain = tm.from_pd(torch.tensor([1.0, 1.2], dtype=DT), torch.tensor([0.5, 0.4], dtype=DT), 4, T) + 0.1 * torch.randn(T, 2, 4, dtype=DT, generator=gen)
    return gain, 0.2 * torch.randn(T, 2, dtype=DT, generator=gen)


def _arm_object(T, pms=None):
    from mc_pilco_amd.policy_learning import Policy

    gain, ff = _arm_law(T)
    par = dict(state_dim=4, input_dim=2, gain=gain, ff=ff, target_traj=G(ARM_TARGET(T)), flg_squash=True, u_max=1.5, dtype=DT, device=dev())
    return clf.arm_object(Policy.TV_linear_controller, par, pms)


@pytest.mark.parametrize("cls_name", ["MC_PILCO", "MC_PILCO4PMS"])
def test_class_path(cls_name):
    """The fused launch against the same object's step loop (fused_feedback = False) in "reference" noise mode: states, inputs and the two
    gradients at the bounds of the same comparison in tests/test_gpu_pid_rollout.py; a short reinforce_policy run moves both tensors and
    lowers the cost."""
    M, T = 16, 8
    sim = clf.sim_args(M, T)
    pms = clf.ARM_PMS if cls_name == "MC_PILCO4PMS" else None

    def rollout(fused):
        obj = _arm_object(T, pms)
        obj.fused_feedback = fused
        torch.manual_seed(5)
        with clf.normal_draws_on_the_cpu():
            st, inp = obj.apply_policy(**sim)
        assert obj.last_feedback_fused is fused and (obj.last_status is not None) is (fused or obj.last_step_fused)
        if fused:
            assert int(obj.last_status.item()) == 0
        cost, _ = obj.cost_function(st, inp, 0)
        cost.backward()
        return st.detach(), inp.detach(), [q.grad.clone() for q in TVL.params(obj.control_policy)]

    fs, fi, fg = rollout(True)
    ss, si, sg = rollout(False)
    es, ei, eg = float((fs - ss).abs().max()), float((fi - si).abs().max()), [relmax(a, b) for a, b in zip(fg, sg)]
    print("%s, fused vs step: states %.3e inputs %.3e %s" % (cls_name, es, ei, TVL.grad_text(eg)))
    assert es < STATE_TOL and ei < INPUT_TOL and max(eg) < GRAD_TOL

    obj = _arm_object(T, pms)
    torch.manual_seed(6)
    buf = io.StringIO()
    with clf.normal_draws_on_the_cpu(), contextlib.redirect_stdout(buf):
        out = obj.reinforce_policy(**clf.reinforce_args(sim, T, 5))
    assert obj.last_feedback_fused is True
    cost = np.asarray(out[0], dtype=float).reshape(-1)
    moved = [float((q.detach().cpu() - v).abs().max()) for q, v in zip(TVL.params(obj.control_policy), _arm_law(T))]
    print("cost sequence:", cost, "gain and ff moved by", moved)
    assert cost.shape == (5,) and min(moved) > 1e-3 and cost[-1] < cost[0]


# ---- 7. class path, two ranks on one device ---------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401

    torch.cuda.set_device(dev())
    with rank_group(rank, world, port):
        res = {}
        for cls_name in ("MC_PILCO", "MC_PILCO4PMS"):
            obj = _arm_object(6, clf.ARM_PMS if cls_name == "MC_PILCO4PMS" else None)
            obj.noise_mode = "philox"
            res[cls_name] = clf.sharded_step(TVL, obj, world, clf.sim_args(17, 6))
        out_q.put((rank, res))


def test_two_rank_particle_sharding_matches_single_process():
    """MC_PILCO and MC_PILCO4PMS with the policy under shard_particles (M = 17, Philox): each rank's states are the matching slice of the
    one-process run bit for bit; the pooled cost, its std and the two tensors' gradients agree to the bounds (another order of the sums)."""
    one = run_ranks(_rank, 1)
    two = run_ranks(_rank, 2)
    clf.two_ranks_match_one_process(TVL, one, two, GRAD_TOL, n_grads=2)
