"""GPU: the fused closed loop under the PID controller (mcp_rollout_pid + mcp_rollout_pid_bwd, ops.rollout_pd with an ops.PackedPID,
MC_PILCO / MC_PILCO4PMS.apply_policy with a PID_controller, and the policy under particle sharding) against torch autograd through the
oracle's step with the law -- and for the measured form the measurement -- written out (tests/pid_models.pid_truth, checked on the CPU by
tests/test_pid_cpu.py, which also asserts the clamp conditions of every case on the truth alone), and the bitwise contracts it shares with
mcp_rollout_pd and the open-loop kernels.

Bounds: those of tests/test_gpu_pd_rollout.py and tests/test_gpu_pd_meas.py, unchanged -- states (and measured states)
1e-9 absolute, inputs 2e-9 absolute, gradients 1e-9 relative to the gradient's largest magnitude; the integral is held to the states' bound.
Every case keeps | |q| - i_max | >= 1e-7, two orders above that bound, so the launch clamps the entries the truth clamps."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
import noise_truth
import pd_models
import pid_models as pm
from closed_loop_family import Family, controller
from closed_loop_family import meas_spec as spec
from gpu_helpers import DT, G, dev, relmax
from pd_meas_models import meas_model, pos_noise_for
from pd_models import inputs_for
from rank_harness import rank_group, run_ranks

pytestmark = pytest.mark.gpu
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9
TOLS = (STATE_TOL, INPUT_TOL, GRAD_TOL)
INF = pm.INF

PID = Family("rollout_pd", lambda pol: [pol.sqrt_Kp_gains, pol.sqrt_Kd_gains, pol.sqrt_Ki_gains],
             lambda e: "g_sqrt_kp %.3e g_sqrt_kd %.3e g_sqrt_ki %.3e" % tuple(e), pd_models, lambda N, deg: N + deg)


def pair(shape, N, deg):
    """PID.pair with the sampling time a measurement model needs on the delta-state layout too (the true form never reads it)."""
    return PID.pair(shape, N, deg, None, measured=True)


def pid_controller(c, kp, kd, ki, target, i_max=INF, u_max=1.0, squash=True, trainable=True, dt=pm.DT_STEP):
    from mc_pilco_amd.policy_learning import Policy

    return Policy.PID_controller(state_dim=c["S"], input_dim=c["U"], sqrt_Kp_gains=kp.numpy(), sqrt_Kd_gains=kd.numpy(), sqrt_Ki_gains=ki.numpy(),
                                 T_sampling=dt, i_max=None if i_max == INF else i_max, target_traj=G(target), flg_squash=squash, u_max=u_max,
                                 flg_trainable=trainable, dtype=DT, device=dev())


def truth_of(t):
    return clf.Truth(t.states, t.inputs, t.meas, list(t.grads), t.g_x0, t.vmin)


def integ_error(pol, truth):
    return float((pol.packed().integ.cpu() - truth.integ).abs().max())


# ---- 1. parity with the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pm.CASES, ids=pm.case_id)
def test_parity_with_the_truth(case):
    mode, shape, deg, N, T, M, variant, opt = case
    sample = mode == "sampled"
    c, m, pmod = pair(shape, N, deg)
    torch.set_num_threads(1)
    truth, (x0, kp, kd, ki, target, eps, w, wu, ms, pn, kw) = pm.case_truth(case, m)
    share, margin = pm.clamp_figures(truth, kw["i_max"])
    print("%s: clamped share %.2f margin %.3e" % (pm.case_id(case), share, margin))
    assert margin >= pm.MARGIN and ("i_max" not in opt or pm.SHARE[0] <= share <= pm.SHARE[1])
    if sample and T > 1:
        assert truth.vmin > 0.0  # the oracle alone keeps every step's variance positive on this seed
    pol = pid_controller(c, kp, kd, ki, target, **kw)
    got = PID.run(pmod, pol, x0, T, clf.noise_buffer(eps) if sample else None, w, wu, sample, meas=spec(ms, pn))
    ei = integ_error(pol, truth)
    print("integ %.3e" % ei)
    clf.check_against(PID, pm.case_id(case), truth_of(truth), got, TOLS)
    assert ei < STATE_TOL


# ---- 2. the term switched off, and with a zero gain ------------------------------------------------------------------------------------------
def raw_run(pmod, pk, gains, term, ms, nz, x0, T, w, wu, sample=True):
    """One recording launch and one sweep through mcp_rollout_pid / mcp_rollout_pid_bwd: (states, inputs, meas, integ, g_gains, g_x0).
    ``term``: None (pid NULL), "off" (on == 0) or "on"; ``ms``: a MeasSpec or None (meas NULL)."""
    from mc_pilco_amd import hipabi as abi

    M, S, U = x0.shape[0], pmod.S, pmod.U
    x = G(x0)
    st, inp = torch.empty(T, M, S, dtype=DT, device=dev()), torch.empty(T, M, U, dtype=DT, device=dev())
    jac = torch.empty(max(T - 1, 1), M, pmod.G, pmod.D, dtype=DT, device=dev())
    ym, integ = torch.zeros(T, M, S, dtype=DT, device=dev()), torch.zeros(T, M, U, dtype=DT, device=dev())
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    ng = 3 if term == "on" else 2
    gg, gx = torch.empty(M, ng, U, dtype=DT, device=dev()), torch.empty(M, S, dtype=DT, device=dev())
    pc, nc = pk.to_c(*gains), nz.to_c()
    tc = None
    if term is not None:
        tc = pk.term_c(integ)
        tc.on = int(term == "on")
    mc = None
    if ms is not None:
        mc = abi.Meas()
        ms.fill(mc, T, M, ym)
    ref = lambda s: None if s is None else C.byref(s)
    gs, gi = G(w), G(wu)  # (named: the buffers must outlive the launches that read them)
    lib = abi.lib()
    abi.check(lib.mcp_rollout_pid(C.byref(pmod.c), C.byref(pc), ref(tc), ref(mc), C.byref(nc), M, T, int(sample), abi.ptr(x), abi.ptr(st), abi.ptr(inp),
                                  abi.ptr(jac), None, None, abi.ptr(status), abi.stream()), "mcp_rollout_pid")
    abi.check(lib.mcp_rollout_pid_bwd(C.byref(pmod.c), C.byref(pc), ref(tc), ref(mc), M, T, abi.ptr(st), abi.ptr(inp), abi.ptr(jac), abi.ptr(gs),
                                      abi.ptr(gi), abi.ptr(gg), abi.ptr(gx), abi.stream()), "mcp_rollout_pid_bwd")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return st, inp, ym, integ, gg, gx


def _pd_run(pmod, c, kp, kd, target, x0, T, w, wu, ms, pn):
    """ops.rollout_pd under the PD controller with the same gains, Philox at seed 4 / call 2."""
    from mc_pilco_amd import ops

    return clf.PD.run(pmod, controller(c, kp, kd, target), x0, T, ops.NoiseSpec(seed=4, call=2), w, wu, True, meas=spec(ms, pn))


@pytest.mark.parametrize("measured", [False, True])
def test_term_off_is_the_pd_launch(measured):
    """pid NULL and on == 0 through the new entries: the kernels of mcp_rollout_pd(_meas) and their sweeps -- states, inputs, measurements,
    g_gains [M,2,U] and g_x0 carry the bits of ops.rollout_pd; nothing is written to integ."""
    from mc_pilco_amd import ops

    c, m, pmod = pair("arm2", 37, 2)
    M, T = 17, 6
    x0, kp, kd, target, _, w, wu = inputs_for(c, M, T, seed=9)
    ms = meas_model("arm2") if measured else None
    pd = _pd_run(pmod, c, kp, kd, target, x0, T, w, wu, ms, None)
    pk = pid_controller(c, kp, kd, pm.ki_for(c, 9), target, i_max=0.05).packed()
    for term in (None, "off"):
        st, inp, ym, integ, gg, gx = raw_run(pmod, pk, (G(kp), G(kd), G(pm.ki_for(c, 9))), term, spec(ms), ops.NoiseSpec(seed=4, call=2), x0, T, w, wu)
        assert torch.equal(st, pd.states) and torch.equal(inp, pd.inputs) and float(integ.abs().max()) == 0.0
        assert (not measured) or torch.equal(ym, pd.meas)
        assert torch.equal(gg.sum(0)[0], pd.grads[0]) and torch.equal(gg.sum(0)[1], pd.grads[1]) and torch.equal(gx, pd.g_x0)


@pytest.mark.parametrize("measured", [False, True])
def test_zero_integral_gain_is_the_pd_launch_bit_for_bit(measured):
    """sqrt_ki = 0 with the term on and a live clamp: states and inputs carry the bits of ops.rollout_pd, and so do the kp / kd / x0
    gradients; the integral is formed all the same (both sides of the clamp), its gain's gradient is zero."""
    from mc_pilco_amd import ops

    c, m, pmod = pair("arm2", 37, 2)
    M, T = 17, 6
    x0, kp, kd, target, _, w, wu = inputs_for(c, M, T, seed=9)
    ms = meas_model("arm2") if measured else None
    pd = _pd_run(pmod, c, kp, kd, target, x0, T, w, wu, ms, None)
    pol = pid_controller(c, kp, kd, torch.zeros(2, dtype=DT), target, i_max=0.02)
    got = PID.run(pmod, pol, x0, T, ops.NoiseSpec(seed=4, call=2), w, wu, True, meas=spec(ms))
    assert got.status == 0 and torch.equal(got.states, pd.states) and torch.equal(got.inputs, pd.inputs)
    assert torch.equal(got.grads[0], pd.grads[0]) and torch.equal(got.grads[1], pd.grads[1]) and torch.equal(got.g_x0, pd.g_x0)
    assert float(got.grads[2].abs().max()) == 0.0
    on_bound = (pol.packed().integ.abs() == 0.02).to(DT).mean()
    assert 0.1 < float(on_bound) < 0.9


# ---- 3. the family's checks, on the true and on the measured form ------------------------------------------------------------------------------
def _family_case(measured, M, T, seed, N=37, deg=1, i_max=0.02):
    c, m, pmod = pair("arm2", N, deg)
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=seed)
    ms = meas_model("arm2") if measured else None
    pn = pos_noise_for(T, M, 2, seed=seed) if measured else None
    return c, m, pmod, x0, (kp, kd, pm.ki_for(c, seed), target), eps, w, wu, ms, pn, i_max


@pytest.mark.parametrize("measured", [False, True])
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_plain_launch_recording_launch_and_open_loop_launch_carry_the_same_bits(noise, measured):
    c, m, pmod, x0, gains, eps, w, wu, ms, pn, i_max = _family_case(measured, 17, 6, 21)
    pol = pid_controller(c, *gains, i_max=i_max)
    meas = (lambda: spec(ms, None if noise == "philox" else pn)) if measured else None
    seen = []

    class Watched(Family):  # (the integral of each launch, as the packed policy holds it right after)
        def op(self, *a, **kw):
            out = Family.op(self, *a, **kw)
            seen.append(a[1].integ.clone())
            return out

    clf.three_way_bit_identity(Watched(PID.op_name, PID.params, PID.grad_text, PID.models, PID.pair_seed), pmod, pol, x0, eps, 6, noise, meas=meas,
                               sweep=(w, wu))
    assert len(seen) == 2 and torch.equal(seen[0], seen[1])  # plain against recording launch
    assert 0.1 < float((seen[0].abs() == i_max).to(DT).mean()) < 0.9


def _rung(N, deg, measured):
    c, m, pmod, x0, gains, eps, w, wu, ms, pn, i_max = _family_case(measured, 5, 3, 305, N, deg)
    torch.set_num_threads(1)
    truth = pm.pid_truth("arm2", m, x0, *gains[:3], gains[3], eps, w, wu, True, i_max=i_max, ms=ms, pos_noise=pn)
    share, margin = pm.clamp_figures(truth, i_max)
    print("rung N %d: clamped share %.2f margin %.3e" % (N, share, margin))
    assert truth.vmin > 0.0 and margin >= pm.MARGIN
    return c, pmod, gains, x0, eps, 3, w, wu, truth, ((lambda: spec(ms, pn)) if measured else None), i_max


@pytest.mark.parametrize("measured", [False, True])
def test_the_four_trajectory_rung_of_the_recording_form(measured):
    """Sampled, degree 0, N = 640, M = 5, T = 3 on arm2: the recording launch runs 4 trajectories per workgroup.  Status 0; states, inputs
    (and measurements) carry the bits of the launch without a record, whose states carry the bits of the open-loop launch on its inputs;
    everything against the truth."""
    c, pmod, gains, x0, eps, T, w, wu, truth, meas, i_max = _rung(640, 0, measured)
    pol = pid_controller(c, *gains, i_max=i_max)
    clf.rung_of_the_recording_form(PID, "rung N 640", pmod, pol, x0, eps, T, w, wu, truth_of(truth), TOLS, meas)
    assert integ_error(pol, truth) < STATE_TOL


@pytest.mark.parametrize("measured", [False, True])
def test_the_four_trajectory_tile_without_a_record(measured):
    """Sampled, N = 1200 (the k panel of 16 trajectories does not fit), nothing requires grad: status 0, the states carry the bits of the
    open-loop launch on the inputs; states, inputs (and measurements) and the integral against the truth."""
    c, pmod, gains, x0, eps, T, w, wu, truth, meas, i_max = _rung(1200, 0 if measured else 2, measured)
    pol = pid_controller(c, *gains, i_max=i_max, trainable=False)
    clf.four_trajectory_tile_without_a_record(PID, "rung N 1200", pmod, pol, x0, eps, T, truth_of(truth), TOLS, meas)
    assert integ_error(pol, truth) < STATE_TOL


@pytest.mark.parametrize("measured", [False, True])
def test_saved_record_refuses_in_place_changes(measured):
    """States, inputs (and the measurements) as for the PD law; and the saved integral, changed in place, makes backward raise too."""
    c, m, pmod, x0, gains, eps, w, wu, ms, pn, i_max = _family_case(measured, 2, 4, 3)
    pol = pid_controller(c, *gains, i_max=i_max)
    meas = (lambda: spec(ms, pn)) if measured else None
    clf.saved_record_refuses_in_place_changes(PID, pmod, pol, x0, 4, meas=meas)
    out = PID.op(pmod, pol.packed(), None, G(x0), 4, particle_pred=False, meas=meas() if meas else None)
    with torch.no_grad():
        pol.packed().integ.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (out[0].sum() + out[1].sum()).backward()


@pytest.mark.parametrize("measured", [False, True])
def test_status_word(measured):
    """clf.status_word on the true form; on the measured form the same three words through ``meas=``.  A NaN integral gain and a NaN target
    row reach the inputs and raise STATUS_NAN."""
    from mc_pilco_amd import hipabi, ops

    c, m, pmod, x0, gains, eps, w, wu, ms, pn, i_max = _family_case(measured, 5, 4, 31, deg=0)
    kp, kd, ki, target = gains
    T = 4
    good = pid_controller(c, kp, kd, ki, target, i_max=i_max, trainable=False).packed()
    bad = x0.clone()
    bad[3, 1] = float("nan")
    zero = pid_controller(c, kp, kd, ki, torch.zeros(4, 4, dtype=DT), i_max=i_max, trainable=False).packed()  # target 0, x = 0: e = 0, I = 0, u = 0 exactly

    class Form(Family):
        def op(self, *a, **kw):
            if measured and a[0] is pmod:
                kw = dict(kw, meas=spec(ms, pn))  # (its launches on this model are the mean and the eps-buffer ones: the position noise is a buffer too)
            return Family.op(self, *a, **kw)

    fam = Form(PID.op_name, PID.params, PID.grad_text, PID.models, PID.pair_seed)
    clf.status_word(fam, pmod, c, good, (good, bad), zero, x0, eps, T)
    nan_ki = ki.clone()
    nan_ki[1] = float("nan")
    nan_target = target.clone()
    nan_target[2, 0] = float("nan")
    for pol in (pid_controller(c, kp, kd, nan_ki, target, i_max=i_max, trainable=False), pid_controller(c, kp, kd, ki, nan_target, i_max=i_max, trainable=False)):
        st, inp, status = fam.op(pmod, pol.packed(), None, G(x0), T, particle_pred=False)
        assert int(status.item()) & hipabi.STATUS_NAN and bool(torch.isnan(inp).any())


# ---- 4. run to run, and a split of the swarm ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measured", [False, True])
def test_run_to_run_and_shard_invariance(measured):
    """Two runs give the same bits; rows [a, b) launched with particle_offset = a (a 16 + 1 split, Philox) give the bits of one launch over
    all rows: states, inputs, measurements, integ and the per-trajectory g_gains [M,3,U] and g_x0 rows."""
    from mc_pilco_amd import ops

    c, m, pmod, x0, gains, eps, w, wu, ms, pn, i_max = _family_case(measured, 17, 6, 9, deg=0)
    pk = pid_controller(c, *gains, i_max=i_max).packed()
    gg3 = tuple(G(g) for g in gains[:3])

    def run(a, b):
        return raw_run(pmod, pk, gg3, "on", spec(ms), ops.NoiseSpec(seed=4, call=2, particle_offset=a), x0[a:b], 6, w[:, a:b], wu[:, a:b])

    whole, again = run(0, 17), run(0, 17)
    assert all(torch.equal(p, q) for p, q in zip(whole, again))
    assert float(whole[4][:, 2].abs().max()) > 0 and 0.1 < float((whole[3].abs() == i_max).to(DT).mean()) < 0.9
    for a, b in ((0, 16), (16, 17)):
        part = run(a, b)
        for i in (0, 1, 2, 3):
            assert torch.equal(part[i], whole[i][:, a:b])
        assert torch.equal(part[4], whole[4][a:b]) and torch.equal(part[5], whole[5][a:b])


# ---- 5. Philox mode: central differences of the op ---------------------------------------------------------------------------------------------
def test_philox_mode_against_central_differences():
    """Step 1e-6, bound 1e-5 relative with floor 1e-3, as tests/test_gpu_pd_rollout.py has it, on the case whose truth (the Philox draws
    restated by tests/noise_truth.py) keeps | |q| - i_max | >= 1e-3 -- asserted by tests/test_pid_cpu.py and again here, with the launch's
    own integral against that truth: no clamp changes side within the step."""
    F = pm.FD_CASE
    c, m, pmod = pair(F["shape"], F["N"], F["deg"])
    x0, kp, kd, ki, target, w, wu = pm.fd_inputs()
    eps = torch.as_tensor(noise_truth.eps_table(F["philox"][0], F["philox"][1], F["T"], F["M"], c["G"]), dtype=DT)
    torch.set_num_threads(1)
    truth = pm.pid_truth(F["shape"], m, x0, kp, kd, ki, target, eps, w, wu, True, i_max=F["i_max"])
    share, margin = pm.clamp_figures(truth, F["i_max"])
    assert margin >= pm.FD_MARGIN and pm.SHARE[0] <= share <= pm.SHARE[1]
    policy_of = lambda gains, trainable: pid_controller(c, gains[0], gains[1], gains[2], target, i_max=F["i_max"], trainable=trainable)
    pol = policy_of([kp, kd, ki], False)
    with torch.no_grad():
        from mc_pilco_amd import ops

        PID.op(pmod, pol.packed(), ops.NoiseSpec(seed=F["philox"][0], call=F["philox"][1]), G(x0), F["T"], particle_pred=True)
    assert integ_error(pol, truth) < STATE_TOL
    checks = [("sqrt_kp[1]", 0, 1), ("sqrt_kd[0]", 1, 0), ("sqrt_ki[0]", 2, 0), ("sqrt_ki[1]", 2, 1), ("x0[2,1]", 3, 2 * c["S"] + 1)]
    clf.central_differences(PID, pmod, policy_of, [kp, kd, ki], x0, w, wu, F["T"], checks, step=1e-6, bound=(1e-5, 1e-3))


# ---- 6. class path ---------------------------------------------------------------------------------------------------------------------------
ARM_TARGET = lambda T: 0.3 * np.sin(0.3 * np.arange(T + 2).reshape(-1, 1) + np.array([0.0, 1.0, 2.0, 3.0]).reshape(1, -1))


def _arm_par(target, i_max=0.02):
    return dict(clf.arm_pd_par([1.0, 1.2], [0.5, 0.4], target), sqrt_Ki_gains=np.asarray([0.8, 0.6]), T_sampling=0.05, i_max=i_max)


def _arm_object(target, pms=None):
    from mc_pilco_amd.policy_learning import Policy

    return clf.arm_object(Policy.PID_controller, _arm_par(target), pms)


@pytest.mark.parametrize("cls_name", ["MC_PILCO", "MC_PILCO4PMS"])
def test_class_path(cls_name):
    """The fused launch against the same object's step loop (fused_feedback = False) in "reference" noise mode: states, inputs and the
    three gradients at the bounds of the same comparison in tests/test_gpu_pd_rollout.py / test_gpu_pd_meas.py; a short reinforce_policy
    run moves all three gains and lowers the cost."""
    M, T = 16, 8
    target = ARM_TARGET(T)
    sim = clf.sim_args(M, T)
    pms = clf.ARM_PMS if cls_name == "MC_PILCO4PMS" else None

    def rollout(fused):
        obj = _arm_object(target, pms)
        obj.fused_feedback = fused
        torch.manual_seed(5)
        with clf.normal_draws_on_the_cpu():
            st, inp = obj.apply_policy(**sim)
        assert obj.last_feedback_fused is fused and (obj.last_status is not None) is (fused or obj.last_step_fused)
        if fused:
            assert int(obj.last_status.item()) == 0
            integ = obj.control_policy.packed().integ
            assert 0.1 < float((integ.abs() == 0.02).to(DT).mean()) < 0.9  # both sides of the clamp
        cost, _ = obj.cost_function(st, inp, 0)
        cost.backward()
        pol = obj.control_policy
        return st.detach(), inp.detach(), [q.grad.clone() for q in PID.params(pol)]

    fs, fi, fg = rollout(True)
    ss, si, sg = rollout(False)
    es, ei, eg = float((fs - ss).abs().max()), float((fi - si).abs().max()), [relmax(a, b) for a, b in zip(fg, sg)]
    print("%s, fused vs step: states %.3e inputs %.3e %s" % (cls_name, es, ei, PID.grad_text(eg)))
    assert es < STATE_TOL and ei < INPUT_TOL and max(eg) < GRAD_TOL

    obj = _arm_object(target, pms)
    torch.manual_seed(6)
    buf = io.StringIO()
    with clf.normal_draws_on_the_cpu(), contextlib.redirect_stdout(buf):
        out = obj.reinforce_policy(**clf.reinforce_args(sim, T, 5))
    assert obj.last_feedback_fused is True
    cost = np.asarray(out[0], dtype=float).reshape(-1)
    pol = obj.control_policy
    moved = [float(np.abs(q.detach().cpu().numpy() - np.asarray(v)).max()) for q, v in zip(PID.params(pol), ([1.0, 1.2], [0.5, 0.4], [0.8, 0.6]))]
    print("cost sequence:", cost, "gains moved by", moved)
    assert cost.shape == (5,) and min(moved) > 1e-3 and cost[-1] < cost[0]


# ---- 7. class path, two ranks on one device ---------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401

    torch.cuda.set_device(dev())
    with rank_group(rank, world, port):
        res = {}
        for cls_name in ("MC_PILCO", "MC_PILCO4PMS"):
            obj = _arm_object(ARM_TARGET(6), clf.ARM_PMS if cls_name == "MC_PILCO4PMS" else None)
            obj.noise_mode = "philox"
            res[cls_name] = clf.sharded_step(PID, obj, world, clf.sim_args(17, 6))
        out_q.put((rank, res))


def test_two_rank_particle_sharding_matches_single_process():
    """MC_PILCO and MC_PILCO4PMS with the PID policy under shard_particles (M = 17, Philox): each rank's states are the matching slice of
    the one-process run bit for bit; the pooled cost, its std and the three gains' gradients agree to the bounds (another order of the sums)."""
    one = run_ranks(_rank, 1)
    two = run_ranks(_rank, 2)
    clf.two_ranks_match_one_process(PID, one, two, GRAD_TOL, n_grads=3)
