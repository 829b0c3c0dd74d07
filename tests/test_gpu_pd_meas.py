"""GPU: the fused closed loop under the PD controller on a simulated measurement (mcp_rollout_pd_meas + mcp_rollout_pd_meas_bwd,
ops.rollout_pd(meas=...), MC_PILCO4PMS.apply_policy with a PD_controller, and the PD policy under particle sharding) against torch autograd
through the oracle's step with the measurement and the policy written out (tests/pd_meas_models.pd_meas_truth, pinned to the reference by
tests/test_pd_meas_cpu.py), and the bitwise contracts it shares with mcp_rollout_pd and the open-loop kernels.

Bounds: those of tests/test_gpu_pd_rollout.py, unchanged -- states 1e-9 absolute, inputs 2e-9 absolute, gradients 1e-9 relative to the
gradient's largest magnitude; the measured states are held to the states' bound.

The tiles: as in tests/test_gpu_pd_rollout.py, CASES stops at N = 300 (16 trajectories per workgroup).  The measured form's recording
kernels with 4 and 1 trajectories (N = 640, N = 2600) and its 4-trajectory kernel without a record (N = 1200) are launched by the two rung
tests below, at degree class 0; degree class 2 at those sizes is left out on purpose (see tests/test_gpu_pd_rollout.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_family as clf
import conftest
from closed_loop_family import PD, controller
from closed_loop_family import meas_spec as spec
from gpu_helpers import DT, G, dev, rbf_dict, relmax
from pd_meas_models import CASES, FILTER, case_id, meas_model, pd_meas_truth, pos_noise_for
from pd_models import inputs_for
from rank_harness import rank_group, run_ranks

pytestmark = pytest.mark.gpu
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9
TOLS = (STATE_TOL, INPUT_TOL, GRAD_TOL)


def pair(shape, N, deg, vs=None):
    """PD.pair with the sampling time a measurement model needs on the delta-state layout too."""
    return PD.pair(shape, N, deg, vs, measured=True)


def gpu_run(pm, pol, x0, eps, pn, w, wu, sample, T, ms, noise=None):
    """The Run of the op with L = sum w states + sum wu inputs."""
    nz = noise if noise is not None else (clf.noise_buffer(eps) if sample else None)
    return PD.run(pm, pol, x0, T, nz, w, wu, sample, meas=spec(ms, pn))


# ---- 1. parity with the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_truth(case):
    mode, shape, deg, N, T, M, variant, opt = case
    sample = mode == "sampled"
    vs = opt.get("var_scale")
    c, m, pm = pair(shape, N, deg, None if vs is None else tuple(vs))
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=T * 100 + M)
    if opt.get("no_g_inputs"):
        wu = None
    ms = meas_model(shape, variant, std=opt.get("std", 0.1))
    pn = pos_noise_for(T, M, len(ms["pos"]), seed=T * 100 + M)
    u_max, squash = opt.get("u_max", 1.0), opt.get("squash", True)
    torch.set_num_threads(1)
    truth = clf.pd_truth_of(pd_meas_truth(shape, m, x0, kp, kd, target, eps, pn, w, wu, sample, ms, u_max=u_max, squash=squash, var_scale=vs))
    if sample and T > 1:
        assert truth.vmin > 0.0  # the oracle alone keeps every step's variance positive on this seed
    pol = controller(c, kp, kd, target, u_max=u_max, squash=squash)
    clf.check_against(PD, case_id(case), truth, gpu_run(pm, pol, x0, eps, pn, w, wu, sample, T, ms), TOLS)


# ---- 2. bit identities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_plain_launch_recording_launch_and_open_loop_launch_carry_the_same_bits(noise):
    c, m, pm = pair("arm2", 37, 1)
    M, T = 17, 6
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=21)
    ms = meas_model("arm2")
    pn = pos_noise_for(T, M, 2, seed=21)
    clf.three_way_bit_identity(PD, pm, controller(c, kp, kd, target), x0, eps, T, noise, meas=lambda: spec(ms, None if noise == "philox" else pn))


# The rungs are held to the bounds of the N = 300 case of CASES (STATE_TOL for states and measurements, INPUT_TOL, GRAD_TOL): the library of
# the commit before the host path was unified measured below them on an MI355X at every rung (states / inputs / meas / g_sqrt_kp /
# g_sqrt_kd / g_x0; a case measuring above would have been given four times its measurement, as in tests/test_gpu_pd_rollout.py):
#   N 640   5.4e-13 / 5.3e-14 / 9.1e-14 / 2.1e-13 / 5.8e-13 / 4.9e-13      N 2600  1.1e-11 / 2.0e-12 / 2.2e-12 / 1.7e-12 / 8.5e-12 / 3.1e-12
#   N 1200, no record  3.2e-12 / 6.8e-13 / 9.5e-13
def _rung_case(N):
    c, m, pm = pair("arm2", N, 0)
    M, T = 5, 3
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=T * 100 + M)
    ms = meas_model("arm2")
    pn = pos_noise_for(T, M, 2, seed=T * 100 + M)
    torch.set_num_threads(1)
    truth = clf.pd_truth_of(pd_meas_truth("arm2", m, x0, kp, kd, target, eps, pn, w, wu, True, ms))
    assert truth.vmin > 0.0
    return c, pm, (kp, kd, target), x0, eps, T, w, wu, truth, lambda: spec(ms, pn)


@pytest.mark.parametrize("N", [640, 2600])
def test_the_smaller_tiles_of_the_recording_form(N):
    """Sampled, degree 0, M = 5, T = 3 on arm2, every joint measured: the recording launch runs 4 trajectories per workgroup at N = 640 and
    one at N = 2600.  Status 0; states, inputs and measurements carry the bits of the launch without a record, whose states carry the bits of
    the open-loop launch on its inputs; states, inputs, measurements and the three gradients against the truth."""
    c, pm, gains, x0, eps, T, w, wu, truth, meas = _rung_case(N)
    clf.rung_of_the_recording_form(PD, "rung N %d" % N, pm, controller(c, *gains), x0, eps, T, w, wu, truth, TOLS, meas)


def test_the_four_trajectory_tile_without_a_record():
    """Sampled, degree 0, N = 1200 (the k panel of 16 trajectories does not fit), nothing requires grad: status 0, the states carry the bits
    of the open-loop launch on the inputs, states, inputs and measurements against the truth.  (No record, so no gradient to compare.)"""
    c, pm, gains, x0, eps, T, w, wu, truth, meas = _rung_case(1200)
    clf.four_trajectory_tile_without_a_record(PD, "rung N 1200 deg 0", pm, controller(c, *gains, trainable=False), x0, eps, T, truth, TOLS, meas)


def raw_run(pm, pd, kpg, kdg, ms, nz, x0, T, w, wu, sample=True, entry="meas"):
    """One forward (recording) and one sweep through the C entry points: (states, inputs, meas, g_gains [M,2,U], g_x0)."""
    from mc_pilco_amd import hipabi as abi

    M = x0.shape[0]
    S, U = pm.S, pm.U
    x = G(x0)
    st, inp = torch.empty(T, M, S, dtype=DT, device=dev()), torch.empty(T, M, U, dtype=DT, device=dev())
    jac = torch.empty(max(T - 1, 1), M, pm.G, pm.D, dtype=DT, device=dev())
    ym = torch.zeros(T, M, S, dtype=DT, device=dev())
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    gg, gx = torch.empty(M, 2, U, dtype=DT, device=dev()), torch.empty(M, S, dtype=DT, device=dev())
    pc, nc = pd.to_c(kpg, kdg), nz.to_c()
    gs, gi = G(w), G(wu)  # (named: the buffers must outlive the launches that read them)
    lib = abi.lib()
    if entry == "plain":
        abi.check(lib.mcp_rollout_pd(C.byref(pm.c), C.byref(pc), C.byref(nc), M, T, int(sample), abi.ptr(x), abi.ptr(st), abi.ptr(inp), abi.ptr(jac),
                                     None, None, abi.ptr(status), abi.stream()), "mcp_rollout_pd")
        abi.check(lib.mcp_rollout_pd_bwd(C.byref(pm.c), C.byref(pc), M, T, abi.ptr(st), abi.ptr(inp), abi.ptr(jac), abi.ptr(gs), abi.ptr(gi),
                                         abi.ptr(gg), abi.ptr(gx), abi.stream()), "mcp_rollout_pd_bwd")
    else:
        mc = abi.Meas()
        if ms is not None:
            ms.fill(mc, T, M, ym)
        abi.check(lib.mcp_rollout_pd_meas(C.byref(pm.c), C.byref(pc), C.byref(mc), C.byref(nc), M, T, int(sample), abi.ptr(x), abi.ptr(st),
                                          abi.ptr(inp), abi.ptr(jac), None, None, abi.ptr(status), abi.stream()), "mcp_rollout_pd_meas")
        abi.check(lib.mcp_rollout_pd_meas_bwd(C.byref(pm.c), C.byref(pc), C.byref(mc), M, T, abi.ptr(st), abi.ptr(inp), abi.ptr(jac), abi.ptr(gs),
                                              abi.ptr(gi), abi.ptr(gg), abi.ptr(gx), abi.stream()), "mcp_rollout_pd_meas_bwd")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return st, inp, ym, gg, gx


def test_no_pairs_is_the_plain_feedback_launch():
    """meas.n == 0 through the new entry points: the kernels of mcp_rollout_pd / mcp_rollout_pd_bwd, the same bits."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 2)
    M, T = 17, 6
    x0, kp, kd, target, _, w, wu = inputs_for(c, M, T, seed=9)
    pd = controller(c, kp, kd, target).packed()
    nz = ops.NoiseSpec(seed=4, call=2)
    a = raw_run(pm, pd, G(kp), G(kd), None, nz, x0, T, w, wu, entry="plain")
    b = raw_run(pm, pd, G(kp), G(kd), None, nz, x0, T, w, wu, entry="meas")
    for i in (0, 1, 3, 4):
        assert torch.equal(a[i], b[i])
    assert float(b[2].abs().max()) == 0.0  # (no measurement buffer was named: nothing was written)


@pytest.mark.parametrize("noise", ["buffers", "philox"])
def test_shard_invariance(noise):
    """Rows [a, b) launched with particle_offset = a (buffers: the matching slices): states, inputs, meas and the per-trajectory g_gains and g_x0
    rows are bitwise those of one launch over all rows."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    M, T, cut = 17, 6, 9
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=9)
    ms = meas_model("arm2")
    pn = pos_noise_for(T, M, 2, seed=9)
    pd = controller(c, kp, kd, target).packed()
    kpg, kdg = G(kp), G(kd)

    def run(a, b):
        if noise == "buffers":
            nz, sp = ops.NoiseSpec(eps=G(eps[:, a:b])), spec(ms, pn[:, a:b])
        else:
            nz, sp = ops.NoiseSpec(seed=4, call=2, particle_offset=a), spec(ms)
        return raw_run(pm, pd, kpg, kdg, sp, nz, x0[a:b], T, w[:, a:b], wu[:, a:b])

    whole = run(0, M)
    assert float(whole[3].abs().max()) > 0
    for a, b in ((0, cut), (cut, M)):
        st, inp, ym, gg, gx = run(a, b)
        assert torch.equal(st, whole[0][:, a:b]) and torch.equal(inp, whole[1][:, a:b]) and torch.equal(ym, whole[2][:, a:b])
        assert torch.equal(gg, whole[3][a:b]) and torch.equal(gx, whole[4][a:b])


# ---- 3. Philox ----------------------------------------------------------------------------------------------------------------------------
def test_philox_position_noise_is_the_closed_loop_kernels():
    """The position noise recovered as (meas[t][p] - states[t][p]) / std (std = 0.1, |x| < 1: good to ~1e-15) equals the noise recovered the
    same way from ops.rollout under an RBF policy at the same seed / call / offset; fed back as a buffer with the recovered eps it
    reproduces the Philox run to the case bounds."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    M, T, off = 5, 6, 3
    x0, kp, kd, target, _, w, wu = inputs_for(c, M, T, seed=13)
    ms = meas_model("arm2")
    ms["std"] = [0.1, 0.1]
    pol = controller(c, kp, kd, target)
    nz = lambda: ops.NoiseSpec(seed=21, call=7, particle_offset=off)
    st, inp, ym, (gkp, gkd), gx, status = gpu_run(pm, pol, x0, None, None, w, wu, True, T, ms, noise=nz())
    assert status == 0 and float(st[:, :, :2].abs().max()) < 1.0  # (the measured components: the positions)
    rec = (ym[1:, :, :2] - st[1:, :, :2]) / 0.1
    B = 8
    rbf = ops.PackedPolicy("plain", 4, G(np.zeros((1, 4))), G(0.1 * np.arange(B * 4).reshape(B, 4) / (B * 4)), G(0.05 * np.ones((2, B))), 1.0, True)
    sr, _, _, status_r, yr = ops.rollout_forward_raw(pm, rbf, nz(), G(x0), T, 0.0, True, need_jac=False, meas=spec(ms))
    assert int(status_r.item()) == 0 and float(sr[:, :, :2].abs().max()) < 1.0
    rec_r = (yr[1:, :, :2] - sr[1:, :, :2]) / 0.1
    print("recovered position noise, PD vs RBF: %.3e" % float((rec - rec_r).abs().max()))
    assert float(rec.abs().max()) > 0.5 and float((rec - rec_r).abs().max()) < 1e-12
    # eps recovered through the open-loop launch's moments on the same inputs: x' [vel] = x[vel] + mu + sqrt(var) eps
    _, mu, var, _ = ops.rollout_open(pm, G(x0), inp[:T - 1].contiguous(), noise=nz(), particle_pred=True, moments=True)
    vel = c["vel"]
    eps = (st[1:, :, vel] - st[:-1, :, vel] - mu) / torch.sqrt(var)
    pol2 = controller(c, kp, kd, target)
    st2, inp2, ym2, (gkp2, gkd2), gx2, status2 = gpu_run(pm, pol2, x0, eps.cpu(), rec.cpu(), w, wu, True, T, ms)
    es, ei, em = float((st2 - st).abs().max()), float((inp2 - inp).abs().max()), float((ym2 - ym).abs().max())
    ep, ed, ex = relmax(gkp2, gkp), relmax(gkd2, gkd), relmax(gx2, gx)
    print("buffers of the recovered noise vs Philox: states %.3e inputs %.3e meas %.3e grads %.3e %.3e %.3e" % (es, ei, em, ep, ed, ex))
    assert status2 == 0 and es < STATE_TOL and ei < INPUT_TOL and em < STATE_TOL and max(ep, ed, ex) < GRAD_TOL


# ---- 4. arguments -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_status_word_alone():
    from mc_pilco_amd import hipabi as abi
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    M, T = 5, 4
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=31)
    pd = controller(c, kp, kd, target, trainable=False).packed()
    kpg, kdg = G(kp), G(kd)
    x, st, inp = G(x0), torch.zeros(T, M, 4, dtype=DT, device=dev()), torch.zeros(T, M, 2, dtype=DT, device=dev())
    ym = torch.zeros(T, M, 4, dtype=DT, device=dev())
    jac = torch.zeros(T - 1, M, pm.G, pm.D, dtype=DT, device=dev())
    status = torch.full((1,), 0x40, dtype=torch.int32, device=dev())
    gg = torch.zeros(M, 2, 2, dtype=DT, device=dev())
    pc, nc = pd.to_c(kpg, kdg), ops.NoiseSpec(seed=1, call=1).to_c()
    lib = abi.lib()

    def both(mc, model=pm.c):
        mp_ = None if mc is None else C.byref(mc)
        f = lib.mcp_rollout_pd_meas(C.byref(model), C.byref(pc), mp_, C.byref(nc), M, T, 1, abi.ptr(x), abi.ptr(st), abi.ptr(inp), None, None, None,
                                    abi.ptr(status), abi.stream())
        b = lib.mcp_rollout_pd_meas_bwd(C.byref(model), C.byref(pc), mp_, M, T, abi.ptr(st), abi.ptr(inp), abi.ptr(jac), abi.ptr(st), None,
                                        abi.ptr(gg), None, abi.stream())
        return f, b

    def meas(**edit):
        mc = abi.Meas()
        spec(meas_model("arm2")).fill(mc, T, M, ym)
        for k, v in edit.items():
            if isinstance(v, tuple):
                getattr(mc, k)[v[0]] = v[1]
            else:
                setattr(mc, k, v)
        return mc

    no_ts = abi.Model.from_buffer_copy(pm.c)
    no_ts.Ts = 0.0
    for name, got in (("meas NULL", both(None)), ("pos out of range", both(meas(pos=(0, 4)))), ("vel negative", both(meas(vel=(1, -1)))),
                      ("pos repeated", both(meas(pos=(1, 0)))), ("vel repeated", both(meas(vel=(1, 2)))), ("listed as both", both(meas(vel=(1, 0)))),
                      ("no meas buffer", both(meas(meas=None))), ("a0 == 0", both(meas(a0=0.0))), ("a0 NaN", both(meas(a0=float("nan")))),
                      ("Ts <= 0", both(meas(), no_ts))):
        assert got == (-1, -1), name
    # Ts <= 0 is refused by the measurement's own check: the same model passes every other check when no pair is measured
    assert lib.mcp_rollout_pd_meas_bwd(C.byref(no_ts), C.byref(pc), C.byref(abi.Meas()), M, T, abi.ptr(st), abi.ptr(inp), abi.ptr(jac), abi.ptr(st),
                                       None, None, None, abi.stream()) == 0  # (nothing asked for: no launch)
    torch.cuda.synchronize()
    assert int(status.item()) == 0x40 and float(st.abs().max()) == 0.0 and float(gg.abs().max()) == 0.0  # no launch
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rollout_pd(pm, pd, None, x0, T, particle_pred=False, meas=spec(meas_model("arm2")))
    with pytest.raises(RuntimeError, match="pos_noise"):
        bad = ops.MeasSpec(pos=[0, 1], vel=[2, 3], std_pos=[0.1, 0.1], b=FILTER["b"], a=FILTER["a"], pos_noise=torch.zeros(T - 1, M, 2, dtype=DT))
        ops.rollout_pd(pm, pd, ops.NoiseSpec(eps=G(eps)), x, T, meas=bad)
    mc = meas(meas=None)  # a missing meas buffer: refused by the library, raised by the host layer's check of the return code
    with pytest.raises(RuntimeError, match="MCP_ERR_ARG"):
        abi.check(lib.mcp_rollout_pd_meas(C.byref(pm.c), C.byref(pc), C.byref(mc), C.byref(nc), M, T, 1, abi.ptr(x), abi.ptr(st), abi.ptr(inp), None,
                                          None, None, abi.ptr(status), abi.stream()), "mcp_rollout_pd_meas")


# ---- 5. class path, one process -----------------------------------------------------------------------------------------------------------
def _fixture_object(fx, kind, cls_name="MC_PILCO4PMS", num_particles=None):
    """MC_PILCO4PMS (or MC_PILCO) over the model of a rollout_pd_pms.npz fixture -- trained here, on the fixture's recorded trajectory -- with the
    fixture's trainable PD controller and measurement model."""
    from mc_pilco_amd.model_learning import Model_learning as ML
    from mc_pilco_amd.policy_learning import Policy

    k = lambda n: fx[kind + "_" + n]
    Ts = float(k("Ts"))
    angle, not_angle = [int(i) for i in k("angle")], [int(i) for i in k("not_angle")]
    with clf.quiet():
        if kind == "speed":
            ml = ML.Speed_Model_learning_RBF_angle_state(num_gp=2, init_dict_list=[rbf_dict(8, k("lengthscales"), float(k("sigma_n")))] * 2, T_sampling=Ts,
                                                         angle_indeces=angle, not_angle_indeces=not_angle, vel_indeces=[int(i) for i in k("vel")],
                                                         not_vel_indeces=[int(i) for i in k("not_vel")], dtype=DT, device=dev())
        else:
            ml = ML.Model_learning_RBF_angle_state(num_gp=4, init_dict_list=[rbf_dict(8, k("lengthscales"), float(k("sigma_n")))] * 4,
                                                   angle_indeces=angle, not_angle_indeces=not_angle, dtype=DT, device=dev())
    ppar = dict(clf.arm_pd_par(k("sqrt_kp"), k("sqrt_kd"), k("target")), u_max=float(k("u_max")))
    pms = dict(pos_indeces=[int(i) for i in k("pos_indeces")], vel_indeces=[int(i) for i in k("vel_indeces")],
               std_meas_noise=np.asarray(k("std_meas_noise")), filtering_dict={"fc": float(k("fc"))})
    ml = clf.trained(ml, k("states_tr"), k("inputs_tr"))
    return clf.policy_learning_object(ml, Ts, Policy.PD_controller, ppar, pms if cls_name == "MC_PILCO4PMS" else None)


def _sim(fx, kind, M, T):
    return clf.sim_args(M, T, fx[kind + "_x0_mean"], fx[kind + "_x0_var"])


@pytest.mark.parametrize("kind", ["speed", "delta"])
def test_class_path_against_the_reference(golden, kind):
    """MC_PILCO4PMS with the trainable PD controller in "reference" noise mode: the fused launch is taken, and states / inputs / the weighted-sum
    cost / the gains' gradients are the reference's own (tests/golden/rollout_pd_pms.npz); the step loop (fused_feedback = False) gives the same
    numbers to the bounds."""
    fx = golden("rollout_pd_pms")
    k = lambda n: fx[kind + "_" + n]
    T, M = k("states").shape[:2]
    seed = 311 if kind == "speed" else 312  # (tests/golden/make_golden_pd_pms.py)

    def rollout(fused):
        obj = _fixture_object(fx, kind)
        obj.noise_mode = "reference"
        obj.fused_feedback = fused
        torch.manual_seed(seed)
        with clf.normal_draws_on_the_cpu():
            st, inp = obj.apply_policy(**_sim(fx, kind, M, T))
        assert obj.last_feedback_fused is fused and (obj.last_status is not None) is fused
        if fused:
            assert int(obj.last_status.item()) == 0
        cost = (G(k("w")) * st).sum() + (G(k("wu")) * inp).sum()
        cost.backward()
        pol = obj.control_policy
        return st.detach(), inp.detach(), float(cost), pol.sqrt_Kp_gains.grad.clone(), pol.sqrt_Kd_gains.grad.clone()

    ref_cost = float((k("w") * k("states")).sum() + (k("wu") * k("inputs")).sum())
    scale = float(np.abs(k("w") * k("states")).sum() + np.abs(k("wu") * k("inputs")).sum())
    for fused in (True, False):
        st, inp, cost, gkp, gkd = rollout(fused)
        es, ei = float((st.cpu() - torch.as_tensor(k("states"))).abs().max()), float((inp.cpu() - torch.as_tensor(k("inputs"))).abs().max())
        ep, ed = relmax(gkp, torch.as_tensor(k("g_sqrt_kp"))), relmax(gkd, torch.as_tensor(k("g_sqrt_kd")))
        print("%s fused=%s vs the reference: states %.3e inputs %.3e cost %.3e g_sqrt_kp %.3e g_sqrt_kd %.3e" % (kind, fused, es, ei, abs(cost - ref_cost), ep, ed))
        assert es < STATE_TOL and ei < INPUT_TOL and ep < GRAD_TOL and ed < GRAD_TOL
        assert abs(cost - ref_cost) < INPUT_TOL * scale  # (a sum of |w| x entries each within its bound)


# ---- 6. class path, two ranks on one device -------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401

    torch.cuda.set_device(dev())
    with rank_group(rank, world, port):
        fx = conftest.load_golden("rollout_pd_pms")
        out_q.put((rank, {cls_name: clf.sharded_step(PD, _fixture_object(fx, "speed", cls_name), world, _sim(fx, "speed", 17, 6))
                          for cls_name in ("MC_PILCO", "MC_PILCO4PMS")}))


def test_two_rank_particle_sharding_matches_single_process():
    """MC_PILCO and MC_PILCO4PMS with the PD policy under shard_particles (M = 17, Philox): each rank's states are the matching slice of the
    one-process run bit for bit; the pooled cost, its std and the gains' gradients agree to the bounds (another order of the sums)."""
    one = run_ranks(_rank, 1)
    two = run_ranks(_rank, 2)
    clf.two_ranks_match_one_process(PD, one, two, GRAD_TOL, n_grads=2)
