"""GPU: the fused closed loop under the PD controller (mcp_rollout_pd + mcp_rollout_pd_bwd, ops.rollout_pd, MC_PILCO.apply_policy with a
PD_controller) against torch autograd through the oracle's step with the policy formula written out (tests/pd_models.pd_truth, pinned to the
reference by tests/test_pd_rollout_cpu.py), and the bitwise contracts with the open-loop kernels it shares its phases with.

Bounds (on the oracle's own Kinv / alpha): states 1e-9 absolute, inputs 2e-9 absolute, gradients 1e-9 relative to the
gradient's largest magnitude.

The tiles (the ladder the feedback form shares with the open-loop form): CASES stops at N = 300, where every launch with a variance runs
16 trajectories per workgroup.  test_the_smaller_tiles_of_the_recording_form launches the recording form's 4- and 1-trajectory kernels
(N = 640, N = 2600) and test_the_four_trajectory_tile_without_a_record the plain launch's 4-trajectory kernel (N = 1200).  The recording
kernels of degree class 2 at those sizes are left out on purpose: four more long training-set builds for kernels that differ from the ones
launched here by the degree template argument of the same ladder code, which the open-loop module's rungs exercise at both classes."""
import contextlib
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
from closed_loop_family import PD, controller
from gpu_helpers import DT, G, dev, relmax
from pd_models import CASES, case_id, inputs_for, pd_truth

pytestmark = pytest.mark.gpu
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9
TOLS = (STATE_TOL, INPUT_TOL, GRAD_TOL)
pair = PD.pair


# ---- 1. parity with the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_truth(case):
    mode, shape, deg, N, T, M, opt = case
    sample = mode == "sampled"
    vs = opt.get("var_scale")
    c, m, pm = pair(shape, N, deg, None if vs is None else tuple(vs))
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=T * 100 + M)
    if opt.get("no_g_inputs"):
        wu = None
    u_max, squash = opt.get("u_max", 1.0), opt.get("squash", True)
    torch.set_num_threads(1)
    truth = clf.pd_truth_of(pd_truth(shape, m, x0, kp, kd, target, eps, w, wu, sample, u_max=u_max, squash=squash, var_scale=vs))
    if sample and T > 1:
        assert truth.vmin > 0.0  # the oracle alone keeps every step's variance positive on this seed
    pol = controller(c, kp, kd, target, u_max=u_max, squash=squash)
    got = PD.run(pm, pol, x0, T, clf.noise_buffer(eps) if sample else None, w, wu, sample)
    clf.check_against(PD, case_id(case), truth, got, TOLS)


# ---- 2. the feedback launch against the open-loop launch on its inputs -------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_states_carry_the_bits_of_the_open_loop_launch(noise):
    c, m, pm = pair("arm2", 37, 1)
    M, T = 17, 6
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=21)
    clf.three_way_bit_identity(PD, pm, controller(c, kp, kd, target), x0, eps, T, noise)


# ---- 2b. the ladder's smaller tiles ---------------------------------------------------------------------------------------------------------
# The rungs are held to the bounds of the N = 300 cases of CASES (STATE_TOL, INPUT_TOL, GRAD_TOL): the library of the commit before the host
# path was unified measured below them on an MI355X at every rung (states / inputs / g_sqrt_kp / g_sqrt_kd / g_x0; a case measuring above
# would have been given four times its measurement, the headroom the N = 1100 / 1500 bounds of tests/test_gpu_open_rollout.py carry):
#   N 640   6.2e-13 / 1.9e-13 / 5.6e-13 / 5.6e-13 / 2.9e-13      N 2600  7.4e-12 / 4.2e-12 / 8.5e-12 / 1.1e-11 / 2.8e-12
#   N 1200, degree 2, no record  3.2e-12 / 1.2e-12
def _rung(N, deg):
    """Sampled, M = 5, T = 3 on arm2: (cfg, PackedModel, the policy's arguments, x0, eps, T, w, wu, truth)."""
    c, m, pm = pair("arm2", N, deg)
    M, T = 5, 3
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=T * 100 + M)
    torch.set_num_threads(1)
    truth = clf.pd_truth_of(pd_truth("arm2", m, x0, kp, kd, target, eps, w, wu, True))
    assert truth.vmin > 0.0
    return c, pm, (kp, kd, target), x0, eps, T, w, wu, truth


@pytest.mark.parametrize("N", [640, 2600])
def test_the_smaller_tiles_of_the_recording_form(N):
    """Sampled, degree 0, M = 5, T = 3 on arm2: the recording launch runs 4 trajectories per workgroup at N = 640 and one at N = 2600.
    Status 0; states and inputs carry the bits of the launch without a record, whose states carry the bits of the open-loop launch on its
    inputs; states, inputs and the three gradients against the truth."""
    c, pm, gains, x0, eps, T, w, wu, truth = _rung(N, 0)
    clf.rung_of_the_recording_form(PD, "rung N %d" % N, pm, controller(c, *gains), x0, eps, T, w, wu, truth, TOLS)


def test_the_four_trajectory_tile_without_a_record():
    """Sampled, degree 2, N = 1200 (the k panel of 16 trajectories does not fit), nothing requires grad: status 0, the states carry the bits
    of the open-loop launch on the inputs, states and inputs against the truth.  (No record, so no gradient to compare.)"""
    c, pm, gains, x0, eps, T, w, wu, truth = _rung(1200, 2)
    clf.four_trajectory_tile_without_a_record(PD, "rung N 1200 deg 2", pm, controller(c, *gains, trainable=False), x0, eps, T, truth, TOLS)


# ---- 3. Philox mode: central differences of the op ------------------------------------------------------------------------------------------
def test_philox_mode_against_central_differences():
    """Step 1e-6, bound 1e-5 relative with floor 1e-3, as tests/test_gpu_open_rollout_grad.py::test_philox_mode_against_central_differences."""
    c, m, pm = pair("arm2", 37, 2)
    M, T = 3, 6
    x0, kp, kd, target, _, w, wu = inputs_for(c, M, T, seed=5)
    policy_of = lambda gains, trainable: controller(c, gains[0], gains[1], target, trainable=trainable)
    checks = [("sqrt_kp[1]", 0, 1), ("x0[2,1]", 2, 2 * c["S"] + 1)]
    clf.central_differences(PD, pm, policy_of, [kp, kd], x0, w, wu, T, checks, step=1e-6, bound=(1e-5, 1e-3))


# ---- 4. shard invariance -------------------------------------------------------------------------------------------------------------------
def test_shard_invariance():
    """Rows [a, b) launched with particle_offset = a: states, inputs and the per-trajectory g_gains rows are bitwise those of one launch over
    all rows (Philox)."""
    import ctypes as C

    from mc_pilco_amd import hipabi as abi
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    M, T, cut = 20, 6, 7
    x0, kp, kd, target, _, w, wu = inputs_for(c, M, T, seed=9)
    pd = controller(c, kp, kd, target).packed()
    kpg, kdg = G(kp), G(kd)

    def run(a, b):
        x = G(x0[a:b])
        st, inp, jac = ops._closed_launch(pm, pd, (kpg, kdg), ops.NoiseSpec(seed=4, call=2, particle_offset=a), x, T, True,
                                          torch.zeros(1, dtype=torch.int32, device=dev()), True)
        gg = torch.empty(b - a, 2, c["U"], dtype=DT, device=dev())
        gx = torch.empty(b - a, c["S"], dtype=DT, device=dev())
        pc = pd.to_c(kpg, kdg)
        gs, gi = G(w[:, a:b]), G(wu[:, a:b])  # (named: the buffers must outlive the launch that reads them)
        abi.check(abi.lib().mcp_rollout_pd_bwd(C.byref(pm.c), C.byref(pc), b - a, T, abi.ptr(st), abi.ptr(inp), abi.ptr(jac), abi.ptr(gs),
                                               abi.ptr(gi), abi.ptr(gg), abi.ptr(gx), abi.stream()), "mcp_rollout_pd_bwd")
        torch.cuda.synchronize()
        return st, inp, gg, gx

    st, inp, gg, gx = run(0, M)
    assert float(gg.abs().max()) > 0
    for a, b in ((0, cut), (cut, M)):
        sa, ia, ga, xa = run(a, b)
        assert torch.equal(sa, st[:, a:b]) and torch.equal(ia, inp[:, a:b])
        assert torch.equal(ga, gg[a:b]) and torch.equal(xa, gx[a:b])


# ---- 5. status word --------------------------------------------------------------------------------------------------------------------------
def test_status_word():
    c, m, pm = pair("arm2", 37, 0)
    M, T = 5, 4
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=31)
    pd = controller(c, kp, kd, target, trainable=False).packed()
    bad = x0.clone()
    bad[3, 1] = float("nan")
    pd0 = controller(c, kp, kd, torch.zeros(4, 4, dtype=DT), trainable=False).packed()  # target 0: the PD law gives u = 0 exactly
    clf.status_word(PD, pm, c, pd, (pd, bad), pd0, x0, eps, T)


# ---- 6. class path ---------------------------------------------------------------------------------------------------------------------------
def _arm_object(kp, kd, target, M):
    """MC_PILCO over a fused-layout arm2 speed model trained on a short recorded trajectory, with the trainable PD controller."""
    from mc_pilco_amd.policy_learning import Policy

    return clf.arm_object(Policy.PD_controller, clf.arm_pd_par(kp, kd, target))


def test_class_path():
    M, T = 16, 8
    target = 0.3 * np.sin(0.3 * np.arange(T + 2).reshape(-1, 1) + np.array([0.0, 1.0, 2.0, 3.0]).reshape(1, -1))
    sim = clf.sim_args(M, T)

    def rollout(fused):
        obj = _arm_object([1.0, 1.2], [0.5, 0.4], target, M)
        obj.fused_feedback = fused
        torch.manual_seed(5)
        with clf.normal_draws_on_the_cpu():
            st, inp = obj.apply_policy(**sim)
        assert obj.last_feedback_fused is fused and (obj.last_status is not None) is fused
        cost, _ = obj.cost_function(st, inp, 0)
        cost.backward()
        pol = obj.control_policy
        return st.detach(), inp.detach(), pol.sqrt_Kp_gains.grad.clone(), pol.sqrt_Kd_gains.grad.clone()

    fs, fi, fkp, fkd = rollout(True)
    ss, si, skp, skd = rollout(False)
    es, ei, ep, ed = float((fs - ss).abs().max()), float((fi - si).abs().max()), relmax(fkp, skp), relmax(fkd, skd)
    print("class path, fused vs step: states %.3e inputs %.3e g_sqrt_kp %.3e g_sqrt_kd %.3e" % (es, ei, ep, ed))
    assert es < STATE_TOL and ei < INPUT_TOL and ep < GRAD_TOL and ed < GRAD_TOL

    def optimise(fused):
        obj = _arm_object([1.0, 1.2], [0.5, 0.4], target, M)
        obj.fused_feedback = fused
        torch.manual_seed(6)
        buf = io.StringIO()
        with clf.normal_draws_on_the_cpu(), contextlib.redirect_stdout(buf):
            out = obj.reinforce_policy(**clf.reinforce_args(sim, T, 5))
        assert obj.last_feedback_fused is fused
        pol = obj.control_policy
        return np.asarray(out[0], dtype=float).reshape(-1), pol.sqrt_Kp_gains.detach().cpu().numpy(), pol.sqrt_Kd_gains.detach().cpu().numpy()

    fc, fkp2, fkd2 = optimise(True)
    sc, skp2, skd2 = optimise(False)
    print("cost sequences:", fc, sc)
    assert fc.shape == sc.shape == (5,)
    assert np.abs(fkp2 - np.array([1.0, 1.2])).max() > 1e-3 and np.abs(fkd2 - np.array([0.5, 0.4])).max() > 1e-3  # the gains changed
    assert np.max(np.abs(fc - sc) / np.abs(sc)) < 1e-8


# ---- 7. saved record -------------------------------------------------------------------------------------------------------------------------
def test_saved_record_refuses_in_place_changes():
    c, m, pm = pair("arm2", 37, 0)
    x0, kp, kd, target, _, w, wu = inputs_for(c, 2, 4, seed=3)
    clf.saved_record_refuses_in_place_changes(PD, pm, controller(c, kp, kd, target), x0, 4)
