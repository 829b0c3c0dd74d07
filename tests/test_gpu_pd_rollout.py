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
import functools
import io

import numpy as np
import pytest
import torch

from pd_models import CASES, SHAPES, build_pair, case_id, family, inputs_for, pd_truth

pytestmark = pytest.mark.gpu
DT = torch.float64
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9


def dev():
    return torch.device("cuda", 0)


def G(a):
    return torch.as_tensor(np.asarray(a), dtype=DT).to(dev()).contiguous()


def relmax(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


@functools.lru_cache(maxsize=None)
def pair(shape, N, deg, vs=None):
    """(cfg, oracle model, PackedModel on the oracle's own Kinv / alpha); built once per process and shared, never modified."""
    from gpu_helpers import spec_from
    from mc_pilco_amd import ops

    c, m, specs = build_pair(shape, N, deg, seed=N + deg)
    gps = [ops.PackedGP(spec_from(*specs[g]), G(m.cache[g].X), G(m.cache[g].alpha), G(m.cache[g].Kinv)) for g in range(c["G"])]
    scale = None if vs is None else list(vs)
    if family(shape) == "delta":
        pm = ops.PackedModel.delta(gps, c["S"], c["U"], c["angle"], c["not_angle"], var_scale=scale)
    else:
        pm = ops.PackedModel(gps, c["S"], c["U"], c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"], var_scale=scale)
    return c, m, pm


def controller(c, kp, kd, target, u_max=1.0, squash=True, trainable=True):
    from mc_pilco_amd.policy_learning import Policy

    return Policy.PD_controller(state_dim=c["S"], input_dim=c["U"], sqrt_Kp_gains=kp.numpy(), sqrt_Kd_gains=kd.numpy(), target_traj=G(target),
                                flg_squash=squash, u_max=u_max, flg_trainable=trainable, dtype=DT, device=dev())


def gpu_run(pm, pol, x0, eps, w, wu, sample, T, noise=None, x0_grad=True):
    """(states, inputs, g_sqrt_kp, g_sqrt_kd, g_x0, status) of the op with L = sum w states + sum wu inputs."""
    from mc_pilco_amd import ops

    for q in pol.parameters():
        q.grad = None
    xg = G(x0).requires_grad_(x0_grad)
    nz = noise if noise is not None else (ops.NoiseSpec(eps=G(eps)) if sample else None)
    st, inp, status = ops.rollout_pd(pm, pol.packed(), nz, xg, T, particle_pred=sample)
    L = (G(w) * st).sum() + (0.0 if wu is None else (G(wu) * inp).sum())
    L.backward()
    return st.detach(), inp.detach(), pol.sqrt_Kp_gains.grad.clone(), pol.sqrt_Kd_gains.grad.clone(), xg.grad, int(status.item())


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
    ost, oin, ogp, ogd, ogx, vmin = pd_truth(shape, m, x0, kp, kd, target, eps, w, wu, sample, u_max=u_max, squash=squash, var_scale=vs)
    if sample and T > 1:
        assert vmin > 0.0  # the oracle alone keeps every step's variance positive on this seed
    pol = controller(c, kp, kd, target, u_max=u_max, squash=squash)
    st, inp, gp_, gd_, gx, status = gpu_run(pm, pol, x0, eps, w, wu, sample, T)
    es, ei = float((st.cpu() - ost).abs().max()), float((inp.cpu() - oin).abs().max())
    ep, ed, ex = relmax(gp_, ogp), relmax(gd_, ogd), relmax(gx, ogx)
    print("%s: states %.3e inputs %.3e g_sqrt_kp %.3e g_sqrt_kd %.3e g_x0 %.3e (min var %.3e)" % (case_id(case), es, ei, ep, ed, ex, vmin))
    assert status == 0
    assert es < STATE_TOL and ei < INPUT_TOL
    assert ep < GRAD_TOL and ed < GRAD_TOL and ex < GRAD_TOL


# ---- 2. the feedback launch against the open-loop launch on its inputs -------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_states_carry_the_bits_of_the_open_loop_launch(noise):
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 1)
    M, T = 17, 6
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=21)
    pol = controller(c, kp, kd, target)
    sample = noise != "mean"
    nz = lambda: None if not sample else (ops.NoiseSpec(eps=G(eps)) if noise == "eps" else ops.NoiseSpec(seed=11, call=3))
    with torch.no_grad():
        st, inp, status = ops.rollout_pd(pm, pol.packed(), nz(), G(x0), T, particle_pred=sample)
    assert int(status.item()) == 0 and not st.requires_grad
    so, status_o = ops.rollout_open(pm, G(x0), inp[:T - 1].contiguous(), noise=nz(), particle_pred=sample)
    assert int(status_o.item()) == 0
    assert torch.equal(st, so)  # the same phases on the same operands
    sr, ir, status_r = ops.rollout_pd(pm, pol.packed(), nz(), G(x0), T, particle_pred=sample)  # the gains require grad: the recording launch
    assert sr.requires_grad and int(status_r.item()) == 0
    assert torch.equal(sr.detach(), st) and torch.equal(ir.detach(), inp)


# ---- 2b. the ladder's smaller tiles ---------------------------------------------------------------------------------------------------------
# The rungs are held to the bounds of the N = 300 cases of CASES (STATE_TOL, INPUT_TOL, GRAD_TOL): the library of the commit before the host
# path was unified measured below them on an MI355X at every rung (states / inputs / g_sqrt_kp / g_sqrt_kd / g_x0; a case measuring above
# would have been given four times its measurement, the headroom the N = 1100 / 1500 bounds of tests/test_gpu_open_rollout.py carry):
#   N 640   6.2e-13 / 1.9e-13 / 5.6e-13 / 5.6e-13 / 2.9e-13      N 2600  7.4e-12 / 4.2e-12 / 8.5e-12 / 1.1e-11 / 2.8e-12
#   N 1200, degree 2, no record  3.2e-12 / 1.2e-12
@pytest.mark.parametrize("N", [640, 2600])
def test_the_smaller_tiles_of_the_recording_form(N):
    """Sampled, degree 0, M = 5, T = 3 on arm2: the recording launch runs 4 trajectories per workgroup at N = 640 and one at N = 2600.
    Status 0; states and inputs carry the bits of the launch without a record, whose states carry the bits of the open-loop launch on its
    inputs; states, inputs and the three gradients against the truth."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", N, 0)
    M, T = 5, 3
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=T * 100 + M)
    torch.set_num_threads(1)
    ost, oin, ogp, ogd, ogx, vmin = pd_truth("arm2", m, x0, kp, kd, target, eps, w, wu, True)
    assert vmin > 0.0
    pol = controller(c, kp, kd, target)
    st, inp, gp_, gd_, gx, status = gpu_run(pm, pol, x0, eps, w, wu, True, T)
    with torch.no_grad():
        s0, i0, status0 = ops.rollout_pd(pm, pol.packed(), ops.NoiseSpec(eps=G(eps)), G(x0), T, particle_pred=True)
    so, status_o = ops.rollout_open(pm, G(x0), i0[:T - 1].contiguous(), noise=ops.NoiseSpec(eps=G(eps)), particle_pred=True)
    es, ei = float((st.cpu() - ost).abs().max()), float((inp.cpu() - oin).abs().max())
    ep, ed, ex = relmax(gp_, ogp), relmax(gd_, ogd), relmax(gx, ogx)
    print("rung N %d: states %.3e inputs %.3e g_sqrt_kp %.3e g_sqrt_kd %.3e g_x0 %.3e (min var %.3e)" % (N, es, ei, ep, ed, ex, vmin))
    assert status == 0 and int(status0.item()) == 0 and int(status_o.item()) == 0
    assert torch.equal(st, s0) and torch.equal(inp, i0) and torch.equal(s0, so)
    assert es < STATE_TOL and ei < INPUT_TOL
    assert ep < GRAD_TOL and ed < GRAD_TOL and ex < GRAD_TOL


def test_the_four_trajectory_tile_without_a_record():
    """Sampled, degree 2, N = 1200 (the k panel of 16 trajectories does not fit), nothing requires grad: status 0, the states carry the bits
    of the open-loop launch on the inputs, states and inputs against the truth.  (No record, so no gradient to compare.)"""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 1200, 2)
    M, T = 5, 3
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=T * 100 + M)
    torch.set_num_threads(1)
    ost, oin, _, _, _, vmin = pd_truth("arm2", m, x0, kp, kd, target, eps, w, wu, True)
    assert vmin > 0.0
    pd = controller(c, kp, kd, target, trainable=False).packed()
    st, inp, status = ops.rollout_pd(pm, pd, ops.NoiseSpec(eps=G(eps)), G(x0), T, particle_pred=True)
    so, status_o = ops.rollout_open(pm, G(x0), inp[:T - 1].contiguous(), noise=ops.NoiseSpec(eps=G(eps)), particle_pred=True)
    es, ei = float((st.cpu() - ost).abs().max()), float((inp.cpu() - oin).abs().max())
    print("rung N 1200 deg 2, no record: states %.3e inputs %.3e (min var %.3e)" % (es, ei, vmin))
    assert int(status.item()) == 0 and int(status_o.item()) == 0 and not st.requires_grad
    assert torch.equal(st, so)
    assert es < STATE_TOL and ei < INPUT_TOL


# ---- 3. Philox mode: central differences of the op ------------------------------------------------------------------------------------------
def test_philox_mode_against_central_differences():
    """Step 1e-6, bound 1e-5 relative with floor 1e-3, as tests/test_gpu_open_rollout_grad.py::test_philox_mode_against_central_differences."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 2)
    M, T = 3, 6
    x0, kp, kd, target, _, w, wu = inputs_for(c, M, T, seed=5)
    nz = lambda: ops.NoiseSpec(seed=77, call=5)
    pol = controller(c, kp, kd, target)
    _, _, gkp, gkd, gx, status = gpu_run(pm, pol, x0, None, w, wu, True, T, noise=nz())
    assert status == 0

    def loss(kp_, x0_):
        p2 = controller(c, kp_, kd, target, trainable=False)
        st, inp, s = ops.rollout_pd(pm, p2.packed(), nz(), G(x0_), T, particle_pred=True)
        assert int(s.item()) == 0
        return float((G(w) * st).sum() + (G(wu) * inp).sum())

    h = 1e-6
    kpp, kpm = kp.clone(), kp.clone()
    kpp[1] += h
    kpm[1] -= h
    fd, g = (loss(kpp, x0) - loss(kpm, x0)) / (2 * h), float(gkp[1])
    print("sqrt_kp[1]: fd %.9e adjoint %.9e" % (fd, g))
    assert abs(fd - g) < 1e-5 * max(abs(g), 1e-3)
    xp, xm = x0.clone(), x0.clone()
    xp[2, 1] += h
    xm[2, 1] -= h
    fd, g = (loss(kp, xp) - loss(kp, xm)) / (2 * h), float(gx[2, 1])
    print("x0[2,1]: fd %.9e adjoint %.9e" % (fd, g))
    assert abs(fd - g) < 1e-5 * max(abs(g), 1e-3)


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
    from mc_pilco_amd import hipabi, ops

    c, m, pm = pair("arm2", 37, 0)
    M, T = 5, 4
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=31)
    pd = controller(c, kp, kd, target, trainable=False).packed()
    for sample in (False, True):
        nz = ops.NoiseSpec(eps=G(eps)) if sample else None
        assert int(ops.rollout_pd(pm, pd, nz, G(x0), T, particle_pred=sample)[-1].item()) == 0
        bad = x0.clone()
        bad[3, 1] = float("nan")
        assert int(ops.rollout_pd(pm, pd, nz, G(bad), T, particle_pred=sample)[-1].item()) & hipabi.STATUS_NAN
    # a known non-positive variance, by the recipe of tests/test_gpu_dropin.py::test_zero_predictive_variance_raises_like_the_reference_normal:
    # one training point exactly at the GP input of x = 0, u = 0 (target 0: the PD law gives u = 0 exactly), no noise, Kinv = I -> var = 1 - 1 = 0
    from gpu_helpers import spec_from

    X = np.zeros((16, 8))
    X[:, 4:6] = 1.0                  # z = [x2, x3, sin x0, sin x1, cos x0, cos x1, u0, u1]
    X[1:, 0] = 50.0 + np.arange(15)  # the other rows far away (k = 0 there)
    gp = ops.PackedGP(spec_from(np.ones(8), 0.0), G(X), G(np.zeros(16)), G(np.eye(16)))
    zero = ops.PackedModel([gp, gp], c["S"], c["U"], c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    pd0 = controller(c, kp, kd, torch.zeros(4, 4, dtype=DT), trainable=False).packed()
    st, _, status = ops.rollout_pd(zero, pd0, ops.NoiseSpec(seed=1, call=1), G(np.zeros((8, 4))), 2, particle_pred=True)
    assert int(status.item()) & hipabi.STATUS_NONPOS_VAR and not (int(status.item()) & hipabi.STATUS_NAN)
    assert bool(torch.isfinite(st).all())


# ---- 6. class path ---------------------------------------------------------------------------------------------------------------------------
def _arm_object(kp, kd, target, M):
    """MC_PILCO over a fused-layout arm2 speed model trained on a short recorded trajectory, with the trainable PD controller."""
    from mc_pilco_amd.model_learning import Model_learning as ML
    from mc_pilco_amd.policy_learning import MC_PILCO, Cost_function, Policy
    from test_gpu_dropin import rbf_dict

    c = SHAPES["arm2"]
    rs = np.random.RandomState(3)
    n, Ts = 60, c["Ts"]
    tt = Ts * np.arange(n + 1).reshape(-1, 1)
    u = 0.8 * np.sin(2 * np.pi * (0.3 + 0.9 * rs.rand(1, 2)) * tt + 6.28 * rs.rand(1, 2))
    x = np.zeros((n + 1, 4))
    x[0] = [0.3, -0.2, 0.0, 0.0]
    for i in range(n):
        q, qd = x[i, :2], x[i, 2:]
        qdd = -4.0 * np.sin(q) - 0.4 * qd + 3.0 * u[i]
        x[i + 1, 2:] = qd + Ts * qdd
        x[i + 1, :2] = q + Ts * qd + 0.5 * Ts * Ts * qdd
    with contextlib.redirect_stdout(io.StringIO()):
        ml = ML.Speed_Model_learning_RBF_angle_state(num_gp=2, init_dict_list=[rbf_dict(8, np.ones(8) * 2.0, 0.05)] * 2, T_sampling=Ts,
                                                     angle_indeces=c["angle"], not_angle_indeces=c["not_angle"], vel_indeces=c["vel"],
                                                     not_vel_indeces=c["not_vel"], dtype=DT, device=dev())
        ml.add_data(x, u)
        with torch.no_grad():
            for g in range(2):
                ml.pretrain_gp(g)
        ml.set_eval_mode()
        ppar = dict(state_dim=4, input_dim=2, sqrt_Kp_gains=np.asarray(kp), sqrt_Kd_gains=np.asarray(kd), target_traj=G(target), flg_squash=True,
                    u_max=1.5, flg_trainable=True, dtype=DT, device=dev())
        obj = MC_PILCO.MC_PILCO(T_sampling=Ts, state_dim=4, input_dim=2, f_sim=lambda y, t, u: None, f_model_learning=lambda **kw: ml,
                                model_learning_par={}, f_rand_exploration_policy=Policy.Random_exploration,
                                rand_exploration_policy_par=dict(state_dim=4, input_dim=2, u_max=1.0, dtype=DT),
                                f_control_policy=Policy.PD_controller, control_policy_par=ppar,
                                f_cost_function=Cost_function.Expected_saturated_distance,
                                cost_function_par=dict(target_state=G([0.2, -0.1]), lengthscales=G([0.5, 0.5]), active_dims=np.array([0, 1])),
                                log_path=None, dtype=DT, device=dev())
    obj.noise_mode = "reference"
    return obj


@contextlib.contextmanager
def _normal_draws_on_the_cpu():
    """The step path samples with Normal(mu, sigma).rsample() on the model's device; the reference runs on the CPU, and "reference" noise mode
    replays ITS draws.  For the comparison the step path's standard normals are taken from the CPU generator, as the reference takes them."""
    import torch.distributions.normal as tdn

    orig = tdn._standard_normal
    tdn._standard_normal = lambda shape, dtype, device: torch.empty(tuple(shape), dtype=dtype).normal_().to(device)
    try:
        yield
    finally:
        tdn._standard_normal = orig


def test_class_path():
    M, T = 16, 8
    target = 0.3 * np.sin(0.3 * np.arange(T + 2).reshape(-1, 1) + np.array([0.0, 1.0, 2.0, 3.0]).reshape(1, -1))
    sim = dict(particles_initial_state_mean=G([0.1, -0.1, 0.0, 0.05]), particles_initial_state_var=G([1e-2, 1e-2, 2e-2, 2e-2]),
               flg_particles_init_uniform=False, particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
               num_particles=M, T_control=T)

    def rollout(fused):
        obj = _arm_object([1.0, 1.2], [0.5, 0.4], target, M)
        obj.fused_feedback = fused
        torch.manual_seed(5)
        with _normal_draws_on_the_cpu():
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
        with _normal_draws_on_the_cpu(), contextlib.redirect_stdout(buf):
            out = obj.reinforce_policy(T_control=0.05 * T, num_particles=M, trial_index=0, particles_initial_state_mean=sim["particles_initial_state_mean"],
                                       particles_initial_state_var=sim["particles_initial_state_var"], flg_particles_init_uniform=False,
                                       particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
                                       opt_steps_list=[5], lr_list=[0.01], f_optimizer="lambda p, lr : torch.optim.Adam(p, lr)", num_step_print=10,
                                       policy_reinit_dict=None)
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
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    x0, kp, kd, target, _, w, wu = inputs_for(c, 2, 4, seed=3)
    pol = controller(c, kp, kd, target)
    for which in (0, 1):
        out = ops.rollout_pd(pm, pol.packed(), None, G(x0), 4, particle_pred=False)
        with torch.no_grad():
            out[which].mul_(2.0)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            (out[0].sum() + out[1].sum()).backward()
