"""GPU: the fused closed loop under the tanh-MLP policy (mcp_rollout_mlp + mcp_rollout_mlp_bwd, ops.rollout_mlp, MC_PILCO.apply_policy with
a Policy.MLP_policy) against torch autograd through the oracle's step with the network written out (tests/mlp_models.mlp_truth; conditioning
checked by tests/test_mlp_models_cpu.py), and the bitwise contracts with the open-loop kernels it shares its phases with.

Bounds (tests/test_gpu_pd_rollout.py:25, on the oracle's own Kinv / alpha): states 1e-9 absolute, inputs 2e-9 absolute,
every parameter gradient and g_x0 1e-9 relative to that tensor's largest magnitude."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

from mlp_models import CASES, PAIR_SEED, SHAPES, build_pair, case_id, case_truth, family, inputs_for, network

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


def packed_model(c, m, specs, shape, vs=None):
    from gpu_helpers import spec_from
    from mc_pilco_amd import ops

    gps = [ops.PackedGP(spec_from(*specs[g]), G(m.cache[g].X), G(m.cache[g].alpha), G(m.cache[g].Kinv)) for g in range(c["G"])]
    scale = None if vs is None else list(vs)
    if family(shape) == "delta":
        return ops.PackedModel.delta(gps, c["S"], c["U"], c["angle"], c["not_angle"], var_scale=scale)
    return ops.PackedModel(gps, c["S"], c["U"], c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"], var_scale=scale)


@functools.lru_cache(maxsize=None)
def pair(shape, N, deg, vs=None):
    """(cfg, oracle model, PackedModel on the oracle's own Kinv / alpha); built once per process and shared, never modified."""
    c, m, specs = build_pair(shape, N, deg, seed=PAIR_SEED)
    return c, m, packed_model(c, m, specs, shape, vs)


def policy(c, params, hidden, angle=None, non_angle=None, u_max=1.0, squash=True, trainable=True):
    from mc_pilco_amd.policy_learning import Policy

    angle = c["angle"] if angle is None else angle
    non_angle = c["not_angle"] if non_angle is None else non_angle
    pol = Policy.MLP_policy(state_dim=c["S"], input_dim=c["U"], hidden_sizes=list(hidden), angle_indices=angle or None, non_angle_indices=non_angle or None,
                            u_max=u_max, flg_squash=squash, weight_init=params, dtype=DT, device=dev())
    for q in pol.parameters():
        q.requires_grad_(trainable)
    return pol


def gpu_run(pm, pol, x0, eps, w, wu, sample, T, noise=None, x0_grad=True):
    """(states, inputs, [parameter gradients or None], g_x0, status) of the op with L = sum w states + sum wu inputs."""
    from mc_pilco_amd import ops

    for q in pol.parameters():
        q.grad = None
    xg = G(x0).requires_grad_(x0_grad)
    nz = noise if noise is not None else (ops.NoiseSpec(eps=G(eps)) if sample else None)
    st, inp, status = ops.rollout_mlp(pm, pol.packed(), nz, xg, T, particle_pred=sample)
    L = (G(w) * st).sum() + (0.0 if wu is None else (G(wu) * inp).sum())
    L.backward()
    return st.detach(), inp.detach(), [None if q.grad is None else q.grad.clone() for q in pol.mlp_parameters()], xg.grad, int(status.item())


# ---- 1. parity with the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_truth(case):
    mode, shape, deg, N, T, M, hidden, opt = case
    sample = mode == "sampled"
    vs = opt.get("var_scale")
    c, m, ins, (ost, oin, ograds, ogx, vmin) = case_truth(case)
    _, _, pm = pair(shape, N, deg, None if vs is None else tuple(vs))
    if sample and T > 1:
        assert vmin > 0.0
    pol = policy(c, ins["params"], hidden, ins["angle"], ins["non_angle"], u_max=ins["u_max"], squash=ins["squash"])
    only = opt.get("only_grad")
    if only is not None:  # requires_grad on one tensor alone: neither x0 nor the other parameters get a gradient
        for i, q in enumerate(pol.mlp_parameters()):
            q.requires_grad_(i == only)
    st, inp, grads, gx, status = gpu_run(pm, pol, ins["x0"], ins["eps"], ins["w"], ins["wu"], sample, T, x0_grad=only is None)
    es, ei = float((st.cpu() - ost).abs().max()), float((inp.cpu() - oin).abs().max())
    if only is None:
        eg, ex = [relmax(g, o) for g, o in zip(grads, ograds)], relmax(gx, ogx)
    else:
        assert gx is None and all((g is None) == (i != only) for i, g in enumerate(grads))
        eg, ex = [relmax(grads[only], ograds[only])], 0.0
    print("%s: states %.3e inputs %.3e g_params %s g_x0 %.3e (min var %.3e)" % (case_id(case), es, ei, " ".join("%.3e" % e for e in eg), ex, vmin))
    assert status == 0
    assert es < STATE_TOL and ei < INPUT_TOL
    assert max(eg) < GRAD_TOL and ex < GRAD_TOL


# ---- 2. bit identities: against the open-loop launch on the launch's own inputs; the plain against the recording launch -----------------------
def _bit_identities(pm, c, hidden, M, T, noise, seed):
    from mc_pilco_amd import ops

    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=seed)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], seed), hidden)
    sample = noise != "mean"
    nz = lambda: None if not sample else (ops.NoiseSpec(eps=G(eps)) if noise == "eps" else ops.NoiseSpec(seed=11, call=3))
    with torch.no_grad():
        st, inp, status = ops.rollout_mlp(pm, pol.packed(), nz(), G(x0), T, particle_pred=sample)
    assert int(status.item()) == 0 and not st.requires_grad
    so, status_o = ops.rollout_open(pm, G(x0), inp[:T - 1].contiguous(), noise=nz(), particle_pred=sample)
    assert int(status_o.item()) == 0
    assert torch.equal(st, so)  # the same phases on the same operands
    sr, ir, status_r = ops.rollout_mlp(pm, pol.packed(), nz(), G(x0), T, particle_pred=sample)  # the parameters require grad: the recording launch
    assert sr.requires_grad and int(status_r.item()) == 0
    assert torch.equal(sr.detach(), st) and torch.equal(ir.detach(), inp)
    ((G(w) * sr).sum() + (G(wu) * ir).sum()).backward()  # the sweep over that record runs and leaves finite gradients
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0 for q in pol.mlp_parameters())


@pytest.mark.parametrize("M", [17, 1041])  # 4 trajectories per workgroup up to MLP_SMALL_SWARM = 1024 of them, 16 beyond: the bits of either
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_states_carry_the_bits_of_the_open_loop_launch(noise, M):
    c, m, pm = pair("arm2", 37, 1)
    _bit_identities(pm, c, (7, 3), M, 6, noise, seed=21)


# ---- 3. the ladder's smaller tiles (no oracle at these sizes: the bit identities of 2) -----------------------------------------------------------
# (N, M, hidden) and what the two launches run by LDS fit (doubles of 20 480; layouts of csrc/rollout_mlp.hip worked out by hand):
#   640, 5     recording 4 per workgroup, plain 4 (a small swarm)            2600, 5   recording 1, plain 4
#   640, 1041  M > MLP_SMALL_SWARM: the ladder starts at 16; the recording launch falls through to 4 (two k panels of 16: 23 040), plain runs 16
#   2600, 1041 the recording launch falls through 16 -> 4 -> 1; the plain launch 16 -> 4
#   1900, 5 with (64, 64)   recording 4 per workgroup WITHOUT the weights' LDS copy (two panels 15 232 + the copy 4 868 do not fit: the forms
#              that read the weights from global memory through the address table in LDS); the plain launch has the copy -- and the same bits
@pytest.mark.parametrize("N,M,hidden", [(640, 5, (33, 64)), (2600, 5, (33, 64)), (640, 1041, (33, 64)), (2600, 1041, (33, 64)), (1900, 5, (64, 64))])
def test_the_smaller_tiles_of_the_recording_form(N, M, hidden):
    """Sampled, degree 0, T = 3 on arm2, built as tests/test_gpu_pd_rollout.py builds its rungs."""
    c, m, pm = pair("arm2", N, 0)
    _bit_identities(pm, c, hidden, M, 3, "eps", seed=305)


def test_the_wide_model_without_the_weights_copy():
    """UR5 shape, degree 1, N = 1700, (64, 64): the recording launch runs 4 per workgroup and reads the weights from global memory (15 658 doubles
    without the copy, 5 900 more with it); the plain launch has the copy."""
    c, m, pm = pair("ur5", 1700, 1)
    _bit_identities(pm, c, (64, 64), 5, 3, "eps", seed=305)


def test_the_four_trajectory_tile_without_a_record():
    """Sampled, degree 2, N = 1200: the k panel of 16 trajectories does not fit, the plain launch runs 4 per workgroup."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 1200, 2)
    M, T = 5, 3
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=305)
    pol = policy(c, network(c, (64,), c["angle"], c["not_angle"], 305), (64,), trainable=False)
    st, inp, status = ops.rollout_mlp(pm, pol.packed(), ops.NoiseSpec(eps=G(eps)), G(x0), T, particle_pred=True)
    so, status_o = ops.rollout_open(pm, G(x0), inp[:T - 1].contiguous(), noise=ops.NoiseSpec(eps=G(eps)), particle_pred=True)
    assert int(status.item()) == 0 and int(status_o.item()) == 0 and not st.requires_grad
    assert torch.equal(st, so) and bool(torch.isfinite(inp).all())


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------------
def test_determinism_and_shard_invariance():
    """Two runs: bit-equal slabs and gradients.  Rows [a, b) launched with particle_offset = a, a a multiple of 16: states, inputs, g_x0 and
    the workgroups' slabs are bitwise those of one launch over all rows (Philox)."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    M, T, cut, hidden = 37, 6, 16, (7, 3)
    x0, _, _, _, _, w, wu = inputs_for(c, M, T, seed=9)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 9), hidden)
    mlp = pol.packed()
    tensors = [q.detach() for q in pol.mlp_parameters()]

    def run(a, b):
        x = G(x0[a:b])
        st, inp, jac = ops._closed_launch(pm, mlp, tensors, ops.NoiseSpec(seed=4, call=2, particle_offset=a), x, T, True,
                                          torch.zeros(1, dtype=torch.int32, device=dev()), True)
        slabs, gx = ops._closed_sweep(pm, mlp, tensors, st, inp, jac, G(w[:, a:b]), G(wu[:, a:b]), True, True)
        torch.cuda.synchronize()
        return st, inp, slabs, gx

    st, inp, slabs, gx = run(0, M)
    assert tuple(slabs.shape) == (3, mlp.n_param) and all(float(slabs[i].abs().max()) > 0 for i in range(3))
    st2, inp2, slabs2, gx2 = run(0, M)
    assert torch.equal(st, st2) and torch.equal(inp, inp2) and torch.equal(slabs, slabs2) and torch.equal(gx, gx2)
    for a, b in ((0, cut), (cut, M)):
        sa, ia, la, xa = run(a, b)
        assert torch.equal(sa, st[:, a:b]) and torch.equal(ia, inp[:, a:b])
        assert torch.equal(la, slabs[a // 16:(b + 15) // 16]) and torch.equal(xa, gx[a:b])
    # the op: two backward passes leave the same bits in every .grad
    _, _, g1, x1, _ = gpu_run(pm, pol, x0, None, w, wu, True, T, noise=ops.NoiseSpec(seed=4, call=2))
    _, _, g2, x2, _ = gpu_run(pm, pol, x0, None, w, wu, True, T, noise=ops.NoiseSpec(seed=4, call=2))
    assert all(torch.equal(p, q) for p, q in zip(g1, g2)) and torch.equal(x1, x2)
    assert all(torch.equal(g.reshape(-1), f) for g, f in zip(g1, torch.split(slabs.sum(0), [q.numel() for q in tensors])))


# ---- 5. Philox mode: central differences of the op ------------------------------------------------------------------------------------------
def test_philox_mode_against_central_differences():
    """Step 1e-6, bound 1e-5 relative with floor 1e-3, as tests/test_gpu_open_rollout_grad.py::test_philox_mode_against_central_differences;
    two entries of every parameter tensor and of x0."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 2)
    M, T, hidden = 3, 6, (7, 3)
    x0, _, _, _, _, w, wu = inputs_for(c, M, T, seed=5)
    params = network(c, hidden, c["angle"], c["not_angle"], 5)
    nz = lambda: ops.NoiseSpec(seed=77, call=5)
    _, _, grads, gx, status = gpu_run(pm, policy(c, params, hidden), x0, None, w, wu, True, T, noise=nz())
    assert status == 0

    def loss(params_, x0_):
        st, inp, s = ops.rollout_mlp(pm, policy(c, params_, hidden, trainable=False).packed(), nz(), G(x0_), T, particle_pred=True)
        assert int(s.item()) == 0
        return float((G(w) * st).sum() + (G(wu) * inp).sum())

    h = 1e-6
    for i, q in enumerate(params + [x0]):
        g = (grads + [gx])[i].cpu().reshape(-1)
        for e in (0, q.numel() - 1):
            plus, minus = [t.clone() for t in params + [x0]], [t.clone() for t in params + [x0]]
            plus[i].reshape(-1)[e] += h
            minus[i].reshape(-1)[e] -= h
            fd = (loss(plus[:-1], plus[-1]) - loss(minus[:-1], minus[-1])) / (2 * h)
            print("tensor %d entry %d: fd %.9e adjoint %.9e" % (i, e, fd, float(g[e])))
            assert abs(fd - float(g[e])) < 1e-5 * max(abs(float(g[e])), 1e-3)


# ---- 6. status word --------------------------------------------------------------------------------------------------------------------------
def test_status_word():
    from gpu_helpers import spec_from
    from mc_pilco_amd import hipabi, ops

    c, m, pm = pair("arm2", 37, 0)
    M, T, hidden = 5, 4, (5,)
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=31)
    params = network(c, hidden, c["angle"], c["not_angle"], 31)
    for sample in (False, True):
        nz = ops.NoiseSpec(eps=G(eps)) if sample else None
        assert int(ops.rollout_mlp(pm, policy(c, params, hidden, trainable=False).packed(), nz, G(x0), T, particle_pred=sample)[-1].item()) == 0
        bad = [q.clone() for q in params]
        bad[2][1, 3] = float("nan")  # a NaN weight of the output layer: input 1 of every trajectory
        assert int(ops.rollout_mlp(pm, policy(c, bad, hidden, trainable=False).packed(), nz, G(x0), T, particle_pred=sample)[-1].item()) & hipabi.STATUS_NAN
    # a known non-positive variance, as tests/test_gpu_pd_rollout.py::test_status_word builds it: one training point exactly at the GP input of
    # x = 0, u = 0 (a network of zeros gives u = 0 exactly), no noise, Kinv = I -> var = 1 - 1 = 0
    X = np.zeros((16, 8))
    X[:, 4:6] = 1.0                  # z = [x2, x3, sin x0, sin x1, cos x0, cos x1, u0, u1]
    X[1:, 0] = 50.0 + np.arange(15)  # the other rows far away (k = 0 there)
    gp = ops.PackedGP(spec_from(np.ones(8), 0.0), G(X), G(np.zeros(16)), G(np.eye(16)))
    zero = ops.PackedModel([gp, gp], c["S"], c["U"], c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    pol0 = policy(c, [torch.zeros_like(q) for q in params], hidden, trainable=False)
    st, _, status = ops.rollout_mlp(zero, pol0.packed(), ops.NoiseSpec(seed=1, call=1), G(np.zeros((8, 4))), 2, particle_pred=True)
    assert int(status.item()) & hipabi.STATUS_NONPOS_VAR and not (int(status.item()) & hipabi.STATUS_NAN)
    assert bool(torch.isfinite(st).all())


# ---- 7. class path ---------------------------------------------------------------------------------------------------------------------------
def _arm_object(params, hidden, M):
    """MC_PILCO over a fused-layout arm2 speed model trained on a short recorded trajectory (the object of tests/test_gpu_pd_rollout.py's class
    path), with the MLP policy."""
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
        ppar = dict(state_dim=4, input_dim=2, hidden_sizes=list(hidden), angle_indices=c["angle"], non_angle_indices=c["not_angle"], u_max=1.5,
                    flg_squash=True, weight_init=params, dtype=DT, device=dev())
        obj = MC_PILCO.MC_PILCO(T_sampling=Ts, state_dim=4, input_dim=2, f_sim=lambda y, t, u: None, f_model_learning=lambda **kw: ml,
                                model_learning_par={}, f_rand_exploration_policy=Policy.Random_exploration,
                                rand_exploration_policy_par=dict(state_dim=4, input_dim=2, u_max=1.0, dtype=DT),
                                f_control_policy=Policy.MLP_policy, control_policy_par=ppar,
                                f_cost_function=Cost_function.Expected_saturated_distance,
                                cost_function_par=dict(target_state=G([0.2, -0.1]), lengthscales=G([0.5, 0.5]), active_dims=np.array([0, 1])),
                                log_path=None, dtype=DT, device=dev())
    obj.noise_mode = "reference"
    return obj


def test_class_path():
    from test_gpu_pd_rollout import _normal_draws_on_the_cpu

    M, T, c = 16, 8, SHAPES["arm2"]
    sim = dict(particles_initial_state_mean=G([0.1, -0.1, 0.0, 0.05]), particles_initial_state_var=G([1e-2, 1e-2, 2e-2, 2e-2]),
               flg_particles_init_uniform=False, particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
               num_particles=M, T_control=T)
    net = lambda hidden: network(c, hidden, c["angle"], c["not_angle"], 40)

    def rollout(fused, hidden=(7, 3), expect=None, edit=None):
        obj = _arm_object(net(hidden), hidden, M)
        obj.fused_feedback = fused
        if edit:
            edit(obj)
        torch.manual_seed(5)
        with _normal_draws_on_the_cpu():
            st, inp = obj.apply_policy(**sim)
        expect = fused if expect is None else expect
        assert obj.last_feedback_fused is expect and (obj.last_status is not None) is expect
        cost, _ = obj.cost_function(st, inp, 0)
        cost.backward()
        return st.detach(), inp.detach(), [q.grad.clone() for q in obj.control_policy.mlp_parameters()]

    fs, fi, fg = rollout(True)
    ss, si, sg = rollout(False)  # fused_feedback off: the same object runs the generic loop
    es, ei, eg = float((fs - ss).abs().max()), float((fi - si).abs().max()), [relmax(a, b) for a, b in zip(fg, sg)]
    print("class path, fused vs step: states %.3e inputs %.3e g_params %s" % (es, ei, " ".join("%.3e" % e for e in eg)))
    assert es < STATE_TOL and ei < INPUT_TOL and max(eg) < GRAD_TOL
    # what the kernels do not take falls through to the generic branch
    rollout(True, hidden=(65,), expect=False)  # a width beyond MCP_MAX_HIDDEN

    def no_layout(obj):
        obj.model_learning.has_fused_layout = lambda: False

    rollout(True, expect=False, edit=no_layout)  # a model without a fused layout

    obj = _arm_object(net((7, 3)), (7, 3), M)
    before = [q.detach().clone() for q in obj.control_policy.mlp_parameters()]
    torch.manual_seed(6)
    with _normal_draws_on_the_cpu(), contextlib.redirect_stdout(io.StringIO()):
        out = obj.reinforce_policy(T_control=0.05 * T, num_particles=M, trial_index=0, particles_initial_state_mean=sim["particles_initial_state_mean"],
                                   particles_initial_state_var=sim["particles_initial_state_var"], flg_particles_init_uniform=False,
                                   particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
                                   opt_steps_list=[3], lr_list=[0.01], f_optimizer="lambda p, lr : torch.optim.Adam(p, lr)", num_step_print=10,
                                   policy_reinit_dict=None)
    assert obj.last_feedback_fused is True
    costs = np.asarray(out[0], dtype=float).reshape(-1)
    assert costs.shape == (3,) and np.isfinite(costs).all()
    assert all(float((q.detach() - b).abs().max()) > 1e-4 for q, b in zip(obj.control_policy.mlp_parameters(), before))  # every tensor moved


# ---- 8. saved record -------------------------------------------------------------------------------------------------------------------------
def test_saved_record_refuses_in_place_changes():
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    x0, _, _, _, _, w, wu = inputs_for(c, 2, 4, seed=3)
    pol = policy(c, network(c, (5,), c["angle"], c["not_angle"], 3), (5,))
    for which in (0, 1):
        out = ops.rollout_mlp(pm, pol.packed(), None, G(x0), 4, particle_pred=False)
        with torch.no_grad():
            out[which].mul_(2.0)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            (out[0].sum() + out[1].sum()).backward()
