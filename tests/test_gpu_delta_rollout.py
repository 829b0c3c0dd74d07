"""GPU: the delta-state models (Model_learning_RBF, Model_learning_RBF_angle_state, Model_learning_RBF_MPK_angle_state; reference
model_learning/Model_learning.py:471-618) on the fused rollout and its adjoint -- mcp_model with every not_vel = -1.  Against the
reference's golden rollouts (tests/golden/make_golden_delta.py) on every kernel variant, through the drop-in MC_PILCO / MC_PILCO4PMS,
teacher-forced at the real size, and particle-sharded over two ranks."""
import contextlib
import io

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (registers the package, also in spawned workers)
from gpu_helpers import VARIANTS, mpk_dict, rbf_dict
from rank_harness import rank_group, run_ranks

pytestmark = pytest.mark.gpu
DT = torch.float64
DELTA_FIXTURES = ["rollout_delta", "rollout_delta_mpk", "rollout_delta_rbf"]
SEEDS = {"rollout_delta": 201, "rollout_delta_mpk": 202, "rollout_delta_rbf": 203}


def dev():
    return torch.device("cuda", 0)


def T(a):
    return torch.as_tensor(np.asarray(a), dtype=DT)


def G(a):
    return T(a).to(dev()).contiguous()


def relerr(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=float)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def abserr(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=float)
    return float(np.max(np.abs(a - np.asarray(b, dtype=float))))


def _poly(fx, g):
    ws = [fx["poly_w%d_gp%d" % (k, g)] for k in (1, 2) if "poly_w%d_gp%d" % (k, g) in fx]
    return ws or None


def delta_packed_model(fx):
    from gpu_helpers import spec_from
    from mc_pilco_amd import ops

    S = fx["states"].shape[2]
    gps = [ops.PackedGP(spec_from(fx["lengthscales"], float(fx["sigma_n"]), 1.0, _poly(fx, g)), G(fx["Xtr%d" % g]), G(fx["alpha%d" % g]),
                        G(fx["Kinv%d" % g])) for g in range(S)]
    U = fx["inputs"].shape[2]
    return ops.PackedModel.delta(gps, S, U, [int(i) for i in fx["angle"]], [int(i) for i in fx["not_angle"]])


def cartpole_policy(fx):
    from mc_pilco_amd import ops

    log_ls = torch.log(G(fx["pol_ls"])).reshape(-1).contiguous().requires_grad_(True)
    centers = G(fx["pol_centers"]).requires_grad_(True)
    weight = G(fx["pol_weight"]).requires_grad_(True)
    return ops.PackedPolicy("angles", 4, log_ls, centers, weight, 10.0, True, angle=[2], non_angle=[0, 1, 3])


def cartpole_cost():
    from mc_pilco_amd import ops

    return ops.PackedCost("cartpole", 4, dev(), target_state=[np.pi, 0.0], lengthscales=[3.0, 1.0], angle_index=2, pos_index=0)


def test_delta_descriptor_layout():
    """PackedModel.delta: G = S, vel = 0..S-1, every not_vel written as -1 (the ctypes default 0 would be a valid position)."""
    from gpu_helpers import spec_from
    from mc_pilco_amd import ops

    gp = ops.PackedGP(spec_from(np.ones(6), 0.1), G(np.zeros((16, 6))), G(np.zeros(16)), G(np.eye(16)))
    m = ops.PackedModel.delta([gp] * 4, 4, 1, [2], [0, 1, 3])
    assert m.is_delta and m.G == 4
    assert [m.c.vel[g] for g in range(4)] == [0, 1, 2, 3]
    assert [m.c.not_vel[g] for g in range(4)] == [-1] * 4
    with pytest.raises(ValueError):
        ops.PackedModel.delta([gp] * 3, 4, 1, [2], [0, 1, 3])


# ---- (a) every kernel variant against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ppw", VARIANTS)
@pytest.mark.parametrize("name", DELTA_FIXTURES)
def test_delta_rollout_every_variant(golden, name, ppw):
    from gpu_helpers import forced_variant, noise_from
    from mc_pilco_amd import hipabi, ops

    fx = golden(name)
    model = delta_packed_model(fx)
    pol = cartpole_policy(fx)
    x0 = G(fx["states"][0])
    Tn, p = fx["states"].shape[0], float(fx["p_drop"])
    L = hipabi.lib()
    with forced_variant(ppw) as fv:
        st, inp, status = ops.rollout(model, pol, noise_from(fx), x0, Tn, p)
        c, s = ops.expected_cost(cartpole_cost(), st)
        c.backward()
        fv.check(sharding_optional=True)
        ran = dict(ppw=L.mcp_debug_last_particles_per_wg(), sharded=L.mcp_debug_last_gp_sharded(), lean=L.mcp_debug_last_fwd_lean())
    print("%s variant %d ran %s" % (name, ppw, ran))
    if ppw:  # the forced tile size ran; a GP-sharded request the dispatch cannot take for this model runs unsharded (recorded above)
        assert ran["ppw"] == ppw % 100
        if ppw < 100:
            assert not ran["sharded"]
    assert int(status.item()) == 0
    assert abserr(st, fx["states"]) < 1e-9
    assert abserr(inp, fx["inputs"]) < 1e-9
    assert abs(float(c) - float(fx["cost"])) < 1e-11 * abs(float(fx["cost"]))
    assert abs(float(s) - float(fx["std"])) < 1e-10 * max(abs(float(fx["std"])), 1e-3)
    assert relerr(pol.log_ls.grad, fx["g_log_ls"]) < 1e-8
    assert relerr(pol.centers.grad, fx["g_centers"]) < 1e-8
    assert relerr(pol.weight.grad, fx["g_weight"]) < 1e-8


@pytest.mark.parametrize("lean,bwd", [(1, 0), (0, 0), (0, 1), (0, 4)])
@pytest.mark.parametrize("name", DELTA_FIXTURES)
def test_delta_backward_forms(golden, name, lean, bwd):
    """The backward sweep forced to each form: the latency-lean sweep (rollout_bwd_lat_kernel: G <= 4, S <= 8) and the wide one
    (rollout_bwd_kernel), automatic or with 1 / 4 particles per workgroup."""
    from gpu_helpers import forced_variant, noise_from
    from mc_pilco_amd import hipabi, ops

    fx = golden(name)
    model = delta_packed_model(fx)
    pol = cartpole_policy(fx)
    Tn, p = fx["states"].shape[0], float(fx["p_drop"])
    L = hipabi.lib()
    try:
        L.mcp_debug_set_bwd_lean(-1 if lean else 0)
        with forced_variant(0, bwd_particles=bwd):
            st, inp, status = ops.rollout(model, pol, noise_from(fx), G(fx["states"][0]), Tn, p)
            c, s = ops.expected_cost(cartpole_cost(), st)
            c.backward()
        assert L.mcp_debug_last_bwd_lean() == lean
    finally:
        L.mcp_debug_set_bwd_lean(-1)
    assert int(status.item()) == 0
    assert abserr(st, fx["states"]) < 1e-9
    assert relerr(pol.log_ls.grad, fx["g_log_ls"]) < 1e-8
    assert relerr(pol.centers.grad, fx["g_centers"]) < 1e-8
    assert relerr(pol.weight.grad, fx["g_weight"]) < 1e-8


# ---- (b) drop-in: the project's own MC_PILCO with a delta model -----------------------------------------------------------------------
def build_delta_model(fx, states_tr=None, inputs_tr=None):
    from mc_pilco_amd.model_learning import Model_learning as ML

    S, sig, ls = fx["states"].shape[2], float(fx["sigma_n"]), fx["lengthscales"]
    D = len(ls)
    with contextlib.redirect_stdout(io.StringIO()):
        if len(fx["angle"]) == 0:
            ml = ML.Model_learning_RBF(num_gp=S, init_dict_list=[rbf_dict(D, ls, sig)] * S, dtype=DT, device=dev())
        elif _poly(fx, 0) is None:
            ml = ML.Model_learning_RBF_angle_state(num_gp=S, init_dict_list=[rbf_dict(D, ls, sig)] * S, angle_indeces=[2], not_angle_indeces=[0, 1, 3],
                                                   dtype=DT, device=dev())
        else:
            ml = ML.Model_learning_RBF_MPK_angle_state(num_gp=S, init_dict_list=[[rbf_dict(D, ls, sig), mpk_dict(D, 2, _poly(fx, g))] for g in range(S)],
                                                       angle_indeces=[2], not_angle_indeces=[0, 1, 3], dtype=DT, device=dev())
        ml.add_data(fx["states_tr"] if states_tr is None else states_tr, fx["inputs_tr"] if inputs_tr is None else inputs_tr)
        with torch.no_grad():
            for g in range(S):
                ml.pretrain_gp(g)
        ml.set_eval_mode()
    return ml


def build_mcpilco(fx, ml, pms=False):
    from mc_pilco_amd.policy_learning import MC_PILCO, Cost_function, Policy

    B = fx["pol_centers"].shape[0]
    ppar = dict(state_dim=4, input_dim=1, num_basis=B, angle_indices=np.array([2]), non_angle_indices=np.array([0, 1, 3]),
                lengthscales_init=fx["pol_ls"].reshape(-1), centers_init=fx["pol_centers"], weight_init=fx["pol_weight"], flg_squash=True,
                u_max=10.0, flg_drop=True, dtype=DT, device=dev())
    kw = dict(T_sampling=0.05, state_dim=4, input_dim=1, f_sim=lambda y, t, u: None, f_model_learning=lambda **k: ml, model_learning_par={},
              f_rand_exploration_policy=Policy.Random_exploration, rand_exploration_policy_par=dict(state_dim=4, input_dim=1, u_max=1.0, dtype=DT),
              f_control_policy=Policy.Sum_of_gaussians_with_angles, control_policy_par=ppar, f_cost_function=Cost_function.Cart_pole_cost,
              cost_function_par=dict(target_state=T([np.pi, 0.0]), lengthscales=T([3.0, 1.0]), angle_index=2, pos_index=0), log_path=None,
              dtype=DT, device=dev())
    with contextlib.redirect_stdout(io.StringIO()):
        if pms:
            return MC_PILCO.MC_PILCO4PMS(pos_indeces=[0, 2], vel_indeces=[1, 3], std_meas_noise=np.array([1e-3, 1e-3, 2e-3, 2e-3]),
                                         filtering_dict={"fc": 0.5}, **kw)
        return MC_PILCO.MC_PILCO(**kw)


def _apply(obj, fx, M=None, Tn=None):
    return obj.apply_policy(particles_initial_state_mean=T(fx["x0_mean"]), particles_initial_state_var=T(fx["x0_var"]), flg_particles_init_uniform=False,
                            particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
                            num_particles=fx["states"].shape[1] if M is None else M, T_control=fx["states"].shape[0] if Tn is None else Tn,
                            p_dropout=float(fx["p_drop"]))


@pytest.mark.parametrize("name", DELTA_FIXTURES)
def test_delta_dropin_mcpilco_matches_reference(golden, name):
    fx = golden(name)
    ml = build_delta_model(fx)
    assert ml.has_fused_layout()
    for g in range(4):  # pretrain on the device reproduces the reference's cached operands
        assert relerr(ml.alpha_list[g], fx["alpha%d" % g]) < 1e-8
    obj = build_mcpilco(fx, ml)
    obj.noise_mode = "reference"
    torch.manual_seed(SEEDS[name])
    st, inp = _apply(obj, fx)
    assert obj.last_status is not None  # the fused launch ran
    cost, std = obj.cost_function(st, inp, 0)
    cost.backward()
    assert int(obj.last_status.reshape(-1)[0].item()) == 0
    assert np.array_equal(st[0].detach().cpu().numpy(), fx["states"][0])
    assert abserr(st, fx["states"]) < 1e-8
    assert abserr(inp, fx["inputs"]) < 1e-8
    assert abs(float(cost) - float(fx["cost"])) < 1e-10 * abs(float(fx["cost"]))
    pol = obj.control_policy
    assert relerr(pol.log_lengthscales.grad, fx["g_log_ls"]) < 1e-7
    assert relerr(pol.centers.grad, fx["g_centers"]) < 1e-7
    assert relerr(pol.f_linear.weight.grad, fx["g_weight"]) < 1e-7


def test_delta_layout_invalidated_by_pretrain(golden):
    fx = golden("rollout_delta")
    ml = build_delta_model(fx)
    pm = ml.packed()
    assert ml.packed() is pm and pm.is_delta
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        ml.pretrain_gp(0)
    assert ml.packed() is not pm


# ---- (c) real size, teacher-forced ------------------------------------------------------------------------------------------------------
def test_delta_real_size_teacher_forced(golden):
    """4 GPs, N = 300, M = 400, T = 150, reference-mode noise: every fused x_{t+1} equals x_t + mu(z_t) + sqrt(var(z_t)) eps_t with the
    single-step posterior (ops.posterior) on the fused x_t, u_t; u_t equals the policy on x_t with the step's mask."""
    from mc_pilco_amd import ops
    from mc_pilco_amd import synthetic as sy

    fx = golden("rollout_delta")
    cp = sy.cartpole_rollouts()
    x = np.concatenate([r[0] for r in cp], 0)[:301]
    u = np.concatenate([r[1] for r in cp], 0)[:301]
    ml = build_delta_model(fx, x, u)
    assert all(ml.packed_gp(g).N == 300 for g in range(4))
    obj = build_mcpilco(fx, ml)
    obj.noise_mode = "reference"
    M, Tn = 400, 150
    torch.manual_seed(7)
    with torch.no_grad():
        st, inp = _apply(obj, fx, M=M, Tn=Tn)
    assert int(obj.last_status.reshape(-1)[0].item()) == 0
    # replay the reference-mode draws (apply_policy: eps0, mask_0, then per step eps_t, mask_t)
    torch.manual_seed(7)
    B = fx["pol_centers"].shape[0]
    p = float(fx["p_drop"])
    torch.empty(M, 4, dtype=DT).normal_()
    masks = [torch.empty(M, 1, B, dtype=DT).bernoulli_(1 - p).reshape(M, B)]
    eps = []
    for _ in range(1, Tn):
        eps.append(torch.empty(M, 4, dtype=DT).normal_())
        masks.append(torch.empty(M, 1, B, dtype=DT).bernoulli_(1 - p).reshape(M, B))
    eps = torch.stack(eps).to(dev())
    xs, us = st[:-1].reshape(-1, 4), inp[:-1].reshape(-1, 1)
    z = ml.data_to_gp_input(xs, us)
    nxt = []
    for g in range(4):
        mu, var = ops.posterior(ml.packed_gp(g), z)
        nxt.append(mu.reshape(-1) + torch.sqrt(var.reshape(-1)) * eps[:, :, g].reshape(-1))
    pred = xs + torch.stack(nxt, 1)
    # (mu = m + k.alpha cancels at N = 300: the fused and the single-step kernel sum it in different orders -- the posterior bound of
    # test_gpu_parity, rel 1e-10 of the terms, is a few 1e-10 here)
    assert float((pred - st[1:].reshape(-1, 4)).abs().max()) < 1e-9
    from oracle import mcpilco_oracle as orc

    pp = orc.PolicyPar(torch.log(T(fx["pol_ls"])).reshape(1, -1), T(fx["pol_centers"]), T(fx["pol_weight"]), 10.0, "angles", angle=[2],
                       non_angle=[0, 1, 3])
    for t in range(Tn):
        u_t = orc.policy_forward(pp, st[t].detach().cpu(), t, masks[t], p)
        assert float((u_t - inp[t].detach().cpu()).abs().max()) < 1e-9


# ---- (d) the optimizer loop: synchronous, pipelined and HIP-graph attempts take the same steps ----------------------------------------
def test_delta_reinforce_policy_loops_agree(golden):
    """30 steps of reinforce_policy with a delta model: the synchronous loop, the pipelined one and the pipelined one replaying its attempts
    from HIP graphs give the same cost list and final parameters, bit for bit (x0's moments on the device: nothing to upload in a capture)."""
    fx = golden("rollout_delta")
    out = []
    for depth, capture in ((0, False), (1, False), (1, True)):
        ml = build_delta_model(fx)
        obj = build_mcpilco(fx, ml)
        obj.noise_mode = "philox"
        obj.pipeline_depth = depth
        obj.capture_attempts = capture
        torch.manual_seed(1234)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = obj.reinforce_policy(T_control=0.5, num_particles=48, trial_index=0, particles_initial_state_mean=G(fx["x0_mean"]),
                                       particles_initial_state_var=G(fx["x0_var"]), flg_particles_init_uniform=False, particles_init_up_bound=None,
                                       particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
                                       f_optimizer="lambda p, lr : torch.optim.Adam(p, lr)", opt_steps_list=[30], lr_list=[0.01],
                                       p_dropout_list=[0.25], num_step_print=100)
        assert obj.last_status is not None  # the fused rollout ran
        if capture:
            assert obj.attempts_replayed > 0, buf.getvalue()[-2000:]
        pol = obj.control_policy
        out.append((np.asarray(res[0]), [q.detach().cpu().numpy().copy() for q in (pol.log_lengthscales, pol.centers, pol.f_linear.weight)]))
    c0, p0 = out[0]
    assert c0.shape == (30,) and np.isfinite(c0).all()
    for c, prm in out[1:]:
        assert np.array_equal(c, c0)
        for a, b in zip(prm, p0):
            assert np.array_equal(a, b)


# ---- (e) particle sharding over two ranks -----------------------------------------------------------------------------------------------
def _shard_run(rank, world, port, out_q, fx):
    import mcp_boot  # noqa: F401

    torch.cuda.set_device(dev())
    with rank_group(rank, world, port) as group:
        ml = build_delta_model(fx)
        obj = build_mcpilco(fx, ml)
        obj.noise_mode = "philox"
        if world > 1:
            obj.shard_particles(group)
        M, Tn = 48, 10
        torch.manual_seed(3)
        st, inp = _apply(obj, fx, M=M, Tn=Tn)
        cost, std, flags = obj._cost_backward(st, inp, 0)
        torch.cuda.synchronize()
        pol = obj.control_policy
        res = (float(cost), float(std), [q.grad.cpu().numpy().copy() for q in (pol.log_lengthscales, pol.centers, pol.f_linear.weight)],
               st.detach().cpu().numpy(), obj._shard[0], obj._shard[1])
        if rank == 0:
            out_q.put(res)


def test_delta_two_rank_sharding_matches_single_process(golden):
    fx = dict(golden("rollout_delta"))
    c1, s1, g1, st1, _, _ = run_ranks(_shard_run, 1, args=(fx,))[0]
    c2, s2, g2, st2, off, cnt = run_ranks(_shard_run, 2, args=(fx,), expect=1)[0]
    assert cnt < st1.shape[1]
    assert np.array_equal(st2, st1[:, off:off + cnt])  # same noise per GLOBAL particle
    assert abs(c2 - c1) < 1e-13 * abs(c1)
    assert abs(s2 - s1) < 1e-10 * abs(s1)
    for a, b in zip(g2, g1):
        assert np.max(np.abs(a - b)) < 1e-12 * max(1.0, np.max(np.abs(b)))


# ---- (f) MC_PILCO4PMS with a delta model: fused against the step-wise path -----------------------------------------------------------
def test_delta_pms_fused_matches_stepwise(golden):
    fx = golden("rollout_delta")
    res = []
    for fused in (True, False):
        ml = build_delta_model(fx)
        obj = build_mcpilco(fx, ml, pms=True)
        obj.noise_mode = "reference"
        obj.fused = fused
        torch.manual_seed(41)
        st, inp = _apply(obj, fx)
        assert (obj.last_status is not None) == fused
        cost, std = obj.cost_function(st, inp, 0)
        cost.backward()
        pol = obj.control_policy
        res.append((st.detach().cpu(), inp.detach().cpu(), float(cost), [q.grad.detach().cpu() for q in (pol.log_lengthscales, pol.centers,
                                                                                                       pol.f_linear.weight)]))
    (sf, uf, cf, gf), (ss, us, cs, gs) = res
    assert float((sf - ss).abs().max()) < 1e-9
    assert float((uf - us).abs().max()) < 1e-9
    assert abs(cf - cs) < 1e-11 * abs(cs)
    for a, b in zip(gf, gs):
        assert relerr(a, b) < 1e-8
