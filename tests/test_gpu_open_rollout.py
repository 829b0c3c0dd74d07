"""GPU: the fused open-loop rollout (mcp_rollout_open, ops.rollout_open) -- against the reference's fixtures, the oracle's step loops, the
closed-loop kernels at the sizes that ship, and through MC_PILCO.rollout / rollout_ensemble."""
import contextlib
import io

import numpy as np
import pytest
import torch

from helpers import T as CT, hyper, oracle_model
from oracle import mcpilco_oracle as orc

pytestmark = pytest.mark.gpu
DT = torch.float64
quiet = lambda: contextlib.redirect_stdout(io.StringIO())


def dev():
    return torch.device("cuda", 0)


def G(a):
    return torch.as_tensor(np.asarray(a), dtype=DT).to(dev()).contiguous()


def err(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.max(np.abs(a - b)))


# ---- 1. the reference's own mean rollout ---------------------------------------------------------------------------------------------
def test_mean_mode_matches_the_reference_fixture(golden):
    """tests/golden/mean_rollout.npz (MC_PILCO.rollout of the reference) through the operator, at the tolerances of the step-wise test on
    the same file (test_gpu_dropin.test_mean_rollout_matches_reference: 1e-8 full length, 1e-9 at T_rollout = 12)."""
    from mc_pilco_amd import ops
    from test_gpu_dropin import build_cartpole

    fx = golden("mean_rollout")
    model = build_cartpole(fx, 0, False).packed()
    for n, key, tol in ((fx["x_rec"].shape[0], "traj", 1e-8), (12, "traj12", 1e-9)):
        st, status = ops.rollout_open(model, G(fx["x_rec"][0:1]), G(fx["u_rec"][:n - 1]))
        e = err(st[:, 0, :], fx[key])
        print("mean_rollout T=%d: %.3e" % (n, e))
        assert int(status.item()) == 0 and st.shape == (n, 1, 4) and e < tol


# ---- 2. the oracle's step loops, both families, all degrees -------------------------------------------------------------------------
def _delta_oracle(fx):
    S = fx["states"].shape[2]
    ws = lambda g: [fx["poly_w%d_gp%d" % (k, g)] for k in (1, 2) if "poly_w%d_gp%d" % (k, g) in fx] or None
    hyp = [hyper(fx["lengthscales"], float(fx["sigma_n"]), 1.0, ws(g)) for g in range(S)]
    cache = [orc.GPCache(CT(fx["Xtr%d" % g]), CT(fx["alpha%d" % g]), CT(fx["Kinv%d" % g]), torch.zeros(fx["Xtr%d" % g].shape[0], 1, dtype=DT), None)
             for g in range(S)]
    return orc.DeltaModel(hyp, cache, [int(i) for i in fx["angle"]], [int(i) for i in fx["not_angle"]])


def _oracle_loop(step, m, x0, u, eps, sample):
    xs, mus, vrs = [CT(x0)], [], []
    for t in range(u.shape[0]):
        nx, mu, var = step(m, xs[-1], CT(u[t]), CT(eps[t]) if sample else None, sample)
        xs.append(nx)
        mus.append(mu)
        vrs.append(var)
    return torch.stack(xs), torch.stack(mus), torch.stack(vrs)


CASES = [("rollout_se", "se"), ("rollout_se_poly2", "se"), ("rollout_ur5", "ur5"), ("rollout_delta", "delta"), ("rollout_delta_mpk", "delta"),
         ("rollout_delta_rbf", "delta")]


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("name,kind", CASES)
def test_against_the_oracle_loops(golden, name, kind, sample):
    """Cart-pole SE and SE + poly(2), the D = 24 six-GP shape with SE + poly(1), the delta model with angles (SE, SE + poly(1, 2)) and
    without: the open-loop kernel on the reference's recorded inputs against a loop over orc.next_state / orc.delta_next_state on the
    same operands (the fixture's Kinv / alpha) and the same eps.  1e-9 on states, means and variances: the bound test_gpu_parity /
    test_gpu_delta_rollout hold the closed-loop forward to on these very fixtures (same model, N, T).  Sampled, the trajectories are also the
    reference's own recorded ones (the policy's inputs are fed back as data)."""
    from mc_pilco_amd import ops

    fx = golden(name)
    if kind == "delta":
        from test_gpu_delta_rollout import delta_packed_model

        model, m, step = delta_packed_model(fx), _delta_oracle(fx), orc.delta_next_state
    else:
        from gpu_helpers import packed_model

        model, m, step = packed_model(fx, kind), oracle_model(fx, kind), orc.next_state
    x0, u, eps = fx["states"][0], fx["inputs"][:-1], fx["eps"]
    ost, omu, ovar = _oracle_loop(step, m, x0, u, eps, sample)
    st, mu, var, status = ops.rollout_open(model, G(x0), G(u), noise=ops.NoiseSpec(eps=G(eps)), particle_pred=sample, moments=True)
    es, em, ev = err(st, ost), err(mu, omu), err(var, ovar)
    print("%s sample=%d: states %.3e mu %.3e var %.3e" % (name, sample, es, em, ev))
    assert int(status.item()) == 0
    assert es < 1e-9 and em < 1e-9 and ev < 1e-9
    if sample:
        assert err(st, fx["states"]) < 1e-9
    else:  # the mean chain alone (no Kinv read: the one-trajectory-per-workgroup kernel) gives the same trajectories
        st1, status1 = ops.rollout_open(model, G(x0), G(u))
        assert int(status1.item()) == 0 and err(st1, ost) < 1e-9


# ---- 2b. the oracle's step loop at the real sizes, on the oracle's own Kinv / alpha -------------------------------------------------
@pytest.mark.parametrize("key,tol", [("se300", 1e-9), ("sep1_300", 1e-9), ("sep2_300", 1e-9), ("ur5_400", 1e-9), ("sep2_1100", 2e-8), ("se1500", 2e-8)])
def test_against_the_oracle_loop_at_real_sizes(key, tol):
    """test_gpu_realsize's builders: the oracle's own pretrain (N = 300 SE / SE + poly(1) / SE + poly(2), N = 400 D = 24 six GPs, N = 1100 and
    1500) packed into the HIP descriptors, the oracle's x0, eps and (closed-loop) inputs as data.  Mean chain without moments (one
    trajectory per workgroup; at the UR5 shape with X^T and alpha in global memory), mean with moments and sampled (16 trajectories per
    workgroup, 4 beyond ~1000 rows) against a loop over orc.next_state: states, mu and var at the bound test_gpu_realsize holds the
    closed-loop forward to on the same key (1e-9 states; 2e-8 beyond 1024 rows).  Sampled, the states are also the oracle's own closed-loop
    trajectories."""
    from mc_pilco_amd import ops
    from test_gpu_realsize import Tt, hip_workload_on_oracle_operands, one_cpu_thread, oracle_answer

    o = oracle_answer(key)
    w = hip_workload_on_oracle_operands(key)
    pb, c = o["problem"], o["problem"]["cfg"]
    hyp = []
    for g in range(c["G"]):
        pw = None if pb["poly"] is None else [torch.log(Tt(q)) for q in pb["poly"][g]]
        hyp.append(orc.GPHyper(torch.log(Tt(c["lengthscales"])), torch.log(Tt([c["lam"]])), torch.log(Tt([c["sigma_n"]])), poly_log_par=pw))
    m = orc.SpeedModel(hyp, o["caches"], c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    x0, u, eps = o["x0"].numpy(), o["inputs"][:-1].numpy(), o["eps"].numpy()
    for sample in (False, True):
        with one_cpu_thread():
            ost, omu, ovar = _oracle_loop(orc.next_state, m, x0, u, eps, sample)
        st, mu, var, status = ops.rollout_open(w.model, G(x0), G(u), noise=ops.NoiseSpec(eps=G(eps)), particle_pred=sample, moments=True)
        es, em, ev = err(st, ost), err(mu, omu), err(var, ovar)
        print("real size %s sample=%d: states %.3e mu %.3e var %.3e" % (key, sample, es, em, ev))
        assert int(status.item()) == 0
        assert es < tol and em < tol and ev < tol
        if sample:
            assert err(st, o["states"]) < tol
        else:
            st1, status1 = ops.rollout_open(w.model, G(x0), G(u))
            e1 = err(st1, ost)
            print("real size %s mean chain alone: states %.3e" % (key, e1))
            assert int(status1.item()) == 0 and e1 < tol


def test_every_training_set_size_the_limits_allow():
    """N = MCP_MAX_TRAIN = 4096 (4 trajectories per workgroup: the k panel of 16 does not fit the LDS): the first step's mean and variance
    against the posterior written out in torch (fp64) on a synthetic, well-scaled SE model -- X uniform, alpha ~ N(0, 1) / N,
    Kinv = I / N, so every sum has 4096 terms of total magnitude O(1) and the worst-case rounding of either side is N eps sum|terms| ~ 1e-12:
    bound 1e-10.  The mean chain alone (no Kinv) gives the same states."""
    from gpu_helpers import spec_from
    from mc_pilco_amd import hipabi, ops

    N, M = hipabi.MAX_TRAIN, 6
    gen = torch.Generator().manual_seed(3)
    X = G(torch.rand(N, 6, dtype=DT, generator=gen) * 2 - 1)
    ls = [np.ones(6) * 1.5, np.linspace(1.0, 2.0, 6)]
    al = [G(torch.randn(N, dtype=DT, generator=gen) / N) for _ in range(2)]
    gps = [ops.PackedGP(spec_from(ls[g], 0.1), X, al[g], G(torch.eye(N, dtype=DT) / N)) for g in range(2)]
    model = ops.PackedModel(gps, 4, 1, 0.05, [2], [0, 1, 3], [1, 3], [0, 2])
    x0 = G(torch.rand(M, 4, dtype=DT, generator=gen) - 0.5)
    u = G(torch.rand(1, M, 1, dtype=DT, generator=gen))
    st, mu, var, status = ops.rollout_open(model, x0, u, moments=True)
    assert int(status.item()) == 0
    z = torch.cat([x0[:, [0, 1, 3]], torch.sin(x0[:, [2]]), torch.cos(x0[:, [2]]), u[0]], 1)
    for g in range(2):
        k = torch.exp(-(((z[:, None, :] - X[None, :, :]) / G(ls[g])) ** 2).sum(2))  # [M, N], lambda = 1
        em, ev = err(mu[0, :, g], k @ al[g]), err(var[0, :, g], 1.0 - (k * k).sum(1) / N)
        print("N=4096 GP %d: mu %.3e var %.3e" % (g, em, ev))
        assert em < 1e-10 and ev < 1e-10
    st1, status1 = ops.rollout_open(model, x0, u)
    assert int(status1.item()) == 0 and err(st1, st) < 1e-10


# ---- 3. against the closed-loop kernels at the sizes that ship ---------------------------------------------------------------------
@pytest.mark.parametrize("wl,N,M,Tn,full", [("c1", 300, 400, 150, 1e-6), ("ur5_script", 400, 200, 200, 2e-8), ("c1", 1100, 48, 10, 2e-8)])
def test_against_the_closed_loop_kernels(wl, N, M, Tn, full):
    """ops.rollout_forward_raw with an eps buffer, its inputs and x0 fed to the open-loop kernel with the same eps.  The two kernels sum
    in different orders, so they agree to rounding grown by the dynamics: over the first 10 steps 2e-8, the bound of the existing
    variant-against-variant comparisons at 10 steps (test_gpu_parity.test_two_launch_sharding_matches_the_unsharded_kernels, N = 300; the
    oracle bound at N = 1100 / 1500 is 2e-8 as well).  Over the full horizon: the cart-pole's 150 steps 1e-6, the bound test_gpu_realsize holds
    the 150-step rollout at the real N to (no variant-against-variant comparison exists at that length); the UR5 shape (its
    tracked trajectories do not amplify rounding) and the 10-step N = 1100 case stay at 2e-8 over all rows.

    Measured on an MI355X (first 10 rows / all rows): cart-pole N = 300, M = 400, T = 150 8.5e-10 / 6.4e-7; UR5 shape 6.6e-11 / 9.3e-10;
    N = 1100 4.5e-9.  The full-horizon figure of the cart-pole case is rounding grown by 150 steps of dynamics over the most sensitive of 400
    particles: pairs of the closed-loop kernels themselves (forced variants 1 / 4 / 16 and the automatic one, same x0 and eps) end 1.6e-7 ..
    1.4e-6 apart there while every pair stays below 1.5e-7 up to step 100.  With the weighted distance in its difference form the open-loop kernel
    was equally close up to step 100 and ended 2.7e-6 away on one particle; it now uses the reference's expanded form like the closed-loop
    kernels (csrc/rollout_open.hip, phase K)."""
    from gpu_helpers import forced_variant
    from mc_pilco_amd import ops, workloads

    w = workloads.build(wl, device=dev(), M=M, T=Tn, N=N)
    torch.manual_seed(3)
    x0 = w.sample_x0()
    eps = torch.randn(Tn - 1, M, w.model.G, dtype=DT, device=dev())
    with torch.no_grad():
        st, inp, _, status = ops.rollout_forward_raw(w.model, w.policy, ops.NoiseSpec(eps=eps, seed=1, call=1), x0, Tn, 0.0, True, need_jac=False)
        so, status_o = ops.rollout_open(w.model, x0, inp[:-1].contiguous(), noise=ops.NoiseSpec(eps=eps), particle_pred=True)
        # (measured only: how far two closed-loop kernels -- the automatic choice and the 16-particle tile kernel -- are from each other here)
        with forced_variant(16):
            s16 = ops.rollout_forward_raw(w.model, w.policy, ops.NoiseSpec(eps=eps, seed=1, call=1), x0, Tn, 0.0, True, need_jac=False)[0]
    e10, efull = err(so[:10], st[:10]), err(so, st)
    print("%s N=%d M=%d T=%d: first 10 rows %.3e, all rows %.3e; closed-loop automatic vs 16-particle kernel: %.3e / %.3e"
          % (wl, N, M, Tn, e10, efull, err(s16[:10], st[:10]), err(s16, st)))
    assert int(status.item()) == 0 and int(status_o.item()) == 0
    assert e10 < 2e-8 and efull < full


# ---- 4 .. 7: properties -------------------------------------------------------------------------------------------------------------
def _tiny(name="tiny", **kw):
    from mc_pilco_amd import workloads

    return workloads.build(name, device=dev(), **kw)


def test_ragged_lengths_and_shared_inputs():
    from mc_pilco_amd import ops

    w = _tiny(N=100)
    Tn, lens = 12, [12, 7, 2]
    torch.manual_seed(1)
    x0 = w.sample_x0(3)
    u = torch.randn(Tn - 1, 3, w.model.U, dtype=DT, device=dev())
    for sample in (False, True):
        nz = lambda off: ops.NoiseSpec(seed=5, call=2, particle_offset=off)
        st, mu, var, status = ops.rollout_open(w.model, x0, u, lengths=lens, noise=nz(0), particle_pred=sample, moments=True)
        assert int(status.item()) == 0
        for m, n in enumerate(lens):
            one, mu1, var1, _ = ops.rollout_open(w.model, x0[m:m + 1], u[:n - 1, m:m + 1], noise=nz(m), particle_pred=sample, moments=True)
            assert torch.equal(st[:n, m], one[:, 0]) and torch.equal(mu[:n - 1, m], mu1[:, 0]) and torch.equal(var[:n - 1, m], var1[:, 0])
            assert float(st[n:, m].abs().max()) == 0.0 if n < Tn else True
        # inputs beyond a length are never read: poisoning them changes nothing
        up = u.clone()
        up[6:, 1] = float("nan")
        up[1:, 2] = float("nan")
        st2, status2 = ops.rollout_open(w.model, x0, up, lengths=lens, noise=nz(0), particle_pred=sample)
        assert int(status2.item()) == 0 and torch.equal(st2, st)
    # one shared input sequence = the same sequence replicated
    M = 37
    x0 = w.sample_x0(M)
    a, _ = ops.rollout_open(w.model, x0, u[:, 0], noise=ops.NoiseSpec(seed=2), particle_pred=True)
    b, _ = ops.rollout_open(w.model, x0, u[:, 0:1].repeat(1, M, 1), noise=ops.NoiseSpec(seed=2), particle_pred=True)
    assert torch.equal(a, b)
    a, _ = ops.rollout_open(w.model, x0, u[:, 0:1])
    b, _ = ops.rollout_open(w.model, x0, u[:, 0:1].repeat(1, M, 1))
    assert torch.equal(a, b)


def test_philox_determinism_and_shard_invariance():
    from mc_pilco_amd import ops

    w = _tiny("c1", N=120)
    M, Tn = 1000, 8
    torch.manual_seed(2)
    x0 = w.sample_x0(M)
    u = torch.randn(Tn - 1, M, 1, dtype=DT, device=dev())
    run = lambda a, b, call=4: ops.rollout_open(w.model, x0[a:b].contiguous(), u[:, a:b].contiguous(),
                                                noise=ops.NoiseSpec(seed=9, call=call, particle_offset=a), particle_pred=True)[0]
    full = run(0, M)
    assert torch.equal(full, run(0, M))
    assert torch.equal(full, torch.cat([run(0, 500), run(500, M)], 1))
    other = run(0, M, call=5)
    assert torch.equal(other[0], full[0]) and not torch.equal(other[1], full[1])


def test_the_sampler_draws_from_the_reported_moments():
    """4096 trajectories from one x0, one step: the sample mean and variance of every increment within 5 standard errors of the mean and
    variance the kernel reports (se(mean) = sigma / sqrt(M), se(var) = sigma^2 sqrt(2 / (M - 1)) for normal draws)."""
    from mc_pilco_amd import ops

    w = _tiny("c1", N=120)
    M = 4096
    x0 = w.sample_x0(1).repeat(M, 1).contiguous()
    u = torch.full((1, 1, 1), 0.7, dtype=DT, device=dev())
    st, mu, var, status = ops.rollout_open(w.model, x0, u, noise=ops.NoiseSpec(seed=31, call=1), particle_pred=True, moments=True)
    assert int(status.item()) == 0
    assert float((mu - mu[:, 0:1]).abs().max()) == 0.0 and float((var - var[:, 0:1]).abs().max()) == 0.0
    c = w.problem["cfg"]
    for g, v in enumerate(c["vel"]):
        d = (st[1, :, v] - st[0, :, v]).cpu().numpy()
        m_, s2 = float(mu[0, 0, g]), float(var[0, 0, g])
        assert s2 > 0
        assert abs(d.mean() - m_) < 5 * np.sqrt(s2 / M)
        assert abs(d.var(ddof=1) - s2) < 5 * s2 * np.sqrt(2.0 / (M - 1))


def test_status_flags():
    from mc_pilco_amd import hipabi, ops

    w = _tiny()
    x0 = w.sample_x0(5)
    u = torch.zeros(4, 5, 1, dtype=DT, device=dev())
    for sample in (False, True):
        assert int(ops.rollout_open(w.model, x0, u, particle_pred=sample)[-1].item()) == 0
        bad = x0.clone()
        bad[3, 1] = float("nan")
        assert int(ops.rollout_open(w.model, bad, u, particle_pred=sample)[-1].item()) & hipabi.STATUS_NAN
    with pytest.raises(RuntimeError, match="no gradient"):
        ops.rollout_open(w.model, x0.clone().requires_grad_(True), u)


# ---- 8. drop-in ---------------------------------------------------------------------------------------------------------------------
def _cartpole_object(golden, pms=False):
    from mc_pilco_amd import synthetic as sy
    from test_gpu_dropin import build_cartpole, build_mcpilco

    fx = golden("mean_rollout")
    ml = build_cartpole(fx, 0, False)
    pi = sy.cartpole_policy_init(B=16, seed=8)
    if pms:  # through MC_PILCO4PMS's own constructor, as test_gpu_dropin.test_pms_seed_for_seed_parity_with_reference builds it
        from mc_pilco_amd.policy_learning import MC_PILCO, Cost_function, Policy
        from test_gpu_dropin import T as TD

        c = sy.CARTPOLE
        ppar = dict(state_dim=4, input_dim=1, num_basis=16, angle_indices=np.array([2]), non_angle_indices=np.array([0, 1, 3]),
                    lengthscales_init=pi["lengthscales"].reshape(-1), centers_init=pi["centers"], weight_init=pi["weight"], flg_squash=True,
                    u_max=c["u_max"], flg_drop=True, dtype=DT, device=dev())
        with quiet():
            obj = MC_PILCO.MC_PILCO4PMS(T_sampling=c["Ts"], state_dim=4, input_dim=1, f_sim=lambda y, t, u: None, f_model_learning=lambda **kw: ml,
                                        model_learning_par={}, f_rand_exploration_policy=Policy.Random_exploration,
                                        rand_exploration_policy_par=dict(state_dim=4, input_dim=1, u_max=1.0, dtype=DT),
                                        f_control_policy=Policy.Sum_of_gaussians_with_angles, control_policy_par=ppar,
                                        f_cost_function=Cost_function.Cart_pole_cost,
                                        cost_function_par=dict(target_state=TD(c["cost_target"]), lengthscales=TD(c["cost_ls"]), angle_index=2,
                                                               pos_index=0),
                                        pos_indeces=[0, 2], vel_indeces=[1, 3], std_meas_noise=0.01 * np.ones(4), log_path=None,
                                        filtering_dict={"fc": 0.5}, dtype=DT, device=dev())
    else:
        obj = build_mcpilco(dict(pol_ls=pi["lengthscales"], pol_centers=pi["centers"], pol_weight=pi["weight"]), ml, 16)
    rec = sy.cartpole_rollouts(n_roll=3, n_step=25, seed=4)
    obj.state_samples_history = [fx["x_rec"], rec[1][0][:17], rec[2][0][:9]]
    obj.input_samples_history = [fx["u_rec"], rec[1][1][:17], rec[2][1][:9]]
    return obj, fx


@pytest.mark.parametrize("pms", [False, True])
def test_rollout_is_a_drop_in(golden, pms):
    obj, fx = _cartpole_object(golden, pms)
    with torch.no_grad(), quiet():
        fused = obj.rollout(data_collection_index=0)
        assert obj.last_open_loop_fused is True
        fused12 = obj.rollout(0, T_rollout=12)
        obj.fused_open_loop = False
        step = obj.rollout(data_collection_index=0)
        assert obj.last_open_loop_fused is False
        step12 = obj.rollout(0, T_rollout=12)
        obj.fused_open_loop = True
        obj.rollout(0, particle_pred=True)
        assert obj.last_open_loop_fused is False  # the sampled single path keeps the torch generator's order
    assert fused.shape == step.shape == fx["traj"].shape and isinstance(fused, np.ndarray)
    print("fused vs step-wise: %.3e, T=12: %.3e" % (np.abs(fused - step).max(), np.abs(fused12 - step12).max()))
    assert np.abs(fused - step).max() < 1e-8 and np.abs(fused12 - step12).max() < 1e-9
    assert np.abs(fused - fx["traj"]).max() < 1e-8 and np.abs(fused12 - fx["traj12"]).max() < 1e-9


def test_rollout_of_a_delta_model_and_of_an_overridden_step(golden):
    from mc_pilco_amd.model_learning import Model_learning as ML
    from test_gpu_dropin import rbf_dict

    obj, fx = _cartpole_object(golden)
    with quiet():
        ml = ML.Model_learning_RBF_angle_state(num_gp=4, init_dict_list=[rbf_dict(6, np.ones(6) * 2.0, 0.05)] * 4, angle_indeces=[2],
                                               not_angle_indeces=[0, 1, 3], dtype=DT, device=dev())
        ml.add_data(fx["states_tr"], fx["inputs_tr"])
        with torch.no_grad():
            for g in range(4):
                ml.pretrain_gp(g)
        ml.set_eval_mode()
    obj.model_learning = ml
    with torch.no_grad(), quiet():
        fused = obj.rollout(0, T_rollout=12)
        assert obj.last_open_loop_fused is True
        obj.fused_open_loop = False
        step = obj.rollout(0, T_rollout=12)
        obj.fused_open_loop = True
    assert fused.shape == step.shape == (12, 4) and np.abs(fused - step).max() < 1e-9

    class Mine(ML.Speed_Model_learning_RBF_angle_state):
        def get_next_state(self, current_state, current_input, particle_pred=True):
            nxt, a, b = super().get_next_state(current_state, current_input, particle_pred)
            return nxt + 1.0, a, b

    obj2, _ = _cartpole_object(golden)
    base = obj2.rollout(0, T_rollout=3)
    obj2.model_learning.__class__ = Mine
    with torch.no_grad(), quiet():
        mine = obj2.rollout(0, T_rollout=3)
    assert obj2.last_open_loop_fused is False and np.abs(mine[1] - base[1] - 1.0).max() < 1e-12
    with pytest.raises(NotImplementedError):  # the ensemble has no step-wise form: it refuses rather than simulate another model
        obj2.rollout_ensemble(0, num_particles=4)


@pytest.mark.parametrize("pms", [False, True])
def test_rollout_ensemble(golden, pms):
    obj, fx = _cartpole_object(golden, pms)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        parts = obj.rollout_ensemble(num_particles=48, seed=7)
    assert "inside mean +- 2 std" in buf.getvalue()
    assert [p.shape for p in parts] == [(25, 48, 4), (17, 48, 4), (9, 48, 4)]
    assert int(obj.last_status.item()) == 0
    for r, p in enumerate(parts):
        assert np.array_equal(p[0], np.repeat(np.asarray(obj.state_samples_history[r])[0:1], 48, 0))
        assert np.isfinite(p).all() and p[1:].std(1).max() > 0
        with quiet():
            one = obj.rollout_ensemble(r, num_particles=48, seed=7)
            other = obj.rollout_ensemble(r, num_particles=48, seed=8)
        assert np.array_equal(one, p) and not np.array_equal(other, p)
    with quiet():
        short = obj.rollout_ensemble([0, 2], num_particles=48, T_rollout=5, seed=7)
    assert [p.shape for p in short] == [(5, 48, 4), (5, 48, 4)] and np.array_equal(short[0], parts[0][:5]) and np.array_equal(short[1], parts[2][:5])
