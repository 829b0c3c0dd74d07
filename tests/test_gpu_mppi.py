"""GPU: the sampling planner -- mcp_mppi_rollout and mcp_mppi_update through ops.mppi_rollout / ops.mppi_update, the driver
policy_learning/mppi.py and Policy.MPPI_controller -- against the entries that existed before it (bit for bit) and the truth of
tests/mppi_truth.py (pinned on the CPU by tests/test_mppi_truth_cpu.py).  Models: tests/pd_models.py at the sizes of
tests/lqr_models.MODELS, H = 6.

  1. rollout bits   states == ops.rollout_open given the launch's own inputs (Mu == M) and the eps buffer repeated per candidate; candidate
                    0 == rollout_open on the shared nominal; traj_cost the same with and without the optional outputs.  K = 7, P = 3
                    sampled (M = 21: a candidate straddles the 16-tile edge), K = 19, P = 1 mean; the 4-trajectory rung at N = 1200 (the k
                    panel of 16 does not fit), as tests/test_gpu_pd_rollout.py reaches it.  The no-record ladder has no 1-trajectory
                    rung with variances; the mean form IS the 1-trajectory kernel.
  2. cost bits      traj_cost == the ascending sum over t of mcp_cost_u_fwd's costs on those states and inputs, torch.equal: TARGET + ADD
                    effort and rate, TRAJ at t0 = 2 without input terms, TARGET_QUAD + JOINT, each also under non-trivial time weights.
  3. perturbations  a = 0, no squashing, sigma = 1: inputs ARE xi.  Candidate 0 exactly 0, every p of a candidate identical, the values
                    within ULP_BOUND = 8 ulp of the 64-bit-significand truth (tests/test_gpu_noise_truth.py's bound on the eps stream:
                    the same Box-Muller on the same words), other numbers for another call, Philox == the buffer fed those xi.
  4. update         a_new, weights, cand_cost against the float64 truth on the kernel's own traj_cost and xi: max(1e-12, 64 d_ref)
                    relative to the largest entry, d_ref the float64-vs-long-double difference of the truth (tests/test_gpu_lqr.py's
                    bound and meaning); kappa 0 and 0.5, a temperature at which one weight dominates; Philox == buffer bitwise; NaN.
  5. planner        plan == the launches chained by hand, two runs bitwise equal, the nominal's cost after 5 iterations below the
                    initial one on the cases the CPU test vetted, MPPI_controller.forward_np == plan calls on the shifted warm start."""
import numpy as np
import pytest
import torch

import closed_loop_family as clf
import mppi_truth as mt
import noise_truth as nt
import pd_models
from gpu_helpers import DT, G, dev
from lqr_models import MODELS

pytestmark = pytest.mark.gpu
H = mt.H
ULP_BOUND = 8.0  # tests/test_gpu_noise_truth.py, tier a
INPUT_LAW_TOL = 1e-14  # |inputs - squash(a + sigma xi)|, absolute: a handful of roundings of an O(1) value and the kernels' tanh
ORACLE_TOL = 1e-9  # states (absolute) and trajectory costs (relative) against the oracle: the open-loop tests' bound
cid = lambda c: "-".join(str(v) for v in c)


def pair(shape, N, deg):
    return clf.pair(pd_models.build_pair, shape, N, deg, N + deg, None, pd_models.family(shape) == "delta")


def bound(d):
    return max(1e-12, 64.0 * d)


def packed_costs(spec, S, U, t0_rows=None):
    """(PackedCost, PackedCostInputs or None) of a spec of mppi_truth.cost_specs; ``t0_rows`` = (t0, rows): the trajectory cost over the
    target's rows t0 .. t0 + rows - 1 alone (what mcp_cost_u_fwd, which reads row t, is given for a plan that starts at t0)."""
    from mc_pilco_amd import ops

    if spec["kind"] == "traj":
        tg = spec["target"] if t0_rows is None else spec["target"][t0_rows[0]:t0_rows[0] + t0_rows[1]]
        pc = ops.PackedCost("traj", S, dev(), target_traj=tg, lengthscales=spec["ls"], used=spec["idx"])
    else:
        pc = ops.PackedCost("target", S, dev(), target_state=spec["target"], lengthscales=spec["ls"], active_dims=spec["idx"],
                            saturate=spec["kind"] == "target")
    cin = None
    if spec.get("u_idx") is not None:
        cin = ops.PackedCostInputs(U, dev(), spec["u_idx"], spec.get("u_ls"), spec.get("u_rate"), spec.get("u_target"), bool(spec.get("joint")))
    return pc, cin


def operands(c, K, P, seed):
    """x0 [S] within +-0.3, a [H,U] in [-1, 1], xi [H,K,U] and eps [H-1,P,G] standard normals."""
    gen = torch.Generator().manual_seed(8000 + seed)
    x0 = 0.6 * (torch.rand(c["S"], dtype=DT, generator=gen) - 0.5)
    a = torch.rand(H, c["U"], dtype=DT, generator=gen) * 2 - 1
    xi = torch.randn(H, K, c["U"], dtype=DT, generator=gen)
    eps = torch.randn(H - 1, P, c["G"], dtype=DT, generator=gen)
    return G(x0), G(a), G(xi), G(eps)


def launch(pm, c, K, P, sample, spec, seed=0, **kw):
    """One rollout-cost launch with both optional outputs; returns (mp, operands, traj_cost, states, inputs)."""
    from mc_pilco_amd import ops

    x0, a, xi, eps = operands(c, K, P, seed)
    mp = ops.PackedMPPI(K, P, H, c["U"], kw.pop("sigma", 0.3), 1.0, u_max=kw.pop("u_max", 1.0), squash=kw.pop("squash", True))
    pc, cin = packed_costs(spec, c["S"], c["U"])
    nz = ops.NoiseSpec(eps=eps) if sample else None
    J, states, inputs, status = ops.mppi_rollout(pm, mp, pc, x0, a, cost_inputs=cin, noise=nz, particle_pred=sample, xi=xi, want_states=True,
                                                 want_inputs=True, **kw)
    assert int(status.item()) == 0
    return mp, (x0, a, xi, eps, pc, cin, nz), J, states, inputs


# ---- 1. rollout bits ------------------------------------------------------------------------------------------------------------------------
def check_rollout_bits(pm, c, K, P, sample, seed):
    from mc_pilco_amd import ops

    spec = mt.cost_specs(c)["target_add"]
    mp, (x0, a, xi, eps, pc, cin, nz), J, states, inputs = launch(pm, c, K, P, sample, spec, seed)
    M = K * P
    assert tuple(states.shape) == (H, M, c["S"]) and tuple(inputs.shape) == (H, M, c["U"]) and tuple(J.shape) == (M,)
    assert bool(torch.isfinite(J).all())
    x0m = x0.reshape(1, -1).repeat(M, 1).contiguous()
    full = ops.NoiseSpec(eps=eps.repeat(1, K, 1).contiguous()) if sample else None  # trajectory k P + p meets particle p's draws
    ref, status = ops.rollout_open(pm, x0m, inputs[:H - 1].contiguous(), noise=full, particle_pred=sample)
    assert int(status.item()) == 0 and torch.equal(states, ref)
    # the inputs are the law: candidate 0 the nominal, every candidate's particles alike
    um = 1.0
    assert float((inputs[:, :P] - um * torch.tanh(a / um).unsqueeze(1)).abs().max()) < INPUT_LAW_TOL
    assert torch.equal(inputs.reshape(H, K, P, -1), inputs.reshape(H, K, P, -1)[:, :, :1].expand(H, K, P, c["U"]))
    want_u = torch.tanh(a.unsqueeze(1) + 0.3 * xi)
    want_u[:, 0] = torch.tanh(a)
    assert float((inputs.reshape(H, K, P, -1)[:, :, 0] - want_u).abs().max()) < INPUT_LAW_TOL
    # candidate 0 against the open loop on the shared nominal alone
    nom, status = ops.rollout_open(pm, x0m[:P].contiguous(), inputs[:H - 1, 0].contiguous(), noise=ops.NoiseSpec(eps=eps) if sample else None,
                                   particle_pred=sample)
    assert int(status.item()) == 0 and torch.equal(states[:, :P], nom)
    # the same costs without the optional outputs, and with one of them
    for ws, wi in ((False, False), (True, False), (False, True)):
        J2, s2, i2, status = ops.mppi_rollout(pm, mp, pc, x0, a, cost_inputs=cin, noise=nz, particle_pred=sample, xi=xi, want_states=ws, want_inputs=wi)
        assert int(status.item()) == 0 and torch.equal(J2, J) and (s2 is None) == (not ws) and (i2 is None) == (not wi)
        assert (s2 is None or torch.equal(s2, states)) and (i2 is None or torch.equal(i2, inputs))
    return J


@pytest.mark.parametrize("model", MODELS, ids=cid)
def test_rollout_bits_sampled_straddling_the_tile_edge(model):
    shape, deg, N = model
    c, m, pm = pair(shape, N, deg)
    check_rollout_bits(pm, c, 7, 3, True, N)


@pytest.mark.parametrize("model", MODELS, ids=cid)
def test_rollout_bits_mean_model(model):
    shape, deg, N = model
    c, m, pm = pair(shape, N, deg)
    check_rollout_bits(pm, c, 19, 1, False, N + 1)


def test_rollout_bits_on_the_four_trajectory_rung():
    """N = 1200: the k panel of 16 trajectories ([1200][18] doubles) does not fit the LDS, the ladder takes 4 per workgroup; K P = 6 is two
    tiles, the second ragged."""
    c, m, pm = pair("arm2", 1200, 0)
    check_rollout_bits(pm, c, 3, 2, True, 5)


def test_rollout_against_the_oracle():
    """The truth's states and costs (oracle_step, the costs written out) to the open-loop tests' 1e-9."""
    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    spec = mt.cost_specs(c)["target_add"]
    mp, (x0, a, xi, eps, pc, cin, nz), J, states, inputs = launch(pm, c, 7, 3, True, spec, 3)
    n = lambda v: v.cpu().numpy()
    u = mt.candidate_inputs(n(a), 0.3, np.concatenate([np.zeros((H, 1, c["U"])), n(xi)[:, 1:]], 1))
    x, ut = mt.oracle_states(shape, m, n(x0), u, 3, n(eps), True)
    Jt = mt.traj_costs(spec, x, ut)
    es, ej = float(np.abs(n(states) - x).max()), float(np.abs(n(J) - Jt).max() / np.abs(Jt).max())
    print("states %.3e traj_cost %.3e" % (es, ej))
    assert es < ORACLE_TOL and ej < ORACLE_TOL


# ---- 2. cost bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("name,t0", [("target_add", 0), ("traj_plain", 2), ("quad_joint", 0)])
@pytest.mark.parametrize("model,sample", [(MODELS[0], True), (MODELS[2], False)], ids=["arm2-sampled", "ur5-mean"])
def test_cost_bits_against_the_cost_kernels(model, sample, name, t0, weighted):
    from mc_pilco_amd import ops

    shape, deg, N = model
    c, m, pm = pair(shape, N, deg)
    spec = mt.cost_specs(c)[name]
    K, P = (7, 3) if sample else (19, 1)
    w = G(0.25 + np.random.default_rng(2).random(H)) if weighted else None
    mp, (x0, a, xi, eps, pc, cin, nz), J, states, inputs = launch(pm, c, K, P, sample, spec, 11, w=w, t0=t0)
    pc_rows, _ = packed_costs(spec, c["S"], c["U"], (t0, H))  # mcp_cost_u_fwd reads target row t: hand it rows t0 .. t0 + H - 1
    mom, costs, status = ops.cost_moments(pc_rows, states, inputs=None if cin is None else inputs, cost_inputs=cin)
    acc = torch.zeros_like(J)
    for t in range(H):  # ascending, one rounding per product and per sum
        acc = acc + (costs[t] if w is None else w[t] * costs[t])
    assert bool(torch.isfinite(J).all()) and float(J.abs().min()) > 0
    assert torch.equal(J, acc)
    if t0:  # the offset matters: row 0 of the target gives other costs
        J0 = ops.mppi_rollout(pm, mp, pc, x0, a, cost_inputs=cin, noise=nz, particle_pred=sample, xi=xi, w=w, t0=0)[0]
        assert not torch.equal(J0, J)
    if name == "target_add":  # against the truth's formula on the kernel's states and inputs
        Jt = mt.traj_costs(spec, states.cpu().numpy(), inputs.cpu().numpy(), None if w is None else w.cpu().numpy(), t0)
        assert float(np.abs(J.cpu().numpy() - Jt).max() / np.abs(Jt).max()) < 1e-13


def test_a_short_target_trajectory_is_refused():
    from mc_pilco_amd import ops

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    x0, a, xi, eps = operands(c, 4, 1, 0)
    pc, _ = packed_costs(mt.cost_specs(c, target_rows=7)["traj_plain"], c["S"], c["U"])
    mp = ops.PackedMPPI(4, 1, H, c["U"], 0.3, 1.0)
    with pytest.raises(ValueError, match="rows"):
        ops.mppi_rollout(pm, mp, pc, x0, a, t0=2)
    assert bool(torch.isfinite(ops.mppi_rollout(pm, mp, pc, x0, a, t0=1)[0]).all())


# ---- 3. perturbations -----------------------------------------------------------------------------------------------------------------------
def test_the_philox_perturbations_against_the_truth():
    from mc_pilco_amd import ops

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    K, P, U = 7, 3, c["U"]
    x0, a, xi, eps = operands(c, K, P, 1)
    spec = mt.cost_specs(c)["target_add"]
    pc, cin = packed_costs(spec, c["S"], U)
    mp = ops.PackedMPPI(K, P, H, U, 1.0, 1.0, squash=False)
    zero = torch.zeros_like(a)
    seen = {}
    for call, offset in ((3, 0), (4, 0), (3, 5)):
        nz = ops.NoiseSpec(eps=eps, seed=11, call=call, particle_offset=offset)
        J, _, inputs, status = ops.mppi_rollout(pm, mp, pc, x0, zero, cost_inputs=cin, noise=nz, particle_pred=True, want_inputs=True)
        assert int(status.item()) == 0
        got = inputs.reshape(H, K, P, U)
        assert not bool(got[:, 0].any())  # candidate 0 is exactly 0
        assert torch.equal(got, got[:, :, :1].expand(H, K, P, U))  # every p of a candidate
        g = got[:, :, 0].cpu().numpy()
        if nt.have_longdouble():
            ulp = float(nt.ulps(g[:, 1:], mt.xi_table(11, call, H, K, U, offset, hp=True)[:, 1:]).max())
            print("call %d offset %d: %d draws within %.3f ulp of the truth (asserted %.0f)" % (call, offset, g[:, 1:].size, ulp, ULP_BOUND))
            assert ulp <= ULP_BOUND
        else:  # numpy's double evaluation is itself within 4 ulp of that truth (tests/test_noise_truth_cpu.py)
            t64 = mt.xi_table(11, call, H, K, U, offset)[:, 1:]
            assert float((np.abs(g[:, 1:] - t64) / np.spacing(np.abs(t64))).max()) <= ULP_BOUND + 4.0
        seen[(call, offset)] = (J, got[:, :, 0].contiguous())
        if (call, offset) == (3, 0):  # the buffer mode fed those xi
            Jb = ops.mppi_rollout(pm, mp, pc, x0, zero, cost_inputs=cin, noise=ops.NoiseSpec(eps=eps), particle_pred=True, xi=seen[(3, 0)][1])[0]
            assert torch.equal(Jb, J)
    base = seen[(3, 0)][1][:, 1:]
    for other in ((4, 0), (3, 5)):
        assert float((seen[other][1][:, 1:] - base).abs().min()) > 0  # other numbers
    # the model draws are common random numbers whatever the perturbations: in Philox mode too, particle p of every candidate
    nzp = ops.NoiseSpec(seed=11, call=3)
    Jp, sp, ip, status = ops.mppi_rollout(pm, mp, pc, x0, zero, cost_inputs=cin, noise=nzp, particle_pred=True, want_states=True, want_inputs=True)
    ref, status2 = ops.rollout_open(pm, x0.reshape(1, -1).repeat(P, 1).contiguous(), ip[:H - 1, :P].contiguous(), noise=nzp, particle_pred=True)
    assert int(status.item()) == 0 and int(status2.item()) == 0 and torch.equal(sp[:, :P], ref)


# ---- 4. update ------------------------------------------------------------------------------------------------------------------------------
def check_update(what, got, J, a, sigma, xi, K, P, lam, kappa):
    n = lambda v: v.detach().cpu().numpy()
    args = (n(J), n(a), sigma, n(xi), K, P, lam, kappa)
    f64, ld = mt.update(*args), mt.update(*args, dt=np.longdouble)
    d = mt.d_ref(f64, ld)
    a_new, cand, wts, stats = got
    errs = [float(np.abs(n(g) - t).max() / np.abs(t).max()) for g, t in zip((a_new, cand, wts), f64)]
    print("%s: a_new / cand_cost / weights: d_ref %.2e %.2e %.2e, kernel vs float64 truth %.2e %.2e %.2e; largest weight %.6f"
          % ((what,) + tuple(d) + tuple(errs) + (float(f64[2].max()),)))
    for e, dr in zip(errs, d):
        assert e <= bound(dr)
    st = n(stats)
    # the statistics: S_min is an entry of cand_cost; 1 / sum w^2 and sum w S are sums of K positive terms of the weights (their bound twice:
    # the square, the product with S; K eps <= 1.4e-13 of summation below it)
    assert int(st[1]) == int(f64[3][1]) and abs(st[0] - f64[3][0]) <= bound(d[1]) * float(np.abs(f64[1]).max())
    assert abs(st[2] - f64[3][2]) <= 4 * bound(d[2]) * f64[3][2] and abs(st[3] - f64[3][3]) <= 4 * bound(d[2]) * abs(f64[3][3])
    return f64


@pytest.mark.parametrize("kappa", [0.0, 0.5])
@pytest.mark.parametrize("lam", [1.0, 0.05, 1e-3], ids=["lam1", "lam0.05", "one-weight-dominates"])
@pytest.mark.parametrize("model", [MODELS[0], MODELS[2]], ids=cid)
def test_update_against_the_truth(model, lam, kappa):
    from mc_pilco_amd import ops

    shape, deg, N = model
    c, m, pm = pair(shape, N, deg)
    K, P, U = 19, 3, c["U"]
    sigma = np.linspace(0.2, 0.5, U)
    spec = mt.cost_specs(c)["target_add"]
    mp0, (x0, a, xi, eps, pc, cin, nz), J, _, _ = launch(pm, c, K, P, True, spec, 21, sigma=sigma)
    mp = ops.PackedMPPI(K, P, H, U, sigma, lam, kappa)
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    a_new, cand, wts, stats, _ = ops.mppi_update(mp, J, a, xi=xi, status=status)
    assert int(status.item()) == 0
    f64 = check_update("%s lam %g kappa %g" % (cid(model), lam, kappa), (a_new, cand, wts, stats), J, a, sigma, xi, K, P, lam, kappa)
    if lam == 1e-3:
        assert float(wts.max()) > 0.99
    again = ops.mppi_update(mp, J, a, xi=xi)
    assert all(torch.equal(p, q) for p, q in zip(again[:4], (a_new, cand, wts, stats)))  # bitwise reproducible


def test_update_philox_equals_buffer_and_more_than_one_block_of_candidates():
    """K = 600 candidates (each of the 256 threads walks two or three), P = 1; the perturbations regenerated from (seed, call) equal the
    buffer read back from a launch that wrote them."""
    from mc_pilco_amd import ops

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    K, P, U = 600, 1, c["U"]
    x0, a, _, _ = operands(c, 1, 1, 2)
    spec = mt.cost_specs(c)["effort"]
    pc, cin = packed_costs(spec, c["S"], U)
    nz = ops.NoiseSpec(seed=5, call=9)
    raw = ops.PackedMPPI(K, P, H, U, 1.0, 1.0, squash=False)
    xi = ops.mppi_rollout(pm, raw, pc, x0, torch.zeros_like(a), cost_inputs=cin, noise=nz, want_inputs=True)[2].reshape(H, K, U).contiguous()
    mp = ops.PackedMPPI(K, P, H, U, 0.4, 0.05)
    J = ops.mppi_rollout(pm, mp, pc, x0, a, cost_inputs=cin, noise=nz)[0]
    assert torch.equal(J, ops.mppi_rollout(pm, mp, pc, x0, a, cost_inputs=cin, xi=xi)[0])
    by_philox = ops.mppi_update(mp, J, a, noise=nz)
    by_buffer = ops.mppi_update(mp, J, a, xi=xi)
    assert all(torch.equal(p, q) for p, q in zip(by_philox[:4], by_buffer[:4]))
    check_update("K 600", by_philox[:4], J, a, 0.4, xi, K, P, 0.05, 0.0)


def test_update_with_non_finite_candidates():
    from mc_pilco_amd import hipabi, ops

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    K, P, U, lam, kappa = 7, 3, c["U"], 0.7, 0.5
    spec = mt.cost_specs(c)["target_add"]
    x0, a, xi, eps = operands(c, K, P, 4)
    pc, cin = packed_costs(spec, c["S"], U)
    mp = ops.PackedMPPI(K, P, H, U, 0.3, lam, kappa)
    xi_bad = xi.clone()
    xi_bad[2, 2, 0] = float("nan")  # one entry of candidate 2's perturbation
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    J = ops.mppi_rollout(pm, mp, pc, x0, a, cost_inputs=cin, noise=ops.NoiseSpec(eps=eps), particle_pred=True, xi=xi_bad, status=status)[0]
    assert int(status.item()) & hipabi.STATUS_NAN
    assert bool(torch.isnan(J[2 * P:3 * P]).all()) and bool(torch.isfinite(torch.cat([J[:2 * P], J[3 * P:]])).all())
    status.zero_()
    a_new, cand, wts, stats, _ = ops.mppi_update(mp, J, a, xi=xi_bad, status=status)
    assert int(status.item()) == hipabi.STATUS_NAN
    assert float(wts[2]) == 0.0 and bool(torch.isnan(cand[2])) and bool(torch.isfinite(a_new).all())
    keep = [k for k in range(K) if k != 2]
    Jk = J.reshape(K, P)[keep].reshape(-1)
    n = lambda v: v.cpu().numpy()
    f64 = mt.update(n(Jk), n(a), 0.3, n(xi)[:, keep], K - 1, P, lam, kappa)
    ld = mt.update(n(Jk), n(a), 0.3, n(xi)[:, keep], K - 1, P, lam, kappa, dt=np.longdouble)
    d = mt.d_ref(f64, ld)
    assert float(np.abs(n(wts)[keep] - f64[2]).max() / f64[2].max()) <= bound(d[2])  # the weights of the problem without it
    assert float(np.abs(n(a_new) - f64[0]).max() / np.abs(f64[0]).max()) <= bound(d[0])
    assert keep[int(f64[3][1])] == int(stats[1])
    # no finite candidate: the nominal stays
    status.zero_()
    a_same, cand, wts, stats, _ = ops.mppi_update(mp, torch.full_like(J, float("nan")), a, xi=xi, status=status)
    assert int(status.item()) == hipabi.STATUS_NAN and torch.equal(a_same, a) and not bool(wts.any())
    assert float(stats[1]) == -1.0 and float(stats[2]) == 0.0 and bool(torch.isnan(stats[0])) and bool(torch.isnan(stats[3]))


# ---- 5. planner and controller --------------------------------------------------------------------------------------------------------------
def cost_object(spec):
    from mc_pilco_amd.policy_learning import Cost_function as cf

    if spec["kind"] == "traj":
        sc = cf.Expected_saturated_distance_from_trajectory(spec["target"], spec["ls"], used_indeces=spec["idx"])
    else:
        sc = (cf.Expected_saturated_distance if spec["kind"] == "target" else cf.Expected_distance)(spec["target"], spec["ls"], spec["idx"])
    if spec.get("u_idx") is None:
        return sc
    return cf.Input_penalty(sc, spec.get("u_ls"), spec.get("u_rate"), spec.get("u_target"), spec["u_idx"], bool(spec.get("joint")))


@pytest.mark.parametrize("sample", [False, True], ids=["mean", "sampled"])
def test_plan_equals_the_launches_chained_by_hand(sample):
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import mppi

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    K, P = (7, 3) if sample else (19, 1)
    x0, a, _, eps = operands(c, K, P, 6)
    spec = mt.cost_specs(c)["target_add"]
    noise = ops.NoiseSpec(eps=eps if sample else None, seed=21, call=40)
    par = dict(K=K, P=P, iterations=2, sigma=0.4, lam=0.1, kappa=0.5 if sample else 0.0, particle_pred=sample, noise=noise)
    got, info = mppi.plan(pm, x0, a, cost_object(spec), **par)
    again, info2 = mppi.plan(pm, x0, a, cost_object(spec), **par)
    assert torch.equal(got, again) and info == info2 and info["status"] == 0 and info["iterations"] == 2
    pc, cin = packed_costs(spec, c["S"], c["U"])
    mp = ops.PackedMPPI(K, P, H, c["U"], 0.4, 0.1, par["kappa"])
    cur, nominal, smin, ess = a, [], [], []
    for i in range(2):
        nz = ops.NoiseSpec(eps=noise.eps, seed=21, call=40 + i)
        J = ops.mppi_rollout(pm, mp, pc, x0, cur, cost_inputs=cin, noise=nz, particle_pred=sample)[0]
        cur, cand, wts, stats, _ = ops.mppi_update(mp, J, cur, noise=nz)
        nominal.append(float(cand[0])), smin.append(float(stats[0])), ess.append(float(stats[2]))
    assert torch.equal(got, cur) and info["nominal_cost"] == nominal and info["S_min"] == smin and info["ess"] == ess
    assert not torch.equal(got, a) and float((got - a).abs().max()) > 1e-3


@pytest.mark.parametrize("case", mt.BEHAVIOUR, ids=lambda c: "-".join(str(v) for v in c[:3]))
def test_the_planner_lowers_the_nominal_cost(case):
    """The cases tests/test_mppi_truth_cpu.py vetted on the truth alone: the nominal's cost after 5 iterations (what iteration 6 starts
    from) is below the cost of the warm start."""
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import mppi

    shape, deg, N, seed, K, sigma, lam = case
    c, m, pm = pair(shape, N, deg)
    x0, a0 = mt.behaviour_operands(c, seed)
    spec = mt.cost_specs(c)["effort"]
    a, info = mppi.plan(pm, G(x0), G(a0), cost_object(spec), K=K, P=1, iterations=mt.ITERATIONS + 1, sigma=sigma, lam=lam,
                        noise=ops.NoiseSpec(seed=seed, call=0))
    torch.set_num_threads(1)
    _, nominal, every = mt.plan_truth(shape, m, c, x0, a0, spec, K, 1, mt.ITERATIONS + 1, sigma, lam, seed=seed)
    print("%s: nominal cost per iteration %s (truth %s), ess %s" % (cid(case[:3]), ["%.6f" % v for v in info["nominal_cost"]],
                                                                    ["%.6f" % v for v in nominal], ["%.1f" % v for v in info["ess"]]))
    assert info["status"] == 0 and all(np.isfinite(info["nominal_cost"]))
    assert info["nominal_cost"][mt.ITERATIONS] < info["nominal_cost"][0]
    # the truth's planner, iteration by iteration: the open-loop tests' 1e-9 on the states moves a cost of O(1) by as much, the weights by
    # that over lam = 0.02 (5e-8, relative), and so the next nominal; five iterations of it stay below 1e-6
    assert max(abs(p - q) for p, q in zip(info["nominal_cost"], nominal)) < 1e-6


def test_the_controller_replans_from_the_shifted_warm_start():
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import Policy, mppi

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    spec = mt.cost_specs(c)["traj_plain"]  # 12 target rows: steps 0 .. 2 read rows up to 2 + H - 1
    cost = cost_object(spec)
    gen = np.random.default_rng(12)
    xs = [0.3 * (gen.random(c["S"]) - 0.5) for _ in range(3)]
    u_max = [0.8, 1.2]
    par = dict(K=19, P=1, sigma=0.4, lam=0.05)
    ctrl = Policy.MPPI_controller(c["S"], c["U"], pm, cost, horizon=H, iterations=2, noise=ops.NoiseSpec(seed=3, call=100), flg_squash=True,
                                  u_max=u_max, device=dev(), **par)
    policy = ctrl.get_np_policy()
    got = [policy(xs[k], 0.05 * k) for k in range(3)]
    a, want = torch.zeros(H, c["U"], dtype=DT, device=dev()), []
    for k in range(3):
        a, info = mppi.plan(pm, G(xs[k]), a, cost, iterations=2, u_max=u_max, flg_squash=True, noise=ops.NoiseSpec(seed=3, call=100 + 2 * k), t0=k, **par)
        um = torch.as_tensor(u_max, dtype=DT)
        want.append((um * torch.tanh(a[0].cpu() / um)).numpy().reshape(1, -1))
        a = mppi.shift_warm_start(a)
        assert torch.equal(a[-1], a[-2])
    for g, w_ in zip(got, want):
        assert g.shape == (1, c["U"]) and np.array_equal(g, w_) and np.abs(g).max() > 0
    assert ctrl.step == 3 and torch.equal(ctrl.a, a) and list(ctrl.parameters()) == [] and ctrl.info["status"] == 0
    # t = 0 starts an episode over: the same first input
    assert np.array_equal(policy(xs[0], 0.0), got[0]) and ctrl.step == 1
    # a cost that tracks nothing plans at t0 = 0 whatever the step
    still = Policy.MPPI_controller(c["S"], c["U"], pm, cost_object(mt.cost_specs(c)["effort"]), horizon=H, iterations=1, device=dev(), **par)
    for k in range(3):
        still.forward_np(xs[k], 0.05 * k)
    assert still.step == 3 and not still._tracks() and ctrl._tracks()
    with pytest.raises(ValueError, match="rows"):  # the tracked target runs out: 12 rows, step 7 would read row 12
        for k in range(1, 9):
            policy(xs[0], 0.05 * k)
    assert ctrl.step == 7
