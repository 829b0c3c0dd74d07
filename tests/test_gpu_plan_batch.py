"""GPU: the batched planner -- mcp_plan_batch_rollout, mcp_plan_batch_update and mcp_cem_batch_update through ops.plan_batch_rollout /
plan_batch_update / cem_batch_update, the driver policy_learning.mppi.plan_batch and Policy.MPPI_controller.forward -- against the
single-problem entries, whose bits tests/test_gpu_mppi.py, test_gpu_plan_ext.py and test_gpu_plan_layouts.py pin.  The contract is one
sentence: problem b's slice of every output of a batched launch carries the bits of the single-problem launch on problem b's operands with
noise.particle_offset + b * particle_stride and the b-th xi / eps buffer.  Every comparison here is therefore torch.equal; there is no
tolerance in this file except the one on the controller's last squashing (see there).  Models: tests/pd_models.py at the sizes of
tests/lqr_models.MODELS, H = 6.

  1. rollout bits     B = 3, K = 7 x P = 3 sampled (21 trajectories: every problem ends on a ragged 16-tile and the next starts on a fresh
                      one), K = 19 x P = 1 mean; plain and extended (beta 0.6, sigma_rows and u_prev per problem); Philox at particle_stride 0
                      and 1000, buffers shared and per problem; the 4-trajectory rung at N = 1200.
  2. x0 per particle  states == ops.rollout_open from the rows x0[b][m mod P]; P equal rows == the [B,S] form.
  3. update bits      MPPI plain (kappa 0, 0.5) and extended, CEM (3 of 19), K = 600 (more than one candidate per thread) with Philox.
  4. isolation        a NaN start state in problem 1 of 3: its own status word, nominal and std kept, the others bitwise untouched.
  5. driver           plan_batch == B plan calls with shifted particle_offset; B = 1 == plan; reproducible; info on the device.
  6. controller       forward on M = 5 states over 3 steps == five controllers' forward_np; MC_PILCO.apply_policy under the controller."""
import numpy as np
import pytest
import torch

import mppi_truth as mt
from gpu_helpers import DT, G, dev
from lqr_models import MODELS
from test_gpu_mppi import H, cid, cost_object, operands, packed_costs, pair

pytestmark = pytest.mark.gpu
B3 = 3
OFFSET = 5  # the launch's own particle_offset: problem b draws at OFFSET + b * stride


def batch_operands(c, B, K, P, seed):
    """B problems' operands of test_gpu_mppi.operands, stacked: x0 [B,S], a [B,H,U], xi [B,H,K,U], eps [B,H-1,P,G], and per problem a
    std [B,H,U] in (0.1, 0.5) and an input before row 0 [B,U] in (-0.5, 0.5)."""
    ops_ = [operands(c, K, P, seed + 17 * b) for b in range(B)]
    x0, a, xi, eps = (torch.stack([o[i] for o in ops_]).contiguous() for i in range(4))
    gen = torch.Generator().manual_seed(9000 + seed)
    srows = G(0.1 + 0.4 * torch.rand(B, H, c["U"], dtype=DT, generator=gen))
    uprev = G(torch.rand(B, c["U"], dtype=DT, generator=gen) - 0.5)
    return x0, a, xi, eps, srows, uprev


def noise_modes(xi, eps, sample):
    """(name, particle_stride, xi of the batch, eps of the batch, xi of problem b, NoiseSpec of problem b)"""
    from mc_pilco_amd import ops

    nz = lambda e, off=0: ops.NoiseSpec(eps=e if sample else None, seed=7, call=3, particle_offset=off)
    return (("philox-0", 0, None, None, lambda b: None, lambda b: nz(None, OFFSET)),
            ("philox-1000", 1000, None, None, lambda b: None, lambda b: nz(None, OFFSET + 1000 * b)),
            ("shared-buffers", 0, xi[0].contiguous(), eps[0].contiguous(), lambda b: xi[0].contiguous(), lambda b: nz(eps[0].contiguous(), OFFSET)),
            ("buffers-per-problem", 1000, xi, eps, lambda b: xi[b], lambda b: nz(eps[b], OFFSET + 1000 * b)))


def check_rollout_bits(pm, c, B, K, P, sample, extended, seed, modes=None):
    from mc_pilco_amd import ops

    x0, a, xi, eps, srows, uprev = batch_operands(c, B, K, P, seed)
    pc, cin = packed_costs(mt.cost_specs(c)["target_add"], c["S"], c["U"])
    mp = ops.PackedMPPI(K, P, H, c["U"], 0.3, 1.0)
    ext = ops.PackedPlanExt(H, c["U"], beta=0.6) if extended else None
    kw = dict(sigma_rows=srows, u_prev=uprev) if extended else {}
    for name, stride, bxi, beps, xi_of, nz_of in noise_modes(xi, eps, sample):
        if modes is not None and name not in modes:
            continue
        bt = ops.PackedPlanBatch(B, P, particle_stride=stride)
        nzb = ops.NoiseSpec(eps=beps if sample else None, seed=7, call=3, particle_offset=OFFSET)
        J, states, inputs, status = ops.plan_batch_rollout(pm, mp, ext, bt, pc, x0, a, cost_inputs=cin, noise=nzb, particle_pred=sample, xi=bxi,
                                                           want_states=True, want_inputs=True, **kw)
        M = K * P
        assert tuple(J.shape) == (B, M) and tuple(states.shape) == (B, H, M, c["S"]) and tuple(inputs.shape) == (B, H, M, c["U"])
        assert tuple(status.shape) == (B,) and not bool(status.any()) and bool(torch.isfinite(J).all())
        for b in range(B):
            kb = dict(sigma_rows=srows[b], u_prev=uprev[b]) if extended else {}
            J1, s1, i1, st1 = ops.plan_rollout(pm, mp, ext, pc, x0[b], a[b], cost_inputs=cin, noise=nz_of(b), particle_pred=sample, xi=xi_of(b),
                                               want_states=True, want_inputs=True, **kb)
            assert int(st1.item()) == 0
            assert torch.equal(J[b], J1) and torch.equal(states[b], s1) and torch.equal(inputs[b], i1), (name, b)
        if name != "shared-buffers":  # the problems are different problems (under shared buffers too: other x0 and nominals)
            assert not torch.equal(inputs[0], inputs[1])
        assert not torch.equal(J[0], J[1])
        J2, s2, i2, status2 = ops.plan_batch_rollout(pm, mp, ext, bt, pc, x0, a, cost_inputs=cin, noise=nzb, particle_pred=sample, xi=bxi, **kw)
        assert s2 is None and i2 is None and torch.equal(J2, J) and not bool(status2.any())


@pytest.mark.parametrize("extended", [False, True], ids=["plain", "extended"])
@pytest.mark.parametrize("model", MODELS, ids=cid)
def test_rollout_bits_sampled_ragged_tiles(model, extended):
    shape, deg, N = model
    c, m, pm = pair(shape, N, deg)
    check_rollout_bits(pm, c, B3, 7, 3, True, extended, N)


@pytest.mark.parametrize("extended", [False, True], ids=["plain", "extended"])
@pytest.mark.parametrize("model", MODELS, ids=cid)
def test_rollout_bits_mean_model(model, extended):
    shape, deg, N = model
    c, m, pm = pair(shape, N, deg)
    check_rollout_bits(pm, c, B3, 19, 1, False, extended, N + 1)


@pytest.mark.parametrize("extended", [False, True], ids=["plain", "extended"])
def test_rollout_bits_on_the_four_trajectory_rung(extended):
    """N = 1200: the ladder takes 4 trajectories per workgroup; K P = 6 is two tiles per problem, the second ragged."""
    c, m, pm = pair("arm2", 1200, 0)
    check_rollout_bits(pm, c, 2, 3, 2, True, extended, 5, modes=("philox-1000", "buffers-per-problem"))


# ---- 2. x0 per particle ---------------------------------------------------------------------------------------------------------------------
def test_a_start_state_per_model_particle():
    from mc_pilco_amd import ops

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    B, K, P = 2, 5, 3
    _, a, xi, eps, _, _ = batch_operands(c, B, K, P, 31)
    gen = torch.Generator().manual_seed(77)
    x0 = G(0.6 * (torch.rand(B, P, c["S"], dtype=DT, generator=gen) - 0.5))
    pc, cin = packed_costs(mt.cost_specs(c)["target_add"], c["S"], c["U"])
    mp = ops.PackedMPPI(K, P, H, c["U"], 0.3, 1.0)
    run = lambda bt, x: ops.plan_batch_rollout(pm, mp, None, bt, pc, x, a, cost_inputs=cin, noise=ops.NoiseSpec(eps=eps), particle_pred=True, xi=xi,
                                               want_states=True, want_inputs=True)
    J, states, inputs, status = run(ops.PackedPlanBatch(B, P, x0_per_particle=True), x0)
    assert not bool(status.any())
    for b in range(B):
        x0m = x0[b].repeat(K, 1).contiguous()  # trajectory m = k P + p starts at x0[b][m mod P]
        full = ops.NoiseSpec(eps=eps[b].repeat(1, K, 1).contiguous())
        ref, st = ops.rollout_open(pm, x0m, inputs[b, :H - 1].contiguous(), noise=full, particle_pred=True)
        assert int(st.item()) == 0 and torch.equal(states[b], ref)
        assert torch.equal(states[b, 0], x0m) and not torch.equal(x0[b, 0], x0[b, 1])
    # P equal rows: the [B,S] form
    same = x0[:, :1].expand(B, P, c["S"]).contiguous()
    Jp, sp, ip, _ = run(ops.PackedPlanBatch(B, P, x0_per_particle=True), same)
    Js, ss, is_, _ = run(ops.PackedPlanBatch(B, P), x0[:, 0].contiguous())
    assert torch.equal(Jp, Js) and torch.equal(sp, ss) and torch.equal(ip, is_) and not torch.equal(Jp, J)


# ---- 3. update bits -------------------------------------------------------------------------------------------------------------------------
def update_operands(B, K, P, U, seed):
    gen = torch.Generator().manual_seed(4000 + seed)
    J = G(0.5 + 1.5 * torch.rand(B, K * P, dtype=DT, generator=gen))
    a = G(torch.rand(B, H, U, dtype=DT, generator=gen) * 2 - 1)
    xi = G(torch.randn(B, H, K, U, dtype=DT, generator=gen))
    srows = G(0.1 + 0.4 * torch.rand(B, H, U, dtype=DT, generator=gen))
    return J, a, xi, srows


def check_update_bits(B, K, P, kind, kappa=0.0, philox=False, n_elite=3, seed=0):
    """``kind``: "plain" / "ext" (mppi_update_ext under beta 0.6 and a std per problem) / "cem"."""
    from mc_pilco_amd import ops

    U = 2
    J, a, xi, srows = update_operands(B, K, P, U, seed)
    mp = ops.PackedMPPI(K, P, H, U, [0.3, 0.4], 0.7, kappa)
    ext = None if kind == "plain" else ops.PackedPlanExt(H, U, beta=0.6, n_elite=n_elite, alpha=0.1, sigma_min=0.05)
    rows = None if kind == "plain" else srows
    modes = [("philox", 1000, None, lambda b: None)] if philox else [("shared", 0, xi[0].contiguous(), lambda b: xi[0].contiguous()), ("per-problem", 0, xi, lambda b: xi[b]),
                                                                    ("philox", 1000, None, lambda b: None)]
    for name, stride, bxi, xi_of in modes:
        bt = ops.PackedPlanBatch(B, P, particle_stride=stride)
        nzb = ops.NoiseSpec(seed=11, call=4, particle_offset=OFFSET)
        nz_of = lambda b: ops.NoiseSpec(seed=11, call=4, particle_offset=OFFSET + stride * b)
        if kind == "cem":
            got = ops.cem_batch_update(mp, ext, bt, J, a, sigma_rows=rows, noise=nzb, xi=bxi)
            one = lambda b: ops.cem_update(mp, ext, J[b], a[b], sigma_rows=rows[b], noise=nz_of(b), xi=xi_of(b))
        else:
            got = ops.plan_batch_update(mp, ext, bt, J, a, sigma_rows=rows, noise=nzb, xi=bxi)
            one = (lambda b: ops.mppi_update(mp, J[b], a[b], noise=nz_of(b), xi=xi_of(b))) if kind == "plain" else \
                  (lambda b: ops.mppi_update_ext(mp, ext, J[b], a[b], sigma_rows=rows[b], noise=nz_of(b), xi=xi_of(b)))
        assert tuple(got[-1].shape) == (B,) and not bool(got[-1].any())
        for b in range(B):
            want = one(b)
            assert int(want[-1].item()) == 0
            for g, w_ in zip(got[:-1], want[:-1]):
                assert torch.equal(g[b], w_), (kind, name, b)
        assert not torch.equal(got[0][0], got[0][1]) and not torch.equal(got[0], a)


@pytest.mark.parametrize("kappa", [0.0, 0.5])
def test_update_bits_mppi_plain(kappa):
    check_update_bits(B3, 19, 3, "plain", kappa, seed=1)


def test_update_bits_mppi_extended():
    check_update_bits(B3, 19, 3, "ext", 0.5, seed=2)


def test_update_bits_cem():
    check_update_bits(B3, 19, 3, "cem", 0.5, n_elite=3, seed=3)


@pytest.mark.parametrize("kind", ["plain", "ext", "cem"])
def test_update_bits_more_than_one_candidate_per_thread(kind):
    """K = 600: each of the 256 threads walks two or three candidates; B = 2, the perturbations regenerated under particle_stride 1000."""
    check_update_bits(2, 600, 1, kind, philox=True, n_elite=75, seed=4)


# ---- 4. isolation ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["mppi", "cem"])
def test_a_nan_start_state_stays_in_its_problem(method):
    """NaN DATA in one problem's start state, as the non-finite-candidate tests of tests/test_gpu_mppi.py use: every trajectory of problem 1
    is non-finite, so it has no finite candidate."""
    from mc_pilco_amd import hipabi, ops

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    K, P = 7, 3
    x0, a, xi, eps, srows, uprev = batch_operands(c, B3, K, P, 41)
    pc, cin = packed_costs(mt.cost_specs(c)["target_add"], c["S"], c["U"])
    mp = ops.PackedMPPI(K, P, H, c["U"], 0.3, 0.7, 0.5)
    ext = ops.PackedPlanExt(H, c["U"], beta=0.6, n_elite=3, alpha=0.1, sigma_min=0.05)
    bt = ops.PackedPlanBatch(B3, P, particle_stride=1000)
    nz = ops.NoiseSpec(seed=7, call=3, particle_offset=OFFSET)

    def run(x):
        J, _, _, st_r = ops.plan_batch_rollout(pm, mp, ext, bt, pc, x, a, sigma_rows=srows, u_prev=uprev, cost_inputs=cin, noise=nz, particle_pred=True)
        if method == "cem":
            out = ops.cem_batch_update(mp, ext, bt, J, a, sigma_rows=srows, noise=nz)
        else:
            out = ops.plan_batch_update(mp, ext, bt, J, a, sigma_rows=srows, noise=nz)
        return (J,) + tuple(out[:-1]), st_r, out[-1]

    clean, st_r0, st_u0 = run(x0)
    assert not bool(st_r0.any()) and not bool(st_u0.any())
    bad_x0 = x0.clone()
    bad_x0[1, 0] = float("nan")
    got, st_r, st_u = run(bad_x0)
    for st in (st_r, st_u):
        assert int(st[1].item()) & hipabi.STATUS_NAN and int(st[0].item()) == 0 and int(st[2].item()) == 0
    for g, w_ in zip(got, clean):  # problems 0 and 2: the bits of the batch without the NaN
        assert torch.equal(g[0], w_[0]) and torch.equal(g[2], w_[2])
    assert bool(torch.isnan(got[0][1]).all())  # every trajectory cost of problem 1
    assert torch.equal(got[1][1], a[1])  # a_new[1] == a[1]
    stats = got[-1][1]
    assert bool(torch.isnan(stats[0])) and float(stats[1]) == -1.0 and float(stats[2]) == 0.0 and bool(torch.isnan(stats[3]))
    if method == "cem":
        a_new, sigma_new, cand, elite = got[1:5]
        assert torch.equal(sigma_new[1], srows[1]) and bool((elite[1] == -1).all()) and bool((elite[0] >= 0).all())
    else:
        assert not bool(got[3][1].any())  # the weights of problem 1


# ---- 5. driver ------------------------------------------------------------------------------------------------------------------------------
def plan_cases(c, B, K, P, seed):
    x0, a, _, _, srows, uprev = batch_operands(c, B, K, P, seed)
    return x0, a, srows.cpu().numpy(), uprev


@pytest.mark.parametrize("sample", [False, True], ids=["mean", "sampled"])
@pytest.mark.parametrize("method", ["mppi", "cem"])
def test_plan_batch_equals_the_plans_one_by_one(method, sample):
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import mppi

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    K, P = (7, 3) if sample else (19, 1)
    x0, a, srows, uprev = plan_cases(c, B3, K, P, 51)
    cost = cost_object(mt.cost_specs(c)["target_add"])
    par = dict(K=K, P=P, iterations=3, sigma=0.4, lam=0.1, kappa=0.5 if sample else 0.0, particle_pred=sample, method=method)
    if method == "cem":
        par.update(n_elite=3, alpha=0.1, sigma_min=0.05, beta=0.6)
    noise = lambda off: ops.NoiseSpec(seed=21, call=40, particle_offset=off)
    got, info = mppi.plan_batch(pm, x0, a, cost, noise=noise(OFFSET), sigma_rows=srows if method == "cem" else None,
                                u_prev=uprev if method == "cem" else None, **par)
    assert tuple(got.shape) == (B3, H, c["U"]) and info["iterations"] == 3
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for k, v in info.items() if k != "iterations")  # nothing was read back
    assert tuple(info["S_min"].shape) == (3, B3) and tuple(info["status"].shape) == (B3,) and not bool(info["status"].any())
    stride = max(K, P)  # the default: independent numbers per problem
    for b in range(B3):
        kw = dict(sigma_rows=srows[b], u_prev=uprev[b]) if method == "cem" else {}
        one, inf1 = mppi.plan(pm, x0[b], a[b], cost, noise=noise(OFFSET + b * stride), **dict(par, **kw))
        assert torch.equal(got[b], one) and inf1["status"] == 0
        keys = ("S_min", "nominal_cost") + (("elite_cost", "n_elite_used") if method == "cem" else ("ess", "mean_cost"))
        for k in keys:
            assert info[k][:, b].tolist() == inf1[k], (k, b)
        if method == "cem":
            assert torch.equal(info["sigma"][b], inf1["sigma"]) and [[k for k in row if k >= 0] for row in info["elite"][:, b].tolist()] == inf1["elite"]
    assert not torch.equal(got[0], got[1]) and not torch.equal(got, a)
    again, info2 = mppi.plan_batch(pm, x0, a, cost, noise=noise(OFFSET), sigma_rows=srows if method == "cem" else None,
                                   u_prev=uprev if method == "cem" else None, **par)
    assert torch.equal(again, got) and all(torch.equal(info[k], info2[k]) for k in info if k != "iterations")
    # B = 1 is plan; a shared warm start [H,U] is every problem's; stride 0 gives every problem the same numbers
    one, inf1 = mppi.plan(pm, x0[0], a[0], cost, noise=noise(OFFSET), **par)
    b1, _ = mppi.plan_batch(pm, x0[:1], a[0], cost, noise=noise(OFFSET), **par)
    assert torch.equal(b1[0], one)
    crn, _ = mppi.plan_batch(pm, x0[:1].repeat(2, 1), a[0], cost, noise=noise(OFFSET), particle_stride=0, **par)
    assert torch.equal(crn[0], one) and torch.equal(crn[1], one)


# ---- 6. controller --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("charge", [False, True], ids=["plain", "charge-first-rate"])
def test_the_controller_plans_for_m_states_at_once(charge):
    """forward on M = 5 states over 3 steps against five controllers' forward_np, each fed the states its row was given and built with
    noise.particle_offset + b * particle_stride.  The PLANS agree bit for bit (the warm starts both sides carry into the next step: rows
    1 .. H-1 of every plan; the next plan depends on all of them).  The returned input is the plan's row 0 squashed: forward squashes on the
    device, forward_np on the host, so the two are compared within 4 ulp of u_max (two correctly-rounded-to-an-ulp tanh evaluations of the
    same argument and one product each), and forward's own result against its formula, exactly."""
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import Policy

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    Mn, steps, stride = 5, 3, 64
    cost = cost_object(mt.cost_specs(c)["traj_plain" if not charge else "target_add"])  # (a tracked target: t0 = the step; a rate term: u_prev matters)
    u_max = [0.8, 1.2]
    par = dict(K=19, P=1, sigma=0.4, lam=0.05)
    build = lambda off, **kw: Policy.MPPI_controller(c["S"], c["U"], pm, cost, horizon=H, iterations=2,
                                                     noise=ops.NoiseSpec(seed=3, call=100, particle_offset=off), flg_squash=True, u_max=u_max, device=dev(),
                                                     charge_first_rate=charge, **dict(par, **kw))
    ctrl = build(OFFSET, particle_stride=stride)
    singles = [build(OFFSET + b * stride) for b in range(Mn)]
    gen = torch.Generator().manual_seed(12)
    um = G(np.asarray(u_max))
    for k in range(steps):
        X = G(0.3 * (torch.rand(Mn, c["S"], dtype=DT, generator=gen) - 0.5))
        u = ctrl.forward(X, t=k)
        assert tuple(u.shape) == (Mn, c["U"]) and u.is_cuda and not u.requires_grad and not bool(ctrl.batch_info["status"].any())
        for b in range(Mn):
            u1 = singles[b].forward_np(X[b].cpu().numpy(), 0.05 * k)
            assert torch.equal(ctrl._batch_a[b], singles[b].a), (k, b)
            assert singles[b].info["nominal_cost"] == ctrl.batch_info["nominal_cost"][:, b].tolist()
            assert float(np.abs(u[b].cpu().numpy() - u1.reshape(-1)).max()) <= 4 * np.spacing(max(u_max))
        assert float(u.abs().max()) > 0 and not torch.equal(u[0], u[1])
    # the last squashing, against the update's own formula on the plan's row 0 (re-planned from the same warm start: a fresh episode's step 0)
    fresh = build(OFFSET, particle_stride=stride)
    X0 = G(0.3 * (torch.rand(Mn, c["S"], dtype=DT, generator=torch.Generator().manual_seed(12)) - 0.5))
    u0 = fresh.forward(X0, t=0)
    from mc_pilco_amd.policy_learning import mppi

    a0, _ = mppi.plan_batch(pm, X0, torch.zeros(H, c["U"], dtype=DT), cost, iterations=2, u_max=u_max, flg_squash=True,
                            noise=ops.NoiseSpec(seed=3, call=100, particle_offset=OFFSET), t0=0, particle_stride=stride, **par)
    assert torch.equal(u0, um * torch.tanh(a0[:, 0] / um)) and torch.equal(fresh._batch_a, mppi.shift_warm_start(a0))
    assert ctrl.step == 0 and singles[0].step == steps  # forward's episode is its own


def test_mc_pilco_simulates_the_controller_on_particles(golden):
    """MC_PILCO.apply_policy under an MPPI_controller: the generic loop with ``fused_step`` (one launch per model step) calls forward on the
    [M,S] batch each step -- MPC simulated on M particles of the model.  The inputs it returns are the controller's: a fresh controller of
    the same construction, fed the returned states, gives them back bit for bit."""
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import Policy
    from test_gpu_dropin import T as TD
    from test_gpu_open_rollout import _cartpole_object, quiet

    obj, _ = _cartpole_object(golden, False)
    Mn, Tn = 5, 4
    build = lambda: Policy.MPPI_controller(4, 1, obj.model_learning, obj.cost_function, horizon=H, iterations=2, noise=ops.NoiseSpec(seed=9, call=50),
                                           flg_squash=True, u_max=10.0, device=dev(), K=32, P=1, sigma=2.0, lam=0.05)
    obj.control_policy = build()
    obj.fused_step = True
    torch.manual_seed(3)
    with quiet(), torch.no_grad():
        st, inp = obj.apply_policy(particles_initial_state_mean=TD(np.array([0.0, 0.0, 0.1, 0.0])), particles_initial_state_var=TD(1e-2 * np.ones(4)),
                                   flg_particles_init_uniform=False, particles_init_up_bound=None, particles_init_low_bound=None,
                                   flg_particles_init_multi_gauss=False, num_particles=Mn, T_control=Tn)
    assert tuple(st.shape) == (Tn, Mn, 4) and tuple(inp.shape) == (Tn, Mn, 1) and obj.last_step_fused is True and obj.last_feedback_fused is False
    assert bool(torch.isfinite(st).all()) and float(inp.abs().max()) > 0 and float(inp.abs().max()) <= 10.0
    fresh = build()
    for t in range(Tn):
        assert torch.equal(fresh.forward(st[t], t=t), inp[t]), t
    assert not bool(fresh.batch_info["status"].any())
