"""GPU: the planner's extension -- mcp_plan_rollout, mcp_mppi_update_ext and mcp_cem_update through ops.plan_rollout / mppi_update_ext /
cem_update, ``mppi.plan(method="cem", beta, sigma_rows, u_prev)`` and ``Policy.MPPI_controller(charge_first_rate)`` -- against the entries
that existed before it (bit for bit) and the truth of tests/cem_truth.py (pinned on the CPU by tests/test_cem_truth_cpu.py).  Models:
tests/pd_models.py at the sizes of tests/lqr_models.MODELS, H = 6, as tests/test_gpu_mppi.py.

  1. default ext     ext None, an ext with every field at its default, an ext that sets only what the CEM update reads: traj_cost, states,
                     inputs, a_new, weights, cand_cost and stats torch.equal to mcp_mppi_rollout / mcp_mppi_update.
  2. coloured rows   a = 0, no squashing, random sigma_rows, beta = 0.5: inputs == s xi, xi the numpy recursion on the kernel's own white
                     draws (a beta = 0, sigma = 1 launch) within 16 * 2^-52 * max(1, max |xi|) -- at most two roundings per row over 6 rows,
                     numpy has no fma, s <= 1 --; candidate 0 exactly 0; Philox == the buffer fed the white draws; states == ops.rollout_open
                     on the launch's own inputs.  The 16-tile straddle, the mean form, the 4-trajectory rung at N = 1200.
  3. u_prev          traj_cost == the ascending sum of rows 1 .. H of mcp_cost_u_fwd run on H + 1 rows whose row 0 is a dummy state with
                     u_prev as its input (ADD effort + rate, JOINT); without a rate term u_prev changes no bit.
  4. ext update      against the float64 truth on the kernel's own costs and white draws, max(1e-12, 64 d_ref).
  5. CEM update      elite EXACTLY the truth's ranking of the kernel's own cand_cost; a_new, sigma_new within max(1e-12, 64 d_ref).
  6. planner         plan(method="cem") == the launches chained by hand; the vetted cases; every iteration's elite set == the truth's.
  7. controller      charge_first_rate hands over exactly the input returned last; everything default: today's arrays."""
import numpy as np
import pytest
import torch

import cem_truth as ct
import mppi_truth as mt
from gpu_helpers import DT, G, dev
from lqr_models import MODELS
from test_gpu_mppi import bound, cid, cost_object, operands, packed_costs, pair

pytestmark = pytest.mark.gpu
H = mt.H
n_ = lambda v: v.detach().cpu().numpy()
FORMS = [(MODELS[0], 7, 3, True), (MODELS[2], 19, 1, False), (("arm2", 0, 1200), 3, 2, True)]
FORM_IDS = ["straddle-16", "mean", "four-rung-N1200"]


def white_draws(pm, c, K, P, nz, sample):
    """[H, K, U]: the kernel's own white normals of (seed, call) -- the inputs of a beta = 0, sigma = 1, a = 0 launch without squashing."""
    from mc_pilco_amd import ops

    pc, cin = packed_costs(mt.cost_specs(c)["effort"], c["S"], c["U"])
    raw = ops.PackedMPPI(K, P, H, c["U"], 1.0, 1.0, squash=False)
    x0 = torch.zeros(c["S"], dtype=DT, device=dev())
    inputs = ops.mppi_rollout(pm, raw, pc, x0, torch.zeros(H, c["U"], dtype=DT, device=dev()), cost_inputs=cin, noise=nz, particle_pred=sample,
                              want_inputs=True)[2]
    return inputs.reshape(H, K, P, c["U"])[:, :, 0].contiguous()


def rel(got, want):
    return float(np.abs(n_(got) - want).max() / np.abs(want).max())


# ---- 1. default ext -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,P,sample", [(7, 3, True), (19, 1, False)], ids=["sampled", "mean"])
def test_a_default_ext_is_the_old_entries(K, P, sample):
    from mc_pilco_amd import ops

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    x0, a, xi, eps = operands(c, K, P, 31)
    pc, cin = packed_costs(mt.cost_specs(c)["target_add"], c["S"], c["U"])
    mp = ops.PackedMPPI(K, P, H, c["U"], 0.3, 0.7, 0.5 if sample else 0.0)
    for buf in (xi, None):
        nz = ops.NoiseSpec(eps=eps if sample else None, seed=4, call=2)
        kw = dict(cost_inputs=cin, noise=nz, particle_pred=sample, xi=buf, want_states=True, want_inputs=True)
        J, st, inp, status = ops.mppi_rollout(pm, mp, pc, x0, a, **kw)
        old = ops.mppi_update(mp, J, a, noise=nz, xi=buf)
        assert int(status.item()) == 0
        for ext in (None, ops.PackedPlanExt(H, c["U"]), ops.PackedPlanExt(H, c["U"], n_elite=3, alpha=0.3, sigma_min=0.1)):
            J2, st2, inp2, status = ops.plan_rollout(pm, mp, ext, pc, x0, a, **kw)
            assert int(status.item()) == 0 and torch.equal(J2, J) and torch.equal(st2, st) and torch.equal(inp2, inp)
            new = ops.mppi_update_ext(mp, ext, J, a, noise=nz, xi=buf)
            assert all(torch.equal(p, q) for p, q in zip(new[:4], old[:4]))


# ---- 2. coloured perturbations, a std per row -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,K,P,sample", FORMS, ids=FORM_IDS)
def test_coloured_inputs_with_a_std_per_row(model, K, P, sample):
    from mc_pilco_amd import ops

    shape, deg, N = model
    c, m, pm = pair(shape, N, deg)
    U, M, beta = c["U"], K * P, 0.5
    x0, a, _, eps = operands(c, K, P, 5)
    nz = ops.NoiseSpec(eps=eps if sample else None, seed=13, call=6)
    white = white_draws(pm, c, K, P, nz, sample)
    assert not bool(white[:, 0].any()) and float(white[:, 1:].abs().min()) > 0
    s = 0.2 + 0.7 * np.random.default_rng(N).random((H, U))  # <= 1: the bound on xi holds for s xi
    pc, cin = packed_costs(mt.cost_specs(c)["target_add"], c["S"], U)
    mp = ops.PackedMPPI(K, P, H, U, 0.3, 1.0, squash=False)
    ext = ops.PackedPlanExt(H, U, beta=beta, sigma_rows=s)
    zero = torch.zeros_like(a)
    kw = dict(cost_inputs=cin, particle_pred=sample, want_states=True, want_inputs=True)
    J, states, inputs, status = ops.plan_rollout(pm, mp, ext, pc, x0, zero, noise=nz, **kw)
    assert int(status.item()) == 0 and bool(torch.isfinite(J).all())
    got = inputs.reshape(H, K, P, U)
    assert not bool(got[:, 0].any())  # candidate 0 is exactly 0
    assert torch.equal(got, got[:, :, :1].expand(H, K, P, U))
    xi = ct.colour(n_(white), beta)
    err, tol = float(np.abs(n_(got[:, :, 0]) - s[:, None, :] * xi).max()), 16 * 2.0 ** -52 * max(1.0, float(np.abs(xi).max()))
    print("%s: |inputs - s xi| %.3e (asserted %.3e), max |xi| %.3f" % (cid(model), err, tol, float(np.abs(xi).max())))
    assert err <= tol
    assert float(np.abs(n_(got[:, 1:, 0]) - s[:, None, :] * n_(white)[:, 1:]).max()) > 1e-3  # (and not the white draws)
    # Philox == the buffer fed the white draws
    Jb, sb, ib, status = ops.plan_rollout(pm, mp, ext, pc, x0, zero, noise=ops.NoiseSpec(eps=eps if sample else None), xi=white, **kw)
    assert int(status.item()) == 0 and torch.equal(Jb, J) and torch.equal(sb, states) and torch.equal(ib, inputs)
    # beta = 0 under a std per row: the white draws' bits times s
    e0 = ops.PackedPlanExt(H, U, sigma_rows=s)
    i0 = ops.plan_rollout(pm, mp, e0, pc, x0, zero, noise=nz, **kw)[2].reshape(H, K, P, U)[:, :, 0]
    assert torch.equal(i0, G(s).unsqueeze(1) * white)
    # the states are the open loop's on the launch's own inputs (squashed, around a nominal that is not zero)
    mq = ops.PackedMPPI(K, P, H, U, 0.3, 1.0)
    J, states, inputs, status = ops.plan_rollout(pm, mq, ext, pc, x0, a, noise=nz, **kw)
    full = ops.NoiseSpec(eps=eps.repeat(1, K, 1).contiguous()) if sample else None
    ref, status2 = ops.rollout_open(pm, x0.reshape(1, -1).repeat(M, 1).contiguous(), inputs[:H - 1].contiguous(), noise=full, particle_pred=sample)
    assert int(status.item()) == 0 and int(status2.item()) == 0 and torch.equal(states, ref)
    want_u = torch.tanh(a.unsqueeze(1) + G(s).unsqueeze(1) * G(xi))
    assert float((inputs.reshape(H, K, P, U)[:, :, 0] - want_u).abs().max()) < 1e-14
    # traj_cost does not depend on the optional outputs
    assert torch.equal(ops.plan_rollout(pm, mq, ext, pc, x0, a, noise=nz, cost_inputs=cin, particle_pred=sample)[0], J)


# ---- 3. the input applied before row 0 ------------------------------------------------------------------------------------------------------
def joint_rate_spec(c):
    return dict(mt.cost_specs(c)["target_add"], joint=True)


@pytest.mark.parametrize("name", ["target_add", "joint_rate"])
@pytest.mark.parametrize("model,K,P,sample", FORMS[:2], ids=FORM_IDS[:2])
def test_the_rate_term_at_row_zero_is_taken_against_u_prev(model, K, P, sample, name):
    from mc_pilco_amd import ops

    shape, deg, N = model
    c, m, pm = pair(shape, N, deg)
    U, M = c["U"], K * P
    spec = joint_rate_spec(c) if name == "joint_rate" else mt.cost_specs(c)[name]
    x0, a, xi, eps = operands(c, K, P, 17)
    pc, cin = packed_costs(spec, c["S"], U)
    mp = ops.PackedMPPI(K, P, H, U, 0.3, 1.0)
    nz = ops.NoiseSpec(eps=eps) if sample else None
    u_prev = G(np.tanh(np.random.default_rng(3).standard_normal(U)))
    kw = dict(cost_inputs=cin, noise=nz, particle_pred=sample, xi=xi)
    for ext in (None, ops.PackedPlanExt(H, U, beta=0.5, sigma_rows=np.full((H, U), 0.25))):
        J, states, inputs, status = ops.plan_rollout(pm, mp, ext, pc, x0, a, u_prev=u_prev, want_states=True, want_inputs=True, **kw)
        J_without = ops.plan_rollout(pm, mp, ext, pc, x0, a, **kw)[0]
        assert int(status.item()) == 0 and not torch.equal(J, J_without)
        rows_x = torch.cat([x0.reshape(1, 1, -1).expand(1, M, -1), states]).contiguous()  # row 0: a dummy state
        rows_u = torch.cat([u_prev.reshape(1, 1, -1).expand(1, M, -1), inputs]).contiguous()
        mom, costs, status = ops.cost_moments(pc, rows_x, inputs=rows_u, cost_inputs=cin)
        acc = torch.zeros_like(J)
        for t in range(1, H + 1):
            acc = acc + costs[t]
        assert bool(torch.isfinite(J).all()) and torch.equal(J, acc)
        # rows 1 .. H - 1 are what they were: only row 0's cost moved
        assert torch.equal(ops.plan_rollout(pm, mp, ext, pc, x0, a, u_prev=u_prev, want_inputs=True, **kw)[2], inputs)


def test_u_prev_changes_no_bit_without_a_rate_term():
    from mc_pilco_amd import ops

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    K, P, U = 7, 3, c["U"]
    x0, a, xi, eps = operands(c, K, P, 18)
    u_prev = G(np.array([0.7, -0.4])[:U])
    mp = ops.PackedMPPI(K, P, H, U, 0.3, 1.0)
    for name in ("effort", "traj_plain"):  # an effort term alone; no input terms at all
        pc, cin = packed_costs(mt.cost_specs(c)[name], c["S"], U)
        kw = dict(cost_inputs=cin, noise=ops.NoiseSpec(eps=eps), particle_pred=True, xi=xi, want_states=True, want_inputs=True)
        old = ops.mppi_rollout(pm, mp, pc, x0, a, **kw)
        new = ops.plan_rollout(pm, mp, None, pc, x0, a, u_prev=u_prev, **kw)
        assert all(torch.equal(p, q) for p, q in zip(old[:3], new[:3]))


# ---- 4. the MPPI update under the extension -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_row", [False, True], ids=["sigma", "sigma_rows"])
@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("K,P", [(19, 3), (600, 1)])
def test_ext_update_against_the_truth(K, P, beta, per_row):
    from mc_pilco_amd import ops

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    U, sample, lam, kappa = c["U"], P > 1, 0.05, 0.5 if P > 1 else 0.0
    x0, a, _, eps = operands(c, K, P, 22)
    nz = ops.NoiseSpec(eps=eps if sample else None, seed=5, call=9)
    white = white_draws(pm, c, K, P, nz, sample)
    sigma = np.linspace(0.2, 0.5, U)
    s = 0.2 + 0.5 * np.random.default_rng(K).random((H, U)) if per_row else None
    pc, cin = packed_costs(mt.cost_specs(c)["target_add"], c["S"], U)
    mp = ops.PackedMPPI(K, P, H, U, sigma, lam, kappa)
    ext = ops.PackedPlanExt(H, U, beta=beta, sigma_rows=s)
    J, _, _, status = ops.plan_rollout(pm, mp, ext, pc, x0, a, cost_inputs=cin, noise=nz, particle_pred=sample)
    by_philox = ops.mppi_update_ext(mp, ext, J, a, noise=nz, status=status)
    by_buffer = ops.mppi_update_ext(mp, ext, J, a, xi=white)
    assert int(status.item()) == 0 and all(torch.equal(p, q) for p, q in zip(by_philox[:4], by_buffer[:4]))
    args = (n_(J), n_(a), sigma if s is None else s, n_(white), K, P, lam, kappa, beta)
    f64, ld = ct.update_ext(*args), ct.update_ext(*args, dt=np.longdouble)
    d = mt.d_ref(f64, ld)
    errs = [rel(g, t) for g, t in zip(by_philox[:3], f64)]
    print("K %d beta %g rows %s: a_new / cand_cost / weights: d_ref %.2e %.2e %.2e, kernel vs float64 truth %.2e %.2e %.2e"
          % ((K, beta, per_row) + tuple(d) + tuple(errs)))
    for e, dr in zip(errs, d):
        assert e <= bound(dr)
    assert float((by_philox[0] - a).abs().max()) > 1e-3
    if beta != 0.0 or per_row:  # and not the plain update's result
        assert not torch.equal(ops.mppi_update(mp, J, a, noise=nz)[0], by_philox[0])


# ---- 5. the CEM update ----------------------------------------------------------------------------------------------------------------------
def check_cem(what, got, J, a, s, white, K, P, E, alpha, smin, beta, kappa=0.0):
    """elite exactly the truth's ranking of the kernel's own cand_cost; a_new, sigma_new against the float64 truth fitted to that ranking."""
    a_new, s_new, cand, elite, stats = got[:5]
    el = [k for k in elite.cpu().tolist() if k >= 0]
    Sk = n_(cand)
    want = ct.elites_by_sort(Sk, E)
    assert el == want and elite.cpu().tolist()[len(el):] == [-1] * (E - len(el)), what
    args = (n_(J), n_(a), s, n_(white), K, P, E, alpha, smin, beta, kappa)
    f64, ld = ct.cem_update(*args, elite=el), ct.cem_update(*args, dt=np.longdouble, elite=el)
    d = ct.d_ref2(f64, ld)
    errs = [rel(a_new, f64[0]), rel(s_new, f64[1])]
    print("%s: a_new / sigma_new: d_ref %.2e %.2e, kernel vs float64 truth %.2e %.2e; E' %d" % ((what,) + tuple(d) + tuple(errs) + (len(el),)))
    assert errs[0] <= bound(d[0]) and errs[1] <= bound(d[1])
    fin = np.isfinite(Sk)
    assert np.array_equal(fin, np.isfinite(f64[2])) and float(np.abs(Sk[fin] - f64[2][fin]).max()) <= 1e-12 * float(np.abs(Sk[fin]).max())
    st = n_(stats)
    assert st[0] == Sk[el[0]] and int(st[1]) == el[0] and int(st[2]) == len(el) and abs(st[3] - f64[4][3]) <= 1e-12 * abs(f64[4][3])
    return f64


@pytest.mark.parametrize("alpha,beta", [(0.0, 0.0), (0.3, 0.0), (0.0, 0.5), (0.3, 0.5)])
@pytest.mark.parametrize("K,P,E", [(19, 3, 5), (257, 1, 32), (600, 1, 60), (19, 1, 19), (19, 3, 1)], ids=["19-3-5", "257-1-32", "600-1-60", "E-is-K-19", "E-1"])
def test_cem_update_against_the_truth(K, P, E, alpha, beta):
    from mc_pilco_amd import ops

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    U, sample, kappa = c["U"], P > 1, 0.5 if P > 1 else 0.0
    x0, a, _, eps = operands(c, K, P, 23)
    nz = ops.NoiseSpec(eps=eps if sample else None, seed=6, call=1)
    white = white_draws(pm, c, K, P, nz, sample)
    s = 0.2 + 0.5 * np.random.default_rng(K + E).random((H, U))
    s[0, U - 1] = 0.01  # a std so small that the floor of the last input is active there whatever the elites' spread (v <= max xi^2 < 900)
    smin = np.array([0.0, 0.3])[-U:]
    pc, cin = packed_costs(mt.cost_specs(c)["target_add"], c["S"], U)
    mp = ops.PackedMPPI(K, P, H, U, 0.3, 1.0, kappa)
    ext = ops.PackedPlanExt(H, U, beta=beta, sigma_rows=s, n_elite=E, alpha=alpha, sigma_min=smin)
    J, _, _, status = ops.plan_rollout(pm, mp, ext, pc, x0, a, cost_inputs=cin, noise=nz, particle_pred=sample)
    got = ops.cem_update(mp, ext, J, a, noise=nz, status=status)
    assert int(status.item()) == 0
    f64 = check_cem("K %d P %d E %d alpha %g beta %g" % (K, P, E, alpha, beta), got, J, a, s, white, K, P, E, alpha, smin, beta, kappa)
    assert float(got[1][0, U - 1]) == 0.3 and float(f64[1][0, U - 1]) == 0.3
    again, by_buffer = ops.cem_update(mp, ext, J, a, noise=nz), ops.cem_update(mp, ext, J, a, xi=white)
    for other in (again, by_buffer):  # bitwise reproducible; Philox == the buffer
        assert all(torch.equal(p, q) for p, q in zip(other[:5], got[:5]))
    # the same std handed over as a device buffer in place of the descriptor's own
    e2 = ops.PackedPlanExt(H, U, beta=beta, n_elite=E, alpha=alpha, sigma_min=smin)
    assert all(torch.equal(p, q) for p, q in zip(ops.cem_update(mp, e2, J, a, sigma_rows=G(s), noise=nz)[:5], got[:5]))


def synthetic(K, U, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(H, U, dtype=DT, generator=gen) * 2 - 1
    white = torch.randn(H, K, U, dtype=DT, generator=gen)
    white[:, 0] = 0
    return G(a), G(white), gen


def test_cem_update_at_the_largest_plan():
    """K = 65536 candidates, E = 1024 elites, synthetic costs (the update alone: no rollout): every thread of the select walks 256
    candidates, the sort fills its 1024 slots, every thread of the fit carries four chains."""
    from mc_pilco_amd import hipabi, ops

    K, U, E = hipabi.MPPI_MAX_K, 2, hipabi.CEM_MAX_ELITE
    a, white, gen = synthetic(K, U, 1)
    J = G(2.0 + torch.randn(K, dtype=DT, generator=gen))
    mp = ops.PackedMPPI(K, 1, H, U, [0.3, 0.4], 1.0)
    ext = ops.PackedPlanExt(H, U, beta=0.5, n_elite=E, alpha=0.1, sigma_min=0.05)
    got = ops.cem_update(mp, ext, J, a, xi=white)
    assert int(got[5].item()) == 0
    check_cem("K 65536 E 1024", got, J, a, np.array([0.3, 0.4]), white, K, 1, E, 0.1, 0.05, 0.5)
    assert all(torch.equal(p, q) for p, q in zip(ops.cem_update(mp, ext, J, a, xi=white)[:5], got[:5]))


@pytest.mark.parametrize("K,E", [(19, 5), (300, 75), (300, 150), (1024, 256)], ids=["19-5", "300-75", "300-150", "1024-256"])
def test_cem_update_with_equal_costs_across_the_elite_boundary(K, E):
    """Four distinct costs over K candidates (a signed zero among them): the boundary falls inside a run of equals and the lower k wins."""
    from mc_pilco_amd import ops

    U = 2
    a, white, gen = synthetic(K, U, 2 + K)
    vals = torch.tensor([-1.5, -0.0, 0.0, 2.5], dtype=DT)
    J = G(vals[torch.randint(0, 4, (K,), generator=gen)])
    mp = ops.PackedMPPI(K, 1, H, U, 0.3, 1.0)
    ext = ops.PackedPlanExt(H, U, n_elite=E, alpha=0.0)
    got = ops.cem_update(mp, ext, J, a, xi=white)
    f64 = check_cem("ties K %d E %d" % (K, E), got, J, a, 0.3, white, K, 1, E, 0.0, 0.0, 0.0)
    el, Sk = got[3].cpu().tolist(), n_(got[2])
    assert all((Sk[p], p) < (Sk[q], q) for p, q in zip(el[:-1], el[1:]))
    last = Sk[el[-1]]
    out = [k for k in range(K) if Sk[k] == last and k not in el]
    assert out and min(out) > max(k for k in el if Sk[k] == last)  # equals were left out, every one of them behind the elites among them


def test_cem_update_with_non_finite_candidates():
    """The non-finite costs are written into the cost buffer here; nothing is made to fault."""
    from mc_pilco_amd import hipabi, ops

    K, P, U, E = 19, 1, 2, 5
    a, white, gen = synthetic(K, U, 7)
    J = 2.0 + torch.rand(K, dtype=DT, generator=gen)
    keep = [1, 4, 13]
    for i, k in enumerate(k for k in range(K) if k not in keep):
        J[k] = (float("nan"), float("inf"), -float("inf"))[i % 3]
    J = G(J)
    mp = ops.PackedMPPI(K, P, H, U, 0.3, 1.0)
    ext = ops.PackedPlanExt(H, U, beta=0.5, n_elite=E, alpha=0.3, sigma_min=0.01)
    got = ops.cem_update(mp, ext, J, a, xi=white)
    assert int(got[5].item()) == hipabi.STATUS_NAN
    assert sorted(got[3].cpu().tolist()[:3]) == keep and got[3].cpu().tolist()[3:] == [-1, -1] and float(got[4][2]) == 3.0
    check_cem("16 of 19 non-finite", got, J, a, 0.3, white, K, P, E, 0.3, 0.01, 0.5)
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    # none finite: the nominal and the std stay
    s = G(0.1 + torch.rand(H, U, dtype=DT, generator=gen))
    none = ops.cem_update(mp, ext, torch.full_like(J, float("nan")), a, sigma_rows=s, xi=white)
    assert int(none[5].item()) == hipabi.STATUS_NAN and torch.equal(none[0], a) and torch.equal(none[1], s)
    assert none[3].cpu().tolist() == [-1] * E
    st = none[4].cpu()
    assert float(st[1]) == -1.0 and float(st[2]) == 0.0 and bool(torch.isnan(st[0])) and bool(torch.isnan(st[3]))
    flat = ops.cem_update(mp, ext, torch.full_like(J, float("inf")), a, xi=white)
    assert torch.equal(flat[0], a) and torch.equal(flat[1], torch.full_like(a, 0.3))


# ---- 6. the planner -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [False, True], ids=["mean", "sampled"])
def test_cem_plan_equals_the_launches_chained_by_hand(sample):
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import mppi

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    (K, P), U = ((7, 3) if sample else (19, 1)), c["U"]
    x0, a, _, eps = operands(c, K, P, 6)
    spec = mt.cost_specs(c)["target_add"]
    noise = ops.NoiseSpec(eps=eps if sample else None, seed=21, call=40)
    u_prev = np.array([0.3, -0.2])[:U]
    par = dict(K=K, P=P, iterations=3, sigma=[0.4, 0.3][:U], kappa=0.5 if sample else 0.0, particle_pred=sample, noise=noise, method="cem", n_elite=3,
               alpha=0.2, sigma_min=0.05, beta=0.5, u_prev=u_prev)
    got, info = mppi.plan(pm, x0, a, cost_object(spec), **par)
    again, info2 = mppi.plan(pm, x0, a, cost_object(spec), **par)
    sg, sg2 = info.pop("sigma"), info2.pop("sigma")
    assert torch.equal(got, again) and torch.equal(sg, sg2) and info == info2 and info["status"] == 0 and info["iterations"] == 3
    pc, cin = packed_costs(spec, c["S"], U)
    mp = ops.PackedMPPI(K, P, H, U, par["sigma"], 1.0, par["kappa"])
    ext = ops.PackedPlanExt(H, U, beta=0.5, n_elite=3, alpha=0.2, sigma_min=0.05)
    cur, s, nominal, smin, ecost, elites = a, G(np.tile(np.array(par["sigma"]), (H, 1))), [], [], [], []
    for i in range(3):
        nz = ops.NoiseSpec(eps=noise.eps, seed=21, call=40 + i)
        J = ops.plan_rollout(pm, mp, ext, pc, x0, cur, sigma_rows=s, u_prev=G(u_prev), cost_inputs=cin, noise=nz, particle_pred=sample)[0]
        cur, s, cand, elite, stats, _ = ops.cem_update(mp, ext, J, cur, sigma_rows=s, noise=nz)
        nominal.append(float(cand[0])), smin.append(float(stats[0])), ecost.append(float(stats[3])), elites.append(elite.cpu().tolist())
    assert torch.equal(got, cur) and torch.equal(sg, s)
    assert info["nominal_cost"] == nominal and info["S_min"] == smin and info["elite_cost"] == ecost and info["elite"] == elites
    assert info["n_elite_used"] == [3, 3, 3] and not torch.equal(got, a) and float((sg - s.new_tensor(par["sigma"])).abs().max()) > 1e-3
    # the MPPI update under the same extension, chained the same way
    par2 = dict(par, method="mppi", lam=0.1, iterations=2)
    got, info = mppi.plan(pm, x0, a, cost_object(spec), **par2)
    mp = ops.PackedMPPI(K, P, H, U, par["sigma"], 0.1, par["kappa"])
    cur = a
    for i in range(2):
        nz = ops.NoiseSpec(eps=noise.eps, seed=21, call=40 + i)
        J = ops.plan_rollout(pm, mp, ext, pc, x0, cur, u_prev=G(u_prev), cost_inputs=cin, noise=nz, particle_pred=sample)[0]
        cur = ops.mppi_update_ext(mp, ext, J, cur, noise=nz)[0]
    assert torch.equal(got, cur) and info["status"] == 0


@pytest.mark.parametrize("beta", ct.CEM_BETAS)
@pytest.mark.parametrize("case", mt.BEHAVIOUR, ids=lambda c: "-".join(str(v) for v in c[:3]))
def test_the_cem_planner_lowers_the_nominal_cost_with_the_truths_elites(case, beta):
    """The cases tests/test_cem_truth_cpu.py vetted on the truth alone (the drop, and the gap at the elite boundary that lets index sets be
    compared): the nominal's cost after 5 iterations is below the warm start's, no tolerance; every iteration's elite set is the truth's;
    the nominal costs within 1e-6 of the truth's (tests/test_gpu_mppi.py's bound and reasoning: 1e-9 on the states, six iterations)."""
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import mppi

    shape, deg, N, seed, K, sigma, lam = case
    c, m, pm = pair(shape, N, deg)
    x0, a0 = mt.behaviour_operands(c, seed)
    spec = mt.cost_specs(c)["effort"]
    a, info = mppi.plan(pm, G(x0), G(a0), cost_object(spec), K=K, P=1, iterations=ct.CEM_ITERATIONS, sigma=sigma, noise=ops.NoiseSpec(seed=seed, call=0),
                        method="cem", n_elite=K // 8, alpha=ct.CEM_ALPHA, sigma_min=ct.CEM_SIGMA_MIN, beta=beta)
    torch.set_num_threads(1)
    at, st, nominal, elites, every = ct.plan_truth(shape, m, c, x0, a0, spec, K, K // 8, ct.CEM_ITERATIONS, sigma, beta=beta, seed=seed)
    print("%s beta %g: nominal cost per iteration %s (truth %s)" % (cid(case[:3]), beta, ["%.6f" % v for v in info["nominal_cost"]],
                                                                   ["%.6f" % v for v in nominal]))
    assert info["status"] == 0 and all(np.isfinite(info["nominal_cost"])) and info["n_elite_used"] == [K // 8] * ct.CEM_ITERATIONS
    assert info["nominal_cost"][ct.CEM_ITERATIONS - 1] < info["nominal_cost"][0]
    for i, (g, t) in enumerate(zip(info["elite"], elites)):
        assert set(g) == set(t), i
    assert max(abs(p - q) for p, q in zip(info["nominal_cost"], nominal)) < 1e-6
    assert float(np.abs(n_(info["sigma"]) - st).max()) < 1e-6 and float(np.abs(n_(a) - at).max()) < 1e-6


# ---- 7. the controller ----------------------------------------------------------------------------------------------------------------------
def test_the_controller_charges_the_first_rate_against_the_input_it_applied(monkeypatch):
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import Policy, mppi

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    cost = cost_object(mt.cost_specs(c)["target_add"])  # effort and rate
    gen = np.random.default_rng(12)
    xs = [0.3 * (gen.random(c["S"]) - 0.5) for _ in range(3)]
    u_max = [0.8, 1.2]
    par = dict(K=19, P=1, sigma=0.4, lam=0.05)
    seen, plan = [], mppi.plan

    def recording(*args, **kw):
        seen.append(None if kw.get("u_prev") is None else np.array(kw["u_prev"], copy=True))
        return plan(*args, **kw)

    monkeypatch.setattr(mppi, "plan", recording)
    mk = lambda **kw: Policy.MPPI_controller(c["S"], c["U"], pm, cost, horizon=H, iterations=2, noise=ops.NoiseSpec(seed=3, call=100),
                                             flg_squash=True, u_max=u_max, device=dev(), **dict(par, **kw))
    ctrl = mk(charge_first_rate=True, method="cem", n_elite=4, beta=0.5)
    got = [ctrl.forward_np(xs[k], 0.05 * k) for k in range(3)]
    assert seen[0] is None and all(np.array_equal(seen[k], got[k - 1].reshape(-1)) for k in (1, 2))
    assert np.array_equal(ctrl.forward_np(xs[0], 0.0), got[0]) and seen[3] is None and ctrl.step == 1  # t = 0 starts an episode over
    # what it returned: the plans by hand, each from the initial std, each charged for the jump from the input before it
    a, prev = torch.zeros(H, c["U"], dtype=DT, device=dev()), None
    for k in range(3):
        a, info = plan(pm, G(xs[k]), a, cost, iterations=2, u_max=u_max, flg_squash=True, noise=ops.NoiseSpec(seed=3, call=100 + 2 * k), t0=0,
                       method="cem", n_elite=4, beta=0.5, u_prev=prev, **par)
        um = torch.as_tensor(u_max, dtype=DT)
        prev = (um * torch.tanh(a[0].cpu() / um)).numpy()
        assert np.array_equal(got[k], prev.reshape(1, -1))
        a = mppi.shift_warm_start(a)
    # the charge matters, and without the switch nothing is handed over
    del seen[:]
    plain = mk(method="cem", n_elite=4, beta=0.5)
    free = [plain.forward_np(xs[k], 0.05 * k) for k in range(3)]
    assert seen == [None] * 3 and np.array_equal(free[0], got[0]) and not np.array_equal(free[1], got[1])


def test_the_default_controller_returns_what_it_did():
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import Policy, mppi

    shape, deg, N = MODELS[0]
    c, m, pm = pair(shape, N, deg)
    cost = cost_object(mt.cost_specs(c)["target_add"])
    gen = np.random.default_rng(13)
    xs = [0.3 * (gen.random(c["S"]) - 0.5) for _ in range(3)]
    par = dict(K=19, P=1, sigma=0.4, lam=0.05)
    ctrl = Policy.MPPI_controller(c["S"], c["U"], pm, cost, horizon=H, iterations=2, noise=ops.NoiseSpec(seed=3, call=100), device=dev(), **par)
    got = [ctrl.forward_np(xs[k], 0.05 * k) for k in range(3)]
    # the plain planner's launches chained by hand (ops.mppi_rollout, ops.mppi_update: the entries from before the extension)
    pc, cin = packed_costs(mt.cost_specs(c)["target_add"], c["S"], c["U"])
    mp = ops.PackedMPPI(19, 1, H, c["U"], 0.4, 0.05)
    a = torch.zeros(H, c["U"], dtype=DT, device=dev())
    for k in range(3):
        for i in range(2):
            nz = ops.NoiseSpec(seed=3, call=100 + 2 * k + i)
            J = ops.mppi_rollout(pm, mp, pc, G(xs[k]), a, cost_inputs=cin, noise=nz)[0]
            a = ops.mppi_update(mp, J, a, noise=nz)[0]
        assert np.array_equal(got[k], torch.tanh(a[0].cpu()).numpy().reshape(1, -1))
        a = mppi.shift_warm_start(a)
    assert ctrl.charge_first_rate is False and set(ctrl.info) == {"S_min", "nominal_cost", "ess", "mean_cost", "status", "iterations"}
