"""CPU: the truth of the sampling planner (tests/mppi_truth.py) on its own.

  1. the perturbations: stream 3 of tests/noise_truth.py, candidate 0 zero, other numbers for another call, stream, seed or offset.
  2. the update (the header's statement: shift by the minimum, weight 0 for a non-finite candidate) against a direct softmax written another
     way -- no shift, numpy's mean and std, explicit loops, long double -- at kappa = 0 and 0.5 and at a temperature small enough that one
     weight dominates; the float64 and long-double forms of the update agree to rounding (d_ref); the NaN cases: a non-finite candidate has
     weight 0 and the others keep the weights of the problem without it, none finite leaves a = a.
  3. the costs of mppi_truth.point_costs against torch formulas of policy_learning/Cost_function.py (imported as plain functions: CPU tensors).
  4. the planner: for the seeds and sizes of mppi_truth.BEHAVIOUR -- the cases the GPU test of the planner and the controller runs -- the
     nominal's cost after 5 iterations is BELOW the cost at iteration 0 on the truth alone, and every candidate of every iteration stays
     finite.  The margin printed here is what the GPU assertion (the same inequality, no tolerance) has to spare."""
import functools

import numpy as np
import pytest
import torch

import mppi_truth as mt
import noise_truth as nt
import pd_models
from lqr_models import MODELS


@functools.lru_cache(maxsize=None)
def pair(shape, N, deg):
    return pd_models.build_pair(shape, N, deg, seed=N + deg)


# ---- 1. perturbations -------------------------------------------------------------------------------------------------------------------------
def test_the_perturbations_are_stream_three_by_candidate():
    xi = mt.xi_table(11, 3, 6, 7, 2)
    assert xi.shape == (6, 7, 2) and not xi[:, 0].any() and np.isfinite(xi).all()
    for (t, k, u) in ((0, 1, 0), (5, 6, 1), (3, 2, 1)):
        assert xi[t, k, u] == float(nt.normal(11, 3, np.uint64(k), np.uint64(t), 3, np.uint64(u)))
    others = [mt.xi_table(11, 4, 6, 7, 2), mt.xi_table(12, 3, 6, 7, 2), mt.xi_table(11, 3, 6, 7, 2, offset=1)]
    others.append(np.broadcast_to(nt.normal(11, 3, np.arange(7, dtype=np.uint64)[None, :, None], np.arange(6, dtype=np.uint64)[:, None, None], 0,
                                            np.arange(2, dtype=np.uint64)[None, None, :]), (6, 7, 2)))
    for o in others:
        assert np.abs(o[:, 1:] - xi[:, 1:]).min() > 0
    assert abs(xi[:, 1:].mean()) < 0.5 and 0.5 < xi[:, 1:].std() < 1.5  # (60 draws)
    if nt.have_longdouble():
        assert float(nt.ulps(xi[:, 1:], mt.xi_table(11, 3, 6, 7, 2, hp=True)[:, 1:]).max()) < 4.0  # (numpy's own evaluation: 2.8 ulp, tests/test_noise_truth_cpu.py)


# ---- 2. the update ----------------------------------------------------------------------------------------------------------------------------
def _update_case(K, P, U, seed):
    gen = np.random.default_rng(seed)
    J = 2.0 + gen.random(K * P)
    a = gen.standard_normal((mt.H, U))
    sigma = 0.2 + gen.random(U)
    return J, a, sigma, mt.xi_table(5, seed, mt.H, K, U)


@pytest.mark.parametrize("kappa", [0.0, 0.5])
@pytest.mark.parametrize("lam", [1.0, 0.05, 1e-3], ids=["lam1", "lam0.05", "one-weight-dominates"])
def test_the_update_against_a_direct_softmax(lam, kappa):
    K, P, U = 19, 3, 2
    J, a, sigma, xi = _update_case(K, P, U, 7)
    f64 = mt.update(J, a, sigma, xi, K, P, lam, kappa)
    ld = mt.update(J, a, sigma, xi, K, P, lam, kappa, dt=np.longdouble)
    direct = mt.update_direct(J, a, sigma, xi, K, P, lam, kappa)
    d = mt.d_ref(f64, ld)
    e = mt.d_ref(ld, direct)
    print("lam %g kappa %g: float64 vs long double %s, long double vs direct %s, largest weight %.6f, ess %.3f"
          % (lam, kappa, ["%.2e" % v for v in d], ["%.2e" % v for v in e], float(f64[2].max()), float(f64[3][2])))
    # the two long-double statements differ by the rounding of long double alone (S / lam up to 3e3: its exp carries 3e3 ulp); the float64
    # form by that of float64
    assert max(e) < 3e3 * 4 * float(np.finfo(np.longdouble).eps) and max(d) < 3e3 * 4 * float(np.finfo(np.float64).eps)
    w = f64[2]
    assert abs(w.sum() - 1) < 1e-14 and (w >= 0).all() and int(f64[3][1]) == int(np.argmin(f64[1])) and f64[3][0] == f64[1].min()
    assert abs(f64[3][2] - 1 / (w * w).sum()) < 1e-12 and abs(f64[3][3] - (w * f64[1]).sum()) < 1e-12
    if lam == 1e-3:
        assert w.max() > 0.99
    # candidate 0's row of xi is never read
    xi2 = xi.copy()
    xi2[:, 0] = 1e6
    assert np.array_equal(mt.update(J, a, sigma, xi2, K, P, lam, kappa)[0], f64[0])


def test_the_update_gives_a_non_finite_candidate_weight_zero():
    K, P, U = 7, 3, 2
    J, a, sigma, xi = _update_case(K, P, U, 9)
    bad, xi_bad = J.copy(), xi.copy()
    bad[2 * P + 1] = np.nan  # one particle of candidate 2
    xi_bad[:, 2] = np.nan
    a_new, S, w, stats = mt.update(bad, a, sigma, xi_bad, K, P, 0.7, 0.5)
    keep = [k for k in range(K) if k != 2]
    a_ref, S_ref, w_ref, stats_ref = mt.update(J.reshape(K, P)[keep].reshape(-1), a, sigma, xi[:, keep], K - 1, P, 0.7, 0.5)
    assert w[2] == 0 and np.isnan(S[2]) and np.array_equal(w[keep], w_ref) and np.array_equal(a_new, a_ref) and np.isfinite(a_new).all()
    assert stats[0] == stats_ref[0] and keep[int(stats_ref[1])] == int(stats[1]) and stats[2] == stats_ref[2]
    a_all, S_all, w_all, stats_all = mt.update(np.full(K * P, np.inf), a, sigma, xi, K, P, 0.7, 0.0)
    assert np.array_equal(a_all, a) and not w_all.any() and stats_all[1] == -1 and stats_all[2] == 0 and np.isnan(stats_all[0])


# ---- 3. the costs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["target_add", "traj_plain", "quad_joint", "effort"])
def test_point_costs_against_the_torch_formulas(name):
    from mc_pilco_amd.policy_learning import Cost_function as cf

    c = pd_models.SHAPES["arm2"]
    spec = mt.cost_specs(c)[name]
    gen = np.random.default_rng(3)
    x, u, t0 = gen.standard_normal((mt.H, 5, c["S"])), gen.standard_normal((mt.H, 5, c["U"])), (2 if spec["kind"] == "traj" else 0)
    got = mt.point_costs(spec, x, u, t0)
    xt, ut = torch.as_tensor(x), torch.as_tensor(u)
    T_ = lambda v: None if v is None else torch.as_tensor(np.asarray(v))
    if spec["kind"] == "traj":
        dx_f = cf.saturated_distance_from_trajectory(xt, ut, 0, torch.as_tensor(spec["target"][t0:t0 + mt.H]), T_(spec["ls"]), False, spec["idx"])
        want = dx_f
    else:
        dx = cf.distance_from_target(xt, ut, 0, T_(spec["target"]), T_(spec["ls"]), spec["idx"])
        du, dr = cf.input_distance(ut, T_(spec["u_ls"]), T_(spec["u_rate"]), T_(spec["u_target"]), spec["u_idx"])
        f = (lambda d: d) if spec["kind"] == "target_quad" else (lambda d: 1 - torch.exp(-d))
        want = f(dx + du + dr) if spec["joint"] else f(dx) + du + dr
    assert float((torch.as_tensor(got) - want).abs().max()) < 1e-13
    J = mt.traj_costs(spec, x, u, None, t0)
    w = 0.5 + gen.random(mt.H)
    assert np.allclose(J, got.sum(0), rtol=1e-14) and np.allclose(mt.traj_costs(spec, x, u, w, t0), (w[:, None] * got).sum(0), rtol=1e-14)


# ---- 4. the planner ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mt.BEHAVIOUR, ids=lambda c: "-".join(str(v) for v in c[:3]))
def test_the_truth_planner_lowers_the_nominal_cost_and_stays_finite(case):
    shape, deg, N, seed, K, sigma, lam = case
    assert (shape, deg, N) in MODELS
    torch.set_num_threads(1)
    c, m, _ = pair(shape, N, deg)
    x0, a0 = mt.behaviour_operands(c, seed)
    spec = mt.cost_specs(c)["effort"]
    a, nominal, every = mt.plan_truth(shape, m, c, x0, a0, spec, K, 1, mt.ITERATIONS + 1, sigma, lam, seed=seed)
    print("%s deg %d N %d: nominal cost per iteration %s; candidates within [%.4f, %.4f]"
          % (shape, deg, N, ["%.6f" % v for v in nominal], every.min(), every.max()))
    assert np.isfinite(every).all() and np.isfinite(a).all()
    assert nominal[mt.ITERATIONS] < nominal[0]
    # the margin the GPU assertion has to spare: the kernels agree with this truth to ~1e-9 on a cost of O(1)
    assert nominal[0] - nominal[mt.ITERATIONS] > 1e-3
