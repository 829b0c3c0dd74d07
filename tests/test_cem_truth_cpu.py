"""CPU: the truth of the planner's extension (tests/cem_truth.py) on its own.

  1. the coloured table: beta = 0 carries the white normals' values; the recursion against the same table written as explicit weighted sums
     (long double); candidate 0 zero; the stationary variance.
  2. the elite choice written twice -- a full stable sort, a partition around the E'-th value -- on random costs, on costs with ties inside
     and ACROSS the elite boundary (the lower k wins), with NaN / inf candidates, with fewer finite candidates than elites, with none, and
     with -0.0 beside 0.0.
  3. the MPPI update under the extension: the update on the coloured table (the truth's statement) against the filter run over the weighted
     sums of the white normals (the kernels' statement): the sum is linear in n.
  4. the CEM update: float64 against long double (d_ref), the formulas on a case small enough to write out, the floor, the edge cases.
  5. the CEM planner on mppi_truth.BEHAVIOUR with n_elite = K // 8, alpha = 0.1, sigma_min = 0.05, beta in {0, 0.5} and 6 iterations: the
     nominal's cost drops by more than 1e-3, and -- the condition that lets the GPU test compare elite SETS at all -- in every iteration the
     relative gap between the last elite's cost and the first non-elite's exceeds 1e-7 (the kernels agree with the oracle to 1e-9)."""
import functools

import numpy as np
import pytest
import torch

import cem_truth as ct
import mppi_truth as mt
import pd_models
from lqr_models import MODELS

H = mt.H


@functools.lru_cache(maxsize=None)
def pair(shape, N, deg):
    return pd_models.build_pair(shape, N, deg, seed=N + deg)


# ---- 1. the coloured table ------------------------------------------------------------------------------------------------------------------
def test_the_coloured_table():
    n = mt.xi_table(11, 3, H, 9, 2)
    assert np.array_equal(ct.colour(n, 0.0), n)  # beta = 0: c is exactly 1
    for beta in (0.5, 0.9):
        xi = ct.colour(n, beta)
        assert not xi[:, 0].any() and np.array_equal(xi[0], n[0])
        c = np.sqrt(1 - beta * beta)
        assert xi[3, 2, 1] == beta * xi[2, 2, 1] + c * n[3, 2, 1]
        other = ct.colour_by_weights(n, beta)
        ld = ct.colour(n, beta, np.longdouble)
        assert float(np.abs(ld - other).max()) < 64 * float(np.finfo(np.longdouble).eps) * float(np.abs(other).max())
        assert float(np.abs(xi - other.astype(np.float64)).max()) <= 16 * 2.0 ** -52 * max(1.0, float(np.abs(xi).max()))
    # unit variance at every row: var xi_t = beta^2 var xi_{t-1} + (1 - beta^2)
    big = ct.colour(mt.xi_table(5, 0, H, 4000, 1), 0.7)[:, 1:]
    assert np.all(np.abs(big.std(1) - 1.0) < 0.05)
    assert 0.6 < float(np.corrcoef(big[2, :, 0], big[3, :, 0])[0, 1]) < 0.8


# ---- 2. the elite choice --------------------------------------------------------------------------------------------------------------------
def _both(S, E):
    a, b = ct.elites_by_sort(S, E), ct.elites_by_partition(S, E)
    assert a == b, (S, E, a, b)
    return a


def test_the_elite_choice_two_ways():
    gen = np.random.default_rng(0)
    for K, E in ((19, 5), (257, 32), (600, 60), (19, 19), (19, 1), (1, 1)):
        S = gen.standard_normal(K)
        el = _both(S, E)
        assert len(el) == E and sorted(S[el]) == list(S[el]) and max(S[el]) <= min(np.delete(S, el), default=np.inf)
    # ties inside and across the boundary: the lower k wins, equal costs are ranked by k
    S = np.array([3.0, 1.0, 2.0, 1.0, 2.0, 2.0, 0.5, 2.0])
    assert _both(S, 4) == [6, 1, 3, 2] and _both(S, 5) == [6, 1, 3, 2, 4] and _both(S, 1) == [6] and _both(S, 8) == [6, 1, 3, 2, 4, 5, 7, 0]
    S = gen.integers(0, 4, 300).astype(np.float64)  # four values over 300 candidates
    for E in (1, 7, 75, 150, 299, 300):
        el = _both(S, E)
        assert all((S[p], p) < (S[q], q) for p, q in zip(el[:-1], el[1:]))
    # non-finite candidates are never elite
    S = gen.standard_normal(19)
    S[[0, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, 17, 18]] = [np.nan, np.inf, -np.inf] * 5 + [np.nan]
    assert _both(S, 5) == [int(k) for k in sorted((1, 4, 13), key=lambda k: S[k])]
    assert _both(np.full(7, np.nan), 3) == [] and _both(np.array([np.inf, -np.inf]), 1) == []
    assert _both(np.array([0.0, -0.0, 1.0, -0.0]), 2) == [0, 1] and _both(np.array([-1.0, -3.0, -2.0]), 2) == [1, 2]


# ---- 3. the MPPI update under the extension -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("per_row", [False, True], ids=["sigma", "sigma_rows"])
def test_the_ext_update_is_the_filter_over_the_weighted_sums(beta, per_row):
    K, P, U = 19, 3, 2
    gen = np.random.default_rng(7)
    J, a = 2.0 + gen.random(K * P), gen.standard_normal((H, U))
    s = 0.2 + gen.random((H, U)) if per_row else 0.2 + gen.random(U)
    n = mt.xi_table(5, 7, H, K, U)
    f64 = ct.update_ext(J, a, s, n, K, P, 0.05, 0.5, beta)
    ld = ct.update_ext(J, a, s, n, K, P, 0.05, 0.5, beta, np.longdouble)
    d = mt.d_ref(f64, ld)
    assert max(d) < 1e-13
    # the kernels' statement: N_t = sum_k w_k n_t(k), X_0 = N_0, X_t = beta X_{t-1} + c N_t, a_new = a + s X
    w = ld[2]
    N = np.einsum("k,hku->hu", w[1:], n[:, 1:].astype(np.longdouble))
    X = np.zeros_like(N)
    X[0] = N[0]
    c = np.longdouble(np.sqrt(1 - beta * beta))
    for t in range(1, H):
        X[t] = np.longdouble(beta) * X[t - 1] + c * N[t]
    other = a.astype(np.longdouble) + ct.rows(s, H, U, np.longdouble) * X
    assert float(np.abs(other - ld[0]).max()) < 1e3 * float(np.finfo(np.longdouble).eps) * float(np.abs(ld[0]).max())
    if beta == 0.0 and not per_row:  # the plain update
        plain = mt.update(J, a, s, n, K, P, 0.05, 0.5)
        assert all(np.array_equal(p, q) for p, q in zip(plain, f64))


# ---- 4. the CEM update ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("alpha", [0.0, 0.3])
def test_the_cem_update(alpha, beta):
    K, P, U, E = 19, 3, 2, 5
    gen = np.random.default_rng(9)
    J, a, s = 2.0 + gen.random(K * P), gen.standard_normal((H, U)), 0.2 + gen.random((H, U))
    n = mt.xi_table(5, 9, H, K, U)
    smin = np.array([0.0, 0.45])
    f64 = ct.cem_update(J, a, s, n, K, P, E, alpha, smin, beta, 0.5)
    ld = ct.cem_update(J, a, s, n, K, P, E, alpha, smin, beta, 0.5, np.longdouble)
    assert f64[3] == ld[3] == ct.elites_by_partition(f64[2], E) and max(ct.d_ref2(f64, ld)) < 1e-14
    a_new, s_new, S, el, stats = f64
    xi = ct.colour(n, beta)
    # written out for one entry
    t, u = 3, 1
    vals = np.array([xi[t, k, u] for k in el])
    m, v = vals.mean(), vals.var()
    assert abs(a_new[t, u] - (a[t, u] + (1 - alpha) * s[t, u] * m)) < 1e-14
    assert abs(s_new[t, u] - max(smin[u], s[t, u] * np.sqrt(alpha + (1 - alpha) * v))) < 1e-14
    assert (s_new[:, 1] >= 0.45).all() and (s_new[:, 1] == 0.45).any() and (s_new[:, 0] > 0).all()  # the floor is active on some entries
    assert stats[0] == S.min() and int(stats[1]) == el[0] == int(np.argmin(S)) and int(stats[2]) == E and abs(stats[3] - S[el].mean()) < 1e-14
    # the nominal among the elites contributes xi = 0
    J0 = J.copy()
    J0[:P] = 0.0
    el0 = ct.cem_update(J0, a, s, n, K, P, E, alpha, smin, beta, 0.5)[3]
    assert el0[0] == 0
    # E = 1: the mean is that candidate's perturbation, the variance 0
    one = ct.cem_update(J, a, s, n, K, P, 1, alpha, 0.0, beta, 0.5)
    assert np.allclose(one[1], np.sqrt(alpha) * s, rtol=1e-15, atol=0) and one[3] == [int(np.argmin(S))]


def test_the_cem_update_with_non_finite_candidates():
    K, P, U = 19, 1, 2
    gen = np.random.default_rng(4)
    J, a, s = 2.0 + gen.random(K), gen.standard_normal((H, U)), 0.3
    n = mt.xi_table(5, 1, H, K, U)
    bad = J.copy()
    keep = [1, 4, 13]
    bad[[k for k in range(K) if k not in keep]] = [np.nan, np.inf] * 8
    a_new, s_new, S, el, stats = ct.cem_update(bad, a, s, n, K, P, 5)
    assert sorted(el) == keep and int(stats[2]) == 3 and np.isfinite(a_new).all() and np.isfinite(s_new).all()
    # the problem without them (behind a candidate 0 too dear to be elite)
    ref = ct.cem_update(np.concatenate([[99.0], J[keep]]), a, s, np.concatenate([np.zeros((H, 1, U)), n[:, keep]], 1), 4, P, 3)
    assert [keep[k - 1] for k in ref[3]] == el
    assert np.array_equal(ref[0], a_new) and np.array_equal(ref[1], s_new)
    none = ct.cem_update(np.full(K, np.nan), a, s, n, K, P, 5)
    assert np.array_equal(none[0], a) and np.array_equal(none[1], np.full((H, U), 0.3)) and none[3] == []
    assert np.isnan(none[4][0]) and none[4][1] == -1 and none[4][2] == 0 and np.isnan(none[4][3])


# ---- 5. the planner -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", ct.CEM_BETAS)
@pytest.mark.parametrize("case", mt.BEHAVIOUR, ids=lambda c: "-".join(str(v) for v in c[:3]))
def test_the_truth_cem_planner_lowers_the_nominal_cost_with_separated_elites(case, beta):
    shape, deg, N, seed, K, sigma, lam = case
    assert (shape, deg, N) in MODELS
    torch.set_num_threads(1)
    c, m, _ = pair(shape, N, deg)
    x0, a0 = mt.behaviour_operands(c, seed)
    spec = mt.cost_specs(c)["effort"]
    a, s, nominal, elites, every = ct.plan_truth(shape, m, c, x0, a0, spec, K, K // 8, ct.CEM_ITERATIONS, sigma, beta=beta, seed=seed)
    gaps = [ct.boundary_gap(S, K // 8) for S in every]
    print("%s deg %d N %d beta %g: nominal cost %.4f -> %.4f (%s); smallest elite-boundary gap %.2e; std within [%.3f, %.3f]"
          % (shape, deg, N, beta, nominal[0], nominal[-1], ["%.6f" % v for v in nominal], min(gaps), s.min(), s.max()))
    assert np.isfinite(every).all() and np.isfinite(a).all() and np.isfinite(s).all() and (s >= ct.CEM_SIGMA_MIN).all()
    assert all(len(el) == K // 8 for el in elites)
    assert nominal[0] - nominal[-1] > 1e-3
    assert min(gaps) > 1e-7
