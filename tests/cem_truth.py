"""The truth for the planner's extension (mcp_plan_ext: mcp_plan_rollout, mcp_mppi_update_ext, mcp_cem_update, policy_learning/mppi.py's
``method="cem"``): numpy statements of include/mcpilco_hip.h's comments on top of tests/mppi_truth.py -- the AR(1)-coloured perturbation
table, the MPPI update under a std per row and the colouring (written on the coloured table itself: the kernels filter the weighted sums
instead), the CEM update and a CEM planner on the oracle's step.  Everything takes ``dt`` (float64, or numpy.longdouble, whose difference
``mppi_truth.d_ref`` turns into a case's conditioning).  The elite choice is written twice -- a full stable sort, and a partition around the
E'-th value -- and tests/test_cem_truth_cpu.py pins one to the other.  CPU side only imports numpy and the planner's truth."""
import numpy as np

import mppi_truth as mt


def colour(n, beta, dt=np.float64):
    """xi [H, K, U] of the white normals n [H, K, U]: xi_0 = n_0, xi_t = beta xi_{t-1} + c n_t, c = sqrt(1 - beta^2) rounded to a double
    once (the kernels are handed that double).  Candidate 0 is zero.  beta == 0 returns n's values."""
    n = np.asarray(n, dtype=dt)
    c = dt(np.sqrt(np.float64(1.0) - np.float64(beta) * np.float64(beta)))
    xi = np.zeros_like(n)
    xi[0] = n[0]
    for t in range(1, n.shape[0]):
        xi[t] = dt(beta) * xi[t - 1] + c * n[t]
    xi[:, 0, :] = 0
    return xi


def colour_by_weights(n, beta):
    """The same table written another way (long double): xi_t = sum_{j <= t} g(t, j) n_j with g(t, j) = beta^(t - j) c for j >= 1 and
    beta^t for j = 0."""
    ld = np.longdouble
    n = np.asarray(n, dtype=ld)
    c = ld(np.sqrt(np.float64(1.0) - np.float64(beta) * np.float64(beta)))
    xi = np.zeros_like(n)
    for t in range(n.shape[0]):
        for j in range(t + 1):
            xi[t] += ld(beta) ** (t - j) * (c if j else ld(1)) * n[j]
    xi[:, 0, :] = 0
    return xi


def rows(sigma, Hn, U, dt=np.float64):
    """s [H, U] of a scalar, a std per input [U] or a std per row [H, U]."""
    return np.array(np.broadcast_to(np.asarray(sigma, dtype=dt), (Hn, U)))


def cand_costs(J, K, P, kappa=0.0, dt=np.float64):
    """S [K] of J [K P] as mppi_truth.update forms it."""
    Jk = np.asarray(J, dtype=dt).reshape(K, P)
    S = np.zeros(K, dtype=dt)
    for p in range(P):
        S = S + Jk[:, p]
    S = S / dt(P)
    if kappa != 0.0:
        q = np.zeros(K, dtype=dt)
        for p in range(P):
            q = q + (Jk[:, p] - S) ** 2
        S = S + dt(kappa) * np.sqrt(q / dt(P - 1))
    return S


def update_ext(J, a, s, n, K, P, lam, kappa=0.0, beta=0.0, dt=np.float64):
    """The MPPI update under the extension: mppi_truth.update on the COLOURED table with the std per row s [H, U] ->
    (a_new, S, weights, stats)."""
    a = np.asarray(a, dtype=dt)
    return mt.update(J, a, rows(s, a.shape[0], a.shape[1], dt), colour(n, beta, dt), K, P, lam, kappa, dt)


# ---- the elite choice, twice ----------------------------------------------------------------------------------------------------------------
def elites_by_sort(S, n_elite):
    """The E' = min(n_elite, #finite) candidates with the smallest (S_k, k), in that order: a stable sort of the finite costs."""
    S = np.asarray(S)
    fin = np.flatnonzero(np.isfinite(S))
    order = fin[np.argsort(S[fin], kind="stable")]
    return [int(k) for k in order[:min(int(n_elite), fin.size)]]


def elites_by_partition(S, n_elite):
    """The same set and order without sorting the candidates: the E'-th smallest finite cost from numpy's partition, every candidate below
    it, the lowest indices among those equal to it, then the E' survivors ordered as Python orders (cost, index) pairs."""
    S = np.asarray(S)
    fin = np.flatnonzero(np.isfinite(S))
    E = min(int(n_elite), fin.size)
    if E == 0:
        return []
    thr = np.partition(S[fin], E - 1)[E - 1]
    below = [int(k) for k in fin if S[k] < thr]
    equal = [int(k) for k in fin if S[k] == thr][:E - len(below)]
    return [k for _, k in sorted((float(S[k]) + 0.0, k) for k in below + equal)]


def cem_update(J, a, s, n, K, P, n_elite, alpha=0.0, sigma_min=0.0, beta=0.0, kappa=0.0, dt=np.float64, elite=None):
    """The header's CEM update in ``dt``: J [K P], a [H, U], s the current std (scalar, [U] or [H, U]), n [H, K, U] white normals ->
    (a_new [H, U], sigma_new [H, U], S [K], elite (ranked list), stats [4] = S_min, argmin, E', mean elite cost).  ``elite``: a ranking to
    fit to in place of this function's own (the kernel's, once it has been compared).  None finite: a_new = a, sigma_new = s, no elite,
    stats NaN, -1, 0, NaN."""
    a = np.asarray(a, dtype=dt)
    Hn, U = a.shape
    s = rows(s, Hn, U, dt)
    S = cand_costs(J, K, P, kappa, dt)
    el = elites_by_sort(S, n_elite) if elite is None else [int(k) for k in elite]
    if not el:
        return a.copy(), s.copy(), S, el, np.array([np.nan, -1, 0, np.nan], dtype=dt)
    xi = colour(n, beta, dt)[:, el, :]  # [H, E', U]
    E = dt(len(el))
    m = xi.sum(1) / E
    v = ((xi - m[:, None, :]) ** 2).sum(1) / E
    al = dt(alpha)
    a_new = al * a + (dt(1) - al) * (a + s * m)
    smin = np.broadcast_to(np.asarray(sigma_min, dtype=dt), (U,))
    sigma_new = np.maximum(smin[None, :], np.sqrt(al * s * s + (dt(1) - al) * s * s * v))
    stats = np.array([S[el[0]], el[0], len(el), S[el].sum() / E], dtype=dt)
    return a_new, sigma_new, S, el, stats


def d_ref2(f64, ld):
    """(a_new, sigma_new): mppi_truth.d_ref's meaning for the CEM update's two fitted outputs."""
    return mt.d_ref((f64[0], f64[1], f64[1]), (ld[0], ld[1], ld[1]))[:2]


def boundary_gap(S, n_elite):
    """The relative gap between the last elite's cost and the first non-elite's (inf when every finite candidate is elite)."""
    S = np.asarray(S, dtype=np.float64)
    srt = np.sort(S[np.isfinite(S)])
    E = min(int(n_elite), srt.size)
    if E == 0 or E == srt.size:
        return np.inf
    return float((srt[E] - srt[E - 1]) / max(abs(srt[E]), abs(srt[E - 1])))


# ---- the planner ----------------------------------------------------------------------------------------------------------------------------
CEM_ALPHA, CEM_SIGMA_MIN, CEM_BETAS, CEM_ITERATIONS = 0.1, 0.05, (0.0, 0.5), 6


def plan_truth(shape, m, c, x0, a, spec, K, n_elite, iterations, sigma, alpha=CEM_ALPHA, sigma_min=CEM_SIGMA_MIN, beta=0.0, u_max=1.0,
               squashed=True, seed=0, call=0, dt=np.float64):
    """``iterations`` x (candidates a + s xi, oracle rollouts of the mean model, costs, CEM update), iteration i with the white normals of
    call + i.  Returns (a, s, nominal cost per iteration = S[0], every iteration's ranked elites, every iteration's S [iterations, K])."""
    a = np.asarray(a, dtype=dt)
    Hn, U = a.shape
    s = rows(sigma, Hn, U, dt)
    nominal, elites, every = [], [], []
    for i in range(iterations):
        n = mt.xi_table(seed, call + i, Hn, K, U).astype(dt)
        u = mt.squash(a[:, None, :] + s[:, None, :] * colour(n, beta, dt), u_max, squashed)
        x, ut = mt.oracle_states(shape, m, x0, u, 1, None, False)
        J = mt.traj_costs(spec, x, ut, None, 0, dt)
        a, s, S, el, stats = cem_update(J, a, s, n, K, 1, n_elite, alpha, sigma_min, beta, 0.0, dt)
        nominal.append(float(S[0]))
        elites.append(el)
        every.append(np.asarray(S, dtype=np.float64))
    return a, s, nominal, elites, np.stack(every)
