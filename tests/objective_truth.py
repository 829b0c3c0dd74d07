"""The truth of the time-weighted, risk-sensitive objective tests (test_objective_cpu.py, test_gpu_objective.py), written here on its own (no
project code): with c_tm the per-particle costs of a case of tests/input_cost_models.py, mu_t / sigma_t their mean / unbiased std over the n
particles of the swarm,

    J = sum_t w_t (mu_t + kappa sigma_t),   S = sum_t w_t sigma_t,   dJ/dc_tm = w_t [1/n + kappa (c_tm - mu_t) / ((n - 1) sigma_t)]

``truth``: torch autograd on CPU fp64; ``hand``: the hand form in numpy, as the kernels implement it; ``VARIANTS``: the changes the truth
must feel.  A row whose particles all have the same cost takes no part in the sigma term (the stated convention; autograd gives NaN there)."""
import numpy as np
import torch

import input_cost_models as icm

DT = torch.float64
KAPPAS = (0.7, -0.5)
WEIGHT_SETS = ("discount", "explicit", "none")
# what the GPU parity test runs each case with: (weight set, kappa)
OBJECTIVES = (("discount", 0.0), ("none", 0.7), ("explicit", -0.5))


def weights(which, T):
    """discount 0.9; an explicit [T] vector that holds a zero when T >= 3; none."""
    if which == "none":
        return None
    if which == "discount":
        return 0.9 ** np.arange(T)
    w = 0.5 + 0.4 * ((np.arange(T) * 2) % 3)
    if T >= 3:
        w[1] = 0.0
    return w


def _same(row):
    return bool(row.max() == row.min())


def rows_of(costs):
    """[T, 2] = (mean_t, unbiased std_t) of costs [T, M] (a row of identical costs: std 0; M = 1: NaN, as torch.std)."""
    cd = costs.detach()
    sd = [torch.zeros((), dtype=DT) if (cd.shape[1] > 1 and _same(cd[t])) else cd[t].std() for t in range(cd.shape[0])]
    return torch.stack([cd.mean(1), torch.stack(sd)], 1)


def truth(case, w, kappa, n_total=None, pooled_rows=None):
    """J, S, rows [T, 2] and the autograd gradients of J in the states and the inputs of ``case``.  ``n_total`` / ``pooled_rows``: the case is a
    shard of a swarm of n_total particles with these rows -- the gradients are then the shard's rows of the whole swarm's (autograd of
    sum_t w_t [sum_m c / n + kappa sum_m (c - mu_t)^2 / (2 (n - 1) sigma_t)] with mu, sigma held constant, whose derivative in c_tm is the
    factor above), J and S those of the pooled rows."""
    x, u = icm._t(case["x"]).clone().requires_grad_(True), icm._t(case["u"]).clone().requires_grad_(True)
    costs = icm.costs_of(case, x, u)
    T, M = costs.shape
    wt = torch.ones(T, dtype=DT) if w is None else icm._t(w)
    cd = costs.detach()
    if pooled_rows is None:
        assert n_total is None or n_total == M
        rows = rows_of(costs)
        terms = []
        for t in range(T):
            term = costs[t].mean()
            if kappa != 0.0 and not _same(cd[t]):
                term = term + kappa * costs[t].std()
            terms.append(wt[t] * term)
        torch.stack(terms).sum().backward()
    else:
        rows = icm._t(pooled_rows)
        n = int(n_total)
        terms = []
        for t in range(T):
            term = costs[t].sum() / n
            if kappa != 0.0 and float(rows[t, 1]) > 0.0:
                term = term + kappa * ((costs[t] - rows[t, 0]) ** 2).sum() / (2.0 * (n - 1) * rows[t, 1])
            terms.append(wt[t] * term)
        torch.stack(terms).sum().backward()
    J = (wt * (rows[:, 0] + (kappa * rows[:, 1] if kappa != 0.0 else 0.0))).sum()
    S = (wt * rows[:, 1]).sum()
    return dict(J=J, S=S, rows=rows, costs=cd, g_states=x.grad, g_inputs=torch.zeros_like(u) if u.grad is None else u.grad)


VARIANTS = ("kappa dropped", "w dropped", "w shifted", "biased std", "local mean", "neighbour G_t")


def applies(variant, case, w, kappa, sharded):
    T = np.asarray(case["x"]).shape[0]
    if variant in ("kappa dropped", "biased std"):
        return kappa != 0.0
    if variant == "w dropped":
        return w is not None
    if variant == "w shifted":
        return w is not None and T > 1
    if variant == "local mean":
        return kappa != 0.0 and sharded
    return case["r"] is not None and T > 1 and (kappa != 0.0 or w is not None)  # the neighbour's factor differs only then


def hand(case, w, kappa, n_total=None, pooled_rows=None, variant=None):
    """(g_states, g_inputs) by the hand form: input_cost_models.hand_gradients with the scalar G = 1 / M replaced by the per-element
    G_tm = dJ/dc_tm; the rate term's neighbour factor a_{t+1} is built from G_{t+1,m}.  ``variant``: one of VARIANTS, the same with that mistake."""
    x, u = np.asarray(case["x"], dtype=float), np.asarray(case["u"], dtype=float)
    T, M, _ = x.shape
    costs = icm.costs_of(case, icm._t(x), icm._t(u)).numpy()
    n = M if n_total is None else int(n_total)
    rows = rows_of(icm._t(costs)).numpy() if pooled_rows is None else np.asarray(pooled_rows, dtype=float)
    mu, sd = rows[:, 0].copy(), rows[:, 1].copy()
    wt = np.ones(T) if w is None else np.asarray(w, dtype=float).copy()
    n1 = float(n - 1)
    if variant == "kappa dropped":
        kappa = 0.0
    elif variant == "w dropped":
        wt = np.ones(T)
    elif variant == "w shifted":
        wt = np.roll(wt, 1)
    elif variant == "biased std":
        sd, n1 = sd * np.sqrt((n - 1) / n), float(n)
    elif variant == "local mean":
        mu = costs.mean(1)
    G = np.full((T, M), 1.0 / n)
    if kappa != 0.0:
        for t in range(T):
            if sd[t] > 0.0:
                G[t] += kappa * (costs[t] - mu[t]) / (n1 * sd[t])
    G *= wt[:, None]
    d_x, d_u, d_r = (v.numpy() for v in icm.distances(case, icm._t(x), icm._t(u)))
    quad = case["kind"] == "quad"
    fp = (lambda d: np.ones_like(d)) if quad else (lambda d: np.exp(-d))
    fj = fp(d_x + d_u + d_r) if case["joint"] else np.ones_like(d_x)
    a = G * fj
    b = a if case["joint"] else G * fp(d_x)
    gx, gu = np.zeros_like(x), np.zeros_like(u)
    if case["kind"] == "cartpole":
        ai, pi = case["used_x"]
        gx[:, :, ai] = b * 2 * (np.abs(x[:, :, ai]) - case["tg"][0]) / case["ls"][0] ** 2 * np.sign(x[:, :, ai])
        gx[:, :, pi] = b * 2 * (x[:, :, pi] - case["tg"][1]) / case["ls"][1] ** 2
    else:
        for i, s in enumerate(case["used_x"]):
            tg = case["tg"][:, s][:, None] if case["kind"] == "traj" else case["tg"][i]
            gx[:, :, s] = b * 2 * (x[:, :, s] - tg) / case["ls"][i] ** 2
    a_next = (G[:-1] * fj[1:]) if variant == "neighbour G_t" else a[1:]  # the factor of the step INTO t + 1, as row t's thread builds it
    for i, j in enumerate(case["used_u"]):
        v = np.zeros((T, M))
        if case["l"] is not None:
            v += a * 2 * (u[:, :, j] - (0.0 if case["ustar"] is None else case["ustar"][i])) / case["l"][i] ** 2
        if case["r"] is not None:
            step = 2 * (u[1:, :, j] - u[:-1, :, j]) / case["r"][i] ** 2
            v[1:] += a[1:] * step
            v[:-1] -= a_next * step
        gu[:, :, j] = v
    return gx, gu


def conditioning(case):
    """min_t sigma_t / max_m |c_tm| of a case: what bounds the amplification of the mean's error by the sigma term (<= max|c| / sigma)."""
    costs = icm.costs_of(case, icm._t(case["x"]), icm._t(case["u"]))
    if costs.shape[1] < 2:
        return float("inf")
    return float((costs.std(1) / costs.abs().max(1).values).min())


def no_inputs(case):
    """The case with its input terms taken away (cin = NULL): the state cost alone."""
    return dict(case, l=None, r=None, ustar=None)


def gpu_cases():
    """Every GPU parity case: each shape of input_cost_models.SHAPES with kinds sat / quad x ADD / JOINT and both terms; cart-pole and
    trajectory at T3M257 in both modes; each of the four state costs without input terms at T3M257S4.  -> list of (id, case, has_inputs)."""
    out = []
    for sh in icm.SHAPES:
        d = icm.draw(*sh)
        for kind in ("sat", "quad"):
            for joint in (False, True):
                out.append(("%s-%s-%s-both" % (icm.shape_id(sh), kind, "joint" if joint else "add"), icm.make_case(d, kind, joint, "both"), True))
    third = icm.SHAPES[2]
    d = icm.draw(*third)
    for kind in ("cartpole", "traj"):
        for joint in (False, True):
            out.append(("%s-%s-%s-both" % (icm.shape_id(third), kind, "joint" if joint else "add"), icm.make_case(d, kind, joint, "both"), True))
    for kind in ("sat", "quad", "cartpole", "traj"):
        out.append(("T3M257S4-%s-state" % kind, no_inputs(icm.make_case(d, kind, False, "both")), False))
    return out
