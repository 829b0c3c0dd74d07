"""The truth for the sampling planner (mcp_mppi_rollout, mcp_mppi_update, policy_learning/mppi.py): a numpy planner on
tests/open_grad_models.oracle_step with the perturbations of tests/noise_truth.py (Philox stream 3, particle = candidate, index = input),
the costs of include/mcpilco_hip.h written out, and the update of the header's comment -- once in float64 and once in numpy.longdouble,
whose difference measures a case's conditioning -- plus the same update as a direct softmax written another way
(tests/test_mppi_truth_cpu.py pins one to the other).  Models are those of tests/pd_models.py at the sizes of tests/lqr_models.MODELS.
CPU side only imports torch, numpy, the oracle and the noise truth."""
import numpy as np
import torch

import noise_truth as nt
from open_grad_models import oracle_step
from pd_models import family

DT = torch.float64
STREAM_PLAN = 3
H = 6

# The behavioural cases (the planner lowers the nominal's cost): (shape, degree, N, seed, K, sigma, lam).  Mean model, P = 1, cost
# "effort" below, x0 and a_init of ``behaviour_operands``, 5 iterations.  tests/test_mppi_truth_cpu.py shows on the truth alone that each
# ends below where it started and that every candidate stays finite; the GPU test asserts the same of the kernels.
BEHAVIOUR = [("arm2", 0, 37, 3, 64, 0.5, 0.02), ("arm2_delta", 2, 37, 4, 64, 0.5, 0.02), ("ur5", 1, 48, 5, 96, 0.4, 0.02)]
ITERATIONS = 5


def xi_table(seed, call, Hn, K, U, offset=0, hp=False):
    """[H, K, U]: xi(k, t, u) = the normal of (particle k + offset, step t, stream 3, index u); candidate 0 is zero."""
    t = np.arange(Hn, dtype=np.uint64)[:, None, None]
    k = (np.arange(K, dtype=np.uint64) + np.uint64(offset))[None, :, None]
    u = np.arange(U, dtype=np.uint64)[None, None, :]
    xi = nt.normal_hp(seed, call, k, t, STREAM_PLAN, u) if hp else nt.normal(seed, call, k, t, STREAM_PLAN, u)
    xi = np.array(np.broadcast_to(xi, (Hn, K, U)))
    xi[:, 0, :] = 0
    return xi


def squash(a, u_max, on):
    if not on:
        return a
    um = np.asarray(u_max, dtype=a.dtype)
    return um * np.tanh(a / um)


def candidate_inputs(a, sigma, xi, u_max=1.0, squashed=True):
    """u [H, K, U] = squash(a[t] + sigma xi(k, t, .))."""
    return squash(a[:, None, :] + np.asarray(sigma, dtype=a.dtype) * xi, u_max, squashed)


# ---- costs: a spec is a dict -- kind "target" | "target_quad" | "traj", idx, target ([n] or [rows, S]), ls; optional inputs: u_idx, u_ls (effort),
# u_rate (rate), u_target, joint ------------------------------------------------------------------------------------------------------------
def cost_specs(c, target_rows=12, seed=0):
    """The three descriptor pairs of the GPU cost test, and the behavioural tests' cost, for a model config ``c``."""
    gen = np.random.default_rng(40 + seed)
    S, U = c["S"], c["U"]
    idx = list(range(S))
    ph = 6.28 * gen.random((1, S))
    traj = 0.3 * np.sin(0.3 * np.arange(target_rows).reshape(-1, 1) + ph)
    return {
        "target_add": dict(kind="target", idx=idx[::-1][:max(2, S - 1)], target=0.2 * gen.standard_normal(max(2, S - 1)), ls=0.5 + gen.random(max(2, S - 1)),
                           u_idx=list(range(U)), u_ls=1.0 + gen.random(U), u_rate=0.5 + gen.random(U), u_target=0.1 * gen.standard_normal(U), joint=False),
        "traj_plain": dict(kind="traj", idx=idx[:S - 1], target=traj, ls=0.4 + gen.random(S - 1)),
        "quad_joint": dict(kind="target_quad", idx=idx[:2], target=0.2 * gen.standard_normal(2), ls=0.5 + gen.random(2),
                           u_idx=[U - 1], u_ls=np.array([1.5]), u_rate=None, u_target=None, joint=True),
        "effort": dict(kind="target", idx=idx, target=np.zeros(S), ls=np.full(S, 0.5), u_idx=list(range(U)), u_ls=np.full(U, 4.0), u_rate=None,
                       u_target=None, joint=False),
    }


def point_costs(spec, x, u, t0=0):
    """c [H, M] of states x [H, M, S] and inputs u [H, M, U] (numpy, any float dtype): the formulas of mcp_cost / mcp_cost_inputs, the
    target row t0 + t, the rate term 0 at t = 0, row H - 1 included."""
    dt = x.dtype.type
    Hn = x.shape[0]
    ls = np.asarray(spec["ls"], dtype=dt)
    if spec["kind"] == "traj":
        tg = np.asarray(spec["target"], dtype=dt)[t0:t0 + Hn][:, None, :][:, :, spec["idx"]]
    else:
        tg = np.asarray(spec["target"], dtype=dt)
    r = (x[:, :, spec["idx"]] - tg) / ls
    dx = (r * r).sum(2)
    du = dr = np.zeros_like(dx)
    if spec.get("u_idx") is not None:
        uu = u[:, :, spec["u_idx"]]
        if spec.get("u_ls") is not None:
            ut = dt(0) if spec.get("u_target") is None else np.asarray(spec["u_target"], dtype=dt)
            q = (uu - ut) / np.asarray(spec["u_ls"], dtype=dt)
            du = (q * q).sum(2)
        if spec.get("u_rate") is not None:
            q = (uu[1:] - uu[:-1]) / np.asarray(spec["u_rate"], dtype=dt)
            dr = np.concatenate([np.zeros_like(dx[:1]), (q * q).sum(2)])
    f = (lambda d: d) if spec["kind"] == "target_quad" else (lambda d: dt(1) - np.exp(-d))
    if spec.get("joint"):
        return f(dx + du + dr)
    return f(dx) + du + dr


def oracle_states(shape, m, x0, u, P, eps, sample, fam=None, var_scale=None, step=None):
    """states [H, K P, S] of the oracle's step loop from the ONE state x0 [S] on the inputs u [H, K, U] (row H - 1 moves nothing):
    trajectory k P + p takes candidate k's inputs and particle p's draws eps [H-1, P, G] (common random numbers).  ``fam``: the integrator
    by the name oracle_step knows it (tests/plan_models.py hands over layout_models.family(layout)); None: pd_models.family(shape), as
    ever.  ``var_scale``: handed to the step when given.  ``step``: a callable in oracle_step's place -- tests/plan_models.py's recording
    step and its deliberately wrong variants."""
    Hn, K, U = u.shape
    M = K * P
    fam = family(shape) if fam is None else fam
    step = oracle_step if step is None else step
    kw = {} if var_scale is None else dict(var_scale=var_scale)
    ut = torch.as_tensor(np.asarray(u, dtype=np.float64)).repeat_interleave(P, dim=1)
    xs = [torch.as_tensor(np.asarray(x0, dtype=np.float64)).reshape(1, -1).repeat(M, 1)]
    with torch.no_grad():
        for t in range(Hn - 1):
            e = torch.zeros(M, 1, dtype=DT) if eps is None else torch.as_tensor(np.asarray(eps[t], dtype=np.float64)).repeat(K, 1)
            xs.append(step(fam, m, xs[-1], ut[t], e, sample, **kw)[0])
    return torch.stack(xs).numpy(), ut.numpy()


def traj_costs(spec, x, u, w=None, t0=0, dt=np.float64):
    """J [M] = sum_t w_t c_t, added in ascending t."""
    c = point_costs(spec, x.astype(dt), u.astype(dt), t0)
    J = np.zeros(c.shape[1], dtype=dt)
    for t in range(c.shape[0]):
        J = J + (c[t] if w is None else dt(w[t]) * c[t])
    return J


# ---- the update ---------------------------------------------------------------------------------------------------------------------------
def update(J, a, sigma, xi, K, P, lam, kappa=0.0, dt=np.float64):
    """The header's update in ``dt``: J [K P], a [H, U], xi [H, K, U] (row 0 of the candidates is ignored: candidate 0 has xi = 0) ->
    (a_new [H, U], S [K], weights [K], stats [4] = S_min, argmin, 1 / sum w^2, sum w S).  A non-finite S_k has weight 0; none finite:
    a_new = a, weights 0, stats NaN, -1, 0, NaN."""
    J, a, sigma, xi = (np.asarray(v, dtype=dt) for v in (J, a, sigma, xi))
    Jk = J.reshape(K, P)
    S = np.zeros(K, dtype=dt)
    for p in range(P):
        S = S + Jk[:, p]
    S = S / dt(P)
    if kappa != 0.0:
        q = np.zeros(K, dtype=dt)
        for p in range(P):
            q = q + (Jk[:, p] - S) ** 2
        S = S + dt(kappa) * np.sqrt(q / dt(P - 1))
    fin = np.isfinite(S)
    if not fin.any():
        return a.copy(), S, np.zeros(K, dtype=dt), np.array([np.nan, -1, 0, np.nan], dtype=dt)
    kmin = int(np.flatnonzero(fin)[np.argmin(S[fin])])
    with np.errstate(invalid="ignore"):
        e = np.where(fin, np.exp(-(np.where(fin, S, S[kmin]) - S[kmin]) / dt(lam)), dt(0))
    w = e / e.sum()
    xi0 = np.where((w != 0)[None, :, None], xi, dt(0))
    xi0[:, 0, :] = 0
    a_new = a + sigma * np.einsum("k,hku->hu", w, xi0)
    stats = np.array([S[kmin], kmin, dt(1) / (w * w).sum(), (w[fin] * S[fin]).sum()], dtype=dt)
    return a_new, S, w, stats


def update_direct(J, a, sigma, xi, K, P, lam, kappa=0.0):
    """The same step written another way, in long double and for finite costs only: no shift by the minimum -- weights
    exp(-S / lam) / sum exp(-S / lam) --, the std from numpy, the mean as an explicit loop over candidates and rows."""
    ld = np.longdouble
    Jk = np.asarray(J, dtype=ld).reshape(K, P)
    S = Jk.mean(1) + (ld(kappa) * Jk.std(1, ddof=1) if kappa != 0.0 else ld(0))
    e = np.exp(-S / ld(lam))
    w = e / e.sum()
    a_new = np.asarray(a, dtype=ld).copy()
    sig = np.broadcast_to(np.asarray(sigma, dtype=ld), (a_new.shape[1],))
    for h in range(a_new.shape[0]):
        for u in range(a_new.shape[1]):
            acc = ld(0)
            for k in range(1, K):
                acc += w[k] * ld(xi[h, k, u])
            a_new[h, u] += sig[u] * acc
    return a_new, S, w


def d_ref(f64, ld):
    """Per output (a_new, S, weights): the largest difference between the float64 and the long-double update, relative to the output's
    largest entry (tests/lqr_models.d_ref's meaning)."""
    out = []
    for p, q in zip(f64[:3], ld[:3]):
        q = np.asarray(q, dtype=np.longdouble)
        out.append(float(np.abs(np.asarray(p, dtype=np.longdouble) - q).max() / np.abs(q).max()))
    return out


# ---- the planner --------------------------------------------------------------------------------------------------------------------------
def behaviour_operands(c, seed):
    """x0 [S] within +-0.3 and a zero warm start [H, U]."""
    gen = np.random.default_rng(900 + seed)
    return 0.6 * (gen.random(c["S"]) - 0.5), np.zeros((H, c["U"]))


def plan_truth(shape, m, c, x0, a, spec, K, P, iterations, sigma, lam, kappa=0.0, u_max=1.0, squashed=True, seed=0, call=0, eps=None,
               sample=False, t0=0, dt=np.float64):
    """``iterations`` x (candidates, oracle rollouts, costs, update), iteration i with the perturbations of call + i.  Returns
    (a, nominal cost per iteration = S[0], every iteration's S [iterations, K])."""
    a = np.asarray(a, dtype=dt)
    sig = np.full(c["U"], sigma, dtype=dt) if np.ndim(sigma) == 0 else np.asarray(sigma, dtype=dt)
    nominal, every = [], []
    for i in range(iterations):
        xi = xi_table(seed, call + i, a.shape[0], K, c["U"]).astype(dt)
        u = candidate_inputs(a, sig, xi, u_max, squashed)
        x, ut = oracle_states(shape, m, x0, u, P, eps, sample)
        J = traj_costs(spec, x, ut, None, t0, dt)
        a, S, w, stats = update(J, a, sig, xi, K, P, lam, kappa, dt)
        nominal.append(float(S[0]))
        every.append(np.asarray(S, dtype=np.float64))
    return a, nominal, np.stack(every)
