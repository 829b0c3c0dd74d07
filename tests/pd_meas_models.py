"""The truth for the fused closed loop under the PD controller ON A SIMULATED MEASUREMENT (mcp_rollout_pd_meas / mcp_rollout_pd_meas_bwd):
torch autograd through tests/open_grad_models.oracle_step with the measurement formulas of the reference's MC_PILCO4PMS.apply_policy
(policy_learning/MC_PILCO.py:856-899) and the PD law (policy_learning/Policy.py:437-449) written out.  Models, inputs and the PD law are those
of tests/pd_models.py; this module adds the measurement model, its noise and the table of GPU cases.  CPU side only imports torch, helpers and
the oracle."""
import torch

from open_grad_models import oracle_step
from pd_models import SHAPES, family, pd_law

DT = torch.float64

# scipy.signal.butter(1, 0.5) is (b, a) = ([0.5, 0.5], [1, 0]) up to rounding: a filter without memory.  The tests take coefficients of their own
# so that every term of the recursion carries weight (a1 != 0, b0 != b1, a0 != 1).
FILTER = dict(b=[0.42, 0.31], a=[1.25, -0.38])


def meas_model(shape, variant="all", std=0.1, shapes=SHAPES):
    """{pos, vel, std, b, a, Ts} of a case on a shape of the table ``shapes``: every joint measured, one pair only, or the pairs listed in
    reverse order."""
    c = shapes[shape]
    h = c["S"] // 2
    pos, vel = list(range(h)), list(range(h, 2 * h))
    if variant == "one":
        pos, vel = pos[:1], vel[:1]
    elif variant == "reversed":
        pos, vel = pos[::-1], vel[::-1]
    elif variant != "all":
        raise ValueError(variant)
    stds = [std * (1.0 + 0.5 * i) for i in range(len(pos))] if std else [0.0] * len(pos)  # (one std per pair: a swapped column shows)
    return dict(pos=pos, vel=vel, std=stds, b=list(FILTER["b"]), a=list(FILTER["a"]), Ts=c["Ts"])


def pos_noise_for(T, M, n, seed):
    gen = torch.Generator().manual_seed(7000 + seed)
    return torch.randn(max(T - 1, 0), M, n, dtype=DT, generator=gen)


def measure(x, t, ms, pos_noise, hist, defect=None):
    """y_t of the true state x [M,S] (MC_PILCO.py:856-899).  ``hist``: (noisy_{t-1}, meas_{t-1}) or None at t = 0; returns (y_t, new hist).
    ``defect`` names a deliberately wrong variant (the sensitivity checks of tests/test_pd_meas_cpu.py)."""
    pos, vel = list(ms["pos"]), list(ms["vel"])
    b0, b1 = ms["b"]
    a0, a1 = ms["a"]
    if defect == "no_b1":
        b1 = 0.0
    if defect == "no_a1":
        a1 = 0.0
    if t == 0:
        if defect == "row0_filtered":  # row 0 treated like the other rows: the filter starts at rest, the velocity measured in row 0 is its output 0
            x = x * torch.tensor([0.0 if s in vel else 1.0 for s in range(x.shape[1])], dtype=DT)
        return x, (x, x)  # the measurement is the true state, and it starts both histories
    std = torch.as_tensor(ms["std"], dtype=DT)
    n = pos_noise[t - 1]
    if defect == "swap_columns":
        n = n.flip(1)
    noisy_prev, meas_prev = hist
    cols = [None] * x.shape[1]
    npos = x[:, pos] + std * n
    nvel = (npos - noisy_prev[:, pos]) / ms["Ts"]
    mvel = (b0 * nvel + b1 * noisy_prev[:, vel] - a1 * meas_prev[:, vel]) / a0
    for s in range(x.shape[1]):
        cols[s] = x[:, s]
    noisy, meas = list(cols), list(cols)
    for i, (p, v) in enumerate(zip(pos, vel)):
        noisy[p] = meas[p] = npos[:, i]
        noisy[v] = nvel[:, i]
        meas[v] = mvel[:, i]
    noisy, meas = torch.stack(noisy, 1), torch.stack(meas, 1)
    return meas, (noisy, meas)


def pd_meas_truth(shape, m, x0, kp, kd, target, eps, pos_noise, w, wu, sample, ms, u_max=1.0, squash=True, var_scale=None, defect=None):
    """torch autograd through oracle_step with the measurement and the policy written out.  L = sum w * states + sum wu * inputs (wu None:
    states only).  Returns (states [T,M,S], inputs [T,M,U], measurements [T,M,S], dL/dsqrt_kp, dL/dsqrt_kd, dL/dx0, smallest variance met)."""
    S, U = x0.shape[1], kp.shape[0]
    h = S // 2
    ppos, pvel = list(range(U)), list(range(h, h + U))
    x0 = x0.clone().requires_grad_(True)
    kp = kp.clone().requires_grad_(True)
    kd = kd.clone().requires_grad_(True)
    T = w.shape[0]
    y, hist = measure(x0, 0, ms, pos_noise, None, defect)
    xs, ys, us, vmin = [x0], [y], [pd_law(y, 0, kp, kd, target, u_max, squash, ppos, pvel)], float("inf")
    for t in range(1, T):
        nx, var = oracle_step(family(shape), m, xs[-1], us[-1], eps[t - 1], sample, var_scale)
        vmin = min(vmin, float(var.detach().min()))
        y, hist = measure(nx, t, ms, pos_noise, hist, defect)
        xs.append(nx)
        ys.append(y)
        us.append(pd_law(y, t, kp, kd, target, u_max, squash, ppos, pvel))
    st, inp, ym = torch.stack(xs), torch.stack(us), torch.stack(ys)
    L = (w * st).sum() + (0.0 if wu is None else (wu * inp).sum())
    gkp, gkd, gx = torch.autograd.grad(L, [kp, kd, x0])
    return st.detach(), inp.detach(), ym.detach(), gkp, gkd, gx, vmin


def loss_of(shape, m, x0, kp, kd, target, eps, pos_noise, w, wu, sample, ms, **kw):
    """L alone (the central differences of tests/test_pd_meas_cpu.py)."""
    st, inp, *_ = pd_meas_truth(shape, m, x0, kp, kd, target, eps, pos_noise, w, wu, sample, ms, **kw)
    return float((w * st).sum() + (0.0 if wu is None else (wu * inp).sum()))


# (mode, shape, degree, N, T, M, measurement variant, options): the base shapes of pd_models.CASES at N = 37 (Npad 48: a remainder block of
# Kinv) with degree 0 / 1 / 2, mean and sampled, T in {1, 2, 3, 12} (the policy on the true state | the one step whose history is row 0 | the
# first row whose two carries are both live | the recursion proper) and M in {1, 5, 17} spread over them; N = 300 once; one pair only and the
# pairs in reverse order on arm2; std = 0; the UR5 shape with six pairs; squashing off, a bound per input, no upstream g_inputs and
# var_scale != 1 once each
CASES = [
    ("mean", "arm2", 0, 37, 1, 5, "all", {}), ("mean", "arm2", 1, 37, 2, 17, "all", {}), ("mean", "arm2", 2, 37, 12, 1, "all", {}),
    ("mean", "arm2_delta", 0, 37, 12, 17, "all", {}), ("mean", "arm2_delta", 1, 37, 3, 1, "all", {}), ("mean", "arm2_delta", 2, 37, 2, 5, "all", {}),
    ("sampled", "arm2", 0, 37, 12, 17, "all", {}), ("sampled", "arm2", 1, 37, 3, 5, "all", {}), ("sampled", "arm2", 2, 37, 2, 1, "all", {}),
    ("sampled", "arm2_delta", 0, 37, 1, 17, "all", {}), ("sampled", "arm2_delta", 1, 37, 12, 1, "all", {}), ("sampled", "arm2_delta", 2, 37, 12, 5, "all", {}),
    ("sampled", "arm2", 0, 300, 3, 17, "all", {}),
    ("sampled", "arm2", 0, 37, 12, 5, "one", {}), ("mean", "arm2", 1, 37, 12, 5, "one", {}),
    ("sampled", "arm2", 1, 37, 12, 17, "reversed", {}), ("mean", "arm2_delta", 0, 37, 3, 5, "reversed", {}),
    ("sampled", "arm2", 0, 37, 12, 5, "all", {"std": 0.0}),
    ("mean", "ur5", 1, 48, 12, 1, "all", {}), ("sampled", "ur5", 1, 48, 3, 5, "all", {}),
    ("sampled", "arm2", 1, 37, 3, 5, "all", {"squash": False}),
    ("sampled", "arm2", 0, 37, 12, 5, "all", {"u_max": [0.4, 1.7]}),
    ("mean", "arm2", 1, 37, 12, 5, "all", {"no_g_inputs": True}),
    ("sampled", "arm2", 0, 37, 12, 5, "all", {"var_scale": [0.49, 2.25]}),
]


def case_id(c):
    return "-".join(str(v) for v in c[:7]) + ("-" + "-".join(sorted(c[7])) if c[7] else "")
