"""Synthetic model pairs and the truth for the fused closed loop under the PD controller (mcp_rollout_pd / mcp_rollout_pd_bwd): an oracle
model (oracle/mcpilco_oracle.py, its own pretrain) and torch autograd through its step with the policy formula written out
(reference policy_learning/Policy.py:437-449 inside MC_PILCO.apply_policy, MC_PILCO.py:615-674).  Built the way
tests/open_grad_models.py::build_pair builds its pairs, with a table of its own.  CPU side only imports torch, helpers and the oracle."""
import numpy as np
import torch

import layout_models
from helpers import hyper
from open_grad_models import SHAPES as _OPEN_SHAPES
from open_grad_models import oracle_step
from oracle import mcpilco_oracle as orc

DT = torch.float64

SHAPES = {
    # two-joint arm: two angles, D = 2 + 4 + 2 = 8, speed integration with two GPs
    "arm2": dict(S=4, U=2, G=2, angle=[0, 1], not_angle=[2, 3], vel=[2, 3], not_vel=[0, 1], Ts=0.05),
    # the same features as a delta-state model, one GP per state component
    "arm2_delta": dict(S=4, U=2, G=4, angle=[0, 1], not_angle=[2, 3], vel=[0, 1, 2, 3], not_vel=[-1] * 4, Ts=0.05),
    "ur5": dict(_OPEN_SHAPES["ur5"]),
}


def family(shape):
    """The name tests/open_grad_models.oracle_step knows the integrator by (the layouts of tests/layout_models.py: "mixed", and "delta"
    for its delta-state one)."""
    if shape in layout_models.LAYOUTS:
        return layout_models.family(shape)
    return "delta" if shape == "arm2_delta" else "speed"


def build_pair(shape, N, deg, seed):
    """(cfg, oracle model, per-GP (lengthscales, sigma_n, lam, poly_w))."""
    c = SHAPES[shape]
    D = len(c["not_angle"]) + 2 * len(c["angle"]) + c["U"]
    gen = torch.Generator().manual_seed(seed)
    X = torch.rand(N, D, dtype=DT, generator=gen) * 2 - 1
    hyp, caches, specs = [], [], []
    for g in range(c["G"]):
        w = torch.randn(D, 1, dtype=DT, generator=gen) / np.sqrt(D)
        Y = 0.3 * torch.sin(2.0 * X @ w) + 0.01 * torch.randn(N, 1, dtype=DT, generator=gen)
        ls = (1.5 + torch.rand(D, dtype=DT, generator=gen)).numpy()
        poly = None
        if deg >= 1:
            poly = [(0.1 + 0.2 * torch.rand(D + 1, dtype=DT, generator=gen)).numpy()]
        if deg >= 2:
            poly.append((0.05 + 0.1 * torch.rand(2 * D, dtype=DT, generator=gen)).numpy())
        h = hyper(ls, 0.1, 1.0, poly)
        hyp.append(h)
        caches.append(orc.pretrain_gp(h, X, Y))
        specs.append((ls, 0.1, 1.0, poly))
    if family(shape) == "delta":
        m = orc.DeltaModel(hyp, caches, c["angle"], c["not_angle"])
    else:
        m = orc.SpeedModel(hyp, caches, c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    return c, m, specs


def inputs_for(c, M, T, seed):
    """x0 as open_grad_models.inputs_for draws it; gains sqrt_kp in [0.5, 1.5], sqrt_kd in [0.2, 0.8]; a smooth target within +-0.3 (T + 2
    rows); eps; the weights of L on states and inputs."""
    gen = torch.Generator().manual_seed(1000 + seed)
    S, U = c["S"], c["U"]
    x0 = 0.6 * (torch.rand(M, S, dtype=DT, generator=gen) - 0.5)
    kp = 0.5 + torch.rand(U, dtype=DT, generator=gen)
    kd = 0.2 + 0.6 * torch.rand(U, dtype=DT, generator=gen)
    ph = 6.28 * torch.rand(1, S, dtype=DT, generator=gen)
    target = 0.3 * torch.sin(0.3 * torch.arange(T + 2, dtype=DT).reshape(-1, 1) + ph)
    eps = torch.randn(max(T - 1, 0), M, c["G"], dtype=DT, generator=gen)
    w = torch.randn(T, M, S, dtype=DT, generator=gen)
    wu = torch.randn(T, M, U, dtype=DT, generator=gen)
    return x0, kp, kd, target, eps, w, wu


def pd_law(x, t, kp, kd, target, u_max, squash, pos, vel):
    """Policy.py:437-449: e = target[t] - x; u = squash(kp^2 e_pos + kd^2 e_vel)."""
    err = target[t].reshape(1, -1) - x
    a = kp ** 2 * err[:, pos] + kd ** 2 * err[:, vel]
    if not squash:
        return a
    um = torch.as_tensor(u_max, dtype=DT)
    return um * torch.tanh(a / um)


def pd_truth(shape, m, x0, kp, kd, target, eps, w, wu, sample, u_max=1.0, squash=True, var_scale=None, pos=None, step=oracle_step):
    """torch autograd through oracle_step with the policy formula written out.  L = sum w * states + sum wu * inputs (wu None: states only).
    Returns (states [T,M,S], inputs [T,M,U], dL/dsqrt_kp, dL/dsqrt_kd, dL/dx0, smallest variance met).  ``pos`` / ``step``: other position
    indices than the rule's, another step than oracle_step -- the deliberately wrong variants of tests/test_layout_models_cpu.py."""
    S, U = x0.shape[1], kp.shape[0]
    h = S // 2
    pos, vel = list(range(U)) if pos is None else list(pos), list(range(h, h + U))
    x0 = x0.clone().requires_grad_(True)
    kp = kp.clone().requires_grad_(True)
    kd = kd.clone().requires_grad_(True)
    T = w.shape[0]
    xs, us, vmin = [x0], [pd_law(x0, 0, kp, kd, target, u_max, squash, pos, vel)], float("inf")
    for t in range(1, T):
        nx, var = step(family(shape), m, xs[-1], us[-1], eps[t - 1], sample, var_scale)
        vmin = min(vmin, float(var.detach().min()))
        xs.append(nx)
        us.append(pd_law(nx, t, kp, kd, target, u_max, squash, pos, vel))
    st, inp = torch.stack(xs), torch.stack(us)
    L = (w * st).sum() + (0.0 if wu is None else (wu * inp).sum())
    gkp, gkd, gx = torch.autograd.grad(L, [kp, kd, x0])
    return st.detach(), inp.detach(), gkp, gkd, gx, vmin


# (mode, shape, degree, N, T, M, options): every (mode x {arm2, arm2_delta} x degree) at N = 37 (Npad 48: the last 32-row block of Kinv is a
# remainder) with T in {1, 2, 3, 12} and M in {1, 5, 17} (two tiles, the last one ragged) spread over them; N = 48 and N = 300 once per mode;
# the UR5 shape (D = 24, U = 6) at N = 48 in both modes; squashing off, a bound per input, no upstream g_inputs, var_scale != 1 once each
CASES = [
    ("mean", "arm2", 0, 37, 1, 5, {}), ("mean", "arm2", 1, 37, 3, 17, {}), ("mean", "arm2", 2, 37, 12, 1, {}),
    ("mean", "arm2_delta", 0, 37, 12, 17, {}), ("mean", "arm2_delta", 1, 37, 2, 1, {}), ("mean", "arm2_delta", 2, 37, 3, 5, {}),
    ("sampled", "arm2", 0, 37, 12, 17, {}), ("sampled", "arm2", 1, 37, 2, 5, {}), ("sampled", "arm2", 2, 37, 3, 1, {}),
    ("sampled", "arm2_delta", 0, 37, 1, 17, {}), ("sampled", "arm2_delta", 1, 37, 12, 1, {}), ("sampled", "arm2_delta", 2, 37, 12, 5, {}),
    ("mean", "arm2", 0, 48, 3, 5, {}), ("sampled", "arm2", 0, 48, 12, 5, {}),
    ("mean", "arm2", 0, 300, 12, 1, {}), ("sampled", "arm2", 0, 300, 3, 17, {}),
    ("mean", "ur5", 1, 48, 12, 1, {}), ("sampled", "ur5", 1, 48, 3, 5, {}),
    ("sampled", "arm2", 1, 37, 3, 5, {"squash": False}),
    ("sampled", "arm2", 0, 37, 12, 5, {"u_max": [0.4, 1.7]}),
    ("mean", "arm2", 1, 37, 12, 5, {"no_g_inputs": True}),
    ("sampled", "arm2", 0, 37, 12, 5, {"var_scale": [0.49, 2.25]}),
]


def case_id(c):
    return "-".join(str(v) for v in c[:6]) + ("-" + "-".join(sorted(c[6])) if c[6] else "")


def golden_model(fx, kind):
    """The oracle model of a rollout_pd.npz fixture, on the reference's own alpha / Kinv."""
    k = lambda n: fx[kind + "_" + n]
    G = k("eps").shape[2]
    T_ = lambda a: torch.as_tensor(np.asarray(a), dtype=DT)
    hyp = [hyper(k("lengthscales"), float(k("sigma_n")), 1.0, None) for _ in range(G)]
    caches = [orc.GPCache(T_(k("Xtr%d" % g)), T_(k("alpha%d" % g)), T_(k("Kinv%d" % g)), None) for g in range(G)]
    angle, not_angle = [int(i) for i in k("angle")], [int(i) for i in k("not_angle")]
    if kind == "delta":
        return orc.DeltaModel(hyp, caches, angle, not_angle)
    return orc.SpeedModel(hyp, caches, float(k("Ts")), angle, not_angle, [int(i) for i in k("vel")], [int(i) for i in k("not_vel")])
