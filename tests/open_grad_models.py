"""Synthetic model pairs for the open-loop gradient tests: an oracle model (oracle/mcpilco_oracle.py, its own pretrain) and, on the GPU, the
PackedModel on the oracle's own Kinv / alpha -- built the way tests/test_gpu_open_rollout.py::test_against_the_oracle_loops pairs them, at a
training-set size of the test's choosing.  CPU side only imports torch and the oracle."""
import numpy as np
import torch

from helpers import hyper
from oracle import mcpilco_oracle as orc

DT = torch.float64

SHAPES = {
    # cart-pole layout: one angle, D = 6, two GPs (speed integration)
    "speed": dict(S=4, U=1, G=2, angle=[2], not_angle=[0, 1, 3], vel=[1, 3], not_vel=[0, 2], Ts=0.05),
    # delta-state model with S = G = 4 and one angle
    "delta": dict(S=4, U=1, G=4, angle=[2], not_angle=[0, 1, 3], vel=[0, 1, 2, 3], not_vel=[-1] * 4, Ts=0.0),
    # UR5-shaped: six joint angles, D = 6 + 12 + 6 = 24, six GPs (the wide phase-J path: D + 1 > 16, two row blocks)
    "ur5": dict(S=12, U=6, G=6, angle=list(range(6)), not_angle=list(range(6, 12)), vel=list(range(6, 12)), not_vel=list(range(6)), Ts=0.02),
}


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
            poly.append((0.05 + 0.1 * torch.rand(2 * D, dtype=DT, generator=gen)).numpy())  # (small: the rolled-out states stay O(1))
        h = hyper(ls, 0.1, 1.0, poly)
        hyp.append(h)
        caches.append(orc.pretrain_gp(h, X, Y))
        specs.append((ls, 0.1, 1.0, poly))
    if shape == "delta":
        m = orc.DeltaModel(hyp, caches, c["angle"], c["not_angle"])
    else:
        m = orc.SpeedModel(hyp, caches, c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    return c, m, specs


def inputs_for(c, M, T, seed, shared=False):
    gen = torch.Generator().manual_seed(1000 + seed)
    x0 = 0.6 * (torch.rand(M, c["S"], dtype=DT, generator=gen) - 0.5)
    u = torch.rand(T - 1, 1 if shared else M, c["U"], dtype=DT, generator=gen) * 2 - 1
    eps = torch.randn(T - 1, M, c["G"], dtype=DT, generator=gen)
    w = torch.randn(T, M, c["S"], dtype=DT, generator=gen)
    return x0, u, eps, w


def oracle_step(shape, m, x, u, eps, sample, var_scale=None):
    """orc.next_state / orc.delta_next_state; with ``var_scale`` (flg_norm: Model_learning.py:220-221 scales the GP variances by
    norm_list^2 before sampling) the same step written out on the oracle's posterior.  "mixed" (the layouts of tests/layout_models.py: GPs
    with and without an integrated position in one model, components nothing integrates): orc.mixed_next_state, which takes ``var_scale``
    itself.  Returns (next state, scaled variances)."""
    if shape == "mixed":
        nx, _, var = orc.mixed_next_state(m, x, u, eps, sample, var_scale)
        return nx, var
    if var_scale is None:
        nx, _, var = (orc.delta_next_state if shape == "delta" else orc.next_state)(m, x, u, eps, sample)
        return nx, var
    assert shape == "speed"
    _, mus, vrs = orc.one_step_gp_out(m, x, u)
    dmu, dvar = torch.cat(mus, 1), torch.cat(vrs, 1) * torch.as_tensor(var_scale, dtype=DT)
    delta = dmu + torch.sqrt(dvar) * eps if sample else dmu
    nxt = torch.zeros_like(x)
    nxt[:, list(m.vel)] = x[:, list(m.vel)] + delta
    nxt[:, list(m.not_vel)] = x[:, list(m.not_vel)] + m.Ts * x[:, list(m.vel)] + m.Ts / 2 * delta
    return nxt, dvar


def oracle_truth(shape, m, x0, u, eps, w, sample, lengths=None, var_scale=None):
    """Loop of the oracle's differentiable step; L = sum w * states; returns (states [T,M,S] with zero rows beyond a length, dL/dx0, dL/du in
    u's shape, smallest variance met on the rows that count)."""
    x0 = x0.clone().requires_grad_(True)
    u = u.clone().requires_grad_(True)
    T, M = u.shape[0] + 1, x0.shape[0]
    lens = torch.full((M,), T, dtype=torch.long) if lengths is None else torch.as_tensor(lengths, dtype=torch.long)
    xs, vmin = [x0], float("inf")
    for t in range(T - 1):
        nx, var = oracle_step(shape, m, xs[-1], u[t].expand(M, -1), eps[t], sample, var_scale)
        live = (t + 1 < lens)
        if live.any():
            vmin = min(vmin, float(var.detach()[live].min()))
        xs.append(nx)
    st = torch.stack(xs)
    mask = (torch.arange(T).reshape(T, 1) < lens.reshape(1, M)).to(DT).reshape(T, M, 1)
    st = torch.where(mask > 0, st, torch.zeros_like(st))
    L = (w * st).sum()
    gx, gu = torch.autograd.grad(L, [x0, u], allow_unused=True)
    gu = torch.zeros_like(u) if gu is None else gu
    return st.detach(), gx, gu, vmin


# (mode, shape, degree, N, T, M, var_scale): every (mode x family x degree) at N = 37; every N in {37, 48, 300}, T in {2, 3, 12}, M in {1, 5, 17};
# the UR5-shaped D = 24 model at N = 48; var_scale != 1 once
CASES = [
    ("mean", "speed", 0, 37, 2, 1, None), ("mean", "speed", 1, 37, 3, 5, None), ("mean", "speed", 2, 37, 12, 17, None),
    ("mean", "delta", 0, 37, 12, 5, None), ("mean", "delta", 1, 37, 2, 17, None), ("mean", "delta", 2, 37, 3, 1, None),
    ("sampled", "speed", 0, 37, 12, 17, None), ("sampled", "speed", 1, 37, 2, 5, None), ("sampled", "speed", 2, 37, 3, 1, None),
    ("sampled", "delta", 0, 37, 3, 17, None), ("sampled", "delta", 1, 37, 12, 1, None), ("sampled", "delta", 2, 37, 12, 5, None),
    ("sampled", "speed", 0, 48, 12, 5, None), ("mean", "speed", 2, 48, 3, 1, None),
    ("sampled", "speed", 0, 300, 3, 17, None), ("mean", "speed", 0, 300, 12, 1, None),
    ("sampled", "ur5", 1, 48, 3, 5, None), ("mean", "ur5", 1, 48, 12, 1, None), ("sampled", "ur5", 2, 48, 2, 17, None),
    ("sampled", "speed", 0, 37, 12, 5, [0.49, 2.25]),
]
