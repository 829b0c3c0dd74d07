"""The truth for the tanh-MLP policy WITH MEMORY in the fused closed loop (mcp_rollout_mlp_hist / mcp_rollout_mlp_hist_bwd): torch autograd
through tests/open_grad_models.oracle_step with the network and its window written out here -- a list of the rows the policy was shown, the
clamp at row 0, the newest block first.  Models and inputs are those of tests/mlp_models.py (build_pair with PAIR_SEED, inputs_for, seed =
100 T + M).  No GPU and no project code beyond the oracle.  (The fused forms with memory run on the true state only: r_t = x_t.)

    r_t = x_t;   phi(r) = [r[non_angle], sin r[angle], cos r[angle]]  (no lists: r), width P0
    f_t = [phi(r_t), phi(r_{t-1}), ..., phi(r_{t-H+1}), target[t][idx] - r_t[idx]],   r_{t-j} := r_0 for t - j < 0        (every row 0 .. T - 1)
    h_l = keep_l tanh(W_l h_{l-1} + b_l) / (1 - p);   a = Wout h + bout (+ kp^2 (pd_target[t][pos] - r_t[pos]) + kd^2 (pd_target[t][vel] - r_t[vel]))
    u = u_max tanh(a / u_max);   W0 is [h0][H P0 + n]:  the newest block's columns first, the errors' last;  L = sum w states + sum wu inputs
"""
import numpy as np
import torch

import mlp_models as mm
from mlp_models import family, inputs_for
from open_grad_models import oracle_step

DT = torch.float64
VARIANTS = ("zero_pad", "oldest_first", "oldest_dropped")      # the near misses of tests/test_mlp_hist_truth_cpu.py


def phi(r, angle, non_angle):
    return torch.cat([r[:, non_angle], torch.sin(r[:, angle]), torch.cos(r[:, angle])], dim=1) if (angle or non_angle) else r


def window(rows, angle, non_angle, H, variant=None):
    """The H blocks of the evaluation whose row is rows[-1], newest first.  ``variant``: a deliberately wrong window."""
    t = len(rows) - 1
    blocks = []
    for j in range(H):
        if t - j >= 0:
            blocks.append(phi(rows[t - j], angle, non_angle))
        elif variant == "zero_pad":
            blocks.append(torch.zeros_like(phi(rows[0], angle, non_angle)))
        else:
            blocks.append(phi(rows[0], angle, non_angle))  # rows before 0 repeat row 0
    if variant == "oldest_first":
        blocks = blocks[::-1]
    if variant == "oldest_dropped":
        blocks[-1] = torch.zeros_like(blocks[-1])
    return blocks


def hist_law(rows, params, angle, non_angle, H, u_max=1.0, squash=True, target=None, idx=(), res=None, keep=None, p=0.0, variant=None):
    """u_t of the evaluation whose row is rows[-1].  ``res``: dict(kp, kd, pos, vel, target) or None; ``keep``: [M, sum(hidden)] or None."""
    t, r = len(rows) - 1, rows[-1]
    parts = window(rows, angle, non_angle, H, variant)
    if len(idx):
        parts = parts + [target[t][list(idx)].reshape(1, -1) - r[:, list(idx)]]
    h, off, s = torch.cat(parts, dim=1), 0, 1.0 / (1.0 - p)
    for l in range(len(params) // 2 - 1):
        h = torch.tanh(h @ params[2 * l].t() + params[2 * l + 1])
        if keep is not None:
            width = h.shape[1]
            h = torch.where(keep[:, off:off + width].to(DT) > 0, s * h, torch.zeros_like(h))
            off += width
    a = h @ params[-2].t() + params[-1]
    if res is not None:
        e = res["target"][t].reshape(1, -1) - r
        a = a + res["kp"] ** 2 * e[:, res["pos"]] + res["kd"] ** 2 * e[:, res["vel"]]
    if not squash:
        return a
    um = torch.as_tensor(u_max, dtype=DT)
    return um * torch.tanh(a / um)


def hist_truth(shape, m, x0, params, eps, w, wu, sample, angle, non_angle, H, target=None, idx=(), res=None, masks=None, p=0.0, u_max=1.0,
               squash=True, variant=None):
    """Returns (states [T,M,S], inputs [T,M,U], [dL/dparam ... (, dL/dsqrt_kp, dL/dsqrt_kd)], dL/dx0, smallest variance met)."""
    x0 = x0.clone().requires_grad_(True)
    params = [q.clone().requires_grad_(True) for q in params]
    over = list(params)
    if res is not None:
        res = dict(res, kp=res["kp"].clone().requires_grad_(True), kd=res["kd"].clone().requires_grad_(True))
        over += [res["kp"], res["kd"]]
    T = w.shape[0]
    rows = []

    def law(r, t):
        rows.append(r)
        return hist_law(rows, params, angle, non_angle, H, u_max, squash, target, idx, res, None if masks is None else masks[t], p, variant)

    xs, us, vmin = [x0], [law(x0, 0)], float("inf")
    for t in range(1, T):
        nx, var = oracle_step(family(shape), m, xs[-1], us[-1], eps[t - 1], sample, None)
        vmin = min(vmin, float(var.detach().min()))
        xs.append(nx)
        us.append(law(nx, t))
    st, inp = torch.stack(xs), torch.stack(us)
    L = (w * st).sum() + (0.0 if wu is None else (wu * inp).sum())
    grads = torch.autograd.grad(L, over + [x0], allow_unused=True)
    grads = [torch.zeros_like(q) if g is None else g for g, q in zip(grads, over + [x0])]
    return st.detach(), inp.detach(), grads[:-1], grads[-1], vmin


def network(c, hidden, P, seed):
    """[W0 [h0][P], b0, [W1, b1], Wout, bout]: weights randn / sqrt(fan_in), biases 0.1 randn, from the generator seeded 77 + seed."""
    gen = torch.Generator().manual_seed(77 + seed)
    widths = [P] + list(hidden) + [c["U"]]
    out = []
    for l in range(len(widths) - 1):
        out.append(torch.randn(widths[l + 1], widths[l], dtype=DT, generator=gen) / np.sqrt(widths[l]))
        out.append(0.1 * torch.randn(widths[l + 1], dtype=DT, generator=gen))
    return out


def target_for(c, T, x0, phase=0.0):
    """[T, S]: smooth and strongly time-varying around the swarm's mean start, x0_mean[s] + 0.3 sin(0.7 t + s + phase)."""
    t = torch.arange(T, dtype=DT).reshape(-1, 1)
    return x0.mean(0).reshape(1, -1) + 0.3 * torch.sin(0.7 * t + torch.arange(c["S"], dtype=DT).reshape(1, -1) + phase)


def gains_for(U, seed):
    """sqrt_kp in [1.3, 1.7], sqrt_kd in [0.5, 0.8]."""
    gen = torch.Generator().manual_seed(4000 + seed)
    return 1.3 + 0.4 * torch.rand(U, dtype=DT, generator=gen), 0.5 + 0.3 * torch.rand(U, dtype=DT, generator=gen)


def masks_for(T, M, hidden, p, seed):
    """[T, M, sum(hidden)] uint8 keep decisions at probability 1 - p."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(T, M, sum(hidden), dtype=DT, generator=gen) >= p).to(torch.uint8)


def feature_lists(c, opt):
    """(angle, non_angle) of the policy: "state": no lists (f = x); "positions": the first S / 2 components as they are; else the case's own
    lists or the model's."""
    if opt.get("features") == "state":
        return [], []
    if opt.get("features") == "positions":
        return [], list(range(c["S"] // 2))
    return list(opt.get("angle", c["angle"])), list(opt.get("non_angle", c["not_angle"]))


# (mode, shape, degree, N, T, M, hidden, H, options): the smallest shapes at which each piece of the history forms can go wrong -- N = 37
# (Npad 48; UR5: 48).  Options: "features" ("state" / "positions"), "idx" the error indices (default: none), "res" the PD term with trainable
# gains, "p" dropout with buffer masks, "only_grad" requires_grad on that tensor alone.
CASES = [
    ("sampled", "arm2", 0, 37, 12, 17, (5,), 2, {}),                       # two tiles, one ragged; the window proper
    ("sampled", "arm2", 2, 37, 6, 17, (7, 3), 4, {}),                      # P = 24: the deepest window, two hidden layers
    ("mean", "arm2_delta", 1, 37, 2, 5, (5,), 4, {}),                      # T < H: every history block is clamped onto row 0
    ("sampled", "arm2", 1, 37, 1, 5, (5,), 3, {}),                         # T = 1: the policy alone, f_0 = three copies
    ("sampled", "ur5", 1, 48, 6, 5, (33, 64), 2, {"features": "state"}),   # f = x, P = 24
    ("sampled", "ur5", 1, 48, 6, 5, (7, 3), 4, {"features": "positions", "idx": [6, 1, 8, 3, 10, 5]}),  # P = 24 + 6 = 30: the errors behind the last block
    ("sampled", "arm2", 1, 37, 6, 17, (7, 3), 3, {"res": True, "idx": [3, 0]}),  # the PD term, trainable gains, errors
    ("sampled", "arm2", 0, 37, 6, 5, (7, 3), 2, {"p": 0.25}),              # dropout, buffer masks
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), 2, {"only_grad": 0}),         # requires_grad on W0 alone
    ("sampled", "limits", 0, 37, 3, 20, (64, 64), 2, {"features": "state"}),  # P = 32 exactly; the sweep in parts, two tiles
    ("mean", "limits", 0, 37, 2, 5, (64, 64), 2, {"features": "state"}),
    ("sampled", "ur5", 1, 48, 3, 5, (64, 64), 2, {"features": "positions"}),  # the sweep reads the weights from global memory
    ("sampled", "arm2", 0, 37, 3, 1041, (5,), 2, {}),                      # the 16-trajectory forward forms
]

def case_id(c):
    tags = []
    for k in sorted(c[8]):
        v = c[8][k]
        tags.append(k + ".".join(str(i) for i in v) if k == "idx" else "%s%s" % (k, v) if k in ("p", "only_grad", "features") else k)
    return "-".join(str(v) for v in c[:6]) + "-h" + "x".join(str(h) for h in c[6]) + "-H%d" % c[7] + ("-" + "-".join(tags) if tags else "")


def case_inputs(case):
    """(cfg, oracle model, inputs dict) of a case."""
    mode, shape, deg, N, T, M, hidden, H, opt = case
    c, m, specs = mm.build_pair(shape, N, deg, seed=mm.PAIR_SEED)
    seed = T * 100 + M
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=seed)
    angle, non_angle = feature_lists(c, opt)
    idx = list(opt.get("idx", ()))
    P0 = len(non_angle) + 2 * len(angle) if (angle or non_angle) else c["S"]
    params = network(c, hidden, H * P0 + len(idx), seed)
    target = target_for(c, T, x0) if (idx or opt.get("res")) else None
    res = None
    if opt.get("res"):
        kp, kd = gains_for(c["U"], seed)
        res = dict(kp=kp, kd=kd, pos=list(range(c["U"])), vel=list(range(c["S"] // 2, c["S"] // 2 + c["U"])), target=target_for(c, T, x0, 1.3))
    p = opt.get("p", 0.0)
    masks = masks_for(T, M, hidden, p, 5000 + seed) if p > 0.0 else None
    return c, m, dict(x0=x0, eps=eps, w=w, wu=wu, params=params, angle=angle, non_angle=non_angle, H=H, P0=P0, target=target, idx=idx, res=res,
                      masks=masks, p=p, sample=mode == "sampled", shape=shape, specs=specs)


def truth_of(m, ins, variant=None, **edit):
    """hist_truth on a case's inputs; ``edit`` replaces entries of the inputs, ``variant`` names a near miss."""
    q = dict(ins, **edit)
    torch.set_num_threads(1)
    return hist_truth(q["shape"], m, q["x0"], q["params"], q["eps"], q["w"], q["wu"], q["sample"], q["angle"], q["non_angle"], q["H"], q["target"],
                      q["idx"], q["res"], q["masks"], q["p"], variant=variant)


_TRUTHS = {}


def case_truth(case):
    """Everything a case compares against: (cfg, oracle model, inputs dict, truth tuple) -- computed once per process and shared, never modified."""
    key = case_id(case)
    if key not in _TRUTHS:
        c, m, ins = case_inputs(case)
        _TRUTHS[key] = (c, m, ins, truth_of(m, ins))
    return _TRUTHS[key]
