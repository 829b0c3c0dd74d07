"""The truth for the fused closed loop under the tanh-MLP policy (mcp_rollout_mlp / mcp_rollout_mlp_bwd): torch autograd through the oracle's
step (tests/open_grad_models.oracle_step over oracle/mcpilco_oracle.py) with the network written out here, on the model pairs and inputs of
tests/pd_models.py.  No GPU and no project code beyond the oracle.

    f = [x[non_angle], sin x[angle], cos x[angle]]  (no lists: f = x);   h1 = tanh(W0 f + b0);   [h2 = tanh(W1 h1 + b1)];
    a = Wout h + bout;   u = u_max tanh(a / u_max)  (or a);      L = sum w * states + sum wu * inputs
"""
import numpy as np
import torch

import layout_models
import pd_models
from open_grad_models import oracle_step
from pd_models import family, inputs_for  # noqa: F401  (re-exported: the GPU module builds its inputs from these)

DT = torch.float64
PAIR_SEED = 3

# pd_models' shapes and one at every compiled limit of the model at once (S = 16, U = 8, G = 8, D = 8 + 16 + 8 = 32; speed integration): with a
# (64, 64) network the sweep's layout for 16 trajectories does not fit the LDS, and a workgroup sweeps its tile in two parts of 8
SHAPES = dict(pd_models.SHAPES, limits=layout_models.LAYOUTS["limits"])


def build_pair(shape, N, deg, seed):
    """pd_models.build_pair, for the shapes of this module's table: (cfg, oracle model, per-GP (lengthscales, sigma_n, lam, poly_w))."""
    if shape in pd_models.SHAPES:
        return pd_models.build_pair(shape, N, deg, seed)
    return layout_models.build_pair(shape, N, deg, seed)  # (the same recipe and draws)


def feature_lists(c, opt):
    """(angle, non_angle) of the policy: the model's own lists unless the case names others; "state": no lists, f = x."""
    if opt.get("features") == "state":
        return [], []
    return list(opt.get("angle", c["angle"])), list(opt.get("non_angle", c["not_angle"]))


def network(c, hidden, angle, non_angle, seed):
    """[W0, b0, [W1, b1], Wout, bout]: weights randn / sqrt(fan_in), biases 0.1 randn, from the generator seeded 77 + seed."""
    gen = torch.Generator().manual_seed(77 + seed)
    P = len(non_angle) + 2 * len(angle) if (angle or non_angle) else c["S"]
    widths = [P] + list(hidden) + [c["U"]]
    out = []
    for l in range(len(widths) - 1):
        out.append(torch.randn(widths[l + 1], widths[l], dtype=DT, generator=gen) / np.sqrt(widths[l]))
        out.append(0.1 * torch.randn(widths[l + 1], dtype=DT, generator=gen))
    return out


def mlp_law(x, params, angle, non_angle, u_max, squash):
    f = torch.cat([x[:, non_angle], torch.sin(x[:, angle]), torch.cos(x[:, angle])], dim=1) if (angle or non_angle) else x
    h = f
    for l in range(len(params) // 2 - 1):
        h = torch.tanh(h @ params[2 * l].t() + params[2 * l + 1])
    a = h @ params[-2].t() + params[-1]
    if not squash:
        return a
    um = torch.as_tensor(u_max, dtype=DT)
    return um * torch.tanh(a / um)


def mlp_truth(shape, m, x0, params, eps, w, wu, sample, angle, non_angle, u_max=1.0, squash=True, var_scale=None):
    """Returns (states [T,M,S], inputs [T,M,U], [dL/dparam ...], dL/dx0, smallest variance met)."""
    x0 = x0.clone().requires_grad_(True)
    params = [q.clone().requires_grad_(True) for q in params]
    T = w.shape[0]
    law = lambda x: mlp_law(x, params, angle, non_angle, u_max, squash)
    xs, us, vmin = [x0], [law(x0)], float("inf")
    for t in range(1, T):
        nx, var = oracle_step(family(shape), m, xs[-1], us[-1], eps[t - 1], sample, var_scale)
        vmin = min(vmin, float(var.detach().min()))
        xs.append(nx)
        us.append(law(nx))
    st, inp = torch.stack(xs), torch.stack(us)
    L = (w * st).sum() + (0.0 if wu is None else (wu * inp).sum())
    grads = torch.autograd.grad(L, params + [x0], allow_unused=True)
    grads = [torch.zeros_like(q) if g is None else g for g, q in zip(grads, params + [x0])]
    return st.detach(), inp.detach(), grads[:-1], grads[-1], vmin


# (mode, shape, degree, N, T, M, hidden, options).  N = 37 (Npad 48: the last 32-row block of Kinv is a remainder) with T in {1, 2, 3, 12}
# and M in {1, 5, 17} (two tiles, the last one ragged), both modes, arm2 / arm2_delta / the UR5 shape (N = 48), degrees 0..2, the hidden sizes
# (1,), (5,), (64,), (7, 3), (33, 64), (64, 64) spread over them; N = 48 and N = 300 once; then once each: f = x, feature lists other than the
# model's, squashing off, a bound per input, no upstream g_inputs, var_scale != 1, requires_grad on one tensor only (options["only_grad"]: its
# place in the parameter order); M = 1041 three times
CASES = [
    ("mean", "arm2", 0, 37, 12, 17, (5,), {}), ("sampled", "arm2", 2, 37, 12, 17, (64, 64), {}),
    ("sampled", "arm2_delta", 1, 37, 12, 5, (7, 3), {}), ("sampled", "ur5", 1, 48, 3, 5, (64,), {}),
    ("mean", "ur5", 1, 48, 12, 1, (33, 64), {}), ("sampled", "arm2", 0, 300, 3, 17, (16,), {}),
    ("mean", "arm2", 1, 37, 1, 5, (1,), {}), ("sampled", "arm2", 1, 37, 2, 1, (64,), {}),
    ("mean", "arm2_delta", 2, 37, 3, 17, (7, 3), {}), ("sampled", "arm2_delta", 0, 37, 1, 17, (5,), {}),
    ("mean", "arm2", 2, 37, 2, 5, (33, 64), {}), ("mean", "arm2", 0, 48, 3, 5, (5,), {}),
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), {"features": "state"}),
    ("sampled", "arm2", 1, 37, 12, 5, (5,), {"angle": [1], "non_angle": [0, 3]}),
    ("sampled", "arm2", 1, 37, 3, 5, (5,), {"squash": False}),
    ("sampled", "arm2", 0, 37, 12, 5, (5,), {"u_max": [0.4, 1.7]}),
    ("mean", "arm2", 1, 37, 12, 5, (7, 3), {"no_g_inputs": True}),
    ("sampled", "arm2", 0, 37, 12, 5, (5,), {"var_scale": [0.49, 2.25]}),
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), {"only_grad": 2}),
    # swarms of up to 1024 trajectories run 4 per workgroup (csrc/rollout_mlp.hip, MLP_SMALL_SWARM): these three run 16, in 66 tiles, the last ragged
    ("sampled", "arm2", 1, 37, 3, 1041, (33, 64), {}), ("sampled", "ur5", 1, 48, 2, 1041, (5,), {}),
    ("sampled", "arm2", 0, 37, 3, 1041, (5,), {}),  # (the 16-trajectory forms of degree class 0)
    # the sweep's other paths, by its LDS layout (20 480 doubles): UR5 with (64, 64) needs 18 402 + 5 900 for the weights' copy -- 16 trajectories at
    # once with the weights read from global memory; every model limit at once with (64, 64) needs 23 106 even without the copy -- two parts of 8
    # (18 002 with it), here over two tiles, the second ragged (4 trajectories in its first part, none in its second)
    ("sampled", "ur5", 1, 48, 3, 5, (64, 64), {}), ("sampled", "limits", 0, 37, 3, 20, (64, 64), {}), ("mean", "limits", 0, 37, 2, 5, (64, 64), {}),
]


def case_id(c):
    return "-".join(str(v) for v in c[:6]) + "-h" + "x".join(str(h) for h in c[6]) + ("-" + "-".join(sorted(c[7])) if c[7] else "")


def case_truth(case):
    """Everything a case compares against: (cfg, oracle model, inputs dict, truth tuple)."""
    mode, shape, deg, N, T, M, hidden, opt = case
    c, m, specs = build_pair(shape, N, deg, seed=PAIR_SEED)
    seed = T * 100 + M
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=seed)
    if opt.get("no_g_inputs"):
        wu = None
    angle, non_angle = feature_lists(c, opt)
    params = network(c, hidden, angle, non_angle, seed)
    u_max, squash = opt.get("u_max", 1.0), opt.get("squash", True)
    torch.set_num_threads(1)
    truth = mlp_truth(shape, m, x0, params, eps, w, wu, mode == "sampled", angle, non_angle, u_max=u_max, squash=squash,
                      var_scale=opt.get("var_scale"))
    ins = dict(x0=x0, eps=eps, w=w, wu=wu, params=params, angle=angle, non_angle=non_angle, u_max=u_max, squash=squash, specs=specs)
    return c, m, ins, truth
