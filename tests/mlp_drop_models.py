"""The truth for DROPOUT in the fused closed loop under the tanh-MLP policy (mcp_rollout_mlp_drop / mcp_rollout_mlp_drop_bwd): the loops of
tests/mlp_models.mlp_truth and tests/mlp_meas_models.mlp_meas_truth -- torch autograd through tests/open_grad_models.oracle_step -- with the
network written out here WITH its keep-masks.  Models, networks and inputs are those of tests/mlp_models.py (build_pair with PAIR_SEED,
network, inputs_for, seed = 100 T + M), the measurement model and its noise those of tests/mlp_meas_models.py; the masks come from a seeded
CPU generator.  No GPU and no project code beyond the oracle.

    s = 1 / (1 - p);   h_l[j] = keep[t, m, off_l + j] ? s tanh(pre_l[j]) : 0,   off_0 = 0, off_1 = h[0];   features, the output layer and the
    squashing are never dropped;   one mask row per policy evaluation (T rows, row T - 1 included)
"""
import torch

import mlp_meas_models as mmm
import mlp_models as mm
import pd_meas_models as pm
from open_grad_models import oracle_step
from pd_models import family, inputs_for

DT = torch.float64


def mlp_law(x, params, angle, non_angle, u_max, squash, keep=None, p=0.0):
    """mlp_models.mlp_law with one row ``keep`` [M, H] of {0, 1} per trajectory (None: no dropout)."""
    f = torch.cat([x[:, non_angle], torch.sin(x[:, angle]), torch.cos(x[:, angle])], dim=1) if (angle or non_angle) else x
    h, off, s = f, 0, 1.0 / (1.0 - p)
    for l in range(len(params) // 2 - 1):
        h = torch.tanh(h @ params[2 * l].t() + params[2 * l + 1])
        if keep is not None:
            width = h.shape[1]
            k = keep[:, off:off + width].to(DT)
            h = torch.where(k > 0, s * h, torch.zeros_like(h))
            off += width
    a = h @ params[-2].t() + params[-1]
    if not squash:
        return a
    um = torch.as_tensor(u_max, dtype=DT)
    return um * torch.tanh(a / um)


def masks_for(T, M, hidden, p, seed):
    """[T, M, H] uint8 keep-masks (keep with probability 1 - p) from the first generator seed >= ``seed`` whose buffer holds, in every layer
    wider than one unit, a kept and a dropped entry -- so that no case passes with a layer untouched or wiped out; returns (masks, seed used)."""
    H = sum(hidden)
    while True:
        k = torch.empty(T, M, H, dtype=DT).bernoulli_(1.0 - p, generator=torch.Generator().manual_seed(seed)).to(torch.uint8)
        if masks_mixed(k, hidden):
            return k, seed
        seed += 1


def masks_mixed(k, hidden):
    off, ok = 0, True
    for width in hidden:
        part = k[:, :, off:off + width]
        ok = ok and (width == 1 or (bool(part.any()) and not bool(part.all())))
        off += width
    return ok


def drop_truth(shape, m, x0, params, eps, w, wu, sample, angle, non_angle, masks, p, u_max=1.0, squash=True, var_scale=None, ms=None, pos_noise=None):
    """Returns (states [T,M,S], inputs [T,M,U], [dL/dparam ...], dL/dx0, smallest variance met).  ``masks`` None: no dropout; ``ms``: the
    network reads pd_meas_models.measure's measurement of the state."""
    x0 = x0.clone().requires_grad_(True)
    params = [q.clone().requires_grad_(True) for q in params]
    T = w.shape[0]
    law = lambda y, t: mlp_law(y, params, angle, non_angle, u_max, squash, None if masks is None else masks[t], p)
    hist = None
    y = x0
    if ms is not None:
        y, hist = pm.measure(x0, 0, ms, pos_noise, None, None)
    xs, us, vmin = [x0], [law(y, 0)], float("inf")
    for t in range(1, T):
        nx, var = oracle_step(family(shape), m, xs[-1], us[-1], eps[t - 1], sample, var_scale)
        vmin = min(vmin, float(var.detach().min()))
        y = nx
        if ms is not None:
            y, hist = pm.measure(nx, t, ms, pos_noise, hist, None)
        xs.append(nx)
        us.append(law(y, t))
    st, inp = torch.stack(xs), torch.stack(us)
    L = (w * st).sum() + (0.0 if wu is None else (wu * inp).sum())
    grads = torch.autograd.grad(L, params + [x0], allow_unused=True)
    grads = [torch.zeros_like(q) if g is None else g for g, q in zip(grads, params + [x0])]
    return st.detach(), inp.detach(), grads[:-1], grads[-1], vmin


# (mode, shape, degree, N, T, M, hidden, p, options): the smallest shapes at which the dropout forms can go wrong.  N = 37 (Npad 48) with T in
# {1, 2, 3, 12} and M in {1, 5, 17} (two tiles, the second ragged); hidden (1,), (5,), (7, 3) -- H = 10: a Philox block of four across the layer
# boundary, and a remainder --, (33, 64), (64, 64); p in {0.25, 0.5}; arm2, arm2_delta and the UR5 shape (N = 48).  Once each: every model
# limit at once with (64, 64) (the sweep in two parts of 8, over two tiles), UR5 with (64, 64) (the sweep without the weights' LDS copy),
# M = 1041 at T = 2 (the 16-trajectory forward forms), squashing off, no upstream g_inputs, requires_grad on one tensor alone
# (options["only_grad"]: its place in the parameter order), and two cases on a simulated measurement (options["meas"]: the variant of
# mlp_meas_models.meas_model)
CASES = [
    ("mean", "arm2", 0, 37, 12, 17, (5,), 0.25, {}),
    ("sampled", "arm2", 2, 37, 12, 17, (64, 64), 0.5, {}),
    ("sampled", "arm2_delta", 1, 37, 12, 5, (7, 3), 0.25, {}),
    ("sampled", "ur5", 1, 48, 3, 5, (33, 64), 0.5, {}),
    ("mean", "arm2", 1, 37, 1, 5, (1,), 0.5, {}),
    ("sampled", "arm2", 1, 37, 2, 1, (7, 3), 0.25, {}),
    ("mean", "arm2_delta", 2, 37, 3, 17, (7, 3), 0.5, {}),
    ("sampled", "arm2", 0, 37, 3, 5, (5,), 0.5, {"squash": False}),
    ("mean", "arm2", 1, 37, 12, 5, (7, 3), 0.25, {"no_g_inputs": True}),
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), 0.25, {"only_grad": 2}),
    ("sampled", "arm2", 0, 37, 2, 1041, (5,), 0.25, {}),
    ("sampled", "ur5", 1, 48, 3, 5, (64, 64), 0.25, {}),
    ("sampled", "limits", 0, 37, 3, 20, (64, 64), 0.5, {}),
    ("sampled", "arm2", 1, 37, 12, 17, (7, 3), 0.25, {"meas": "all"}),
    ("mean", "arm2_delta", 0, 37, 3, 5, (33, 64), 0.5, {"meas": "reversed"}),
]


def case_id(c):
    return "-".join(str(v) for v in c[:6]) + "-h" + "x".join(str(h) for h in c[6]) + "-p%g" % c[7] + ("-" + "-".join(sorted(c[8])) if c[8] else "")


def case_inputs(case):
    """(cfg, oracle model, inputs dict) of a case: mlp_models' inputs, the masks, and with options["meas"] the measurement model and its noise."""
    mode, shape, deg, N, T, M, hidden, p, opt = case
    c, m, specs = mm.build_pair(shape, N, deg, seed=mm.PAIR_SEED)
    seed = T * 100 + M
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=seed)
    if opt.get("no_g_inputs"):
        wu = None
    angle, non_angle = mm.feature_lists(c, opt)
    params = mm.network(c, hidden, angle, non_angle, seed)
    masks, mask_seed = masks_for(T, M, hidden, p, 5000 + seed)
    ms = pos_noise = None
    if "meas" in opt:
        ms = mmm.meas_model(shape, opt["meas"], 0.1)
        pos_noise = pm.pos_noise_for(T, M, len(ms["pos"]), seed)
    return c, m, dict(x0=x0, eps=eps, w=w, wu=wu, params=params, angle=angle, non_angle=non_angle, u_max=1.0, squash=opt.get("squash", True),
                      specs=specs, masks=masks, mask_seed=mask_seed, p=p, ms=ms, pos_noise=pos_noise, sample=mode == "sampled", shape=shape)


def truth_of(m, ins, **edit):
    """drop_truth on a case's inputs; ``edit`` replaces entries of the inputs (masks=None: the truth without dropout)."""
    q = dict(ins, **edit)
    torch.set_num_threads(1)
    return drop_truth(q["shape"], m, q["x0"], q["params"], q["eps"], q["w"], q["wu"], q["sample"], q["angle"], q["non_angle"], q["masks"], q["p"],
                      u_max=q["u_max"], squash=q["squash"], ms=q["ms"], pos_noise=q["pos_noise"])


def case_truth(case):
    """Everything a case compares against: (cfg, oracle model, inputs dict, truth tuple)."""
    c, m, ins = case_inputs(case)
    return c, m, ins, truth_of(m, ins)
