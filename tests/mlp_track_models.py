"""The truth for TARGET-TRAJECTORY FEATURES in the fused closed loop under the tanh-MLP policy (mcp_rollout_mlp_track / mcp_rollout_mlp_track_bwd):
the loop of tests/mlp_drop_models.drop_truth -- torch autograd through tests/open_grad_models.oracle_step, with the optional measurement and
keep-masks -- and the network written out here WITH its error features.  Models and inputs are those of tests/mlp_models.py (build_pair with
PAIR_SEED, inputs_for, seed = 100 T + M), the measurement model and its noise those of tests/mlp_meas_models.py, the masks those of
tests/mlp_drop_models.py.  No GPU and no project code beyond the oracle.

    f_t = [x[non_angle], sin x[angle], cos x[angle], target[t][idx[i]] - x[idx[i]] (i = 0 .. n - 1)]      (no lists: f_t = [x, errors])
    the error is the plain difference, target - x in that order, not wrapped on angles; every row 0 .. T - 1 has one (row T - 1 included);
    on a simulated measurement every x above is the measurement y_t;   W0 is [h0][P], P = n_non_angle + 2 n_angle + n, the error columns last
"""
import numpy as np
import torch

import mlp_drop_models as mdm
import mlp_meas_models as mmm
import mlp_models as mm
import pd_meas_models as pm
from open_grad_models import oracle_step
from pd_models import family, inputs_for

DT = torch.float64
DEFECTS = ("t-1", "t+1", "sign", "row0", "true_state")  # the near misses of tests/test_mlp_track_cpu.py (the last: measured cases only)


def track_law(x, t, params, angle, non_angle, u_max, squash, target, idx, keep=None, p=0.0, err_on=None):
    """mlp_drop_models.mlp_law with the error features target[t][idx] - x[:, idx] appended behind the cosines.  ``err_on`` (a near miss
    only): the state the error is taken on in x's place."""
    own = [x[:, non_angle], torch.sin(x[:, angle]), torch.cos(x[:, angle])] if (angle or non_angle) else [x]
    e = target[t][idx].reshape(1, -1) - (x if err_on is None else err_on)[:, idx]
    h, off, s = torch.cat(own + [e], dim=1), 0, 1.0 / (1.0 - p)
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


def track_truth(shape, m, x0, params, eps, w, wu, sample, angle, non_angle, target, idx, masks=None, p=0.0, u_max=1.0, squash=True, var_scale=None,
                ms=None, pos_noise=None, defect=None):
    """Returns (states [T,M,S], inputs [T,M,U], measurements [T,M,S] or None, [dL/dparam ...], dL/dx0, smallest variance met).  ``masks``
    None: no dropout; ``ms``: the network reads pd_meas_models.measure's measurement of the state, errors included.  ``defect`` (one of
    DEFECTS): a near miss -- the target read a row early (row 0 stays) or late, the error's sign flipped, row 0 of the target in every
    evaluation, the error taken on the true state of a measured case."""
    x0 = x0.clone().requires_grad_(True)
    params = [q.clone().requires_grad_(True) for q in params]
    T = w.shape[0]
    tgt = -target if defect == "sign" else target

    def law(y, x, t):
        row = {"t-1": max(t - 1, 0), "t+1": t + 1, "row0": 0}.get(defect, t)
        u_of = lambda y_, e_: track_law(y_, row, params, angle, non_angle, u_max, squash, tgt, idx, None if masks is None else masks[t], p, e_)
        if defect == "sign":  # x - target = (-target) - (-x): the error on the negated row
            return u_of(y, -y)
        return u_of(y, x if defect == "true_state" else None)

    hist, y = None, x0
    if ms is not None:
        y, hist = pm.measure(x0, 0, ms, pos_noise, None, None)
    xs, ys, us, vmin = [x0], [y], [law(y, x0, 0)], float("inf")
    for t in range(1, T):
        nx, var = oracle_step(family(shape), m, xs[-1], us[-1], eps[t - 1], sample, var_scale)
        vmin = min(vmin, float(var.detach().min()))
        y = nx
        if ms is not None:
            y, hist = pm.measure(nx, t, ms, pos_noise, hist, None)
        xs.append(nx)
        ys.append(y)
        us.append(law(y, nx, t))
    st, inp = torch.stack(xs), torch.stack(us)
    L = (w * st).sum() + (0.0 if wu is None else (wu * inp).sum())
    grads = torch.autograd.grad(L, params + [x0], allow_unused=True)
    grads = [torch.zeros_like(q) if g is None else g for g, q in zip(grads, params + [x0])]
    return st.detach(), inp.detach(), None if ms is None else torch.stack(ys).detach(), grads[:-1], grads[-1], vmin


def target_for(c, T, x0):
    """[T + 2, S]: smooth and strongly time-varying around the swarm's mean start, x0_mean[s] + 0.3 sin(0.7 t + s) -- a wrong row index moves
    an error by up to 0.2.  A case hands its first ``rows`` rows to the policy (the near miss that reads a row late sees them all)."""
    t = torch.arange(T + 2, dtype=DT).reshape(-1, 1)
    return x0.mean(0).reshape(1, -1) + 0.3 * torch.sin(0.7 * t + torch.arange(c["S"], dtype=DT).reshape(1, -1))


def network(c, hidden, angle, non_angle, n_err, seed):
    """mlp_models.network with W0 [h0][P + n_err]: weights randn / sqrt(fan_in), biases 0.1 randn, from the generator seeded 77 + seed."""
    gen = torch.Generator().manual_seed(77 + seed)
    P = (len(non_angle) + 2 * len(angle) if (angle or non_angle) else c["S"]) + n_err
    widths = [P] + list(hidden) + [c["U"]]
    out = []
    for l in range(len(widths) - 1):
        out.append(torch.randn(widths[l + 1], widths[l], dtype=DT, generator=gen) / np.sqrt(widths[l]))
        out.append(0.1 * torch.randn(widths[l + 1], dtype=DT, generator=gen))
    return out


LIMITS_IDX = [15, 1, 8, 3, 12, 5, 10, 7]  # eight of the sixteen components, angles and velocities mixed, not ascending

# (mode, shape, degree, N, T, M, hidden, options): the smallest shapes of tests/mlp_models.py and tests/mlp_drop_models.py at which the tracking
# forms can go wrong.  N = 37 (Npad 48) with T in {1, 2, 3, 12} and M in {1, 5, 17} (two tiles, the second ragged), M = 1041 once (the
# 16-per-workgroup ladder); arm2, arm2_delta, the UR5 shape (N = 48; S = 12: all errors give P = 30) and every model limit at once.  Options:
# "idx" the error indices (default: all S in order), "rows_extra" rows of the target beyond T (default 0: rows == T), "features": "state" no
# lists (f = [x, errors]), "squash", "no_g_inputs", "only_grad" (requires_grad on that tensor alone: 0 is W0), "meas" the variant of
# mlp_meas_models.meas_model, "p" the dropout probability (buffer masks).  (64, 64) on UR5: the weights read from global memory; on
# ``limits``, with its own lists and eight errors, P = 8 + 16 + 8 = 32 exactly and the sweep runs in parts.
CASES = [
    ("mean", "arm2", 0, 37, 12, 17, (5,), {}),
    ("sampled", "arm2", 2, 37, 12, 17, (64, 64), {"rows_extra": 2}),
    ("sampled", "arm2_delta", 1, 37, 12, 5, (7, 3), {"idx": [3, 0]}),
    ("sampled", "ur5", 1, 48, 3, 5, (64, 64), {}),
    ("mean", "ur5", 1, 48, 12, 1, (33, 64), {"idx": [7, 2, 11], "rows_extra": 2}),
    ("mean", "arm2", 1, 37, 1, 5, (1,), {}),
    ("sampled", "arm2", 1, 37, 2, 1, (64,), {"rows_extra": 2}),
    ("mean", "arm2_delta", 2, 37, 3, 17, (7, 3), {}),
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), {"features": "state"}),
    ("sampled", "arm2", 1, 37, 3, 5, (5,), {"squash": False}),
    ("mean", "arm2", 1, 37, 12, 5, (7, 3), {"no_g_inputs": True}),
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), {"only_grad": 0, "idx": [2, 1]}),
    ("sampled", "arm2", 0, 37, 3, 1041, (5,), {}),
    ("sampled", "limits", 0, 37, 3, 20, (64, 64), {"idx": LIMITS_IDX}),
    ("sampled", "arm2", 1, 37, 12, 17, (7, 3), {"meas": "all"}),
    ("sampled", "arm2", 0, 37, 12, 5, (7, 3), {"p": 0.25}),
    ("mean", "arm2_delta", 0, 37, 3, 5, (33, 64), {"meas": "reversed", "p": 0.25, "idx": [1, 3, 2]}),
]


def case_id(c):
    tags = []
    for k in sorted(c[7]):
        v = c[7][k]
        tags.append(k + ".".join(str(i) for i in v) if k == "idx" else "%s%s" % (k, v) if k in ("p", "meas", "rows_extra", "only_grad") else k)
    return "-".join(str(v) for v in c[:6]) + "-h" + "x".join(str(h) for h in c[6]) + ("-" + "-".join(tags) if tags else "")


def case_inputs(case):
    """(cfg, oracle model, inputs dict) of a case: mlp_models' inputs, the target (``target``: the policy's rows; ``target_full``: T + 2
    rows), the error indices, and with the options the masks, the measurement model and its noise."""
    mode, shape, deg, N, T, M, hidden, opt = case
    c, m, specs = mm.build_pair(shape, N, deg, seed=mm.PAIR_SEED)
    seed = T * 100 + M
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=seed)
    if opt.get("no_g_inputs"):
        wu = None
    angle, non_angle = mm.feature_lists(c, opt)
    idx = list(opt.get("idx", range(c["S"])))
    params = network(c, hidden, angle, non_angle, len(idx), seed)
    full = target_for(c, T, x0)
    p = opt.get("p", 0.0)
    masks = mask_seed = ms = pos_noise = None
    if p > 0.0:
        masks, mask_seed = mdm.masks_for(T, M, hidden, p, 5000 + seed)
    if "meas" in opt:
        ms = mmm.meas_model(shape, opt["meas"], 0.1)
        pos_noise = pm.pos_noise_for(T, M, len(ms["pos"]), seed)
    return c, m, dict(x0=x0, eps=eps, w=w, wu=wu, params=params, angle=angle, non_angle=non_angle, u_max=1.0, squash=opt.get("squash", True),
                      specs=specs, target=full[:T + opt.get("rows_extra", 0)].clone(), target_full=full, idx=idx, masks=masks, mask_seed=mask_seed, p=p,
                      ms=ms, pos_noise=pos_noise, sample=mode == "sampled", shape=shape)


def truth_of(m, ins, defect=None, **edit):
    """track_truth on a case's inputs; ``edit`` replaces entries of the inputs, ``defect`` names a near miss (it reads ``target_full``)."""
    q = dict(ins, **edit)
    torch.set_num_threads(1)
    return track_truth(q["shape"], m, q["x0"], q["params"], q["eps"], q["w"], q["wu"], q["sample"], q["angle"], q["non_angle"],
                       q["target_full"] if defect else q["target"], q["idx"], q["masks"], q["p"], u_max=q["u_max"], squash=q["squash"], ms=q["ms"],
                       pos_noise=q["pos_noise"], defect=defect)


_TRUTHS = {}


def case_truth(case):
    """Everything a case compares against: (cfg, oracle model, inputs dict, truth tuple) -- computed once per process and shared, never modified."""
    key = case_id(case)
    if key not in _TRUTHS:
        c, m, ins = case_inputs(case)
        _TRUTHS[key] = (c, m, ins, truth_of(m, ins))
    return _TRUTHS[key]
