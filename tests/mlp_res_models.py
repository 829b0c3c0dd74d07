"""The truth for the RESIDUAL policy in the fused closed loop (mcp_rollout_mlp_res / mcp_rollout_mlp_res_bwd): the loop of
tests/mlp_track_models.track_truth -- torch autograd through tests/open_grad_models.oracle_step, with the optional measurement and keep-masks
-- under tests/mlp_track_models.track_law's network WITH the PD term added ahead of the one squashing, the two gain vectors among the
differentiated tensors.  Models, inputs, targets, masks and measurement noise are those of tests/mlp_track_models.py (seed = 100 T + M).  No
GPU and no project code beyond the oracle.

    a_mlp = track_law(..., squash off)                                       (dropout, error features, measured form: as there)
    a_pd[k] = sqrt_kp[k]^2 (pd_target[t][pos[k]] - x[pos[k]]) + sqrt_kd[k]^2 (pd_target[t][vel[k]] - x[vel[k]])
    u[k] = u_max tanh((a_mlp + a_pd)[k] / u_max)  (squash)  or  (a_mlp + a_pd)[k]           every row 0 .. T - 1, row T - 1 included
    plain differences, not wrapped; on a simulated measurement every x above is the measurement y_t; dropout never touches a_pd
"""
import torch

import mlp_drop_models as mdm
import mlp_meas_models as mmm
import mlp_models as mm
import pd_meas_models as pm
from mlp_track_models import LIMITS_IDX, network, target_for, track_law
from open_grad_models import oracle_step
from pd_models import family, inputs_for

DT = torch.float64
# the near misses of tests/test_mlp_res_cpu.py (the last: measured cases only)
DEFECTS = ("not_squared", "sign", "outside_squash", "t-1", "t+1", "row0", "swapped", "true_state")


def res_law(x, t, params, kp, kd, angle, non_angle, u_max, squash, target, idx, pd_target, pos, vel, keep=None, p=0.0, defect=None, true_x=None):
    """The law written out.  ``params``: the network's tensors; ``kp``, ``kd``: [U] square roots of the gains.  ``defect``: a near miss of the
    PD term alone (the network is always the truth's); ``true_x``: the true state of a measured case, which "true_state" takes the PD error on."""
    a = track_law(x, t, params, angle, non_angle, u_max, False, target, idx, keep, p)
    row = {"t-1": max(t - 1, 0), "t+1": t + 1, "row0": 0}.get(defect, t)
    e = pd_target[row].reshape(1, -1) - (true_x if defect == "true_state" else x)
    if defect == "sign":
        e = -e
    if defect == "swapped":
        pos, vel = vel, pos
    gp, gd = (kp, kd) if defect == "not_squared" else (kp ** 2, kd ** 2)
    a_pd = gp * e[:, pos] + gd * e[:, vel]
    um = torch.as_tensor(u_max, dtype=DT)
    if defect == "outside_squash":
        return (um * torch.tanh(a / um) if squash else a) + a_pd
    a = a + a_pd
    return um * torch.tanh(a / um) if squash else a


def res_truth(shape, m, x0, params, kp, kd, eps, w, wu, sample, angle, non_angle, target, idx, pd_target, pos, vel, masks=None, p=0.0, u_max=1.0,
              squash=True, ms=None, pos_noise=None, defect=None):
    """Returns (states [T,M,S], inputs [T,M,U], measurements [T,M,S] or None, [dL/dparam ..., dL/dsqrt_kp, dL/dsqrt_kd], dL/dx0, smallest
    variance met): mlp_track_models.track_truth's loop and loss under res_law.  ``kp`` / ``kd`` of one entry: one gain for all inputs (its
    gradient has one entry)."""
    x0 = x0.clone().requires_grad_(True)
    params = [q.clone().requires_grad_(True) for q in params]
    kp, kd = kp.clone().requires_grad_(True), kd.clone().requires_grad_(True)
    U, T = len(pos), w.shape[0]
    wide = lambda g: g.expand(U) if g.numel() == 1 else g

    def law(y, x, t):
        return res_law(y, t, params, wide(kp), wide(kd), angle, non_angle, u_max, squash, target, idx, pd_target, pos, vel,
                       None if masks is None else masks[t], p, defect, x)

    hist, y = None, x0
    if ms is not None:
        y, hist = pm.measure(x0, 0, ms, pos_noise, None, None)
    xs, ys, us, vmin = [x0], [y], [law(y, x0, 0)], float("inf")
    for t in range(1, T):
        nx, var = oracle_step(family(shape), m, xs[-1], us[-1], eps[t - 1], sample, None)
        vmin = min(vmin, float(var.detach().min()))
        y = nx
        if ms is not None:
            y, hist = pm.measure(nx, t, ms, pos_noise, hist, None)
        xs.append(nx)
        ys.append(y)
        us.append(law(y, nx, t))
    st, inp = torch.stack(xs), torch.stack(us)
    L = (w * st).sum() + (0.0 if wu is None else (wu * inp).sum())
    over = params + [kp, kd, x0]
    grads = torch.autograd.grad(L, over, allow_unused=True)
    grads = [torch.zeros_like(q) if g is None else g for g, q in zip(grads, over)]
    return st.detach(), inp.detach(), None if ms is None else torch.stack(ys).detach(), grads[:-1], grads[-1], vmin


def gains_for(U, seed, scalar=False):
    """sqrt_kp in [1.3, 1.7] (gains 1.7 .. 2.9), sqrt_kd in [0.5, 0.8] (gains 0.25 .. 0.64): away from 1, so that a gain that is not squared
    is another gain; ``scalar``: one value for all inputs."""
    gen = torch.Generator().manual_seed(4000 + seed)
    n = 1 if scalar else U
    return 1.3 + 0.4 * torch.rand(n, dtype=DT, generator=gen), 0.5 + 0.3 * torch.rand(n, dtype=DT, generator=gen)


def pd_target_for(c, T, x0):
    """[T + 2, S], another tensor than mlp_track_models.target_for's: x0_mean[s] + 0.25 cos(0.9 t + 2 s) -- as strongly time-varying."""
    t = torch.arange(T + 2, dtype=DT).reshape(-1, 1)
    return x0.mean(0).reshape(1, -1) + 0.25 * torch.cos(0.9 * t + 2.0 * torch.arange(c["S"], dtype=DT).reshape(1, -1))


# (mode, shape, degree, N, T, M, hidden, options): the shapes of tests/mlp_track_models.py.  Options of that table -- "idx" (here [] is legal:
# the network sees no errors, the PD term keeps its target), "rows_extra", "features": "state", "squash", "no_g_inputs", "meas", "p" -- and
# "pos" / "vel" the PD term's lists (default: the reference's layout 0 .. U-1 and S/2 .. S/2+U-1), "only_grad": "kp" (requires_grad on
# sqrt_kp alone), "fixed_gains" (the gains do not require grad, everything else does), "scalar_gain" (one value for all inputs),
# "pd_target": "other" (pd_target_for: a tensor of its own).
CASES = [
    ("mean", "arm2", 0, 37, 12, 17, (5,), {}),
    ("sampled", "arm2", 2, 37, 12, 17, (64, 64), {"rows_extra": 2, "pos": [1, 0], "vel": [3, 2]}),
    ("sampled", "arm2_delta", 1, 37, 12, 5, (7, 3), {"idx": [3, 0], "pd_target": "other"}),
    ("sampled", "ur5", 1, 48, 3, 5, (64, 64), {"idx": [7, 2, 11]}),
    ("mean", "ur5", 1, 48, 12, 1, (33, 64), {"idx": [], "pos": [5, 0, 3, 1, 4, 2], "vel": [6, 11, 8, 10, 7, 9], "rows_extra": 2}),
    ("mean", "arm2", 1, 37, 1, 5, (1,), {}),
    ("sampled", "arm2", 1, 37, 2, 1, (64,), {"rows_extra": 2, "scalar_gain": True}),
    ("mean", "arm2_delta", 2, 37, 3, 17, (7, 3), {"idx": []}),
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), {"features": "state"}),
    ("sampled", "arm2", 1, 37, 3, 5, (5,), {"squash": False}),
    ("mean", "arm2", 1, 37, 12, 5, (7, 3), {"no_g_inputs": True}),
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), {"only_grad": "kp", "idx": [2, 1]}),
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), {"fixed_gains": True}),
    ("sampled", "arm2", 0, 37, 3, 1041, (5,), {}),
    ("sampled", "limits", 0, 37, 3, 20, (64, 64), {"idx": LIMITS_IDX, "pos": [7, 2, 5, 0, 3, 6, 1, 4], "vel": [12, 9, 15, 8, 11, 14, 10, 13]}),
    ("sampled", "arm2", 1, 37, 12, 17, (7, 3), {"meas": "all", "pd_target": "other"}),
    ("sampled", "arm2", 0, 37, 12, 5, (7, 3), {"p": 0.25}),
    ("mean", "arm2_delta", 0, 37, 3, 5, (33, 64), {"meas": "reversed", "p": 0.25, "idx": [1, 3, 2], "pos": [1, 0], "vel": [2, 3]}),
]


def case_id(c):
    tags = []
    for k in sorted(c[7]):
        v = c[7][k]
        tags.append(k + ".".join(str(i) for i in v) if k in ("idx", "pos", "vel") else "%s%s" % (k, v) if k in ("p", "meas", "rows_extra", "only_grad", "pd_target") else k)
    return "-".join(str(v) for v in c[:6]) + "-h" + "x".join(str(h) for h in c[6]) + ("-" + "-".join(tags) if tags else "")


def default_lists(c):
    return list(range(c["U"])), list(range(c["S"] // 2, c["S"] // 2 + c["U"]))


def case_inputs(case):
    """(cfg, oracle model, inputs dict) of a case: mlp_track_models.case_inputs' entries -- ``params`` the network alone -- and the PD term's:
    ``kp``, ``kd``, ``pos``, ``vel``, ``pd_target`` (the policy's rows; the feature target itself unless the case names another),
    ``pd_target_full`` (T + 2 rows)."""
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
    rows = T + opt.get("rows_extra", 0)
    pd_full = pd_target_for(c, T, x0) if opt.get("pd_target") == "other" else full
    kp, kd = gains_for(c["U"], seed, bool(opt.get("scalar_gain")))
    dpos, dvel = default_lists(c)
    p = opt.get("p", 0.0)
    masks = mask_seed = ms = pos_noise = None
    if p > 0.0:
        masks, mask_seed = mdm.masks_for(T, M, hidden, p, 5000 + seed)
    if "meas" in opt:
        ms = mmm.meas_model(shape, opt["meas"], 0.1)
        pos_noise = pm.pos_noise_for(T, M, len(ms["pos"]), seed)
    target = full[:rows].clone()
    return c, m, dict(x0=x0, eps=eps, w=w, wu=wu, params=params, kp=kp, kd=kd, angle=angle, non_angle=non_angle, u_max=1.0,
                      squash=opt.get("squash", True), specs=specs, target=target, target_full=full, idx=idx,
                      pd_target=pd_full[:rows].clone() if opt.get("pd_target") == "other" else target, pd_target_full=pd_full,
                      pos=list(opt.get("pos", dpos)), vel=list(opt.get("vel", dvel)), masks=masks, mask_seed=mask_seed, p=p, ms=ms,
                      pos_noise=pos_noise, sample=mode == "sampled", shape=shape)


def truth_of(m, ins, defect=None, **edit):
    """res_truth on a case's inputs; ``edit`` replaces entries of the inputs, ``defect`` names a near miss (it reads the full targets)."""
    q = dict(ins, **edit)
    torch.set_num_threads(1)
    return res_truth(q["shape"], m, q["x0"], q["params"], q["kp"], q["kd"], q["eps"], q["w"], q["wu"], q["sample"], q["angle"], q["non_angle"],
                     q["target_full"] if defect else q["target"], q["idx"], q["pd_target_full"] if defect else q["pd_target"], q["pos"], q["vel"],
                     q["masks"], q["p"], u_max=q["u_max"], squash=q["squash"], ms=q["ms"], pos_noise=q["pos_noise"], defect=defect)


_TRUTHS = {}


def case_truth(case):
    """Everything a case compares against: (cfg, oracle model, inputs dict, truth tuple) -- computed once per process and shared, never modified."""
    key = case_id(case)
    if key not in _TRUTHS:
        c, m, ins = case_inputs(case)
        _TRUTHS[key] = (c, m, ins, truth_of(m, ins))
    return _TRUTHS[key]
