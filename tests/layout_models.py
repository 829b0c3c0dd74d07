"""Irregular model layouts for the entry points that share the generic step and the generic sweep (rollout_open.hip, rollout_open_phases.h,
model_step.hip, rollout_mlp_kernels.h, lqr.hip): the open loop, the model step, the PD / measured-PD / PID / TVL closed loops, the tanh-MLP
loop, the linearisation and the Riccati pass.  The feature commits tested those on layouts with S = 2 U or U = 1, sorted disjoint lists,
every component integrated and positions first; the table below holds the layouts that break each of these, with what every one pins,
in the manner of tests/width_models.py.  The truth functions are the families' own (pd_models.pd_truth, pd_meas_models.pd_meas_truth,
pid_models.pid_truth, tvl_models.tvl_truth, mlp_models.mlp_truth, open_grad_models.oracle_truth, lqr_models): they are generic in S, U and
the index rule pos = range(U), vel = range(S // 2, S // 2 + U), and reach the integrator through pd_models.family -> "mixed"
(orc.mixed_next_state).  CPU side only imports torch, numpy, helpers and the oracle."""
import collections
import functools

import numpy as np
import torch

from helpers import hyper
from oracle import mcpilco_oracle as orc

DT = torch.float64


def _r(a, b=None):
    return list(range(a)) if b is None else list(range(a, b))


LAYOUTS = {
    "cart": dict(S=4, U=1, G=2, angle=[2], not_angle=[0, 1, 3], vel=[1, 3], not_vel=[0, 2], Ts=0.05,
                 pins="the closed loops at U = 1 (sweep slot q + 4 dead everywhere), with an angle in the middle of the state; D = 6"),
    "all_angle": dict(S=2, U=1, G=2, angle=[0, 1], not_angle=[], vel=[0, 1], not_vel=[-1, -1], Ts=0.05,
                      pins="n_not_angle = 0, S = 2, a delta-state layout with G = S; D = 5"),
    "g1_plain": dict(S=3, U=1, G=1, angle=[], not_angle=[0, 1, 2], vel=[2], not_vel=[1], Ts=0.05,
                     pins="G = 1, n_angle = 0, S odd; component 0 is integrated by no GP: zero from row 1 on, a zero row of A and B; D = 4; the "
                          "measurement model has one pair"),
    "mixed5": dict(S=5, U=3, G=3, angle=[4, 0], not_angle=[0, 1, 3], vel=[3, 1, 2], not_vel=[0, -1, 4], Ts=0.05,
                   pins="unsorted angle list; component 0 in angle AND not_angle, component 2 in neither; GPs listed out of order; speed and delta "
                        "integration in one model; with the PD layout component 2 is the position of input 2 and the velocity of input 0 (two pulls "
                        "on one lambda[s]); U = 3; U (S + 1) = 18: one block of the TVL reduction and a tail of 2; the measurement model leaves "
                        "component 4 in no pair; D = 10"),
    "d15_plain": dict(S=10, U=5, G=5, angle=[], not_angle=_r(10), vel=_r(5, 10), not_vel=_r(5), Ts=0.05,
                      pins="D + 1 = 16 exactly (one full row block of [X^T; 1]); U = 5: sweep slot q + 4 live for q = 0 only; odd G; S % 4 = 2; "
                           "U (S + 1) = 55"),
    "d16_angles": dict(S=7, U=3, G=3, angle=_r(6), not_angle=[6], vel=[3, 4, 5], not_vel=[0, 1, 2], Ts=0.05,
                       pins="D + 1 = 17: the second row block holds one row; S = 7; component 6 is a GP input that nothing integrates (a column of A "
                            "without a row); U (S + 1) = 24: one block and a tail of 8; D % 4 = 0 with S % 4 = 3"),
    # (the record tests/mlp_models.py had, sampling time included: its MLP cases keep their operands)
    "limits": dict(S=16, U=8, G=8, angle=_r(8), not_angle=_r(8, 16), vel=_r(8, 16), not_vel=_r(8), Ts=0.02,
                   pins="every compiled limit at once for PD, PID, TVL, open loop, model_step, linearize and the pass: TVL_ROW = 152 doubles (the "
                        "staging threads overlap the state and input threads of a 16-trajectory tile), U (S + 1) = 136, G D = 256 = LQ_NT, D + 1 = 33"),
}


def family(name):
    """The integrator tests/open_grad_models.oracle_step runs for a layout."""
    return "delta" if name == "all_angle" else "mixed"


def build_pair(layout, N, deg, seed):
    """pd_models.build_pair's recipe on a layout of the table: (record, orc.SpeedModel with the layout's lists, per-GP (lengthscales,
    sigma_n, lam, poly_w))."""
    c = LAYOUTS[layout]
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
    return c, orc.SpeedModel(hyp, caches, c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"]), specs


def pair_seed(N, deg):
    return N + deg


@functools.lru_cache(maxsize=None)
def oracle_pair(layout, N, deg):
    return build_pair(layout, N, deg, pair_seed(N, deg))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# (form, mode, layout, degree, N, T, M, options).  N = 37 (Npad 48: a remainder block of Kinv), T in {2, 3, 12}, M in {1, 5, 17, 33} (33: three
# sweep tiles, the last ragged), degree 0 / 1 / 2 and mean / sampled spread over the table; every layout runs every form at least once sampled.
#   open      rollout_open_diff (states, g_x0, g_u) and the moments mu / var of rollout_open; "lengths": ragged
#   step      model_step forward and backward on one row
#   pd        the PD law;  "meas": on the measurement model pd_meas_models.meas_model(variant)
#   pid       the PID law, "i_max": the bound of input 0 (input k: i_max (1 + k / 4)), finite on every input; "meas" as above
#   tvl       dense per-row gains with feedforward; "shared": one gain; "meas" as above
#   mlp       hidden sizes "hidden"; "features": "state", or "angle" / "non_angle": the policy's own lists
#   lin       ops.linearize of a record;  pass: ops.lqr_pass, "reg"
Case = collections.namedtuple("Case", "form mode layout deg N T M opt")
_S, _M = "sampled", "mean"
CASES = [Case(*r) for r in [
    # open loop
    ("open", _S, "cart", 0, 37, 12, 17, {}), ("open", _S, "all_angle", 1, 37, 3, 5, {}), ("open", _S, "g1_plain", 2, 37, 12, 33, {}),
    ("open", _S, "mixed5", 1, 37, 12, 17, {"lengths": True}), ("open", _M, "mixed5", 0, 37, 3, 33, {}), ("open", _S, "d15_plain", 0, 37, 2, 1, {}),
    ("open", _S, "d16_angles", 2, 37, 12, 5, {}), ("open", _M, "d16_angles", 1, 37, 3, 17, {}),
    ("open", _S, "limits", 0, 37, 3, 33, {"lengths": True}), ("open", _M, "limits", 1, 37, 12, 1, {}),
    # model step
    ("step", _S, "cart", 1, 37, 2, 17, {}), ("step", _S, "all_angle", 0, 37, 2, 17, {}), ("step", _S, "g1_plain", 1, 37, 2, 17, {}),
    ("step", _S, "mixed5", 2, 37, 2, 17, {}), ("step", _M, "mixed5", 0, 37, 2, 5, {}), ("step", _S, "d15_plain", 1, 37, 2, 33, {}),
    ("step", _S, "d16_angles", 0, 37, 2, 17, {}), ("step", _S, "limits", 2, 37, 2, 17, {}),
    # PD on the true state
    ("pd", _S, "cart", 1, 37, 12, 5, {}), ("pd", _S, "all_angle", 2, 37, 12, 17, {}), ("pd", _S, "g1_plain", 0, 37, 3, 5, {}),
    ("pd", _S, "mixed5", 0, 37, 12, 17, {}), ("pd", _M, "mixed5", 2, 37, 2, 1, {}), ("pd", _S, "d15_plain", 2, 37, 3, 17, {}),
    ("pd", _S, "d16_angles", 1, 37, 12, 5, {}), ("pd", _S, "limits", 0, 37, 3, 17, {}), ("pd", _M, "limits", 1, 37, 12, 1, {}),
    # PD on the measurement
    ("pd", _S, "cart", 0, 37, 12, 17, {"meas": "all"}), ("pd", _S, "all_angle", 1, 37, 3, 5, {"meas": "all"}),
    ("pd", _S, "g1_plain", 2, 37, 12, 5, {"meas": "all"}), ("pd", _M, "g1_plain", 0, 37, 3, 1, {"meas": "reversed"}),
    ("pd", _S, "mixed5", 1, 37, 12, 5, {"meas": "all"}), ("pd", _S, "mixed5", 0, 37, 3, 17, {"meas": "reversed"}),
    ("pd", _S, "d15_plain", 0, 37, 12, 5, {"meas": "reversed"}), ("pd", _S, "d16_angles", 2, 37, 3, 17, {"meas": "all"}),
    ("pd", _M, "d16_angles", 0, 37, 12, 5, {"meas": "reversed"}), ("pd", _S, "limits", 1, 37, 3, 5, {"meas": "all"}),
    ("pd", _S, "limits", 0, 37, 2, 17, {"meas": "reversed"}),
    # PID, true and measured
    ("pid", _S, "cart", 2, 37, 12, 5, {"i_max": 0.05}), ("pid", _S, "all_angle", 0, 37, 12, 17, {"i_max": 0.05}),
    ("pid", _S, "g1_plain", 1, 37, 12, 5, {"i_max": 0.05}), ("pid", _S, "mixed5", 2, 37, 12, 17, {"i_max": 0.05}),
    ("pid", _M, "mixed5", 1, 37, 3, 5, {"i_max": 0.02}), ("pid", _S, "d15_plain", 1, 37, 3, 5, {"i_max": 0.02}),
    ("pid", _S, "d16_angles", 0, 37, 12, 17, {"i_max": 0.05}), ("pid", _S, "limits", 1, 37, 3, 5, {"i_max": 0.02}),
    ("pid", _S, "cart", 1, 37, 3, 17, {"i_max": 0.02, "meas": "all"}), ("pid", _S, "all_angle", 2, 37, 12, 5, {"i_max": 0.05, "meas": "all"}),
    ("pid", _S, "g1_plain", 0, 37, 12, 17, {"i_max": 0.05, "meas": "all"}), ("pid", _S, "mixed5", 0, 37, 12, 5, {"i_max": 0.05, "meas": "reversed"}),
    ("pid", _S, "d15_plain", 2, 37, 12, 5, {"i_max": 0.05, "meas": "all"}), ("pid", _S, "d16_angles", 1, 37, 3, 5, {"i_max": 0.02, "meas": "reversed"}),
    ("pid", _S, "limits", 0, 37, 3, 17, {"i_max": 0.02, "meas": "all"}),
    # TVL, true and measured
    ("tvl", _S, "cart", 0, 37, 12, 17, {}), ("tvl", _S, "all_angle", 1, 37, 3, 5, {}), ("tvl", _S, "g1_plain", 2, 37, 12, 17, {}),
    ("tvl", _S, "mixed5", 1, 37, 12, 33, {}), ("tvl", _M, "mixed5", 0, 37, 2, 1, {}), ("tvl", _S, "d15_plain", 0, 37, 12, 17, {"shared": True}),
    ("tvl", _S, "d15_plain", 1, 37, 3, 5, {}), ("tvl", _S, "d16_angles", 2, 37, 12, 33, {}), ("tvl", _S, "limits", 0, 37, 3, 33, {}),
    ("tvl", _S, "limits", 1, 37, 3, 17, {"shared": True}), ("tvl", _M, "limits", 0, 37, 12, 5, {}),
    ("tvl", _S, "cart", 1, 37, 3, 5, {"meas": "all"}), ("tvl", _S, "all_angle", 0, 37, 12, 17, {"meas": "all"}),
    ("tvl", _S, "g1_plain", 1, 37, 3, 5, {"meas": "all"}), ("tvl", _S, "mixed5", 2, 37, 3, 33, {"meas": "all"}),
    ("tvl", _S, "d15_plain", 2, 37, 12, 5, {"meas": "reversed"}), ("tvl", _S, "d16_angles", 0, 37, 3, 33, {"meas": "reversed"}),
    ("tvl", _S, "limits", 2, 37, 3, 33, {"meas": "all"}),
    # tanh MLP
    ("mlp", _S, "cart", 2, 37, 12, 17, {"hidden": (7, 3)}), ("mlp", _S, "all_angle", 0, 37, 12, 5, {"hidden": (7, 3)}),
    ("mlp", _S, "all_angle", 1, 37, 3, 17, {"hidden": (7, 3), "features": "state"}), ("mlp", _S, "g1_plain", 1, 37, 12, 5, {"hidden": (7, 3)}),
    ("mlp", _S, "g1_plain", 0, 37, 3, 17, {"hidden": (7, 3), "features": "state"}),
    ("mlp", _S, "mixed5", 0, 37, 12, 17, {"hidden": (7, 3), "angle": [4, 2], "non_angle": [3, 0, 1]}),
    ("mlp", _M, "mixed5", 1, 37, 3, 5, {"hidden": (7, 3), "angle": [0], "non_angle": [2, 4]}),
    ("mlp", _S, "d15_plain", 1, 37, 3, 17, {"hidden": (7, 3)}), ("mlp", _S, "d15_plain", 0, 37, 3, 5, {"hidden": (64, 64)}),
    ("mlp", _S, "d16_angles", 2, 37, 12, 5, {"hidden": (7, 3)}), ("mlp", _S, "limits", 1, 37, 3, 17, {"hidden": (7, 3)}),
    # linearisation (both modes on every layout: the GPU test runs a mean and a sampled record of each row)
    ("lin", _S, "cart", 0, 37, 12, 5, {}), ("lin", _S, "all_angle", 2, 37, 3, 17, {}), ("lin", _S, "g1_plain", 1, 37, 12, 5, {}),
    ("lin", _S, "mixed5", 2, 37, 12, 5, {}), ("lin", _S, "d15_plain", 0, 37, 3, 17, {}), ("lin", _S, "d16_angles", 1, 37, 12, 5, {}),
    ("lin", _S, "limits", 0, 37, 3, 17, {}),
    # the pass, on the mean record
    ("pass", _M, "cart", 0, 37, 12, 5, {"reg": 0.0}), ("pass", _M, "all_angle", 2, 37, 3, 17, {"reg": 1e-3}), ("pass", _M, "g1_plain", 1, 37, 12, 5, {"reg": 1e-3}),
    ("pass", _M, "mixed5", 2, 37, 12, 5, {"reg": 0.0}), ("pass", _M, "mixed5", 0, 37, 2, 1, {"reg": 1e-3}), ("pass", _M, "d15_plain", 0, 37, 3, 17, {"reg": 1e-3}),
    ("pass", _M, "d16_angles", 1, 37, 12, 5, {"reg": 0.0}), ("pass", _M, "limits", 0, 37, 3, 17, {"reg": 1e-3}), ("pass", _M, "limits", 1, 37, 12, 5, {"reg": 0.0}),
]]


def case_id(c):
    opt = dict(c.opt)
    tags = []
    if "meas" in opt:
        tags.append("meas_" + opt.pop("meas"))
    if "i_max" in opt:
        tags.append("imax_%g" % opt.pop("i_max"))
    if "hidden" in opt:
        tags.append("h" + "x".join(str(h) for h in opt.pop("hidden")))
    if "reg" in opt:
        tags.append("reg_%g" % opt.pop("reg"))
    return "-".join(str(v) for v in c[:7]) + "".join("-" + t for t in tags + sorted(opt))


BY_ID = {case_id(c): c for c in CASES}
assert len(BY_ID) == len(CASES)


def of_form(form):
    return [c for c in CASES if c.form == form]


def case_seed(c):
    return 100 * c.T + c.M


def ragged(M, T):
    """Lengths in 1 .. T: the first trajectory stops at once, the last runs to the end."""
    lens = [1 + (5 * i) % T for i in range(M)]
    lens[-1] = T
    return lens


def i_max_of(c):
    """A finite bound per input: input k gets i_max (1 + k / 4)."""
    return [c.opt["i_max"] * (1.0 + 0.25 * k) for k in range(LAYOUTS[c.layout]["U"])]


def meas_of(c):
    """(measurement model, its position noise) of a case, or (None, None)."""
    from pd_meas_models import meas_model, pos_noise_for

    if "meas" not in c.opt:
        return None, None
    ms = meas_model(c.layout, c.opt["meas"], shapes=LAYOUTS)
    return ms, pos_noise_for(c.T, c.M, len(ms["pos"]), case_seed(c))


def moments_truth(m, states, u, lens=None):
    """mu, var [T-1,M,G] of the GPs along the truth's states (rows from a trajectory's length - 1 on stay zero, as rollout_open leaves them)."""
    T, M = states.shape[0], states.shape[1]
    mus, vrs = [], []
    with torch.no_grad():
        for t in range(T - 1):
            _, mu, var = orc.one_step_gp_out(m, states[t], u[t].expand(M, -1))
            mus.append(torch.cat(mu, 1))
            vrs.append(torch.cat(var, 1))
    mu, var = torch.stack(mus), torch.stack(vrs)
    if lens is not None:
        live = (torch.arange(1, T).reshape(T - 1, 1) < torch.as_tensor(lens).reshape(1, M)).to(DT).unsqueeze(2)
        mu, var = mu * live, var * live
    return mu, var


def step_truth(m, x, u, eps, w, sample):
    """One step of orc.mixed_next_state and autograd through it, as tests/test_gpu_model_step.py has its truth: (x_next, mu, var, g_x, g_u)."""
    xo, uo = x.clone().requires_grad_(True), u.clone().requires_grad_(True)
    nx, mu, var = orc.mixed_next_state(m, xo, uo, eps, sample)
    gx, gu = torch.autograd.grad((w * nx).sum(), [xo, uo])
    return nx.detach(), mu.detach(), var.detach(), gx, gu


def case_truth(c):
    """Everything a case compares against, computed once per process and left unchanged: a dict with the operands ("ins") and the family's
    truth ("truth"; for "lin" / "pass" the CPU rollout and its Jacobians per mode), "states" (every state the truth met) and "vmin" (its
    smallest variance)."""
    return _case_truth(case_id(c))


@functools.lru_cache(maxsize=None)
def _case_truth(cid):
    import lqr_models as lm
    import mlp_models
    import open_grad_models as ogm
    import pd_meas_models
    import pd_models
    import pid_models
    import tvl_models as tm

    c = BY_ID[cid]
    rec, m, specs = oracle_pair(c.layout, c.N, c.deg)
    fam, sample, seed = family(c.layout), c.mode == "sampled", case_seed(c)
    torch.set_num_threads(1)
    ms, pn = meas_of(c)
    if c.form == "open":
        x0, u, eps, w = ogm.inputs_for(rec, c.M, c.T, seed)
        lens = ragged(c.M, c.T) if c.opt.get("lengths") else None
        t = ogm.oracle_truth(fam, m, x0, u, eps, w, sample, lengths=lens)
        mu, var = moments_truth(m, t[0], u, lens)
        return dict(ins=dict(x0=x0, u=u, eps=eps, w=w, lengths=lens), truth=t, mu=mu, var=var, states=t[0], vmin=t[3])
    if c.form == "step":
        x0, u, eps, w = ogm.inputs_for(rec, c.M, c.T, seed)
        t = step_truth(m, x0, u[0], eps[0], w[1], sample)
        return dict(ins=dict(x=x0, u=u[0], eps=eps[0], w=w[1]), truth=t, states=torch.stack([x0, t[0]]), vmin=float(t[2].min()))
    if c.form == "pd":
        x0, kp, kd, target, eps, w, wu = pd_models.inputs_for(rec, c.M, c.T, seed)
        if ms is None:
            t = pd_models.pd_truth(c.layout, m, x0, kp, kd, target, eps, w, wu, sample)
        else:
            t = pd_meas_models.pd_meas_truth(c.layout, m, x0, kp, kd, target, eps, pn, w, wu, sample, ms)
        return dict(ins=dict(x0=x0, kp=kp, kd=kd, target=target, eps=eps, w=w, wu=wu, ms=ms, pn=pn), truth=t, states=t[0], vmin=t[-1])
    if c.form == "pid":
        x0, kp, kd, target, eps, w, wu = pd_models.inputs_for(rec, c.M, c.T, seed)
        ki, im = pid_models.ki_for(rec, seed), i_max_of(c)
        t = pid_models.pid_truth(c.layout, m, x0, kp, kd, ki, target, eps, w, wu, sample, i_max=im, ms=ms, pos_noise=pn)
        return dict(ins=dict(x0=x0, kp=kp, kd=kd, ki=ki, target=target, eps=eps, w=w, wu=wu, ms=ms, pn=pn, i_max=im), truth=t, states=t.states, vmin=t.vmin)
    if c.form == "tvl":
        x0, kp, kd, target, eps, w, wu, gain, ff = tm.tvl_inputs(rec, c.M, c.T, seed)
        if c.opt.get("shared"):
            gain = gain[0].clone()
        t = tm.tvl_truth(c.layout, m, x0, gain, ff, target, eps, w, wu, sample, ms=ms, pos_noise=pn)
        return dict(ins=dict(x0=x0, gain=gain, ff=ff, target=target, eps=eps, w=w, wu=wu, ms=ms, pn=pn), truth=t, states=t.states, vmin=t.vmin)
    if c.form == "mlp":
        x0, _, _, _, eps, w, wu = pd_models.inputs_for(rec, c.M, c.T, seed)
        angle, non_angle = mlp_models.feature_lists(rec, c.opt)
        params = mlp_models.network(rec, c.opt["hidden"], angle, non_angle, seed)
        t = mlp_models.mlp_truth(c.layout, m, x0, params, eps, w, wu, sample, angle, non_angle)
        return dict(ins=dict(x0=x0, eps=eps, w=w, wu=wu, params=params, angle=angle, non_angle=non_angle), truth=t, states=t[0], vmin=t[-1])
    if c.form in ("lin", "pass"):
        x0, a, u, du, eps, target = o = lm.operands(rec, c.T, c.M, seed)
        out = dict(ins=o)
        for smp in ((False, True) if c.form == "lin" else (False,)):
            st = lm.oracle_rollout(c.layout, m, x0, u[:c.T - 1], eps, smp)
            out[smp] = (st,) + tuple(lm.autograd_AB(c.layout, m, st, u, eps, smp))
        vmin = float("inf")
        with torch.no_grad():
            for smp in [k for k in out if k != "ins"]:
                vmin = min(vmin, float(moments_truth(m, out[smp][0], u[:c.T - 1])[1].min()))
        return dict(out, states=torch.cat([out[k][0] for k in out if k != "ins"]), vmin=vmin)
    raise ValueError(c.form)
