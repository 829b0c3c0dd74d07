"""The truth for the fused closed loop under the PID controller (mcp_rollout_pid / mcp_rollout_pid_bwd): torch autograd through
tests/open_grad_models.oracle_step with the law written out --
    e = target[t] - x (measured form: y);  q_t = I_{t-1} + dt e[pos];  I_t = torch.clamp(q_t, -i_max, +i_max);
    u = squash(kp^2 e[pos] + kd^2 e[vel] + ki^2 I_t)
-- on the models and inputs of tests/pd_models.py (build_pair, inputs_for), with sqrt_ki drawn in [0.5, 1.5] from a generator of its own,
and on the measurement of tests/pd_meas_models.measure for the measured form.  The table of GPU cases and the two clamp conditions every
case is held to (tests/test_pid_cpu.py asserts them on the truth alone).  CPU side only imports torch, helpers and the oracle."""
import collections
import math

import torch

from open_grad_models import oracle_step
from pd_meas_models import meas_model, measure, pos_noise_for
from pd_models import SHAPES, build_pair, family, inputs_for  # noqa: F401  (build_pair: the Family of the GPU module names this module)

DT = torch.float64
DT_STEP = 0.05  # the integration step of every case (a descriptor field of its own: not the model's Ts)
INF = math.inf

PidTruth = collections.namedtuple("PidTruth", "states inputs meas integ q grads g_x0 vmin")


def ki_for(c, seed):
    """sqrt_ki in [0.5, 1.5], from a generator of its own (pd_models.inputs_for's draws stay what they are)."""
    gen = torch.Generator().manual_seed(5000 + seed)
    return 0.5 + torch.rand(c["U"], dtype=DT, generator=gen)


def bounds(i_max, U):
    """[U] tensor of the bounds: a scalar for every input, or one per input (inf: no clamp)."""
    b = torch.as_tensor(i_max, dtype=DT).reshape(-1)
    return b.expand(U).clone() if b.numel() == 1 else b


def pid_law(x, t, integ, kp, kd, ki, target, dt, i_max, u_max, squash, pos, vel):
    """(u, I_t, q_t) of one evaluation on x (the state, or its measurement) with the integral ``integ`` of the row before."""
    err = target[t].reshape(1, -1) - x
    q = integ + dt * err[:, pos]
    b = bounds(i_max, len(pos))
    new = torch.clamp(q, -b, b)
    a = kp ** 2 * err[:, pos] + kd ** 2 * err[:, vel] + ki ** 2 * new
    if not squash:
        return a, new, q
    um = torch.as_tensor(u_max, dtype=DT)
    return um * torch.tanh(a / um), new, q


def pid_truth(shape, m, x0, kp, kd, ki, target, eps, w, wu, sample, dt=DT_STEP, i_max=INF, u_max=1.0, squash=True, var_scale=None, ms=None,
              pos_noise=None):
    """torch autograd through oracle_step with the policy (and with ``ms`` the measurement, pd_meas_models.measure) written out.
    L = sum w * states + sum wu * inputs (wu None: states only).  Returns a PidTruth: states [T,M,S], inputs [T,M,U], measurements [T,M,S]
    or None, I and q [T,M,U], [dL/dsqrt_kp, dL/dsqrt_kd, dL/dsqrt_ki], dL/dx0, the smallest variance met."""
    S, U = x0.shape[1], kp.shape[0]
    h = S // 2
    pos, vel = list(range(U)), list(range(h, h + U))
    x0 = x0.clone().requires_grad_(True)
    kp, kd, ki = (g.clone().requires_grad_(True) for g in (kp, kd, ki))
    T = w.shape[0]
    law = lambda y, t, integ: pid_law(y, t, integ, kp, kd, ki, target, dt, i_max, u_max, squash, pos, vel)
    y, hist = (x0, None) if ms is None else measure(x0, 0, ms, pos_noise, None)
    u, integ, q = law(y, 0, torch.zeros(x0.shape[0], U, dtype=DT))
    xs, ys, us, Is, qs, vmin = [x0], [y], [u], [integ], [q], float("inf")
    for t in range(1, T):
        nx, var = oracle_step(family(shape), m, xs[-1], us[-1], eps[t - 1], sample, var_scale)
        vmin = min(vmin, float(var.detach().min()))
        y = nx
        if ms is not None:
            y, hist = measure(nx, t, ms, pos_noise, hist)
        u, integ, q = law(y, t, Is[-1])
        xs.append(nx), ys.append(y), us.append(u), Is.append(integ), qs.append(q)
    st, inp = torch.stack(xs), torch.stack(us)
    L = (w * st).sum() + (0.0 if wu is None else (wu * inp).sum())
    gkp, gkd, gki, gx = torch.autograd.grad(L, [kp, kd, ki, x0], allow_unused=True)
    gki = torch.zeros_like(ki) if gki is None else gki
    return PidTruth(st.detach(), inp.detach(), None if ms is None else torch.stack(ys).detach(), torch.stack(Is).detach(), torch.stack(qs).detach(),
                    [gkp, gkd, gki], gx, vmin)


def loss_of(*a, **kw):
    """L alone (central differences): the arguments of pid_truth."""
    t = pid_truth(*a, **kw)
    w, wu = a[8], a[9]
    return float((w * t.states).sum() + (0.0 if wu is None else (wu * t.inputs).sum()))


# ---- the clamp conditions ---------------------------------------------------------------------------------------------------------------------
SHARE = (0.1, 0.9)     # a finite-i_max case has clamped and unclamped (t, m, k) entries, each share within these
MARGIN = 1e-7          # min | |q| - i_max | of every parity case: two orders above the bound on the states, so no side of a clamp can flip
FD_MARGIN = 1e-3       # ... of the central-difference case, whose step is 1e-6


def clamp_figures(truth, i_max):
    """(share of the clamped entries, min | |q| - i_max | over the inputs with a finite bound) of a truth; (0, inf) without a finite bound."""
    b = bounds(i_max, truth.q.shape[2])
    fin = torch.isfinite(b)
    if not bool(fin.any()):
        return 0.0, float("inf")
    clamped = (truth.q.abs() >= b).to(DT)
    return float(clamped.mean()), float((truth.q.abs() - b).abs()[:, :, fin].min())


# (mode, shape, degree, N, T, M, measurement variant or None, options): the shapes of pd_models.CASES / pd_meas_models.CASES -- N = 37 (Npad
# 48: the last 32-row block of Kinv is a remainder) with T in {1, 2, 3, 12} and M in {1, 5, 17} (two tiles, the last one ragged), both modes,
# degrees 0 / 1 / 2 on arm2 and arm2_delta; the UR5 shape at N = 48; N = 300 once per mode; squashing off, a bound per input, no upstream
# g_inputs.  i_max: inf, a finite scalar, a list with one inf entry.  T == 1 and T == 2 leave the integral two rows at most: those cases run
# unclamped; the finite bounds (seeds and bounds chosen so that the clamp conditions hold; a case that stopped meeting them would get
# another seed or bound, never another condition) sit on the rows with T >= 3.  "seed": the offset of the inputs' seed T * 100 + M.
CASES = [
    ("mean", "arm2", 0, 37, 1, 5, None, {}), ("mean", "arm2", 1, 37, 3, 17, None, {"i_max": 0.02}), ("mean", "arm2", 2, 37, 12, 1, None, {"i_max": 0.05}),
    ("mean", "arm2_delta", 0, 37, 12, 17, None, {"i_max": 0.05}), ("mean", "arm2_delta", 1, 37, 2, 1, None, {}),
    ("mean", "arm2_delta", 2, 37, 3, 5, None, {"i_max": [0.02, INF]}),
    ("sampled", "arm2", 0, 37, 12, 17, None, {"i_max": 0.05}), ("sampled", "arm2", 1, 37, 2, 5, None, {}), ("sampled", "arm2", 2, 37, 3, 5, None, {"i_max": 0.02}),
    ("sampled", "arm2_delta", 0, 37, 1, 17, None, {}), ("sampled", "arm2_delta", 1, 37, 12, 5, None, {"i_max": 0.05}),
    ("sampled", "arm2_delta", 2, 37, 12, 1, None, {"i_max": [INF, 0.05]}),
    ("mean", "arm2", 0, 300, 12, 1, None, {"i_max": 0.05}), ("sampled", "arm2", 0, 300, 3, 17, None, {"i_max": 0.02}),
    ("mean", "ur5", 1, 48, 12, 1, None, {"i_max": 0.02}), ("sampled", "ur5", 1, 48, 12, 5, None, {"i_max": 0.05}),
    ("sampled", "arm2", 1, 37, 3, 5, None, {"squash": False, "i_max": 0.02}),
    ("sampled", "arm2", 0, 37, 12, 5, None, {"u_max": [0.4, 1.7], "i_max": 0.05}),
    ("mean", "arm2", 1, 37, 12, 5, None, {"no_g_inputs": True, "i_max": 0.05}),
    # the measured form
    ("mean", "arm2", 0, 37, 1, 5, "all", {}), ("mean", "arm2", 1, 37, 2, 17, "all", {}), ("mean", "arm2", 2, 37, 12, 1, "all", {"i_max": 0.05}),
    ("mean", "arm2_delta", 0, 37, 12, 17, "all", {"i_max": 0.05}), ("sampled", "arm2", 0, 37, 12, 17, "all", {"i_max": 0.05}),
    ("sampled", "arm2", 1, 37, 3, 5, "one", {"i_max": 0.02}), ("sampled", "arm2_delta", 2, 37, 12, 5, "reversed", {"i_max": [0.05, INF]}),
    ("sampled", "arm2", 0, 300, 3, 17, "all", {"i_max": 0.02}), ("sampled", "ur5", 1, 48, 12, 5, "all", {"i_max": 0.05}),
    ("sampled", "arm2", 1, 37, 3, 5, "all", {"squash": False, "i_max": 0.02}),
    ("mean", "arm2", 1, 37, 12, 5, "all", {"no_g_inputs": True, "i_max": 0.05}),
]


def case_id(c):
    opt = dict(c[7])
    im = opt.pop("i_max", INF)
    opt.pop("seed", None)
    tag = "imax_" + ("_".join("%g" % v for v in im) if isinstance(im, list) else "%g" % im)
    return "-".join(str(v) for v in c[:6]) + ("-meas_" + c[6] if c[6] else "") + "-" + tag + ("-" + "-".join(sorted(opt)) if opt else "")


def case_inputs(case):
    """What a case launches on, the model apart: (x0, kp, kd, ki, target, eps, w, wu or None, measurement model or None, its noise or None,
    keywords of pid_truth: i_max, u_max, squash)."""
    mode, shape, deg, N, T, M, variant, opt = case
    c = SHAPES[shape]
    seed = T * 100 + M + opt.get("seed", 0)
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=seed)
    ms = None if variant is None else meas_model(shape, variant)
    pn = None if ms is None else pos_noise_for(T, M, len(ms["pos"]), seed)
    kw = dict(i_max=opt.get("i_max", INF), u_max=opt.get("u_max", 1.0), squash=opt.get("squash", True))
    return x0, kp, kd, ki_for(c, seed), target, eps, w, (None if opt.get("no_g_inputs") else wu), ms, pn, kw


def case_truth(case, m):
    """The PidTruth of a case on its oracle model ``m``, and its inputs."""
    mode, shape = case[0], case[1]
    x0, kp, kd, ki, target, eps, w, wu, ms, pn, kw = inp = case_inputs(case)
    return pid_truth(shape, m, x0, kp, kd, ki, target, eps, w, wu, mode == "sampled", ms=ms, pos_noise=pn, **kw), inp


# the central-difference case (Philox mode, seed 77 / call 5: its eps are restated on the CPU by tests/noise_truth.eps_table): arm2, N = 37,
# degree 2, M = 3, T = 6, inputs of seed 5 -- the case of tests/test_gpu_pd_rollout.py -- with the bound below
FD_CASE = dict(shape="arm2", N=37, deg=2, M=3, T=6, seed=5, i_max=0.05, philox=(77, 5))


def fd_inputs():
    """(x0, kp, kd, ki, target, w, wu) of FD_CASE."""
    c = SHAPES[FD_CASE["shape"]]
    x0, kp, kd, target, _, w, wu = inputs_for(c, FD_CASE["M"], FD_CASE["T"], seed=FD_CASE["seed"])
    return x0, kp, kd, ki_for(c, FD_CASE["seed"]), target, w, wu
