"""The truth for the fused closed loop under the time-varying linear feedback law (mcp_rollout_tvl / mcp_rollout_tvl_bwd,
Policy.TV_linear_controller): torch autograd through tests/open_grad_models.oracle_step with the law written out,
    e_t = target[t] - r_t;   a_t = gain[t] e_t + ff[t];   u_t = u_max tanh(a_t / u_max)  (or a_t)
r_t the state, or -- the measured variant -- the simulated measurement of tests/pd_meas_models.measure.  The loop is that of
pd_models.pd_truth (pd_meas_models.pd_meas_truth); models and inputs are those of tests/pd_models.py, this module adds the dense gains, the
feedforward and the table of GPU cases.  CPU side only imports torch, helpers and the oracle."""
import collections

import torch

from open_grad_models import oracle_step
from pd_meas_models import measure
from pd_models import family, inputs_for

DT = torch.float64
Result = collections.namedtuple("Result", "states inputs meas g_gain g_ff g_x0 vmin")


def from_pd(kp, kd, S, T):
    """The PD law as dense gains [T,U,S]: gain[t][k][k] = kp_k^2, gain[t][k][S // 2 + k] = kd_k^2."""
    U = kp.shape[0]
    g = torch.zeros(U, S, dtype=DT)
    for k in range(U):
        g[k, k] = kp[k] ** 2
        g[k, S // 2 + k] = kd[k] ** 2
    return g.unsqueeze(0).repeat(T, 1, 1)


def tvl_inputs(c, M, T, seed):
    """pd_models.inputs_for's draws, and from a generator of its own (5000 + seed) the PD gains perturbed densely and a feedforward:
    (x0, kp, kd, target, eps, w, wu, gain [T,U,S], ff [T,U])."""
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed)
    gen = torch.Generator().manual_seed(5000 + seed)
    gain = from_pd(kp, kd, c["S"], T) + 0.1 * torch.randn(T, c["U"], c["S"], dtype=DT, generator=gen)
    ff = 0.2 * torch.randn(T, c["U"], dtype=DT, generator=gen)
    return x0, kp, kd, target, eps, w, wu, gain, ff


def tvl_law(r, t, gain, ff, target, u_max, squash):
    """gain [rows,U,S] or [U,S] (shared); ff [rows,U] or None."""
    err = target[t].reshape(1, -1) - r
    a = err @ (gain[t] if gain.dim() == 3 else gain).T
    if ff is not None:
        a = a + ff[t].reshape(1, -1)
    if not squash:
        return a
    um = torch.as_tensor(u_max, dtype=DT)
    return um * torch.tanh(a / um)


def tvl_truth(shape, m, x0, gain, ff, target, eps, w, wu, sample, u_max=1.0, squash=True, var_scale=None, ms=None, pos_noise=None):
    """L = sum w * states + sum wu * inputs (wu None: states only).  ``ms``: the measurement model of pd_meas_models.meas_model (None: the
    law reads the true state).  Returns a Result: states [T,M,S], inputs [T,M,U], measurements or None, dL/dgain (gain's shape), dL/dff or
    None, dL/dx0, the smallest variance met."""
    x0 = x0.clone().requires_grad_(True)
    gain = gain.clone().requires_grad_(True)
    ff = None if ff is None else ff.clone().requires_grad_(True)
    T = w.shape[0]
    read = (lambda x, t, hist: measure(x, t, ms, pos_noise, hist)) if ms is not None else (lambda x, t, hist: (x, None))
    y, hist = read(x0, 0, None)
    xs, ys, us, vmin = [x0], [y], [tvl_law(y, 0, gain, ff, target, u_max, squash)], float("inf")
    for t in range(1, T):
        nx, var = oracle_step(family(shape), m, xs[-1], us[-1], eps[t - 1], sample, var_scale)
        vmin = min(vmin, float(var.detach().min()))
        y, hist = read(nx, t, hist)
        xs.append(nx)
        ys.append(y)
        us.append(tvl_law(y, t, gain, ff, target, u_max, squash))
    st, inp = torch.stack(xs), torch.stack(us)
    L = (w * st).sum() + (0.0 if wu is None else (wu * inp).sum())
    grads = torch.autograd.grad(L, [gain, x0] + ([ff] if ff is not None else []), allow_unused=True)
    zero = lambda g, like: torch.zeros_like(like) if g is None else g
    return Result(st.detach(), inp.detach(), torch.stack(ys).detach() if ms is not None else None, zero(grads[0], gain),
                  None if ff is None else zero(grads[2], ff), zero(grads[1], x0), vmin)


# (shape, degree, N, T, M): the sampled cases; the seed of a case is 100 T + M
SAMPLED = [("arm2", 0, 37, 12, 17), ("arm2", 1, 37, 3, 5), ("arm2", 2, 37, 12, 33), ("arm2_delta", 0, 37, 12, 17), ("arm2_delta", 2, 37, 12, 5),
           ("arm2", 0, 300, 3, 17), ("ur5", 1, 48, 12, 5), ("ur5", 1, 48, 3, 17)]
# (mode, shape, degree, N, T, M, measurement variant or None, options): the eight in both modes (M = 33: three tiles of the sweep, the last
# ragged); T in {1, 2} and M = 1; squashing off, a bound per input, no upstream g_inputs, no feedforward, a shared gain; the measured
# variants of pd_meas_models on arm2 and once on ur5
CASES = ([("sampled",) + s + (None, {}) for s in SAMPLED] + [("mean",) + s + (None, {}) for s in SAMPLED] + [
    ("sampled", "arm2", 0, 37, 1, 5, None, {}), ("mean", "arm2", 1, 37, 2, 1, None, {}), ("sampled", "arm2_delta", 1, 37, 2, 17, None, {}),
    ("sampled", "arm2", 1, 37, 3, 5, None, {"squash": False}),
    ("sampled", "arm2", 0, 37, 12, 5, None, {"u_max": [0.4, 1.7]}),
    ("mean", "arm2", 1, 37, 12, 5, None, {"no_g_inputs": True}),
    ("sampled", "arm2", 0, 37, 12, 33, None, {"no_g_inputs": True}),
    ("sampled", "arm2", 0, 37, 12, 17, None, {"no_ff": True}),
    ("sampled", "arm2", 2, 37, 12, 17, None, {"shared": True}),
    ("sampled", "arm2", 0, 37, 12, 17, "all", {}), ("mean", "arm2", 1, 37, 12, 5, "one", {}), ("sampled", "arm2", 1, 37, 12, 33, "reversed", {}),
    ("sampled", "arm2", 2, 37, 1, 5, "all", {}), ("sampled", "arm2_delta", 0, 37, 3, 17, "all", {"no_g_inputs": True}),
    ("sampled", "arm2", 0, 37, 12, 5, "one", {"shared": True, "no_ff": True}),
    ("sampled", "ur5", 1, 48, 3, 5, "all", {}),
])


def case_id(c):
    return "-".join(str(v) for v in c[:6]) + ("-" + c[6] if c[6] else "") + ("-" + "-".join(sorted(c[7])) if c[7] else "")


def case_seed(T, M):
    return 100 * T + M


def case_operands(case, c):
    """(x0, gain, ff, target, eps, w, wu, kw of tvl_truth without the measurement) of a row of CASES on the shape record ``c``."""
    mode, shape, deg, N, T, M, variant, opt = case
    x0, kp, kd, target, eps, w, wu, gain, ff = tvl_inputs(c, M, T, case_seed(T, M))
    if opt.get("shared"):
        gain = gain[0].clone()
    if opt.get("no_ff"):
        ff = None
    if opt.get("no_g_inputs"):
        wu = None
    kw = dict(u_max=opt.get("u_max", 1.0), squash=opt.get("squash", True))
    return x0, gain, ff, target, eps, w, wu, kw
