"""The truth for the fused closed loop under the tanh-MLP policy ON A SIMULATED MEASUREMENT (mcp_rollout_mlp_meas / mcp_rollout_mlp_meas_bwd):
torch autograd through tests/open_grad_models.oracle_step with tests/pd_meas_models.measure (the measurement formulas of the reference's
MC_PILCO4PMS.apply_policy, policy_learning/MC_PILCO.py:856-899, pinned to the reference by tests/golden/rollout_pd_pms.npz) between the state
and tests/mlp_models.mlp_law.  Models, networks and inputs are those of tests/mlp_models.py (build_pair with PAIR_SEED, network, inputs_for,
seed = 100 T + M); the measurement model, its filter (pd_meas_models.FILTER: a1 != 0, b0 != b1, a0 != 1) and its noise (pos_noise_for) are
those of tests/pd_meas_models.py.  No GPU and no project code beyond the oracle.

    y_t = measure(x_t);   u_t = mlp(y_t);   x_{t+1} = step(x_t, u_t);      L = sum w * states + sum wu * inputs
"""
import torch

import mlp_models as mm
import pd_meas_models as pm
from open_grad_models import oracle_step
from pd_models import family, inputs_for

DT = torch.float64


def meas_model(shape, variant="all", std=0.1):
    """pd_meas_models.meas_model for the shapes of mlp_models (``limits`` included)."""
    return pm.meas_model(shape, variant, std, shapes=mm.SHAPES)


def mlp_meas_truth(shape, m, x0, params, eps, pos_noise, w, wu, sample, angle, non_angle, ms, u_max=1.0, squash=True, var_scale=None, defect=None):
    """Returns (states [T,M,S], inputs [T,M,U], measurements [T,M,S], [dL/dparam ...], dL/dx0, smallest variance met)."""
    x0 = x0.clone().requires_grad_(True)
    params = [q.clone().requires_grad_(True) for q in params]
    T = w.shape[0]
    law = lambda y: mm.mlp_law(y, params, angle, non_angle, u_max, squash)
    y, hist = pm.measure(x0, 0, ms, pos_noise, None, defect)
    xs, ys, us, vmin = [x0], [y], [law(y)], float("inf")
    for t in range(1, T):
        nx, var = oracle_step(family(shape), m, xs[-1], us[-1], eps[t - 1], sample, var_scale)
        vmin = min(vmin, float(var.detach().min()))
        y, hist = pm.measure(nx, t, ms, pos_noise, hist, defect)
        xs.append(nx)
        ys.append(y)
        us.append(law(y))
    st, inp, ym = torch.stack(xs), torch.stack(us), torch.stack(ys)
    L = (w * st).sum() + (0.0 if wu is None else (wu * inp).sum())
    grads = torch.autograd.grad(L, params + [x0], allow_unused=True)
    grads = [torch.zeros_like(q) if g is None else g for g, q in zip(grads, params + [x0])]
    return st.detach(), inp.detach(), ym.detach(), grads[:-1], grads[-1], vmin


# (mode, shape, degree, N, T, M, hidden, measurement variant, options): the smallest shapes at which each path can go wrong.  T = 1: the
# policy sees the true state only; T = 2: the one step whose history is row 0 (M = 17: two tiles, the second ragged); T = 3: the first row
# with both carries live; T = 12: the recursion proper.  Then one pair only, the pairs reversed, std = 0, the UR5 shape (six pairs), N = 300,
# feature lists that read one measured velocity and not the other, f = x, and once each on arm2 squashing off, a bound per input, no
# upstream g_inputs, var_scale != 1, requires_grad on one tensor alone; the sweep with the weights read from global memory (UR5 with
# (64, 64)), the sweep in parts over two tiles (limits), and the 16-trajectory forward forms (M = 1041)
CASES = [
    ("mean", "arm2", 0, 37, 1, 5, (5,), "all", {}),
    ("mean", "arm2", 1, 37, 2, 17, (7, 3), "all", {}),
    ("mean", "arm2_delta", 0, 37, 3, 1, (5,), "reversed", {}),
    ("sampled", "arm2", 2, 37, 12, 17, (64, 64), "all", {}),
    ("sampled", "arm2_delta", 1, 37, 12, 5, (7, 3), "all", {}),
    ("sampled", "arm2", 0, 37, 12, 5, (5,), "one", {}),
    ("sampled", "arm2", 0, 37, 12, 5, (5,), "all", {"std": 0.0}),
    ("sampled", "ur5", 1, 48, 3, 5, (64,), "all", {}),
    ("mean", "ur5", 1, 48, 12, 1, (33, 64), "all", {}),
    ("sampled", "arm2", 0, 300, 3, 17, (16,), "all", {}),
    ("sampled", "arm2", 1, 37, 12, 5, (5,), "all", {"angle": [1], "non_angle": [0, 3]}),
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), "all", {"features": "state"}),
    ("sampled", "arm2", 1, 37, 3, 5, (5,), "all", {"squash": False}),
    ("sampled", "arm2", 0, 37, 12, 5, (5,), "all", {"u_max": [0.4, 1.7]}),
    ("mean", "arm2", 1, 37, 12, 5, (7, 3), "all", {"no_g_inputs": True}),
    ("sampled", "arm2", 0, 37, 12, 5, (5,), "all", {"var_scale": [0.49, 2.25]}),
    ("sampled", "arm2", 0, 37, 3, 5, (7, 3), "all", {"only_grad": 2}),
    ("sampled", "ur5", 1, 48, 3, 5, (64, 64), "all", {}),
    ("sampled", "limits", 0, 37, 3, 20, (64, 64), "all", {}),
    ("sampled", "arm2", 0, 37, 3, 1041, (5,), "all", {}),
]


def case_id(c):
    return "-".join(str(v) for v in c[:6]) + "-h" + "x".join(str(h) for h in c[6]) + "-" + c[7] + ("-" + "-".join(sorted(c[8])) if c[8] else "")


def case_inputs(case):
    """(cfg, oracle model, inputs dict) of a case; the truth is ``case_truth``."""
    mode, shape, deg, N, T, M, hidden, variant, opt = case
    c, m, specs = mm.build_pair(shape, N, deg, seed=mm.PAIR_SEED)
    seed = T * 100 + M
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=seed)
    if opt.get("no_g_inputs"):
        wu = None
    angle, non_angle = mm.feature_lists(c, opt)
    params = mm.network(c, hidden, angle, non_angle, seed)
    ms = meas_model(shape, variant, opt.get("std", 0.1))
    pn = pm.pos_noise_for(T, M, len(ms["pos"]), seed)
    ins = dict(x0=x0, eps=eps, w=w, wu=wu, params=params, angle=angle, non_angle=non_angle, u_max=opt.get("u_max", 1.0), squash=opt.get("squash", True),
               specs=specs, ms=ms, pos_noise=pn, var_scale=opt.get("var_scale"), sample=mode == "sampled", shape=shape)
    return c, m, ins


def truth_of(m, ins, defect=None, **edit):
    """mlp_meas_truth on a case's inputs; ``edit`` replaces entries of the inputs (central differences)."""
    q = dict(ins, **edit)
    torch.set_num_threads(1)
    return mlp_meas_truth(q["shape"], m, q["x0"], q["params"], q["eps"], q["pos_noise"], q["w"], q["wu"], q["sample"], q["angle"], q["non_angle"], q["ms"],
                          u_max=q["u_max"], squash=q["squash"], var_scale=q["var_scale"], defect=defect)


def loss_of(m, ins, **edit):
    """L alone."""
    q = dict(ins, **edit)
    st, inp, *_ = truth_of(m, ins, **edit)
    return float((q["w"] * st).sum() + (0.0 if q["wu"] is None else (q["wu"] * inp).sum()))


def case_truth(case):
    """Everything a case compares against: (cfg, oracle model, inputs dict, truth tuple)."""
    c, m, ins = case_inputs(case)
    return c, m, ins, truth_of(m, ins)
