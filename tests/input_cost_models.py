"""The truth of the control-effort / input-rate cost tests (test_input_cost_cpu.py, test_gpu_input_cost.py): the whole cost as torch ops under
autograd on CPU fp64, written here on its own (not taken from the package), the hand gradient form the kernels implement, and the inputs the
GPU cases are drawn from.  A `case` is a dict: kind ("sat" / "quad" / "cartpole" / "traj"), joint, the state part (x, used_x, tg, ls; the
cart-pole reads used_x = [angle, pos]; "traj" holds its target rows in tg [T, S]) and the input part (u, used_u, l, r, ustar -- l / r None:
that term is absent; ustar None: 0)."""
import numpy as np
import torch

DT = torch.float64

# (T, M, S, U, used_x, used_u): the smallest shapes at which the indexing can go wrong
SHAPES = [(1, 2, 1, 1, [0], [0]),                                                # no rate row, no t + 1
          (2, 3, 2, 1, [1], [0]),                                                # a first and a last row only
          (3, 257, 4, 2, [2, 0], [1, 0]),                                        # M = 256 + 1; T M = 771; a middle row with both neighbours
          (2, 64, 16, 8, list(range(15, -1, -1)), list(range(7, -1, -1))),       # both limits, every index, reversed
          (4, 5, 4, 3, [0, 3], [2])]                                             # unused columns of both gradients
TERMS = ("effort", "rate", "both")  # effort only (u* = 0), rate only, both with a non-zero u*


def shape_id(s):
    return "T%dM%dS%dU%d" % tuple(s[:4])


def draw(T, M, S, U, used_x, used_u, seed=7):
    """States and inputs with d_x <= 3, d_u <= 3 and d_r <= 3, so d_x + d_u + d_r <= 9 in every case: 1 - exp(-d) stays away from the
    saturation where its own rounding (one ulp of 1) would decide the std -- the margin tests/test_gpu_target_cost.py::draw keeps.
    Used state i sits within sqrt(3 / n_x) l_i of its target; used input j within sqrt(3 / n_u) min(l_j, r_j / 2) of u*_j, so both its distance
    from u* and its step from one row to the next stay inside their budgets.  The other columns are arbitrary."""
    rs = np.random.RandomState(seed)
    nx, nu = len(used_x), len(used_u)
    x, u = rs.randn(T, M, S), rs.randn(T, M, U)
    ls, tg = 0.5 + 1.5 * rs.rand(nx), 2 * rs.rand(nx) - 1
    l, r = 0.5 + 1.5 * rs.rand(nu), 0.5 + 1.5 * rs.rand(nu)
    ustar = (0.25 + 0.75 * rs.rand(nu)) * np.where(rs.rand(nu) < 0.5, -1.0, 1.0)  # (away from 0: "u* = 0" is one of the changes the truth must feel)
    ax = (2 * rs.rand(T, M, nx) - 1) * np.sqrt(3.0 / nx)
    au = (2 * rs.rand(T, M, nu) - 1) * np.sqrt(3.0 / nu)
    for i, s in enumerate(used_x):
        x[:, :, s] = tg[i] + ls[i] * ax[:, :, i]
    for i, j in enumerate(used_u):
        u[:, :, j] = ustar[i] + min(l[i], r[i] / 2) * au[:, :, i]
    return dict(x=x, u=u, used_x=list(used_x), used_u=list(used_u), tg=tg, ls=ls, l=l, r=r, ustar=ustar)


def make_case(d, kind, joint, terms):
    """One case from a draw.  "effort" measures the effort from 0 (u* None), so its inputs are shifted to keep d_u <= 3."""
    c = dict(d, kind=kind, joint=bool(joint))
    if terms == "effort":
        u = d["u"].copy()
        for i, j in enumerate(d["used_u"]):
            u[:, :, j] -= d["ustar"][i]
        c.update(u=u, r=None, ustar=None)
    elif terms == "rate":
        c.update(l=None, ustar=None)
    else:
        assert terms == "both"
    if kind == "cartpole":
        # (|theta| - theta*) / l: the draw put theta around tg[0]; keep the angle's target positive and the states on its positive side
        c["x"] = d["x"].copy()
        a = d["used_x"][0]
        c["tg"] = d["tg"].copy()
        c["tg"][0] = abs(d["tg"][0]) + 4.0
        c["x"][:, :, a] = (d["x"][:, :, a] - d["tg"][0] + c["tg"][0]) * np.where(np.arange(d["x"].shape[1]) % 2 == 0, 1.0, -1.0)
    if kind == "traj":
        T, _, S = d["x"].shape
        rs = np.random.RandomState(5)
        off = 0.3 * rs.randn(T, S)
        tt = np.zeros((T, S))
        c["x"] = d["x"].copy()
        for i, s in enumerate(d["used_x"]):
            tt[:, s] = d["tg"][i] + off[:, s]
            c["x"][:, :, s] = d["x"][:, :, s] + off[:, s][:, None]
        c["tg"] = tt
    return c


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=DT)


def distances(c, x, u):
    """(d_x, d_u, d_r), each [T, M], as differentiable torch ops in the difference form."""
    T, M = x.shape[0], x.shape[1]
    if c["kind"] == "cartpole":
        a, p = c["used_x"]
        d_x = ((torch.abs(x[:, :, a]) - c["tg"][0]) / c["ls"][0]) ** 2 + ((x[:, :, p] - c["tg"][1]) / c["ls"][1]) ** 2
    elif c["kind"] == "traj":
        e = (x[:, :, c["used_x"]] - _t(c["tg"])[:, None, c["used_x"]]) / _t(c["ls"])
        d_x = (e * e).sum(2)
    else:
        e = (x[:, :, c["used_x"]] - _t(c["tg"])) / _t(c["ls"])
        d_x = (e * e).sum(2)
    uu = u[:, :, c["used_u"]]
    d_u = d_r = torch.zeros(T, M, dtype=DT)
    if c["l"] is not None:
        e = (uu - (0.0 if c["ustar"] is None else _t(c["ustar"]))) / _t(c["l"])
        d_u = (e * e).sum(2)
    if c["r"] is not None:
        e = (uu[1:] - uu[:-1]) / _t(c["r"])
        d_r = torch.cat([torch.zeros(1, M, dtype=DT), (e * e).sum(2)])
    return d_x, d_u, d_r


def costs_of(c, x, u):
    d_x, d_u, d_r = distances(c, x, u)
    if c["kind"] == "quad":
        return d_x + d_u + d_r
    if c["joint"]:
        return 1 - torch.exp(-(d_x + d_u + d_r))
    return 1 - torch.exp(-d_x) + d_u + d_r


def truth(c, gscale=None):
    """Per-particle costs [T, M], cost = sum_t mean_m c, std = sum_t std_m c (unbiased) and the autograd gradients of cost in the states
    and the inputs (``gscale``: of gscale sum_t sum_m c instead -- what a shard of a larger swarm computes), CPU fp64."""
    x, u = _t(c["x"]).clone().requires_grad_(True), _t(c["u"]).clone().requires_grad_(True)
    costs = costs_of(c, x, u)
    cost = torch.sum(torch.mean(costs, 1))
    std = torch.sum(torch.std(costs.detach(), 1)) if costs.shape[1] > 1 else torch.zeros((), dtype=DT)
    (cost if gscale is None else gscale * costs.sum()).backward()
    return dict(costs=costs.detach(), cost=cost.detach(), std=std, g_states=x.grad, g_inputs=u.grad)


def hand_gradients(c):
    """The issue's hand form, in numpy: g_states = b_t d d_x / dx and
    g_inputs[t] = a_t (2 (u_t - u*) / l^2 + [t >= 1] 2 (u_t - u_{t-1}) / r^2) - [t + 1 < T] a_{t+1} 2 (u_{t+1} - u_t) / r^2, with G = 1 / M,
    a = G (ADD) or G f'(d_x + d_u + d_r) (JOINT), b = G f'(d_x) (ADD) or a (JOINT)."""
    x, u = np.asarray(c["x"], dtype=float), np.asarray(c["u"], dtype=float)
    T, M, S = x.shape
    d_x, d_u, d_r = (v.numpy() for v in distances(c, _t(x), _t(u)))
    G = 1.0 / M
    quad = c["kind"] == "quad"
    fp = (lambda d: np.ones_like(d)) if quad else (lambda d: np.exp(-d))
    a = G * fp(d_x + d_u + d_r) if c["joint"] else G * np.ones_like(d_x)
    b = a if c["joint"] else G * fp(d_x)
    gx, gu = np.zeros_like(x), np.zeros_like(u)
    if c["kind"] == "cartpole":
        ai, pi = c["used_x"]
        gx[:, :, ai] = b * 2 * (np.abs(x[:, :, ai]) - c["tg"][0]) / c["ls"][0] ** 2 * np.sign(x[:, :, ai])
        gx[:, :, pi] = b * 2 * (x[:, :, pi] - c["tg"][1]) / c["ls"][1] ** 2
    else:
        for i, s in enumerate(c["used_x"]):
            tg = c["tg"][:, s][:, None] if c["kind"] == "traj" else c["tg"][i]
            gx[:, :, s] = b * 2 * (x[:, :, s] - tg) / c["ls"][i] ** 2
    for i, j in enumerate(c["used_u"]):
        v = np.zeros((T, M))
        if c["l"] is not None:
            v += a * 2 * (u[:, :, j] - (0.0 if c["ustar"] is None else c["ustar"][i])) / c["l"][i] ** 2
        if c["r"] is not None:
            step = 2 * (u[1:, :, j] - u[:-1, :, j]) / c["r"][i] ** 2  # [T-1, M]: row k is the step into t = k + 1
            v[1:] += a[1:] * step
            v[:-1] -= a[1:] * step
        gu[:, :, j] = v
    return gx, gu


def variants(c):
    """The four changes a kernel that ignores a term would not notice -- the effort term dropped, the rate term dropped, u* set to 0, the
    mode swapped -- each where the case has that term (the modes of the plain distance coincide): (name, changed case)."""
    out = []
    if c["l"] is not None:
        out.append(("effort dropped", dict(c, l=None, ustar=None)))
    if c["r"] is not None and np.asarray(c["u"]).shape[0] > 1:  # (with one time step the rate term is 0 by definition: nothing to feel)
        out.append(("rate dropped", dict(c, r=None)))
    if c["ustar"] is not None:
        out.append(("u* = 0", dict(c, ustar=None)))
    if c["kind"] != "quad" and out:  # (a case whose only term is the rate at T = 1 has no input term left to combine)
        out.append(("mode swapped", dict(c, joint=not c["joint"])))
    return out


def gpu_cases():
    """Every GPU parity case: each shape with the two target kinds x {ADD, JOINT} x TERMS; cart-pole and trajectory at the third shape in
    both modes with both terms.  -> list of (id, case)."""
    out = []
    for sh in SHAPES:
        d = draw(*sh)
        for kind in ("sat", "quad"):
            for joint in (False, True):
                for terms in TERMS:
                    out.append(("%s-%s-%s-%s" % (shape_id(sh), kind, "joint" if joint else "add", terms), make_case(d, kind, joint, terms)))
    d = draw(*SHAPES[2])
    for kind in ("cartpole", "traj"):
        for joint in (False, True):
            out.append(("%s-%s-%s-both" % (shape_id(SHAPES[2]), kind, "joint" if joint else "add"), make_case(d, kind, joint, "both")))
    return out
