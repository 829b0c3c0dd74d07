"""The sampling planner's rollout entries (mcp_mppi_rollout, mcp_plan_rollout: csrc/mppi.hip) on the irregular layouts of
tests/layout_models.py: the table of cases with what every row pins, the operands, the truth glue over tests/mppi_truth.py and
tests/cem_truth.py, the status constructions with their expected word by the rule of tests/status_models.py, and a Python mirror of the
kernel's LDS arithmetic (open_layout of rollout_open_phases.h, mppi_extra of mppi.hip) from which the long-horizon rows are derived.
tests/test_plan_models_cpu.py holds every condition the GPU module (tests/test_gpu_plan_layouts.py) relies on, on the truth alone.
CPU side only imports torch, numpy, the oracle and the other truth modules."""
import collections
import dataclasses
import functools

import numpy as np
import torch

import cem_truth as ct
import layout_models as lay
import mppi_truth as mt
import status_models as sm
from open_grad_models import oracle_step
from oracle import mcpilco_oracle as orc

DT = torch.float64

# ---- the LDS arithmetic (doubles) -----------------------------------------------------------------------------------------------------------
LDS_DOUBLES = 160 * 1024 // 8  # MCP_LDS_LIMIT / sizeof(double) = 20480
RF_NW, GPL_DOUBLES = 8, 9  # waves of a workgroup; sizeof(GpL) / 8: four pointers, three doubles, four ints


def _even(n):
    return (n + 1) & ~1


def open_layout(PT, needvar, S, D, G, npad, extra):
    """(total doubles, xl) of open_layout(PT, needvar, S, D, G, NpadMax, false, 0, false, extra): xs | z | red | gpl | kpar | the k panel
    (with variances; row pitch 18 for 16 trajectories) | extra | -- the mean form, if it still fits -- X^T and alpha of every GP."""
    o = _even(2 * PT * S) + _even(PT * D) + _even(2 * G * RF_NW * PT) + _even(G * GPL_DOUBLES) + _even(G * (5 * D + 1))
    if needvar:
        o += _even(npad * (18 if PT == 16 else PT))
    if extra > 0:
        o += _even(extra)
    xl = (not needvar) and o + G * (D + 1) * npad + 4 <= LDS_DOUBLES
    if xl:
        o += _even(G * D * npad) + _even(G * npad)
    return o, xl


def mppi_extra(PT, H, U, ext=False):
    """mppi.hip: the nominal [H][U] | u_t, u_{t-1} of the tile [2][PT][U] | (the extended form) the std's rows [H][U]."""
    return H * U + 2 * PT * U + (H * U if ext else 0)


def dims(layout, N):
    c = lay.LAYOUTS[layout]
    return c["S"], len(c["not_angle"]) + 2 * len(c["angle"]) + c["U"], c["G"], (N + 15) // 16 * 16, c["U"]


def rung(layout, N, H, sample, ext):
    """(trajectories per workgroup, operands staged in LDS) of mppi_ladder: the mean chain 1, with variances 16, then 4; None: refused."""
    S, D, G, npad, U = dims(layout, N)
    for PT in ((16, 4) if sample else (1,)):
        total, xl = open_layout(PT, sample, S, D, G, npad, mppi_extra(PT, H, U, ext))
        if total <= LDS_DOUBLES:
            return PT, xl
    return None


def largest_h(layout, N, PT, sample, ext):
    """The largest H whose rows fit beside the layout of ``PT`` trajectories (the layout is monotone in H)."""
    S, D, G, npad, U = dims(layout, N)
    H = 2
    while open_layout(PT, sample, S, D, G, npad, mppi_extra(PT, H + 1, U, ext))[0] <= LDS_DOUBLES:
        H += 1
    return H


# The long horizons on "limits" (S 16, U 8, G 8, D 32, Npad 48), sampled, 16 trajectories per workgroup:
#   xs 2*16*16 = 512 | z 16*32 = 512 | red 2*8*8*16 = 2048 | gpl 8*9 = 72 | kpar 8*(5*32+1) = 1288 | panel 48*18 = 864  -> 5296 doubles
#   mppi: extra = 8 H + 2*16*8  -> 5296 + 256 + 8 H  <= 20480  <=>  H <= 1866;   H = 1867 falls to the 4-trajectory rung
#   plan: extra = 16 H + 256    -> 5552 + 16 H       <= 20480  <=>  H <= 933;    H = 934 falls to the 4-trajectory rung
# (the 4-rung: 128 + 128 + 512 + 72 + 1288 + 192 = 2320, + 64 + 8 H: H <= 2262; + 64 + 16 H: H <= 1131).  The mean form at these H runs
# WITHOUT the operands staged in LDS (1552 + 16 + 8 H + 12676 > 20480 from H = 780 on; plan: from H = 390 on), the H <= 6 rows with.
LONG = {"mppi": (1866, 1867), "plan": (933, 934)}

# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# (entry, mode, layout, degree, N, H, K, P, options).  entry: mppi = mcp_mppi_rollout, plan = mcp_plan_rollout under a non-default extension.
# N = 37 (Npad 48).  Options: "cost" the descriptor pair of ``cost_specs`` the oracle comparison runs under (every short row runs the cost
# BITS under all of them); "squash": False; for plan "beta", "rows" (a std per row), "u_prev", "t0".  sigma and u_max are distinct per
# input everywhere, and one sigma (one column of the std's rows) is 0 wherever U >= 2 (``sigma_of``).
# (The sampled degree-2 rows on limits and d15_plain run their oracle comparison under "quad_joint" / "wide": their velocities reach 5 .. 6, and
# the fifteen active dimensions of "target_add" would saturate -- tests/test_plan_models_cpu.py refuses a saturated point cost.)
Case = collections.namedtuple("Case", "entry mode layout deg N H K P opt")
_S, _M = "sampled", "mean"
CASES = [Case(*r) for r in [
    # mcp_mppi_rollout
    ("mppi", _S, "cart", 0, 37, 6, 7, 3, dict(cost="target_add")),  # M = 21: candidate 5 straddles the 16-tile edge; U = 1: ONE input thread per trajectory
    ("mppi", _S, "all_angle", 1, 37, 2, 3, 16, dict(cost="traj_plain", t0=2)),  # H = 2: the loop breaks in its second pass, ONE draw a row ahead; a candidate per tile exactly; S = 2, n_not_angle = 0
    ("mppi", _S, "g1_plain", 2, 37, 6, 33, 1, dict(cost="wide")),  # G = 1; component 0 integrated by no GP (og = -1) and in the cost; M = 33: three tiles, the last holds one
    ("mppi", _S, "mixed5", 1, 37, 6, 7, 3, dict(cost="wide", squash=False)),  # zi_ang by the LAST match of an unsorted list, component 0 plain AND angle, component 2 in neither; GPs out of order (og); U = 3 != S / 2; no squashing
    ("mppi", _M, "mixed5", 0, 37, 6, 19, 1, dict(cost="target_add")),  # the mean form (PT = 1, operands staged in LDS) on the same lists
    ("mppi", _S, "d15_plain", 0, 37, 6, 1, 5, dict(cost="quad_joint")),  # K = 1: the nominal alone, xi never read; D + 1 = 16; U = 5 odd
    ("mppi", _S, "d16_angles", 1, 37, 6, 2, 17, dict(cost="wide")),  # M = 34: three tiles, the last holds 2; D + 1 = 17; component 6 a GP input nothing integrates
    ("mppi", _M, "d16_angles", 2, 37, 2, 7, 1, dict(cost="target_add")),  # mean, H = 2, degree 2
    ("mppi", _S, "limits", 2, 37, 6, 7, 3, dict(cost="quad_joint")),  # PT (S + U + 1) = 400 threads, D + 1 = 33, the NEEDVAR && MAXDEG >= 1 barrier at D = 32
    ("mppi", _M, "limits", 1, 37, 3, 19, 1, dict(cost="target_add")),  # mean at the limits, H = 3
    # mcp_plan_rollout
    ("plan", _S, "cart", 1, 37, 3, 7, 3, dict(cost="target_add", beta=0.5, rows=True, u_prev=True)),  # H = 3 with u_prev: rows 0 and 2 share a slot of ub, row -1 shares row 1's
    ("plan", _S, "all_angle", 0, 37, 6, 2, 17, dict(cost="target_add", beta=0.0, rows=True)),  # beta = 0 under a std per row; three tiles, the last holds 2
    ("plan", _S, "g1_plain", 1, 37, 3, 3, 16, dict(cost="wide", beta=0.5, u_prev=True)),  # the colouring without a std per row; the rate term of the one input against u_prev
    ("plan", _S, "mixed5", 2, 37, 3, 7, 3, dict(cost="traj_rate", beta=0.5, rows=True, u_prev=True, t0=2)),  # everything at once: t0 > 0 under a trajectory cost, the rate on input U - 1 = 2 alone
    ("plan", _M, "mixed5", 1, 37, 6, 19, 1, dict(cost="wide", beta=0.5, rows=True)),  # the extended mean form
    ("plan", _S, "d15_plain", 2, 37, 6, 33, 1, dict(cost="wide", beta=0.5, u_prev=True)),  # (33, 1) under the extension, U = 5
    ("plan", _S, "d16_angles", 0, 37, 2, 7, 3, dict(cost="wide", beta=0.0, u_prev=True)),  # H = 2 and u_prev ALONE makes the extension non-default
    ("plan", _M, "d16_angles", 1, 37, 3, 7, 1, dict(cost="traj_rate", beta=0.5, rows=True, u_prev=True, t0=1)),  # mean, H = 3 with u_prev
    ("plan", _S, "limits", 2, 37, 3, 7, 3, dict(cost="wide", beta=0.5, rows=True, u_prev=True)),  # the partition at its limit with the std's rows staged; ub's slot parity at U = 8
    ("plan", _M, "limits", 0, 37, 6, 7, 1, dict(cost="target_add", beta=0.0, rows=True)),
    # the long horizons (the arithmetic above): the last H of the 16-trajectory rung and the first of the 4-rung, M = 6; the mean form unstaged
    ("mppi", _S, "limits", 0, 37, 1866, 2, 3, dict(cost="target_add")), ("mppi", _S, "limits", 0, 37, 1867, 2, 3, dict(cost="target_add")),
    ("mppi", _M, "limits", 0, 37, 1867, 3, 1, dict(cost="target_add")),
    ("plan", _S, "limits", 0, 37, 933, 2, 3, dict(cost="target_add", beta=0.5, rows=True, u_prev=True)),
    ("plan", _S, "limits", 0, 37, 934, 2, 3, dict(cost="target_add", beta=0.5, rows=True, u_prev=True)),
    ("plan", _M, "limits", 0, 37, 934, 3, 1, dict(cost="target_add", beta=0.5, rows=True, u_prev=True)),
]]
H_SHORT = 6  # rows up to this horizon are compared with the oracle; the long ones by bits alone


def case_id(c):
    return "-".join(str(v) for v in c[:8])


BY_ID = {case_id(c): c for c in CASES}
assert len(BY_ID) == len(CASES)
SHORT = [c for c in CASES if c.H <= H_SHORT]
LONG_CASES = [c for c in CASES if c.H > H_SHORT]
# the rows the status constructions stand on: sampled, (K, P) = (7, 3) -- candidate 2 is trajectories 6 .. 8, inside the first tile
STATUS_BASE = [c for c in SHORT if c.layout in ("mixed5", "limits") and c.mode == _S]
assert [(c.entry, c.layout, c.K, c.P) for c in STATUS_BASE] == [("mppi", "mixed5", 7, 3), ("mppi", "limits", 7, 3), ("plan", "mixed5", 7, 3),
                                                                  ("plan", "limits", 7, 3)]
K_STAR, T_STAR = 2, 1  # the candidate and the row of the NaN written into xi


def is_ext(c):
    return c.entry == "plan"


def unintegrated(cfg):
    """The components no GP writes."""
    return [s for s in range(cfg["S"]) if s not in cfg["vel"] and s not in cfg["not_vel"]]


def sigma_of(U):
    """A std per input, distinct, one of them 0 where there is more than one input."""
    s = np.linspace(0.2, 0.5, U)
    if U >= 2:
        s[U // 2] = 0.0
    return s


def zero_input(U):
    return U // 2 if U >= 2 else None


def u_max_of(U):
    return np.linspace(0.8, 1.4, U)


def cost_specs(layout, target_rows=12):
    """mppi_truth.cost_specs of the layout (generic in S and U) and two more: "wide", a saturated target cost whose active dimensions are
    the unintegrated components, the last state component and component 0, listed in descending order, with effort, rate and target on
    input U - 1 ALONE (added); "traj_rate", the trajectory cost with the same input terms."""
    c = lay.LAYOUTS[layout]
    S, U = c["S"], c["U"]
    specs = mt.cost_specs(c, target_rows)
    gen = np.random.default_rng(77 + S)
    idx = sorted(set(unintegrated(c) + [S - 1, 0]), reverse=True)
    last = dict(u_idx=[U - 1], u_ls=np.array([1.2]), u_rate=np.array([0.7]), u_target=np.array([0.1]), joint=False)
    specs["wide"] = dict(kind="target", idx=idx, target=0.2 * gen.standard_normal(len(idx)), ls=0.5 + gen.random(len(idx)), **last)
    specs["traj_rate"] = dict(specs["traj_plain"], **last)
    return specs


def case_seed(c):
    return 7000 + 100 * list(lay.LAYOUTS).index(c.layout) + (50 if is_ext(c) else 0) + c.K + c.P


@functools.lru_cache(maxsize=None)
def _operands(cid):
    return _draw(BY_ID[cid])


def _draw(c):
    cfg = lay.LAYOUTS[c.layout]
    S, U, G = cfg["S"], cfg["U"], cfg["G"]
    cap = LONG[c.entry][1] if c.H > H_SHORT else c.H  # (a long row is the prefix of its neighbour: one draw at the longer horizon, sliced)
    gen = np.random.default_rng(case_seed(c))
    x0 = 0.6 * (gen.random(S) - 0.5)
    a = 2.0 * gen.random((cap, U)) - 1.0
    xi = gen.standard_normal((cap, c.K, U))  # (candidate 0's entries are there and must not be read)
    eps = gen.standard_normal((cap - 1, c.P, G))
    rows = 0.2 + 0.5 * gen.random((cap, U))
    u_prev = u_max_of(U) * np.tanh(gen.standard_normal(U))
    w = 0.25 + gen.random(cap)
    if zero_input(U) is not None:
        rows[:, zero_input(U)] = 0.0
    H = c.H
    return dict(x0=x0, a=a[:H].copy(), xi=xi[:H].copy(), eps=eps[:H - 1].copy(), sigma=sigma_of(U), u_max=u_max_of(U),
                rows=rows[:H].copy() if c.opt.get("rows") else None, u_prev=u_prev if c.opt.get("u_prev") else None, w=w[:H].copy(),
                beta=float(c.opt.get("beta", 0.0)), squash=bool(c.opt.get("squash", True)), t0=int(c.opt.get("t0", 0)))


def operands(c):
    """What both sides are given (numpy, computed once, never written to): x0 [S] within +-0.3, a [H,U] in [-1, 1], xi [H,K,U] white
    normals, eps [H-1,P,G], sigma / u_max [U], rows [H,U] or None, u_prev [U] (post-squash) or None, time weights w [H], beta, squash, t0."""
    return _operands(case_id(c))


def std_rows(op, H, U):
    """s [H, U]: the std's rows, or sigma for every row."""
    return ct.rows(op["sigma"] if op["rows"] is None else op["rows"], H, U)


def candidate_inputs(c, op, xi=None, dt=np.float64):
    """u [H, K, U] of a case: squash(a + sigma xi), or under the extension squash(a[t] + s(t) xi_t) with the AR(1) table of
    cem_truth.colour on the white normals."""
    a = np.asarray(op["a"], dtype=dt)
    white = np.array(op["xi"] if xi is None else xi, dtype=dt)
    white[:, 0] = 0
    if not is_ext(c):
        return mt.candidate_inputs(a, np.asarray(op["sigma"], dtype=dt), white, op["u_max"], op["squash"])
    s = std_rows(op, a.shape[0], a.shape[1]).astype(dt)
    return mt.squash(a[:, None, :] + s[:, None, :] * ct.colour(white, op["beta"], dt), op["u_max"], op["squash"])


def _row0_record(spec, x, u, t0, u_prev):
    """The two-row record whose row 1 is row 0 of the plan with ``u_prev`` as the input before it (target row t0 for both rows)."""
    x2, u2 = np.stack([x[0], x[0]]), np.stack([np.broadcast_to(np.asarray(u_prev, dtype=u.dtype), u[0].shape), u[0]])
    sp = dict(spec, target=np.asarray(spec["target"])[[t0, t0]]) if spec["kind"] == "traj" else spec
    return sp, x2, u2


def point_costs(spec, x, u, t0=0, u_prev=None):
    """mppi_truth.point_costs with the rate term of row 0 taken against ``u_prev`` when one is given."""
    c = mt.point_costs(spec, x, u, t0)
    if u_prev is not None and spec.get("u_idx") is not None and spec.get("u_rate") is not None:
        c[0] = mt.point_costs(*_row0_record(spec, x, u, t0, u_prev), 0)[1]
    return c


def traj_costs(spec, x, u, w=None, t0=0, u_prev=None, dt=np.float64):
    """J [M] = sum_t w_t c_t in ascending t (mppi_truth.traj_costs with ``u_prev``)."""
    c = point_costs(spec, x.astype(dt), u.astype(dt), t0, u_prev)
    J = np.zeros(c.shape[1], dtype=dt)
    for t in range(c.shape[0]):
        J = J + (c[t] if w is None else dt(w[t]) * c[t])
    return J


def exponents(spec, x, u, t0=0, u_prev=None):
    """d [H, M] of every 1 - exp(-d) term of a saturated cost (None for the quadratic kind): the state distance, plus the input terms
    when they are joined."""
    if spec["kind"] == "target_quad":
        return None
    state_only = {k: v for k, v in spec.items() if k not in ("u_idx", "u_ls", "u_rate", "u_target", "joint")}
    base = spec if spec.get("joint") else state_only
    if spec["kind"] == "traj":  # (no quadratic trajectory kind: invert the saturation)
        return -np.log1p(-point_costs(base, x, u, t0, u_prev))
    return point_costs(dict(base, kind="target_quad"), x, u, t0, u_prev)


# ---- the truth ------------------------------------------------------------------------------------------------------------------------------
def recording_step(rec):
    """oracle_step that also records mean, scaled variance and k(z, z) of every (t, m, g)."""
    def step(fam, m, x, u, e, sample, var_scale=None):
        out = oracle_step(fam, m, x, u, e, sample, var_scale) if var_scale is not None else oracle_step(fam, m, x, u, e, sample)
        z, mus, _ = orc.one_step_gp_out(m, x, u)
        rec["mu"].append(torch.cat(mus, 1))
        rec["var"].append(out[1])
        rec["kzz"].append(torch.stack([orc.gp_diag(h, z) for h in m.hyp], 1))
        return out
    return step


def variant_step(zero_cols=(), carry=()):
    """orc.mixed_next_state assembled column by column (tests/test_layout_models_cpu.written_out's way); ``zero_cols``: those GP inputs
    read 0; ``carry``: unintegrated components that keep their value -- the deliberately wrong variants of the sensitivity check."""
    def step(fam, m, x, u, e, sample, var_scale=None):
        z = orc.gp_features(x, u, m.angle, m.not_angle).clone()
        for col in zero_cols:
            z[:, col] = 0.0
        out = [orc.gp_estimate_from_alpha(h, cc.X, z, cc.alpha, cc.Kinv) for h, cc in zip(m.hyp, m.cache)]
        dmu, dvar = torch.cat([o[0] for o in out], 1), torch.cat([o[1].reshape(-1, 1) for o in out], 1)
        delta = dmu + torch.sqrt(dvar) * e if sample else dmu
        cols = [x[:, s] if s in carry else torch.zeros_like(x[:, 0]) for s in range(x.shape[1])]
        for g, (v, q) in enumerate(zip(m.vel, m.not_vel)):
            cols[v] = x[:, v] + delta[:, g]
            if q >= 0:
                cols[q] = x[:, q] + m.Ts * x[:, v] + m.Ts / 2 * delta[:, g]
        return torch.stack(cols, 1), dvar
    return step


def rollout(c, op, m, u, sample=None, var_scale=None, step=None, x0=None):
    """(states [H, K P, S], inputs [H, K P, U]) of mppi_truth.oracle_states on the layout's integrator."""
    sample = (c.mode == _S) if sample is None else sample
    return mt.oracle_states(c.layout, m, op["x0"] if x0 is None else x0, u, c.P, op["eps"] if sample else None, sample, fam=lay.family(c.layout),
                            var_scale=var_scale, step=step)


def case_truth(c):
    """Everything a case compares against, computed once per process and left unchanged: dict(x, u, J, S, mu, var, kzz); a long row: the
    MEAN rollout of its candidates alone (x, u)."""
    return _case_truth(case_id(c))


@functools.lru_cache(maxsize=None)
def _case_truth(cid):
    c = BY_ID[cid]
    op = operands(c)
    _, m, _ = lay.oracle_pair(c.layout, c.N, c.deg)
    torch.set_num_threads(1)
    u = candidate_inputs(c, op)
    if c.H > H_SHORT:
        cap = c._replace(H=LONG[c.entry][1])
        if c.H != cap.H and case_id(cap) in BY_ID:  # (the prefix of its neighbour's rollout: the operands are the neighbour's, sliced)
            r = _case_truth(case_id(cap))
            return dict(x=r["x"][:c.H], u=r["u"][:c.H])
        x, ut = rollout(c._replace(P=1), op, m, u, sample=False)
        return dict(x=x, u=ut)
    rec = dict(mu=[], var=[], kzz=[])
    x, ut = rollout(c, op, m, u, step=recording_step(rec))
    spec = cost_specs(c.layout)[c.opt["cost"]]
    J = traj_costs(spec, x, ut, None, op["t0"], op["u_prev"])
    n = lambda q: torch.stack(q).numpy()  # noqa: E731
    return dict(x=x, u=ut, J=J, S=ct.cand_costs(J, c.K, c.P), mu=n(rec["mu"]), var=n(rec["var"]), kzz=n(rec["kzz"]))


# ---- the status constructions ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Con:
    """A: var_scale[g*] = 0;  B: Kinv of g* times a factor that turns every trajectory's variance negative at step 0;  X: a NaN in
    xi[T_STAR, K_STAR, 0];  C: a NaN in one component of x0 (component 0, or S - 1 with ``last``).  ``mean``: the operands in the mean form."""
    kind: str
    last: bool = False
    mean: bool = False
    mid: bool = False  # g* = 1: on mixed5 the GP without a position (its one thread is a velocity thread)

    @property
    def id(self):
        return ("mean-" if self.mean else "") + self.kind + ("-mid" if self.mid else "-last" if self.last else "-first")


CONS = [Con("A"), Con("A", True), Con("A", mid=True), Con("A", False, True), Con("A", True, True), Con("B"), Con("B", True), Con("B", True, True), Con("X"), Con("C"), Con("C", True)]
B_BEYOND = 0.5  # construction B aims at var = -0.5 k_zz for the trajectory nearest the sign change: 500 margins


def ratios_step0(c, op, m, g):
    """r_k = k^T Kinv k / k_zz of GP g at step 0 for every candidate (the trajectories of a candidate share x0 and u_0)."""
    u0 = torch.as_tensor(candidate_inputs(c, op)[0])
    x0 = torch.as_tensor(op["x0"]).reshape(1, -1).repeat(u0.shape[0], 1)
    with torch.no_grad():
        z = orc.gp_features(x0, u0, m.angle, m.not_angle)
        h, q = m.hyp[g], m.cache[g]
        Ks = orc.gp_cov(h, z, q.X)
        return (((Ks @ q.Kinv) * Ks).sum(1) / orc.gp_diag(h, z)).numpy()


def status_operands(c, con):
    """dict(gstar, var_scale, factor, x0, xi, sample): what the construction changes of the case's operands (None: unchanged)."""
    cfg, op = lay.LAYOUTS[c.layout], operands(c)
    _, m, _ = lay.oracle_pair(c.layout, c.N, c.deg)
    g = 1 if con.mid else (cfg["G"] - 1 if con.last else 0)
    out = dict(gstar=g, var_scale=None, factor=None, x0=op["x0"], xi=op["xi"], sample=not con.mean)
    if con.kind == "A":
        out["var_scale"] = tuple(0.0 if i == g else 1.0 for i in range(cfg["G"]))
    elif con.kind == "B":
        out["factor"] = float((1.0 + B_BEYOND) / ratios_step0(c, op, m, g).min())
    elif con.kind == "X":
        xi = op["xi"].copy()
        xi[T_STAR, K_STAR, 0] = np.nan
        out["xi"] = xi
    elif con.kind == "C":
        x0 = op["x0"].copy()
        x0[cfg["S"] - 1 if con.last else 0] = np.nan
        out["x0"] = x0
    return out


def status_model(c, so):
    """The case's oracle model on the construction's Kinv."""
    _, m, _ = lay.oracle_pair(c.layout, c.N, c.deg)
    if so["factor"] is None:
        return m
    cache = [dataclasses.replace(q, Kinv=q.Kinv * so["factor"]) if i == so["gstar"] else q for i, q in enumerate(m.cache)]
    return dataclasses.replace(m, cache=cache)


def status_truth(c, con):
    return _status_truth(case_id(c), con)


@functools.lru_cache(maxsize=None)
def _status_truth(cid, con):
    """The oracle's answer: dict(word, x, u, J, S, mu, var, kzz), the word by status_models.word_of (its module docstring's rule)."""
    c = BY_ID[cid]
    op, so = operands(c), status_operands(c, con)
    m = status_model(c, so)
    torch.set_num_threads(1)
    rec = dict(mu=[], var=[], kzz=[])
    with np.errstate(invalid="ignore"):
        u = candidate_inputs(c, op, so["xi"])
        x, ut = rollout(c, op, m, u, sample=so["sample"], var_scale=so["var_scale"], step=recording_step(rec), x0=so["x0"])
        J = traj_costs(cost_specs(c.layout)[c.opt["cost"]], x, ut, None, op["t0"], op["u_prev"])
    n = lambda q: torch.stack(q).numpy()  # noqa: E731
    tr = sm.Truth(0, x, ut, None, n(rec["mu"]), n(rec["var"]), n(rec["kzz"]), None, so["sample"])
    return dict(word=sm.word_of(tr), x=x, u=ut, J=J, S=ct.cand_costs(J, c.K, c.P), mu=tr.mu, var=tr.var, kzz=tr.kzz)


def expected_word(con):
    if con.mean:
        return 0
    return {"A": sm.STATUS_NONPOS_VAR, "B": sm.STATUS_NONPOS_VAR | sm.STATUS_NAN, "X": sm.STATUS_NAN, "C": sm.STATUS_NAN}[con.kind]
