"""Rollouts that MUST raise a status flag, for tests/test_gpu_status_word.py: constructions on top of the cases of tests/width_models.py, the truth
of each from the oracle (oracle/mcpilco_oracle.py, fp64 on the CPU) and the table of forward forms they are sent through.  CPU side only imports
torch, numpy and the oracle; ``packed`` imports the GPU helpers when called, ``plan`` the library's host-side plan query.

Truth.  The oracle's rollout (``orc.apply_policy`` / ``orc.apply_policy_pms``) runs with a ``step=`` wrapper around ``orc.mixed_next_state`` that
records the mean and the SCALED variance of every (t, m, g).  The oracle does not validate the scale of its sample: sqrt of a negative variance is
NaN there as in the kernels.  The expected word is

  MCP_STATUS_NONPOS_VAR  iff the rollout samples (particle_pred) and some recorded variance is finite and <= 0
  MCP_STATUS_NAN         iff any state, input, measurement, mean or variance is not finite
  never MCP_STATUS_SYNC or MCP_STATUS_NOT_SPD

Constructions (``Con``; g* is GP 0 or GP G - 1), the packed side gets exactly the operands the oracle gets:

  A  var_scale[g*] = 0: the variance of g* is (kzz - k^T Kinv k) * 0 = 0 in every form, at every degree, in any summation order; delta = mu.
     NONPOS_VAR alone; every state and input finite.
  B  Kinv of g* times a factor c > 1.  With r_m = (k^T Kinv k / kzz) of particle m at step 0 (the oracle's values), c = 1 / sqrt(r_a r_b) for the
     two neighbours a, b of the widest ratio gap of the sorted r that leaves at least two particles on either side: var = kzz (1 - c r) < 0 for the
     particles above the gap, > 0 below.  The particles (x0 rows with their eps, mask and position-noise rows) are then ordered: particle 0 the
     healthy one nearest the gap, particle 1 a bad one (interior to the first cluster of 2 / 4 / 16), particle M - 2 healthy, particle M - 1 the
     bad one nearest the gap (the particle whose clones fill a ragged last tile).  NONPOS_VAR | NAN.
  C  one component of x0 of one particle NaN (particle 1, component 0; particle M - 1, component S - 1), operands untouched.  NAN alone: a NaN
     variance is not a finite variance <= 0.
  D  the operands of A and of B with particle_pred False.  0: the variance is never sampled; states and inputs are the oracle's mean rollout.

Conditions (asserted by ``check``; tests/test_status_models_cpu.py runs it over the whole table without a GPU): in B every finite variance of g* at
every step is at least 1e-3 kzz away from 0 and every finite variance of the other GPs is > 1e-3 kzz; in A the other GPs' variances are > 1e-3 kzz;
B has a healthy and a bad particle in its first cluster of two; the word is the one named above.  1e-3 kzz is six orders above the kernels' 1e-9
parity with the oracle: no summation order moves a sign.  In D nothing is sampled, so no sign has a consequence: there the margin is held at step 0
only (B's own choice of c), not along the mean trajectory.  Cases run at their own T but for the overrides in ``T_OVERRIDE`` (none changes a seed).

The row split (``u5_g5_d16_n128``: Npad = 128, four 32-row blocks).  The part that finishes a GP owns the LAST blocks of the rows of Kinv, blocks
[((RS - 1) nblk) / RS, nblk): rows 64 .. 127 with two and with three parts; its own share of k^T Kinv k is sum over those rows i of k_i (Kinv k)_i, the
senders' shares arrive through the exchange.  ``Truth.var_fin`` holds kzz - (own share) for g*: in B it is > 0 for every bad particle, so the
variance is negative only once the senders' sums are added.  The own share of a particle is anything from a fifth to four fifths of the whole, so
on this shape c comes from the widest gap that still leaves c x (own share) < 0.99 kzz for every bad particle (for g* = 0 that is a gap with three
bad particles, not the widest of all: the widest leaves particles 40 % past the sign change, whose own rows alone are already negative)."""
import ctypes as C
import dataclasses
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

import width_models as wm
from helpers import T as TT
from oracle import mcpilco_oracle as orc

STATUS_NAN, STATUS_NONPOS_VAR = 1, 2  # include/mcpilco_hip.h (tests/test_abi_cpu.py holds hipabi's copies against the header)
MARGIN = 1e-3  # of kzz: the sign margin of every finite variance
CUS = 256  # compute units of an MI355X: what the CPU-side plan queries assume; the GPU test asks the device

# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
_ND6, _U5 = wm.BY_NAME["narrow_disjoint_d6"], wm.BY_NAME["u5_g5_d16"]
EXTRA = [
    dataclasses.replace(_ND6, name="narrow_disjoint_d6_pms", pms=((0, 2), (1, 3)), pins="the narrow twin with the measurement model: lean <.., PMS>"),
    dataclasses.replace(_ND6, name="narrow_disjoint_d6_deg1", deg=1, pins="lean kernel, degree 1"),
    dataclasses.replace(_ND6, name="narrow_disjoint_d6_deg2", deg=2, pins="lean kernel, degree 2"),
    dataclasses.replace(_U5, name="u5_g5_d16_n128", N=(128,) * 5, T=3, deg=1, pins="u5_g5_d16's widths at N = Npad = 128: the row-split cluster"),
]
BY_NAME = dict(wm.BY_NAME, **{c.name: c for c in EXTRA})
# case name -> T used here instead of the case's own (a condition of ``check`` fails at the case's T); the seed stays the case's
T_OVERRIDE = {"delta_d11_u3": 2}  # (its own T = 3: at M = 33, B on the last GP, a step-1 variance of a healthy particle is 1.8e-4 kzz)


def case(name):
    c = BY_NAME[name]
    return dataclasses.replace(c, T=T_OVERRIDE[name]) if name in T_OVERRIDE else c


# ---- constructions -------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Con:
    kind: str  # "A" | "B" | "C"
    last: bool  # g* = G - 1 (A, B); the NaN in particle M - 1 (C)
    mean: bool = False  # D: particle_pred False

    @property
    def id(self):
        return ("D" if self.mean else "") + self.kind + ("-last" if self.last else "-first")

    def gstar(self, c):
        return c.G - 1 if self.last else 0


A0, AL, B0, BL, C0, CL = Con("A", False), Con("A", True), Con("B", False), Con("B", True), Con("C", False), Con("C", True)
DA0, DAL, DB0, DBL = Con("A", False, True), Con("A", True, True), Con("B", False, True), Con("B", True, True)
CONS = [A0, AL, B0, BL, C0, CL, DAL, DB0, DBL]
CONS_NO_GRAD = [A0, AL, B0, BL]  # repeated under torch.no_grad() (the states-only call) on one form per kernel family
WORD = {"A": STATUS_NONPOS_VAR, "B": STATUS_NONPOS_VAR | STATUS_NAN, "C": STATUS_NAN}


def expected_word(con):
    return 0 if con.mean else WORD[con.kind]


def fin_rows(c, g, parts=2):
    """Rows of Kinv of GP g that the finishing part of the row-split cluster owns (None: no row split at this Npad)."""
    npad = (c.N[g] + 15) // 16 * 16
    if npad < 128:
        return None
    nblk = (npad + 31) // 32
    return list(range(32 * (((parts - 1) * nblk) // parts), c.N[g]))


def _step0(c, M, rows=None):
    """r_m = k^T Kinv k / kzz of every particle and GP at step 0 of the unmodified case [M, G], and the share of it that the rows ``rows`` of Kinv
    carry (None without ``rows``)."""
    om, pp = wm.model(c)["om"], wm.oracle_policy(c)
    x0, _, masks, _ = wm.noise(c, M)
    with torch.no_grad():
        u0 = orc.policy_forward(pp, x0, 0, masks[0], wm.P_DROP)
        z = orc.gp_features(x0, u0, om.angle, om.not_angle)
        out, own = [], []
        for h, q in zip(om.hyp, om.cache):
            kzz = orc.gp_diag(h, z)
            Ks = orc.gp_cov(h, z, q.X)
            w = Ks @ q.Kinv
            out.append((w * Ks).sum(1) / kzz)
            if rows is not None:
                own.append((w[:, rows] * Ks[:, rows]).sum(1) / kzz)
    return torch.stack(out, 1), (torch.stack(own, 1) if rows is not None else None)


@functools.lru_cache(maxsize=None)
def operands(c, con, M):
    """What both sides are given: dict(Kinv [G] tensors, var_scale tuple or None, x0, eps, masks, pos_noise, sample, factor, order, bad)."""
    x0, eps, masks, pos_noise = wm.noise(c, M)
    om = wm.model(c)["om"]
    kinv = [q.Kinv for q in om.cache]
    vs, factor, order, bad = c.var_scale, None, list(range(M)), []
    g = con.gstar(c)
    if con.kind == "A":
        vs = tuple(0.0 if i == g else (1.0 if c.var_scale is None else c.var_scale[i]) for i in range(c.G))
    elif con.kind == "B":
        r, own = _step0(c, M, fin_rows(c, g))
        r, own = r[:, g], (None if own is None else own[:, g])
        rs, idx = torch.sort(r, descending=True)
        gaps = rs[1:M - 2] / rs[2:M - 1]  # gaps[j]: j + 2 particles above it, M - 2 - j >= 2 below
        for j in torch.argsort(gaps, descending=True):  # the widest gap (on a row-split shape: the widest that meets the condition on the own rows)
            nbad = int(j) + 2
            factor = float(1.0 / torch.sqrt(rs[nbad - 1] * rs[nbad]))
            if own is None or bool((factor * own[idx[:nbad]] < 1.0 - 10 * MARGIN).all()):
                break
        else:
            raise AssertionError("%s: no gap leaves the finishing part's own share below kzz" % c.name)
        bad_ids, ok_ids = [int(i) for i in idx[:nbad]], [int(i) for i in idx[nbad:]]
        first, second, before_last, last = ok_ids[0], bad_ids[-2], ok_ids[1], bad_ids[-1]
        rest = [m for m in range(M) if m not in (first, second, before_last, last)]
        order = [first, second] + rest + [before_last, last]
        bad = [i for i, m in enumerate(order) if m in bad_ids]
        kinv = [q * factor if i == g else q for i, q in enumerate(kinv)]
        x0, eps, masks, pos_noise = x0[order], eps[:, order], masks[:, order], pos_noise[:, order]
    elif con.kind == "C":
        x0 = x0.clone()
        if con.last:
            x0[M - 1, c.S - 1] = float("nan")
        else:
            x0[1, 0] = float("nan")
    return dict(Kinv=kinv, var_scale=vs, x0=x0.contiguous(), eps=eps.contiguous(), masks=masks.contiguous(), pos_noise=pos_noise.contiguous(),
                sample=not con.mean, factor=factor, order=order, bad=bad)


def oracle_model(c, op, permute_gp=None):
    """The case's oracle model on the operands' Kinv; ``permute_gp``: the training rows of that GP in another order (the same GP: only the summation
    order of its posterior changes -- the reference measured against itself, as DESIGN section 2 does)."""
    om = wm.model(c)["om"]
    cache = [dataclasses.replace(q, Kinv=k) for q, k in zip(om.cache, op["Kinv"])]
    if permute_gp is not None:
        q = cache[permute_gp]
        p = torch.from_numpy(np.random.RandomState(7).permutation(q.X.shape[0]))
        cache[permute_gp] = dataclasses.replace(q, X=q.X[p], alpha=q.alpha[p], Kinv=q.Kinv[p][:, p], mX=q.mX[p])
    return orc.SpeedModel(om.hyp, cache, om.Ts, om.angle, om.not_angle, om.vel, om.not_vel)


def measured(c, states, pos_noise):
    """What the policy is fed under the measurement model, from the true states (orc.apply_policy_pms, restated: it does not return them)."""
    b, a = orc.butter1(wm.FC)
    pos, vel = list(c.pms[0]), list(c.pms[1])
    std = TT(wm.policy(c)["std_pos"])
    out = [states[0]]
    noisy_prev, meas_prev = states[0].clone(), states[0].clone()
    for t in range(1, states.shape[0]):
        noisy = states[t].clone()
        noisy[:, pos] = noisy[:, pos] + std * pos_noise[t - 1]
        noisy[:, vel] = (noisy[:, pos] - noisy_prev[:, pos]) / wm.TS
        meas = noisy.clone()
        meas[:, vel] = (b[0] * noisy[:, vel] + b[1] * noisy_prev[:, vel] - a[1] * meas_prev[:, vel]) / a[0]
        out.append(meas)
        noisy_prev, meas_prev = noisy, meas
    return torch.stack(out)


@dataclass
class Truth:
    word: int
    states: np.ndarray  # [T, M, S]
    inputs: np.ndarray  # [T, M, U]
    meas: Optional[np.ndarray]  # [T, M, S] under the measurement model
    mu: np.ndarray  # [T - 1, M, G]
    var: np.ndarray  # [T - 1, M, G] scaled
    kzz: np.ndarray  # [T - 1, M, G]
    var_fin: Optional[np.ndarray]  # [T - 1, M]: kzz - the finishing row part's own share of k^T Kinv k, GP g* (row-split shapes only)
    sample: bool


def word_of(tr, gps=None, particles=None, nan_is_nonpos=False):
    """The status word from the recorded quantities.  The keyword arguments are the WRONG rules the sensitivity tests apply: the flag taken from
    some GPs only, some particles left out, NaN variances counted as non-positive."""
    G, M = tr.var.shape[2], tr.var.shape[1]
    gs = list(range(G)) if gps is None else list(gps)
    ms = list(range(M)) if particles is None else list(particles)
    var, mu = tr.var[:, ms][:, :, gs], tr.mu[:, ms][:, :, gs]
    w = 0
    with np.errstate(invalid="ignore"):
        nonpos = (var <= 0.0) | (np.isnan(var) if nan_is_nonpos else False)
    if tr.sample and bool(nonpos.any()):
        w |= STATUS_NONPOS_VAR
    arrays = [tr.states[:, ms], tr.inputs[:, ms], mu, var] + ([tr.meas[:, ms]] if tr.meas is not None else [])
    if any(not bool(np.isfinite(q).all()) for q in arrays):
        w |= STATUS_NAN
    return w


def _rollout(c, op, om, rows=None, gstar=0):
    rec = dict(mu=[], var=[], kzz=[], fin=[])

    def step(m, x, u, e, _sample):  # (apply_policy_pms always asks for a sample: the construction decides)
        nxt, dmu, dvar = orc.mixed_next_state(m, x, u, e, op["sample"], op["var_scale"])
        z = orc.gp_features(x, u, m.angle, m.not_angle)
        rec["mu"].append(dmu)
        rec["var"].append(dvar)
        rec["kzz"].append(torch.stack([orc.gp_diag(h, z) for h in m.hyp], 1))
        if rows is not None:
            h, q = m.hyp[gstar], m.cache[gstar]
            Ks = orc.gp_cov(h, z, q.X)
            rec["fin"].append(orc.gp_diag(h, z) - ((Ks @ q.Kinv)[:, rows] * Ks[:, rows]).sum(1))
        return nxt, dmu, dvar

    pp = wm.oracle_policy(c)
    with torch.no_grad():
        if c.pms is not None:
            st, inp = orc.apply_policy_pms(om, pp, op["x0"], c.T, list(c.pms[0]), list(c.pms[1]), TT(wm.policy(c)["std_pos"]), wm.FC, wm.P_DROP, op["eps"],
                                           op["masks"], op["pos_noise"], step=step)
        else:
            st, inp = orc.apply_policy(om, pp, op["x0"], c.T, wm.P_DROP, op["eps"], op["masks"], step=step)
        meas = measured(c, st, op["pos_noise"]) if c.pms is not None else None
    n = lambda q: torch.stack(q).numpy()  # noqa: E731
    tr = Truth(0, st.numpy(), inp.numpy(), None if meas is None else meas.numpy(), n(rec["mu"]), n(rec["var"]), n(rec["kzz"]),
               n(rec["fin"]) if rows is not None else None, op["sample"])
    tr.word = word_of(tr)
    return tr


@functools.lru_cache(maxsize=None)
def truth(c, con, M):
    """The oracle's answer for (case, construction, M): computed once, shared, never written to."""
    op = operands(c, con, M)
    g = con.gstar(c)
    return _rollout(c, op, oracle_model(c, op), fin_rows(c, g), g)


def reorder_spread(c, con, M):
    """max |difference| over the finite states and inputs between the oracle and the oracle with the training rows of g* permuted: what the summation
    order alone moves in this construction (the measure for a bound on B, should the project's 1e-9 not hold there)."""
    op = operands(c, con, M)
    a, b = truth(c, con, M), _rollout(c, op, oracle_model(c, op, permute_gp=con.gstar(c)))
    d = 0.0
    for p, q in ((a.states, b.states), (a.inputs, b.inputs)):
        assert np.array_equal(np.isfinite(p), np.isfinite(q))
        f = np.isfinite(p)
        d = max(d, float(np.abs(p[f] - q[f]).max()))
    return d


def check(c, con, M):
    """The conditions of the module docstring on one (case, construction, M).  Returns the smallest |var| / kzz met on g* (finite variances)."""
    tr, op, g = truth(c, con, M), operands(c, con, M), con.gstar(c)
    assert tr.word == expected_word(con), (c.name, con.id, M, tr.word)
    fin = np.isfinite(tr.var)
    rel = np.where(fin, tr.var, 1.0) / np.where(fin, tr.kzz, 1.0)  # (scaled variance over kzz; 1 where the variance is NaN)
    others = [i for i in range(c.G) if i != g]
    smallest = float("inf")
    if con.kind in ("A", "B"):
        assert bool((rel[:, :, others] > MARGIN).all()), (c.name, con.id, M, "another GP's variance within the margin", float(rel[:, :, others].min()))
    if con.kind == "A":
        assert bool((tr.var[:, :, g] == 0.0).all())
        assert np.isfinite(tr.states).all() and np.isfinite(tr.inputs).all()
        smallest = 0.0
    if con.kind == "B":
        smallest = float(np.abs(rel[:, :, g] if tr.sample else rel[0, :, g]).min())  # (D: nothing is sampled, no sign matters; step 0 is B's own)
        assert smallest >= MARGIN, (c.name, con.id, M, "a variance of g* within the margin", smallest)
        v0 = tr.var[0, :, g]
        bad = sorted(int(m) for m in np.nonzero(v0 < 0.0)[0])
        assert bad == op["bad"] and 2 <= len(bad) <= M - 2
        assert 0 not in bad and 1 in bad and M - 1 in bad and M - 2 not in bad  # (a healthy and a bad particle in the first cluster of two; particle M - 1 bad)
        if tr.sample:  # (the step after a negative variance is NaN for exactly the bad particles)
            assert all(np.isfinite(tr.states[1, m]).all() == (m not in bad) for m in range(M))
        else:
            assert np.isfinite(tr.states).all() and np.isfinite(tr.inputs).all()
        if tr.var_fin is not None:  # the row split: negative only with the senders' shares
            neg = fin[:, :, g] & (tr.var[:, :, g] < 0.0)
            assert bool(neg.any()) and bool((tr.var_fin[neg] > MARGIN * tr.kzz[:, :, g][neg]).all()), (c.name, con.id, M, float(tr.var_fin[neg].min()))
    if con.kind == "C":
        with np.errstate(invalid="ignore"):
            assert not bool((tr.var <= 0.0).any())
        m = M - 1 if con.last else 1
        assert not np.isfinite(tr.states[0, m]).all() and np.isfinite(np.delete(tr.states, m, axis=1)).all()
    return smallest


# ---- the packed side -----------------------------------------------------------------------------------------------------------------------------
def packed(c, con, M):
    """(model, policy, noise, meas, x0) on the GPU on the operands of ``operands(c, con, M)``: wm.packed with the construction's Kinv, var_scale, x0
    and noise rows."""
    return packed_op(c, operands(c, con, M))


def packed_op(c, op, philox=None):
    """``packed`` on any operand dict of the layout of ``operands``.  ``philox``: a NoiseSpec without buffers that takes the place of the
    operands' eps, masks and position noise (the in-kernel generator draws all three)."""
    from gpu_helpers import G as GG
    from gpu_helpers import dev, spec_from
    from mc_pilco_amd import ops

    md, pi = wm.model(c), wm.policy(c)
    pol = ops.PackedPolicy(c.kind, c.S, torch.log(GG(pi["ls"])).reshape(1, -1).requires_grad_(True), GG(pi["centers"]).requires_grad_(True),
                           GG(pi["weight"]).requires_grad_(True), c.u_max if np.isscalar(c.u_max) else list(c.u_max), True, angle=list(c.pol_angle),
                           non_angle=list(c.pol_non_angle), target_traj=pi["traj"] if c.kind == "traj" else None,
                           bias=None if pi["bias"] is None else GG(pi["bias"]).requires_grad_(True))
    gps = [ops.PackedGP(spec_from(q["ls"], wm.SIGMA_N, 1.0, q["poly"]), GG(q["cache"].X.numpy()), GG(q["cache"].alpha.numpy()), GG(k.numpy()))
           for q, k in zip(md["gps"], op["Kinv"])]
    pm = ops.PackedModel(gps, c.S, c.U, wm.TS, list(c.angle), list(c.not_angle), list(c.vel), list(c.not_vel), var_scale=op["var_scale"])
    nz = philox if philox is not None else ops.NoiseSpec(eps=GG(op["eps"].numpy()), masks=op["masks"].to(torch.uint8).to(dev()).contiguous())
    meas = None
    if c.pms is not None:
        b, a = orc.butter1(wm.FC)
        meas = ops.MeasSpec(pos=list(c.pms[0]), vel=list(c.pms[1]), std_pos=list(pi["std_pos"]), b=b, a=a,
                            pos_noise=None if philox is not None else GG(op["pos_noise"].numpy()))
    return pm, pol, nz, meas, GG(op["x0"].numpy())


# ---- the forms -----------------------------------------------------------------------------------------------------------------------------------
FWD_SMALL_SHARDED, FWD_LEAN, FWD_TILE_SHARDED, FWD_TILE, FWD_SMALL = 1, 2, 3, 4, 5  # mcp_fwd_plan.family (hipabi's copies)


@dataclass(frozen=True)
class Form:
    """One forced launch form on one case.  ``code``: gpu_helpers.forced_variant; the hooks as the mcp_debug_set_* methods take them (None: not
    set); ``want``: what the plan of the call must say -- (family, particles, GP-sharded, row parts, policy split, LDS staging, GPs per pass), None
    in a slot: not pinned (automatic dispatch pins nothing: the report must equal the plan)."""
    label: str
    case: str
    M: int
    code: int
    want: Optional[Tuple] = None
    policy_split: Optional[int] = None
    row_split: Optional[int] = None
    cluster_map: Optional[int] = None
    xlds: Optional[int] = None
    gb: Optional[int] = None
    no_grad: bool = False

    @property
    def id(self):
        return "%s-%s-f%d-M%d%s" % (self.label, self.case, self.code, self.M, "-nograd" if self.no_grad else "")

    def request(self):
        """The dispatch request of this form as a hipabi.Dispatch (what forced_variant and the hooks leave in hipabi.DISPATCH)."""
        from mc_pilco_amd import hipabi

        d = hipabi.Dispatch()
        d.fwd_particles = self.code % 100
        d.gp_sharding = 2 if self.code >= 100 else (0 if self.code == 0 else 1)
        d.fwd_lean = 0 if (self.code >= 200 or self.code == 0) else 1
        d.policy_split = {None: 0, 0: 1, 1: 2}[self.policy_split]
        d.row_split = {None: 0, 0: 1, 2: 2, 3: 3}[self.row_split]
        d.cluster_map = {None: 0, 0: 1, 1: 2}[self.cluster_map]
        d.fwd_no_xlds = 1 if self.xlds == 0 else 0
        d.fwd_gb = self.gb or 0
        return d


def _forms():
    S, L, TS_, TL, SM = FWD_SMALL_SHARDED, FWD_LEAN, FWD_TILE_SHARDED, FWD_TILE, FWD_SMALL
    f = []
    # lean kernel: 1 / 2 / 4 particles, with and without the measurement model, degree 1 and 2
    for name in ("narrow_disjoint_d6", "narrow_disjoint_d6_pms"):
        f += [Form("lean", name, 5, 200 + p, (L, p, 1, 0, 0, 1, 1)) for p in (1, 2, 4)]
    for name in ("narrow_disjoint_d6_deg1", "narrow_disjoint_d6_deg2"):
        f += [Form("lean", name, 5, 200 + p, (L, p, 1, 0, 0, 1, 1)) for p in (1, 4)]
    # small-tile kernel, unsharded and GP-sharded
    for name in ("d15_p10_g3", "u5_g5_d16", "d8_u3_pms"):
        G = BY_NAME[name].G
        f += [Form("small", name, 5, p, (SM, p, 0, 0, 0, 1, G)) for p in (1, 2, 4)]
        f += [Form("small-sharded", name, 5, 100 + p, (S, p, 1, 0, 0, 1, 1)) for p in (1, 2, 4)]
    # ... without LDS staging (5 + 3 GPs per pass are what fits then) and with at most 3 GPs per pass requested (2 fit beside the staged operands at
    # four particles, 3 unstaged at two): g* = G - 1 = 7 lands in the last pass
    f += [Form("small-noxlds", "d25_s16_g8", 5, 4, (SM, 4, 0, 0, 0, 0, 5), xlds=0), Form("small-gb3", "d25_s16_g8", 5, 4, (SM, 4, 0, 0, 0, 1, 2), gb=3),
          Form("small-noxlds-gb3", "d25_s16_g8", 5, 2, (SM, 2, 0, 0, 0, 0, 3), xlds=0, gb=3)]
    # tile kernel, classes 0 / 1 / 2
    for name in ("narrow_traj_d7", "d15_p10_g3", "d25_s16_g8"):
        f += [Form("tile", name, M, 16, (TL, 16, 0, 0, 0, None, None)) for M in (17, 33)]
    # ... GP-sharded; the policy split; the row split in two and three parts under both deals
    for name in ("narrow_disjoint_d6", "u5_g5_d16"):
        f += [Form("tile-sharded", name, M, 116, (TS_, 16, 1, 0, 0, None, None)) for M in (17, 33)]
    f += [Form("tile-sharded-psplit", "d15_p10_g3", 17, 116, (TS_, 16, 1, 0, 1, None, None), policy_split=1),
          Form("tile-sharded-nopsplit", "d15_p10_g3", 17, 116, (TS_, 16, 1, 0, 0, None, None), policy_split=0)]
    f += [Form("tile-rowsplit%d-deal%d" % (rs, cm), "u5_g5_d16_n128", 17, 116, (TS_, 16, 1, rs, 0, None, None), row_split=rs, cluster_map=cm)
          for rs in (2, 3) for cm in (0, 1)]
    f += [Form("tile-norowsplit", "u5_g5_d16_n128", 17, 116, (TS_, 16, 1, 0, 0, None, None), row_split=0)]
    # D = 32 (no tile kernel: a forced 16 runs four particles per workgroup), the delta model, var_scale != 1
    f += [Form("d32-fallback", "d32_u8_pms", 17, 16, (SM, 4, 0, 0, 0, None, None)), Form("d32-fallback", "d32_u8_pms", 17, 116, (SM, 4, 0, 0, 0, None, None)),
          Form("small", "d32_u8_pms", 5, 4, (SM, 4, 0, 0, 0, None, None))]
    for name in ("delta_d11_u3", "speed_mixed_p9"):
        f += [Form("small", name, 5, 4, (SM, 4, 0, 0, 0, None, None)), Form("small-sharded", name, 5, 104, (S, 4, 1, 0, 0, 1, 1)),
              Form("tile", name, 17, 16, (TL, 16, 0, 0, 0, None, None)), Form("tile-sharded", name, 33, 116, (TS_, 16, 1, 0, None, None, None))]
    # automatic dispatch: every case above
    for name in sorted({q.case for q in f}):
        f += [Form("auto", name, M, 0) for M in (5, 17)]
    # the states-only call (no Jacobian record): one form per kernel family
    f += [Form("lean", "narrow_disjoint_d6", 5, 204, (L, 4, 1, 0, 0, 1, 1), no_grad=True), Form("small", "d15_p10_g3", 5, 4, (SM, 4, 0, 0, 0, 1, 3), no_grad=True),
          Form("small-sharded", "u5_g5_d16", 5, 104, (S, 4, 1, 0, 0, 1, 1), no_grad=True), Form("tile", "d25_s16_g8", 17, 16, (TL, 16, 0, 0, 0, None, None), no_grad=True),
          Form("tile-rowsplit3-deal1", "u5_g5_d16_n128", 17, 116, (TS_, 16, 1, 3, 0, None, None), row_split=3, cluster_map=1, no_grad=True)]
    return f


FORMS = _forms()
TRUTH_KEYS = sorted({(q.case, q.M) for q in FORMS})


def plan_words(fp):
    return (fp.family, fp.particles, 1 if fp.ran_gp_sharded else 0, fp.ran_row_split, fp.policy_split, fp.xlds, fp.gb)


def matches(want, got):
    return all(w is None or w == g for w, g in zip(want, got))


def plan(c, M, request, sample=True, cus=CUS):
    """mcp_rollout_fwd_plan for the case's descriptors (scalars only, dummy pointers: the query never follows them -- the way of
    tests/test_dispatch_plan_cpu.py) on a first call with a workspace of the size the library asks for.  Runs without a GPU."""
    from mc_pilco_amd import hipabi
    from test_dispatch_plan_cpu import make_model, make_policy

    s = dict(S=c.S, U=c.U, G=c.G, D=c.D, angle=list(c.angle), not_angle=list(c.not_angle), vel=list(c.vel), not_vel=list(c.not_vel), N=list(c.N),
             Npad=[(n + 15) // 16 * 16 for n in c.N], poly_deg=[c.deg] * c.G)
    ps = dict(kind={"plain": 0, "angles": 1, "traj": 2}[c.kind], S=c.S, P=c.P, B=c.B, U=c.U, angle=list(c.pol_angle), non_angle=list(c.pol_non_angle),
              traj_len=c.T if c.kind == "traj" else 0, p_drop=wm.P_DROP,
              meas=dict(n=0 if c.pms is None else len(c.pms[0]), pos=list(c.pms[0]) if c.pms else [], vel=list(c.pms[1]) if c.pms else []), bias=c.bias)
    m, p = make_model(s), make_policy(ps)
    L = hipabi.lib()
    size = L.mcp_rollout_workspace_bytes(C.byref(m), C.byref(p), M, c.T)
    fp = hipabi.FwdPlan()
    rc = L.mcp_rollout_fwd_plan(C.byref(m), C.byref(p), M, c.T, int(bool(sample)), size, cus, C.byref(request), C.byref(fp))
    assert rc == 0, (c.name, M, rc)
    return fp
