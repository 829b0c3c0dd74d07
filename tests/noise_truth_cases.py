"""The cases of tests/test_gpu_noise_truth.py, CPU side: which (seed, call, particle offset) every Philox launch of that module uses, the tables
tests/noise_truth.py gives for it in the oracle's buffer layouts, and the oracle's rollout fed those tables.  Imports torch, numpy and the oracle
only; tests/test_noise_truth_cpu.py checks the conditions of every case here and that every wrong generator of ``noise_truth.MUTANTS`` changes
the tables (``specs()``: one entry per table set a GPU test compares against).

Conditions (``check``, as status_models.check words them): the truth-fed oracle's status word is 0, every scaled variance is > 1e-3 kzz and every
state, input and measured state is finite.  A (seed, call) that does not meet them is replaced in ``SEED_CALL``; no case is dropped."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

import noise_truth as nt
import status_models as sm
import width_models as wm

DT = torch.float64
SEED_HI = 0xA5A5A5A5  # every seed has a non-zero high word: the key's second word is in play in every launch
SEED_CALL = {}  # (case name, M) -> (seed, call) where the rule of ``seed_call`` does not meet the conditions


def seed_call(c, M):
    return SEED_CALL.get((c.name, M), ((SEED_HI << 32) | c.seed, 1 + M))


@dataclass(frozen=True)
class Spec:
    """One set of tables: what a launch with NoiseSpec(seed, call, particle_offset=offset, call_dev -> dev) of M particles over T rows draws."""
    name: str
    seed: int
    call: int
    T: int
    M: int
    G: int = 0  # eps [T - 1, M, G]
    B: int = 0  # masks [T, M, B]
    n: int = 0  # pos_noise [T - 1, M, n]
    p: float = wm.P_DROP
    offset: int = 0
    dev: int = 0  # the device word added to ``call``
    t0: int = 0  # eps rows start at this step (a single mcp_model_step at index t0 is T = 2)

    def tables(self, mutant=None, hp=False):
        """dict(eps, masks, pos) of numpy arrays; absent tables are left out.  ``hp``: eps at the 64-bit significand."""
        call = nt.total_call(self.call, self.dev, mutant)
        out = {}
        if self.G:
            out["eps"] = nt.eps_table(self.seed, call, self.T, self.M, self.G, self.offset, mutant, hp=hp, t0=self.t0)
        if self.B:
            out["masks"] = nt.mask_table(self.seed, call, self.T, self.M, self.B, self.p, self.offset, mutant)
        if self.n:
            out["pos"] = nt.pos_table(self.seed, call, self.T, self.M, self.n, self.offset, mutant)
        return out


def spec_of(c, M, **kw):
    """The tables of a width-class case (tests/width_models.py, tests/status_models.py) at M particles."""
    seed, call = seed_call(c, M)
    base = dict(name="%s-M%d" % (c.name, M), seed=seed, call=call, T=c.T, M=M, G=c.G, B=c.B, n=0 if c.pms is None else len(c.pms[0]))
    base.update(kw)
    return Spec(**base)


def torch_tables(spec):
    """(eps, masks as float64, pos_noise [T - 1, M, n], n possibly 0) as the oracle's rollouts take them."""
    tb = spec.tables()
    return (torch.from_numpy(tb["eps"]), torch.from_numpy(tb["masks"].astype(np.float64)),
            torch.from_numpy(tb["pos"]) if "pos" in tb else torch.zeros(spec.T - 1, spec.M, 0, dtype=DT))


def operands(c, spec, x0=None):
    """status_models.operands' layout on the case's own model, x0 of wm.noise and the truth's tables."""
    eps, masks, pos = torch_tables(spec)
    om = wm.model(c)["om"]
    return dict(Kinv=[q.Kinv for q in om.cache], var_scale=c.var_scale, x0=(wm.noise(c, spec.M)[0] if x0 is None else x0).contiguous(), eps=eps, masks=masks,
                pos_noise=pos, sample=True)


@functools.lru_cache(maxsize=None)
def truth_spec(c, spec):
    """The oracle's rollout (status_models.Truth: states, inputs, measured states, variances, word) fed the tables of ``spec``."""
    op = operands(c, spec)
    return sm._rollout(c, op, sm.oracle_model(c, op))


def truth(c, M):
    return truth_spec(c, spec_of(c, M))


def check(c, spec):
    """The conditions of the module docstring.  Returns the smallest variance / kzz."""
    tr = truth_spec(c, spec)
    assert tr.word == 0, (spec.name, tr.word)
    rel = tr.var / tr.kzz
    assert bool((rel > sm.MARGIN).all()), (spec.name, float(rel.min()))
    assert np.isfinite(tr.states).all() and np.isfinite(tr.inputs).all() and (tr.meas is None or np.isfinite(tr.meas).all()), spec.name
    return float(rel.min())


# ---- tier c: every forward form -------------------------------------------------------------------------------------------------------------------
# (every entry of status_models.FORMS, the states-only duplicates too: they are other instantiations of the kernels and cost nothing)
FORM_KEYS = sorted({(f.case, f.M) for f in sm.FORMS})

# ---- tier d: one case per sweep instantiation (the table in the docstring of tests/test_gpu_width_classes.py) ------------------------------------
# (case, forward code, sweep particles per workgroup or None = automatic, pipelined sweep request or None, M)
SWEEPS = [
    ("narrow_disjoint_d6", 204, None, None, 5),  # the lean sweep (automatic on the lean forward)
    ("narrow_disjoint_d6", 4, 4, None, 5),       # <8,2> / 256, four particles per workgroup
    ("narrow_b257", 1, 1, None, 5),              # <8,2> / 1024
    ("d8_u3_pms", 2, 2, None, 5),                # <16,4> / 256, two particles, the measurement-model form
    ("d15_p10_g3", 1, 1, None, 5),               # <16,4> / 1024
    ("u5_g5_d16", 16, 2, None, 17),              # <24,6> / 256
    ("p17_u2_b257", 4, 8, None, 17),             # <24,6> / 512, eight particles per workgroup
    ("p17_u2_b257", 4, 4, None, 5),              # ... four
    ("p17_u2_b257", 1, 1, 1, 5),                 # ... the pipelined sweep
    ("p17_u2_b257", 1, 1, 0, 5),                 # ... and its sequential form
    ("p25_u2", 2, 2, None, 5),                   # <32,8> / 256
    ("u7_g7_b257", 1, 1, 1, 5),                  # <32,8> / 512, pipelined
    ("u7_g7_b257", 2, 2, 0, 5),                  # ... sequential, two particles
]
SWEEP_KEYS = sorted({(s[0], s[4]) for s in SWEEPS})


@functools.lru_cache(maxsize=None)
def oracle_grad(c, M):
    """wm.oracle on the truth's tables: (states, inputs, cost, gradients [log_ls, centers, weight, bias or None, x0])."""
    from oracle import mcpilco_oracle as orc

    pp = wm.oracle_policy(c)
    x0 = wm.noise(c, M)[0].clone().requires_grad_(True)
    prm = [pp.log_ls, pp.centers, pp.weight] + ([pp.bias] if pp.bias is not None else [])
    for q in prm:
        q.requires_grad_(True)
    st, inp = wm.oracle_rollout(c, M, pp, x0, tables=torch_tables(spec_of(c, M)))
    cost, _ = orc.expected_cost(wm.oracle_cost(c, st))
    cost.backward()
    g = [q.grad.numpy().copy() for q in prm[:3]] + [pp.bias.grad.numpy().copy() if pp.bias is not None else None, x0.grad.numpy().copy()]
    return st.detach().numpy(), inp.detach().numpy(), float(cost.detach()), g


# ---- tier f: addressing edges, on one cheap form (the four-particle small-tile kernel under the measurement model: all three streams) -----------------
EDGE_CASE, EDGE_M = "d8_u3_pms", 5
_ES, _EC = (SEED_HI << 32) | 77, 9
# name -> (seed, by-value call, device word or 0, particle offset)
EDGES = {
    "call-2^32-1": (_ES, 2 ** 32 - 1, 0, 0),
    "call-2^32": (_ES, 2 ** 32, 0, 0),
    "call-2^40+3": (_ES, 2 ** 40 + 3, 0, 0),
    "seed-high-word-only": (0xDEADBEEF << 32, _EC, 0, 0),
    "seed-2^64-1": (2 ** 64 - 1, _EC, 0, 0),
    "call_dev-carry": (_ES, 2 ** 32 - 1, 1, 0),  # (the same bits as call-2^32)
    "call-split-a": (_ES, 2 ** 40, 3, 0),  # (the same bits as call-2^40+3, and as each other)
    "call-split-b": (_ES, 3, 2 ** 40, 0),
    "call_dev-wrap": (_ES, 2 ** 64 - 1, 2 ** 32 + 1, 0),  # mod 2^64: call 2^32
    "offset-7": (_ES, _EC, 0, 7),
    "offset-2^32-2": (_ES, _EC, 0, 2 ** 32 - 2),  # (the five particles straddle the word boundary)
    "offset-2^32+5": (_ES, _EC, 0, 2 ** 32 + 5),
    "offset-2^40-5": (_ES, _EC, 0, 2 ** 40 - 5),  # (the last supported particle ids)
}
SAME_BITS = [("call_dev-carry", "call-2^32"), ("call-split-a", "call-2^40+3"), ("call-split-b", "call-2^40+3"), ("call_dev-wrap", "call-2^32")]


def edge_spec(name):
    seed, call, devw, off = EDGES[name]
    return spec_of(sm.case(EDGE_CASE), EDGE_M, name="edge-" + name, seed=seed, call=call, dev=devw, offset=off)


# ---- tier a: the last-bit tier ----------------------------------------------------------------------------------------------------------------
# A draw that tells 32-bit uniforms from 52-bit ones by more than 1e-3 has its first word below ~2^5: one in 2^27.  Found by a search over the
# particle id at (LASTBIT_SEED, LASTBIT_CALL, t = 0, GP 0): particle 61547808 draws x = 19, normal 6.19195840..., 6.19687563... from 32 bits.
LASTBIT_SEED, LASTBIT_CALL, RARE_PARTICLE = (SEED_HI << 32) | 7, 3, 61547808
LASTBIT_M, LASTBIT_G = 65536, 2
LASTBIT_OFFSET = RARE_PARTICLE - 1000
LASTBIT_STEPS = (0, 255, 256, nt.T_LIMIT - 1)
LASTBIT_ROLLOUT_M = 4099  # the T = 2 rollout forms (a ragged last tile of 16 and of 4)
LASTBIT_SHARDED_M = 261  # ... the GP-sharded small-swarm forms (the lean kernel among them) take what one resident grid holds


def lastbit_step_spec(t):
    return Spec("lastbit-step-t%d" % t, LASTBIT_SEED, LASTBIT_CALL, 2, LASTBIT_M, G=LASTBIT_G, offset=LASTBIT_OFFSET, t0=t)


def lastbit_rollout_spec(sharded=False):
    return Spec("lastbit-rollout" + ("-sharded" if sharded else ""), LASTBIT_SEED, LASTBIT_CALL + 1, 2, LASTBIT_SHARDED_M if sharded else LASTBIT_ROLLOUT_M,
                G=LASTBIT_G, offset=5)


# ---- tier b: keep bits -----------------------------------------------------------------------------------------------------------------------------
KEEP_SEED, KEEP_CALL, KEEP_M, KEEP_T = (SEED_HI << 32) | 3, 2 ** 32 + 1, 37, 3  # (37: a ragged last tile of 2, 4 and 16)


def p_on_a_drawn_word():
    """A probability whose threshold IS one of the words the (KEEP_SEED, KEEP_CALL) launch draws, so that word >= threshold holds with equality
    at that (t, particle, basis function): the case that tells > from >=.  Among the words of particle 0 at t = 0, the one nearest 0.3 x 2^32;
    p = word / 2^32 is exact in a double.  Returns (p, basis function)."""
    b = np.arange(200, dtype=np.uint64)
    x, y, z, w = nt.draw(KEEP_SEED, KEEP_CALL, 0, 0, nt.STREAM_MASK, b >> np.uint64(2))
    sel = b & np.uint64(3)
    v = np.where(sel == 0, x, np.where(sel == 1, y, np.where(sel == 2, z, w))).astype(np.int64)
    i = int(np.argmin(np.abs(v - int(0.3 * 2 ** 32))))
    p = float(v[i]) / 2.0 ** 32
    assert nt.drop_threshold(p) == int(v[i])
    return p, i


KEEP_PS = (0.25, 0.1, p_on_a_drawn_word()[0])
KEEP_BS = (200, 197)
KEEP_CODES = (0, 1, 4, 16)
# the MLP's hidden shapes: 16 units alone; 16 behind a layer of 7 (units 7 .. 22: the block of units 4 .. 7 spans both layers)
MLP_HIDDEN = ((16,), (7, 16))
MLP_KEEP_M, MLP_KEEP_T, MLP_KEEP_OFFSET = 37, 3, 32


def keep_spec(p, B, M=KEEP_M, T=KEEP_T, offset=0):
    return Spec("keep-p%.4f-B%d" % (p, B), KEEP_SEED, KEEP_CALL, T, M, B=B, p=p, offset=offset)


# ---- every table set a GPU test compares against ------------------------------------------------------------------------------------------------------
def specs():
    out = [spec_of(sm.case(name), M) for name, M in sorted(set(FORM_KEYS) | set(SWEEP_KEYS))]
    out += [edge_spec(k) for k in EDGES]
    out += [lastbit_step_spec(t) for t in LASTBIT_STEPS] + [lastbit_rollout_spec(), lastbit_rollout_spec(True)]
    out += [keep_spec(p, B) for p in KEEP_PS for B in KEEP_BS]
    out += [keep_spec(p, sum(h), MLP_KEEP_M, MLP_KEEP_T, MLP_KEEP_OFFSET) for p in KEEP_PS[:2] for h in MLP_HIDDEN]
    out += [family_spec(f) for f in FAMILIES]
    return out


# ---- tier e: the other families -----------------------------------------------------------------------------------------------------------------------
# Each on its own truth function (tests/open_grad_models.py, pd_models.py, pd_meas_models.py, mlp_drop_models.py, mlp_track_models.py) with the
# recorded eps, masks and position noise replaced by the truth's tables.  arm2 (S 4, U 2, G 2), degree 1, N = 37 (Npad 48), T = 3, M = 17 (two
# tiles of 16, the second ragged; five of four), hidden (7, 3): H = 10, the Philox block of units 4 .. 7 spans both layers.
FAM_SEED, FAM_CALL, FAM_OFFSET = (SEED_HI << 32) | 11, 2 ** 32 + 3, 2 ** 32 - 9  # (the 17 particles straddle the word boundary)
FAM_SHAPE, FAM_N, FAM_DEG, FAM_T, FAM_M, FAM_HIDDEN, FAM_P = "arm2", 37, 1, 3, 17, (7, 3), 0.25
FAM_LENGTHS = [3, 1, 2, 3, 2, 3, 3, 1, 3, 2, 3, 3, 3, 2, 1, 3, 2]  # the open-loop forms: ragged
FAMILIES = ("open", "pd", "pd_meas", "mlp", "mlp_meas", "mlp_drop", "mlp_drop_meas", "mlp_track", "mlp_track_meas", "step_chain")
VAR_FLOOR = 1e-2  # kzz >= lambda = 1 on these models: ten times the margin


def family_spec(fam):
    """One (seed, call) per family: FAM_CALL + its place in FAMILIES."""
    return Spec("family-" + fam, FAM_SEED, FAM_CALL + FAMILIES.index(fam), FAM_T, FAM_M, G=2, B=sum(FAM_HIDDEN) if "drop" in fam or "track" in fam else 0,
                n=2 if "meas" in fam else 0, p=FAM_P, offset=FAM_OFFSET)


@functools.lru_cache(maxsize=None)
def family_truth(fam):
    """(cfg, inputs dict, closed_loop_family-style tuple of the family's truth function) on the truth's tables."""
    import mlp_drop_models as mdm
    import mlp_track_models as mtm
    import open_grad_models as ogm
    import pd_meas_models as pmm
    import pd_models as pdm

    spec = family_spec(fam)
    eps, masks, pos = torch_tables(spec) if spec.B else (torch.from_numpy(spec.tables()["eps"]), None, torch.from_numpy(spec.tables()["pos"]) if spec.n else None)
    if masks is not None:
        masks = masks.to(torch.uint8)
    torch.set_num_threads(1)
    if fam in ("open", "step_chain"):
        c, m, _ = ogm.build_pair("speed", FAM_N, FAM_DEG, seed=FAM_N + FAM_DEG)
        x0, u, _, w = ogm.inputs_for(c, FAM_M, FAM_T, seed=41)
        lengths = FAM_LENGTHS if fam == "open" else None
        return c, dict(x0=x0, u=u, w=w, lengths=lengths), ogm.oracle_truth("speed", m, x0, u, eps, w, True, lengths)
    if fam in ("pd", "pd_meas"):
        c, m, _ = pdm.build_pair(FAM_SHAPE, FAM_N, FAM_DEG, seed=FAM_N + FAM_DEG)
        x0, kp, kd, target, _, w, wu = pdm.inputs_for(c, FAM_M, FAM_T, seed=42)
        ins = dict(x0=x0, kp=kp, kd=kd, target=target, w=w, wu=wu, ms=None)
        if fam == "pd":
            return c, ins, pdm.pd_truth(FAM_SHAPE, m, x0, kp, kd, target, eps, w, wu, True)
        ins["ms"] = pmm.meas_model(FAM_SHAPE, "all", 0.1)
        return c, ins, pmm.pd_meas_truth(FAM_SHAPE, m, x0, kp, kd, target, eps, pos, w, wu, True, ins["ms"])
    opt = {"meas": "all"} if "meas" in fam else {}
    if "track" in fam:
        c, m, ins = mtm.case_inputs(("sampled", FAM_SHAPE, FAM_DEG, FAM_N, FAM_T, FAM_M, FAM_HIDDEN, dict(opt, p=FAM_P, idx=[3, 0])))
        return c, ins, mtm.truth_of(m, ins, eps=eps, masks=masks, pos_noise=pos)
    c, m, ins = mdm.case_inputs(("sampled", FAM_SHAPE, FAM_DEG, FAM_N, FAM_T, FAM_M, FAM_HIDDEN, FAM_P, opt))
    ins = dict(ins, masks=masks)  # (None: the forms without dropout)
    return c, ins, mdm.truth_of(m, ins, eps=eps, masks=masks, pos_noise=pos)


def family_vmin(fam):
    return family_truth(fam)[2][-1]
