"""Small generic systems for the width-class tests (tests/test_gpu_width_classes.py): one record per case, random training data, hyper-parameters,
policy parameters, x0 and recorded noise from seeded generators.  The oracle side (oracle/mcpilco_oracle.py, fp64 on the CPU, torch autograd for the
gradients) pretrains each GP itself; the packed side consumes the oracle's own X, alpha and Kinv, so only the evaluation is compared -- the pattern of
tests/test_gpu_lean_chain.py with the widths as parameters.  CPU side only imports torch and the oracle; ``packed`` imports the GPU helpers when called.

The instantiation a case lands in follows from its widths alone (``classes``): D = n_not_angle + 2 n_angle + U is the GP input, P the policy feature
count (plain: S; angles: n_non_angle + 2 n_angle; traj: 2 S).

  16-particle forward  class 0: D <= 7 and P <= 8 and U <= 2;  class 1: D <= 24 and P <= 24 and U <= 6, with RT = ceil((D + 1) / 16) row tiles of
                       [X^T; 1];  class 2 otherwise;  no tile kernel at D + 1 > 32 (a forced 16 then runs 4 particles per workgroup); the GP-sharded
                       16-particle launch exists in classes 0 and 1 with G >= 2
  adjoint sweep        <8,2>: P <= 8 and U <= 2;  <16,4>: P <= 16 and U <= 4;  <24,6>: P <= 24 and U <= 6;  <32,8> otherwise;  thread class 256 for
                       B <= 256, else 1024 (<8,2>, <16,4>: one particle per workgroup) or 512 (<24,6>, <32,8>: B <= 512)"""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from helpers import T as TT
from helpers import hyper
from oracle import mcpilco_oracle as orc

TS, SIGMA_N, P_DROP, FC = 0.05, 0.1, 0.25, 0.5


@dataclass(frozen=True)
class Case:
    name: str
    S: int
    U: int
    angle: Tuple[int, ...]
    not_angle: Tuple[int, ...]
    vel: Tuple[int, ...]  # one per GP
    not_vel: Tuple[int, ...]  # -1: that GP integrates no position
    N: Tuple[int, ...]  # training points per GP
    kind: str  # policy: "plain" | "angles" | "traj"
    B: int
    T: int
    deg: int = 0  # polynomial degree of every GP's kernel
    var_scale: Optional[Tuple[float, ...]] = None
    pol_angle: Tuple[int, ...] = ()
    pol_non_angle: Tuple[int, ...] = ()
    u_max: object = 2.0  # float or one per input
    bias: bool = False
    pms: Optional[Tuple[Tuple[int, ...], Tuple[int, ...]]] = None  # measurement model: (pos, vel)
    cost: str = "traj"  # "traj" (over ``used``) | "target" (saturated distance over ``used``)
    used: Tuple[int, ...] = ()
    gx0: bool = False  # also compare dJ/dx0
    pins: str = ""

    @property
    def G(self):
        return len(self.vel)

    @property
    def D(self):
        return len(self.not_angle) + 2 * len(self.angle) + self.U

    @property
    def P(self):
        return {"plain": self.S, "traj": 2 * self.S, "angles": len(self.pol_non_angle) + 2 * len(self.pol_angle)}[self.kind]

    @property
    def seed(self):
        return sum((i + 1) * ord(ch) for i, ch in enumerate(self.name)) % 100003


def classes(c):
    """What the dispatch rules of rollout_fwd_tile.hip / rollout_bwd.hip give for the widths of ``c`` (restated here from the rules in the module
    docstring, not read from the library: tests/test_dispatch_plan_cpu.py compares the two): tile class (None: no tile kernel), row tiles, sweep <PFM,UM>, its thread class, GP-sharded tile launch."""
    D, P, U = c.D, c.P, c.U
    tile = None if D + 1 > 32 else (0 if (D <= 7 and P <= 8 and U <= 2) else (1 if (D <= 24 and P <= 24 and U <= 6) else 2))
    sweep = (8, 2) if (P <= 8 and U <= 2) else ((16, 4) if (P <= 16 and U <= 4) else ((24, 6) if (P <= 24 and U <= 6) else (32, 8)))
    nt = 64 * max(1, (c.B + 63) // 64)
    maxnt = 256 if nt <= 256 else (1024 if sweep[0] <= 16 else 512)
    return dict(tile=tile, row_tiles=(D + 1 + 15) // 16, sweep=sweep, maxnt=maxnt, nt=nt, tile_sharded=tile in (0, 1) and c.G >= 2,
                pipe=sweep[0] > 16 and 256 < nt <= 448 and c.pms is None)


def sweep_widths(c):
    """Particles per workgroup the general sweep can launch for ``c``, restated from plan_bwd (csrc/rollout_plan.h): the instantiations that exist
    for (sweep class, thread class) and, of those, the ones whose prefetched record fits (PB x record <= 5 per chain-free thread, the record being
    2 S + 2 U + G D (+ S with the measurement model)).  A forced width that is not among them is halved by the library until one is.  The dispatch
    report has no field for the width that ran, but the plan query has (mcp_bwd_plan.particles): tests/test_dispatch_plan_cpu.py holds this
    restatement against it for every case and every forced width; the GPU tests request only these."""
    k = classes(c)
    have = {((8, 2), 256): (1, 2, 4), ((16, 4), 256): (1, 2), ((24, 6), 256): (1, 2), ((32, 8), 256): (1, 2), ((8, 2), 1024): (1,),
            ((16, 4), 1024): (1,), ((24, 6), 512): (1, 2, 4, 8), ((32, 8), 512): (1, 2)}
    rec = 2 * c.S + 2 * c.U + c.G * c.D + (c.S if c.pms is not None else 0)
    out = []
    for pb in (1, 2, 4, 8):
        nt = max(k["nt"], 64 * pb)  # a wave per particle at least: a wide request lifts the thread class (eight particles: 512 threads)
        maxnt = 256 if nt <= 256 else (1024 if k["sweep"][0] <= 16 else 512)
        if pb in have[(k["sweep"], maxnt)] and nt <= maxnt and pb * rec <= 5 * (nt - 64 * pb if nt // 64 > pb else nt):
            out.append(pb)
    return out


def lists_overlap(c):
    return bool(set(c.angle) & set(c.not_angle)) or bool(set(c.pol_angle) & set(c.pol_non_angle))


def _r(n):
    return tuple(range(n))


def _r2(a, b):
    return tuple(range(a, b))


CASES = [
    # ---- <8,2> -------------------------------------------------------------------------------------------------------------------------------
    Case("narrow_traj_d7", 4, 2, (2,), (0, 1, 3), (1, 3), (0, 2), (30, 44), "traj", 17, 2, used=(0, 2, 3), gx0=True,
         pins="D = 7, P = 8, U = 2: the top of tile class 0; sweep <8,2> / 256; a traj policy on a narrow model (no lean kernel)"),
    Case("narrow_overlap_d7", 4, 1, (2,), (0, 1, 2, 3), (1, 3), (0, 2), (30, 30), "angles", 17, 4, pol_angle=(2,), pol_non_angle=(0, 1, 3), used=(0, 2),
         pins="state 2 in angle AND not_angle (D = 7): neither lean kernel may take it; tile class 0; the general sweep <8,2> / 256"),
    Case("narrow_disjoint_d6", 4, 1, (2,), (0, 1, 3), (1, 3), (0, 2), (30, 30), "angles", 129, 4, pol_angle=(2,), pol_non_angle=(0, 1, 3), used=(0, 2),
         pins="the twin of narrow_overlap_d7 with disjoint lists: both lean kernels DO run (the report distinguishes the two); <8,2> / 256 at B = 129"),
    Case("narrow_b257", 4, 1, (2,), (0, 1, 3), (1, 3), (0, 2), (44, 30), "angles", 257, 2, pol_angle=(2,), pol_non_angle=(0, 1, 3), used=(0, 1, 2, 3),
         gx0=True, pins="<8,2> / 1024 at B = 257 (five waves); B > 256: no lean sweep, while the lean forward kernel (no limit on B) runs on request"),
    Case("narrow_b1024", 4, 1, (2,), (0, 1, 3), (1, 3), (0, 2), (30, 44), "angles", 1024, 2, pol_angle=(2,), pol_non_angle=(0, 1, 3), used=(2, 0),
         pins="<8,2> / 1024 at B = 1024 = MCP_MAX_BASIS (sixteen waves); the lean forward kernel at that B"),
    Case("g1_plain_d16", 8, 2, _r(6), (6, 7), (7,), (3,), (37,), "plain", 600, 4, cost="target", used=(0, 3, 7), gx0=True,
         pins="G = 1 (nothing to shard); D = 16: class 1 with TWO row tiles (D + 1 = 17); plain policy at T = 4 on a narrow policy width (P = 8); "
              "<8,2> / 1024 at B = 600; target-state cost"),
    # ---- <16,4> ------------------------------------------------------------------------------------------------------------------------------
    Case("d8_u3_pms", 4, 3, (2,), (0, 1, 3), (1, 3), (0, 2), (44, 30), "angles", 129, 4, pol_angle=(2,), pol_non_angle=(0, 1, 3), u_max=(2.0, 0.7, 1.3),
         bias=True, pms=((0, 2), (1, 3)), used=(0, 2, 3), gx0=True,
         pins="D = 8: class 1 with ONE row tile; <16,4> / 256 through U = 3 alone (P = 5), its measurement-model form; policy bias, a bound per input"),
    Case("d15_p10_g3", 8, 1, _r(6), (6, 7), (5, 6, 7), (2, 3, 4), (24, 37, 48), "angles", 257, 3, pol_angle=(0, 1, 2, 3), pol_non_angle=(6, 7),
         used=(1, 4, 6), pins="D = 15: class 1 with D + 1 = 16 exactly (one row tile); <16,4> / 1024 through P = 10 alone (U = 1) at B = 257; G = 3; "
                              "a different N per GP (Npad 32 / 48 / 48)"),
    Case("d25_s16_g8", 16, 1, _r(8), _r2(8, 16), _r2(8, 16), _r(8), (24,) * 8, "plain", 17, 2, used=(0, 5, 9, 15), gx0=True,
         pins="D = 25: tile class 2 through D alone (no GP-sharded tile launch); S = 16, G = 8; plain policy P = 16: <16,4> / 256 through P alone at B = 17"),
    Case("speed_mixed_p9", 6, 2, (2,), (0, 1, 3, 4, 5), (3, 4, 5), (0, -1, 2), (30, 44, 37), "angles", 129, 4, var_scale=(0.49, 1.0, 2.25),
         pol_angle=(1, 2, 4), pol_non_angle=(0, 3, 5), cost="target", used=(0, 2, 4),
         pins="speed model where GP 1 integrates no position (not_vel = -1 beside real positions; state 1 has no role and becomes 0), var_scale != 1; "
              "D = 9, P = 9: <16,4> / 256 through P alone"),
    Case("delta_d11_u3", 6, 3, (1, 4), (0, 2, 3, 5), _r(6), (-1,) * 6, (24, 37, 48, 60, 30, 44), "plain", 65, 3, deg=1, used=(0, 1, 4, 5), gx0=True,
         pins="delta-state model at S = G = 6, U = 3 (D = 11), degree-1 kernels, every GP its own N (Npad 32 / 48 / 48 / 64 / 32 / 48); <16,4> / 256 at B = 65"),
    Case("u4_b513", 4, 4, (2,), (0, 1, 3), (1, 3), (0, 2), (30, 30), "angles", 513, 2, pol_angle=(2,), pol_non_angle=(0, 1, 3), used=(0, 2),
         pins="<16,4> / 1024 through U = 4 at B = 513 (nine waves); D = 9"),
    # ---- <24,6> ------------------------------------------------------------------------------------------------------------------------------
    Case("u5_g5_d16", 8, 5, (0, 1, 2), _r2(3, 8), _r2(3, 8), (0, 1, 2, -1, -1), (30,) * 5, "plain", 17, 4, used=(0, 4, 7),
         pins="<24,6> / 256 through U = 5 alone (P = 8); G = 5 (prime: the sharded tile launch has cs = G only); D = 16, two row tiles"),
    Case("p17_u2_b257", 9, 2, (0,), _r2(1, 9), (6, 7, 8), (3, 4, 5), (44, 30, 37), "angles", 257, 4, pol_angle=_r(8), pol_non_angle=(8,), used=(0, 3, 8),
         gx0=True, pins="<24,6> / 512 through P = 17 alone (U = 2) at B = 257: the pipelined sweep and its sequential form, and 8 / 4 / 2 particles per "
                        "workgroup; D = 12, class 1 with one row tile"),
    Case("ur5_angles_pms", 12, 6, _r(6), _r2(6, 12), _r2(6, 12), _r(6), (37,) * 6, "angles", 129, 2, pol_angle=_r(12), pol_non_angle=(),
         pms=(_r(6), _r2(6, 12)), used=(0, 3, 7, 11),
         pins="D = 24 and P = 24 (all twelve states as angles): the top of tile class 1 and of the <24,6> accumulators; an angles policy on a wide "
              "model; <24,6> / 256 with the measurement model"),
    # ---- <32,8> ------------------------------------------------------------------------------------------------------------------------------
    Case("p25_u2", 13, 2, (0,), (1, 2, 3, 4), (11, 12), (5, 6), (30, 44), "angles", 129, 3, pol_angle=_r(12), pol_non_angle=(12,), used=(0, 6, 12),
         pins="P = 25 with U = 2: <32,8> / 256 through P alone, tile class 2 through P alone (D = 8)"),
    Case("u7_g7_b257", 8, 7, (0, 1), _r2(2, 8), _r2(1, 8), (0, -1, -1, -1, -1, -1, -1), (30,) * 7, "plain", 257, 2, used=(0, 1, 7), gx0=True,
         pins="U = 7 with P = 8: <32,8> / 512 through U alone at B = 257 (pipelined and sequential), tile class 2 through U alone (D = 17); G = 7"),
    Case("d31_traj_p32", 16, 7, _r(8), _r2(8, 16), _r2(8, 16), _r(8), (24,) * 8, "traj", 17, 2, used=(1, 8, 15),
         pins="D = 31: the top of the tile kernel (class 2, D + 1 = 32); traj policy at P = 32 = MCP_MAX_PFEAT; S = 16, G = 8; <32,8> / 256"),
    Case("d32_u8_pms", 16, 8, _r(8), _r2(8, 16), _r2(8, 16), _r(8), (24,) * 8, "plain", 129, 2, u_max=tuple(0.5 + 0.25 * i for i in range(8)), bias=True,
         pms=(_r(8), _r2(8, 16)), used=(0, 9), gx0=True,
         pins="D = 32 = MCP_MAX_GPDIM: no tile kernel (a forced 16 runs 4 particles per workgroup); U = 8 = MCP_MAX_INPUT; <32,8> / 256 with the "
              "measurement model; bias, a bound per input"),
]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def model(c):
    """Oracle model (its own pretrain on random data) and the per-GP kernel parameters the packed side needs."""
    rng = np.random.RandomState(c.seed)
    D, G = c.D, c.G
    gps = []
    for g in range(G):
        Z = rng.randn(c.N[g], D)
        ls = (1.5 + rng.rand(D)) * np.sqrt(max(D, 6) / 6.0)  # (wide inputs: the kernel values stay O(0.1 .. 1))
        poly = None
        if c.deg >= 1:
            poly = [0.01 * (0.8 + 0.4 * rng.rand(D + 1))] + ([0.01 * (0.8 + 0.4 * rng.rand(2 * D))] if c.deg >= 2 else [])
        Y = np.sin(Z @ (rng.randn(D, 1) / np.sqrt(D / 6.0))) * 0.3
        h = hyper(ls, SIGMA_N, 1.0, poly)
        gps.append(dict(ls=ls, poly=poly, hyp=h, cache=orc.pretrain_gp(h, TT(Z), TT(Y))))
    om = orc.SpeedModel([q["hyp"] for q in gps], [q["cache"] for q in gps], TS, list(c.angle), list(c.not_angle), list(c.vel), list(c.not_vel))
    return dict(gps=gps, om=om)


@functools.lru_cache(maxsize=None)
def policy(c):
    rng = np.random.RandomState(c.seed + 1)
    P = c.P
    return dict(ls=(1.0 + rng.rand(P)) * np.sqrt(max(P, 4) / 4.0), centers=0.7 * rng.randn(c.B, P), weight=rng.randn(c.U, c.B) * 0.5,
                bias=0.3 * rng.randn(c.U) if c.bias else None, traj=0.3 * rng.randn(c.T, c.S), cost_ls=1.0 + 2.0 * rng.rand(len(c.used)),
                std_pos=None if c.pms is None else 0.01 + 0.01 * rng.rand(len(c.pms[0])))


@functools.lru_cache(maxsize=None)
def noise(c, M):
    g = torch.Generator().manual_seed(1000 * c.seed + M)
    x0 = 0.3 * torch.randn(M, c.S, dtype=torch.float64, generator=g)
    eps = torch.randn(c.T - 1, M, c.G, dtype=torch.float64, generator=g)
    masks = (torch.rand(c.T, M, c.B, dtype=torch.float64, generator=g) >= P_DROP).to(torch.float64)
    pos_noise = torch.randn(c.T - 1, M, 0 if c.pms is None else len(c.pms[0]), dtype=torch.float64, generator=g)
    return x0, eps, masks, pos_noise


def oracle_policy(c):
    pi = policy(c)
    return orc.PolicyPar(torch.log(TT(pi["ls"])).reshape(1, -1), TT(pi["centers"]), TT(pi["weight"]), c.u_max if np.isscalar(c.u_max) else list(c.u_max),
                         c.kind, angle=list(c.pol_angle), non_angle=list(c.pol_non_angle), target_traj=TT(pi["traj"]) if c.kind == "traj" else None,
                         bias=None if pi["bias"] is None else TT(pi["bias"]))


def oracle_cost(c, st):
    pi = policy(c)
    if c.cost == "target":
        return orc.saturated_distance_cost(st, TT(pi["traj"][-1, list(c.used)]), TT(pi["cost_ls"]), list(c.used))
    return orc.traj_cost(st, TT(pi["traj"]), TT(pi["cost_ls"]), list(c.used))


def oracle_rollout(c, M, pp, x0, tables=None):
    """``tables``: (eps, masks, pos_noise) in the place of the recorded noise of ``noise(c, M)``."""
    eps, masks, pos_noise = noise(c, M)[1:] if tables is None else tables
    om = model(c)["om"]
    step = lambda m, x, u, e, sample: orc.mixed_next_state(m, x, u, e, sample, c.var_scale)  # noqa: E731
    if c.pms is not None:
        return orc.apply_policy_pms(om, pp, x0, c.T, list(c.pms[0]), list(c.pms[1]), TT(policy(c)["std_pos"]), FC, P_DROP, eps, masks, pos_noise, step=step)
    return orc.apply_policy(om, pp, x0, c.T, P_DROP, eps, masks, step=step)


@functools.lru_cache(maxsize=None)
def oracle(c, M):
    """(states, inputs, cost, gradients [log_ls, centers, weight, bias or None, x0]) of the oracle: computed once per (case, M), shared by the tests."""
    pp = oracle_policy(c)
    x0 = noise(c, M)[0].clone().requires_grad_(True)
    prm = [pp.log_ls, pp.centers, pp.weight] + ([pp.bias] if pp.bias is not None else [])
    for q in prm:
        q.requires_grad_(True)
    st, inp = oracle_rollout(c, M, pp, x0)
    cost, _ = orc.expected_cost(oracle_cost(c, st))
    cost.backward()
    g = [q.grad.numpy().copy() for q in prm[:3]] + [pp.bias.grad.numpy().copy() if pp.bias is not None else None, x0.grad.numpy().copy()]
    return st.detach().numpy(), inp.detach().numpy(), float(cost.detach()), g


def packed(c, M, philox=None):
    """(model, policy, cost, noise, meas, x0) on the GPU, on the oracle's own X / alpha / Kinv.  ``philox``: a NoiseSpec without buffers in the
    place of the recorded eps, masks and position noise."""
    from gpu_helpers import G as GG
    from gpu_helpers import dev, spec_from
    from mc_pilco_amd import ops

    md, pi = model(c), policy(c)
    x0, eps, masks, pos_noise = noise(c, M)
    gps = [ops.PackedGP(spec_from(q["ls"], SIGMA_N, 1.0, q["poly"]), GG(q["cache"].X.numpy()), GG(q["cache"].alpha.numpy()), GG(q["cache"].Kinv.numpy()))
           for q in md["gps"]]
    pm = ops.PackedModel(gps, c.S, c.U, TS, list(c.angle), list(c.not_angle), list(c.vel), list(c.not_vel), var_scale=c.var_scale)
    pol = ops.PackedPolicy(c.kind, c.S, torch.log(GG(pi["ls"])).reshape(1, -1).requires_grad_(True), GG(pi["centers"]).requires_grad_(True),
                           GG(pi["weight"]).requires_grad_(True), c.u_max if np.isscalar(c.u_max) else list(c.u_max), True, angle=list(c.pol_angle),
                           non_angle=list(c.pol_non_angle), target_traj=pi["traj"] if c.kind == "traj" else None,
                           bias=None if pi["bias"] is None else GG(pi["bias"]).requires_grad_(True))
    if c.cost == "target":
        cost = ops.PackedCost("target", c.S, dev(), target_state=pi["traj"][-1, list(c.used)], lengthscales=pi["cost_ls"], active_dims=list(c.used))
    else:
        cost = ops.PackedCost("traj", c.S, dev(), target_traj=pi["traj"], lengthscales=pi["cost_ls"], used=list(c.used))
    nz = philox if philox is not None else ops.NoiseSpec(eps=GG(eps.numpy()), masks=masks.to(torch.uint8).to(dev()).contiguous())
    meas = None
    if c.pms is not None:
        b, a = orc.butter1(FC)
        meas = ops.MeasSpec(pos=list(c.pms[0]), vel=list(c.pms[1]), std_pos=list(pi["std_pos"]), b=b, a=a,
                            pos_noise=None if philox is not None else GG(pos_noise.numpy()))
    return pm, pol, cost, nz, meas, GG(x0.numpy())
