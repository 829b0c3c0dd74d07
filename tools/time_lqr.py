"""Times the iLQR backward pass, ops.lqr_pass (mcp_lqr_pass: one launch, one workgroup per trajectory), against the same recursion written as
torch operations on the device, batched over the trajectories, and one iteration of policy_learning/ilqr.py:

    a  fused        ops.lqr_pass on the record
    b  torch loop   A, B from ops.linearize (one launch -- the loop is not charged a step loop for them), then per row matmul / cholesky /
                    cholesky_solve on [M, ., .] tensors: about a dozen launches per row, T - 1 rows

    python tools/time_lqr.py [--blocks 9] [--reps 3] [--shapes arm,ur5] [--no-ilqr]

Shapes: arm (S = 4, U = 2, G = 2, D = 8, T = 150) and ur5 (S = 12, U = 6, G = 6, D = 24, T = 300), each with M = 1 and M = 64.  The pass
reads a record and the model's index maps, no GP array, so its operands here are synthetic: states within +-0.5, a record with entries of
size 0.1, du_da in (0.4, 1), unit hxx, huu in (0.25, 1.25), random gradients.  The forms alternate block by block; median [min, max] of the
blocks, one JSON line per (shape, M) with the largest relative difference between the two forms' outputs and the status word.  The ilqr
line: ``ilqr(iterations=0)`` (nominal + expansion + pass) and ``ilqr(iterations=1)`` on the trained two-joint arm of
tools/time_pd_rollout.py at T = 150; their difference is one iteration (a pass, the forward passes of its line search, the next nominal)."""
import argparse
import json

import numpy as np
import torch

from time_pd_rollout import DT, build_object  # (puts the repository on sys.path and registers the package)

from mc_pilco_amd import hipabi as abi  # noqa: E402
from mc_pilco_amd import ops  # noqa: E402
from mc_pilco_amd.policy_learning.ilqr import Quadratic_tracking_cost, ilqr  # noqa: E402

SHAPES = {
    "arm": dict(S=4, U=2, G=2, angle=[0, 1], not_angle=[2, 3], vel=[2, 3], not_vel=[0, 1], Ts=0.05, T=150),
    "ur5": dict(S=12, U=6, G=6, angle=list(range(6)), not_angle=list(range(6, 12)), vel=list(range(6, 12)), not_vel=list(range(6)), Ts=0.02, T=300),
}


class RecordModel:
    """What ops.linearize / ops.lqr_pass read of a model: its scalars and index lists (mcp_model without GP operands)."""

    def __init__(self, c, dev):
        m = abi.Model()
        m.S, m.U, m.G, m.Ts = c["S"], c["U"], c["G"], c["Ts"]
        m.n_angle, m.n_not_angle = len(c["angle"]), len(c["not_angle"])
        m.D = m.n_not_angle + 2 * m.n_angle + m.U
        for name in ("angle", "not_angle", "vel", "not_vel"):
            for i, v in enumerate(c[name]):
                getattr(m, name)[i] = v
        self.c, self.S, self.U, self.G, self.D, self.device = m, m.S, m.U, m.G, m.D, dev


def operands(c, M, dev, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    T, S, U, G = c["T"], c["S"], c["U"], c["G"]
    D = len(c["not_angle"]) + 2 * len(c["angle"]) + U
    r = lambda *s: torch.rand(*s, dtype=DT, device=dev, generator=gen)
    return dict(states=r(T, M, S) - 0.5, jac=0.2 * (r(T - 1, M, G, D) - 0.5), du_da=0.4 + 0.6 * r(T, M, U), lx=r(T, M, S) - 0.5, lu=r(T, M, U) - 0.5,
                hxx=torch.ones(T, M, S, dtype=DT, device=dev), huu=0.25 + r(T, M, U))


def torch_pass(model, o, reg):
    """The recursion of include/mcpilco_hip.h in torch, batched over M."""
    A, B = ops.linearize(model, o["states"], o["jac"], du_da=o["du_da"])
    lx, lu, hxx, huu = o["lx"], o["lu"], o["hxx"], o["huu"]
    T, M, S = lx.shape
    U = lu.shape[2]
    gain, kff = torch.zeros(M, T, U, S, dtype=DT, device=lx.device), torch.zeros(M, T, U, dtype=DT, device=lx.device)
    eye = reg * torch.eye(U, dtype=DT, device=lx.device)
    den = huu[T - 1] + reg
    kff[:, T - 1] = -lu[T - 1] / den
    d0, d1 = [(kff[:, T - 1] * lu[T - 1]).sum(1)], [(kff[:, T - 1] * den * kff[:, T - 1]).sum(1)]
    Vx, Vxx = lx[T - 1], torch.diag_embed(hxx[T - 1])
    for t in range(T - 2, -1, -1):
        At, Bt = A[t], B[t]
        AtT, BtT = At.transpose(1, 2), Bt.transpose(1, 2)
        Qx, Qu = lx[t] + (AtT @ Vx.unsqueeze(2)).squeeze(2), lu[t] + (BtT @ Vx.unsqueeze(2)).squeeze(2)
        VA, VB = Vxx @ At, Vxx @ Bt
        Qxx, Qux, Quu = torch.diag_embed(hxx[t]) + AtT @ VA, BtT @ VA, torch.diag_embed(huu[t]) + BtT @ VB + eye
        L = torch.linalg.cholesky(Quu)
        X = torch.cholesky_solve(torch.cat([Qu.unsqueeze(2), Qux], 2), L)
        k, K = -X[:, :, 0], X[:, :, 1:]
        kff[:, t], gain[:, t] = k, K
        d0.append((k * Qu).sum(1))
        d1.append((k * (Quu @ k.unsqueeze(2)).squeeze(2)).sum(1))
        Vx = Qx + (Qux.transpose(1, 2) @ k.unsqueeze(2)).squeeze(2)
        W = Qxx - Qux.transpose(1, 2) @ K
        Vxx = 0.5 * (W + W.transpose(1, 2))
    dv = torch.stack([torch.stack(d0[::-1]).sum(0), torch.stack(d1[::-1]).sum(0)], 1)
    return gain, kff, dv


def block_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stat(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="arm,ur5")
    ap.add_argument("--no-ilqr", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    reg = 1e-6
    for shape in args.shapes.split(","):
        c = SHAPES[shape]
        model = RecordModel(c, dev)
        for M in (1, 64):
            o = operands(c, M, dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            fused = lambda: ops.lqr_pass(model, o["states"], o["jac"], o["lx"], o["lu"], o["hxx"], o["huu"], reg=reg, du_da=o["du_da"], status=status)
            loop = lambda: torch_pass(model, o, reg)
            got, ref = fused(), loop()  # warm-up of both forms, and their agreement
            torch.cuda.synchronize()
            diff = [float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, ref)]
            ms = dict(a=[], b=[])
            for _ in range(args.blocks):
                ms["a"].append(block_ms(fused, args.reps))
                ms["b"].append(block_ms(loop, 1))
            out = dict(shape=shape, S=c["S"], U=c["U"], T=c["T"], M=M, status=int(status.item()), rel_diff_gain_kff_dv=[float("%.3e" % d) for d in diff],
                       a_fused_ms=stat(ms["a"]), b_torch_loop_ms=stat(ms["b"]))
            out["ratio_b_over_a"] = round(out["b_torch_loop_ms"][0] / out["a_fused_ms"][0], 2)
            out["fused_faster"] = out["a_fused_ms"][0] < out["b_torch_loop_ms"][0]
            print(json.dumps(out), flush=True)
    if not args.no_ilqr:
        obj, sim, N, M, T = build_object("arm2", dev)
        pm = obj.model_learning.packed()
        target = obj.control_policy.target_traj
        cost = Quadratic_tracking_cost(target, [0.5, 0.5, 2.0, 2.0], input_lengthscales=[3.0, 3.0])
        x0, a0 = target[0].clone(), torch.zeros(T, 2, dtype=DT, device=dev)
        run = lambda n: ilqr(pm, x0, a0, cost, iterations=n, u_max=1.5)
        info = run(1)[1]
        run(0)
        torch.cuda.synchronize()
        ms = {0: [], 1: []}
        for _ in range(args.blocks):
            for n in (0, 1):
                ms[n].append(block_ms(lambda: run(n), 1))
        out = dict(shape="arm2 (trained, N = %d)" % N, T=T, cost=[round(v, 6) for v in info["cost"]], alpha=info["alpha"], status=info["status"],
                   ilqr_0_iterations_ms=stat(ms[0]), ilqr_1_iteration_ms=stat(ms[1]))
        out["one_iteration_ms"] = round(out["ilqr_1_iteration_ms"][0] - out["ilqr_0_iterations_ms"][0], 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
