"""Times the batched planner (policy_learning.mppi.plan_batch: B plans in the launches of one) against the loop of B single plans
(policy_learning.mppi.plan, one call per state, as a caller had to write it before the batched form existed):

    a  batched   mppi.plan_batch over the B states: per iteration ONE rollout launch on a grid of (tiles, B) and the update's two launches on
                 B workgroups / (H, B) workgroups; nothing is read back
    b  loop      B calls of mppi.plan: per state and iteration three launches, and one host synchronisation per state

    python tools/time_plan_batch.py [--blocks 7] [--reps 3] [--shapes cartpole_mean,cartpole_sampled,ur5_mean] [--iterations 5]

Shapes of tools/time_mppi.py (H = 30): cart-pole (N = 300) with K = 1024 on the mean model at B = 1, 8, 64 and K = 256 x P = 16 sampled at
B = 1, 8, 50; UR5 (N = 400) with K = 256 on the mean model at B = 1, 8, 50.  The B start states are the workload's initial state plus a small
spread; both forms plan from the same states with the same seeds (problem b at particle_offset b * max(K, P), which is plan_batch's
default), so their results agree bit for bit and the tool asserts it.  Device events around the calls (the loop's synchronisations fall
inside its interval; the batched form's interval ends at the last kernel), `reps` calls per block, the two forms alternate block by block;
median [min, max] of the blocks; one JSON line per (shape, B): one iteration and a control step of --iterations iterations of both forms, and
the single-problem iteration of tools/time_mppi.py (rollout-cost + update at B = 1 through ops) as the check that the single path has not
moved."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcp_boot  # noqa: E402,F401

from mc_pilco_amd import ops, workloads  # noqa: E402
from mc_pilco_amd.policy_learning import Cost_function as cf  # noqa: E402
from mc_pilco_amd.policy_learning import mppi  # noqa: E402

DT = torch.float64
H = 30
SHAPES = {
    "cartpole_mean": dict(workload="c1", K=1024, P=1, sample=False, sigma=2.0, lam=0.05, B=(1, 8, 64)),
    "cartpole_sampled": dict(workload="c1", K=256, P=16, sample=True, sigma=2.0, lam=0.05, B=(1, 8, 50)),
    "ur5_mean": dict(workload="ur5_script", K=256, P=1, sample=False, sigma=0.3, lam=0.05, B=(1, 8, 50)),
}


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
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--batches", default="", help="comma-separated B in place of the shape's own")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in args.shapes.split(","):
        s = SHAPES[name]
        w = workloads.build(s["workload"], dev, T=H)
        pm, c = w.model, w.problem["cfg"]
        U, K, P = pm.U, s["K"], s["P"]
        u_max = float(np.max(c["u_max"]))
        cartpole = w.problem["system"] == "cartpole"
        cin = ops.PackedCostInputs(U, dev, lengthscales=[4.0 * u_max] * U) if cartpole else None
        cost_obj = (cf.Input_penalty(cf.Cart_pole_cost(c["cost_target"], c["cost_ls"], c["cost_angle_index"], c["cost_pos_index"]),
                                     lengthscales=[4.0 * u_max] * U)
                    if cartpole else cf.Expected_saturated_distance_from_trajectory(w.problem["target_traj"], c["cost_ls"]))
        par = dict(K=K, P=P, sigma=s["sigma"], lam=s["lam"], u_max=u_max, particle_pred=s["sample"])
        a0 = torch.zeros(H, U, dtype=DT, device=dev)
        # the single-problem iteration of tools/time_mppi.py
        mp = ops.PackedMPPI(K, P, H, U, s["sigma"], s["lam"], u_max=u_max)
        x1 = w.x0_mean.reshape(-1).contiguous()
        traj, a_new = torch.empty(K * P, dtype=DT, device=dev), torch.empty(H, U, dtype=DT, device=dev)
        out_buf = (torch.empty(K, dtype=DT, device=dev), torch.empty(K, dtype=DT, device=dev), torch.empty(4, dtype=DT, device=dev))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        nz1 = ops.NoiseSpec(seed=1, call=0)

        def single_iteration():
            ops.mppi_rollout(pm, mp, w.cost, x1, a0, cost_inputs=cin, noise=nz1, particle_pred=s["sample"], traj_cost=traj, status=status)
            return ops.mppi_update(mp, traj, a0, noise=nz1, a_new=a_new, out=out_buf, status=status)

        for B in ([int(v) for v in args.batches.split(",")] if args.batches else s["B"]):
            gen = torch.Generator().manual_seed(B)
            X = (x1.reshape(1, -1) + 0.05 * torch.randn(B, pm.S, dtype=DT, generator=gen).to(dev)).contiguous()
            stride = max(K, P)

            def batched(n_it):
                return mppi.plan_batch(pm, X, a0, cost_obj, iterations=n_it, noise=ops.NoiseSpec(seed=1, call=0), **par)

            def loop(n_it):
                return [mppi.plan(pm, X[b], a0, cost_obj, iterations=n_it, noise=ops.NoiseSpec(seed=1, call=0, particle_offset=b * stride), **par)
                        for b in range(B)]

            got, ref = batched(args.iterations), loop(args.iterations)  # warm-up of both forms, and their agreement
            single_iteration()
            torch.cuda.synchronize()
            same = all(torch.equal(got[0][b], ref[b][0]) for b in range(B))
            ms = dict(batched_1=[], loop_1=[], batched_n=[], loop_n=[], single=[])
            for _ in range(args.blocks):
                ms["batched_1"].append(block_ms(lambda: batched(1), args.reps))
                ms["loop_1"].append(block_ms(lambda: loop(1), args.reps))
                ms["batched_n"].append(block_ms(lambda: batched(args.iterations), args.reps))
                ms["loop_n"].append(block_ms(lambda: loop(args.iterations), args.reps))
                ms["single"].append(block_ms(single_iteration, args.reps))
            out = dict(shape=name, N=w.problem["N"], G=pm.G, D=pm.D, H=H, K=K, P=P, B=B, bitwise_equal=bool(same),
                       status=int(got[1]["status"].any().item()), single_problem_iteration_ms=stat(ms["single"]),
                       a_batched_iteration_ms=stat(ms["batched_1"]), b_loop_iteration_ms=stat(ms["loop_1"]), iterations=args.iterations,
                       a_batched_step_ms=stat(ms["batched_n"]), b_loop_step_ms=stat(ms["loop_n"]))
            out["iteration_ratio_b_over_a"] = round(out["b_loop_iteration_ms"][0] / out["a_batched_iteration_ms"][0], 2)
            out["step_ratio_b_over_a"] = round(out["b_loop_step_ms"][0] / out["a_batched_step_ms"][0], 2)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
