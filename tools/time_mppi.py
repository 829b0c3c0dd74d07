"""Times one MPPI planning iteration, fused (ops.mppi_rollout + ops.mppi_update: three launches, no buffer of size [H][M]) against the
same iteration composed from the entries that existed before it:

    a  fused         ops.mppi_rollout (inputs generated, rolled out and reduced to one cost per trajectory on the chip), ops.mppi_update
    b  composition   torch.randn [H,K,U] -> inputs squash(a + sigma xi) repeated per particle [H,M,U] -> ops.rollout_open (Mu == M, an eps
                     buffer repeated per candidate in the sampled form) -> ops.cost_moments (mcp_cost_u_fwd) -> sum over t -> mean over
                     the particles -> torch.softmax -> torch.einsum

    python tools/time_mppi.py [--blocks 9] [--reps 5] [--shapes cartpole_mean,cartpole_sampled,ur5_mean] [--iterations 5]

Shapes, from the project's workloads (mc_pilco_amd.workloads), H = 30: cart-pole (2 GPs, D = 6, N = 300) with K = 1024, P = 1 on the mean
model and K = 256, P = 16 sampled; UR5 (6 GPs, D = 24, N = 400, degree 1) with K = 256 on the mean model.  Costs: the cart-pole cost with an
effort term (ADD), the UR5 trajectory cost.  Events around the calls, `reps` calls per block, the forms alternate block by block; median
[min, max] of the blocks; one JSON line per shape: the rollout-cost and the update alone, the fused iteration, the composed iteration, and a
control step of --iterations fused iterations through policy_learning.mppi.plan (its one synchronisation included).  The two forms draw
different perturbations (Philox against torch.randn), so their results are compared in distribution only: both report the nominal's cost,
which is the same trajectory in both."""
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
    "cartpole_mean": dict(workload="c1", K=1024, P=1, sample=False, sigma=2.0, lam=0.05),
    "cartpole_sampled": dict(workload="c1", K=256, P=16, sample=True, sigma=2.0, lam=0.05),
    "ur5_mean": dict(workload="ur5_script", K=256, P=1, sample=False, sigma=0.3, lam=0.05),
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
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iterations", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in args.shapes.split(","):
        s = SHAPES[name]
        w = workloads.build(s["workload"], dev, T=H)
        pm, c = w.model, w.problem["cfg"]
        U, K, P, M = pm.U, s["K"], s["P"], s["K"] * s["P"]
        u_max = float(np.max(c["u_max"]))
        cin = ops.PackedCostInputs(U, dev, lengthscales=[4.0 * u_max] * U) if w.problem["system"] == "cartpole" else None
        mp = ops.PackedMPPI(K, P, H, U, s["sigma"], s["lam"], u_max=u_max)
        x0 = w.x0_mean.reshape(-1).contiguous()
        a = torch.zeros(H, U, dtype=DT, device=dev)
        eps = torch.randn(H - 1, P, pm.G, dtype=DT, device=dev) if s["sample"] else None
        nz = ops.NoiseSpec(eps=eps, seed=1, call=0)
        traj, a_new = torch.empty(M, dtype=DT, device=dev), torch.empty(H, U, dtype=DT, device=dev)
        out_buf = (torch.empty(K, dtype=DT, device=dev), torch.empty(K, dtype=DT, device=dev), torch.empty(4, dtype=DT, device=dev))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        sig = torch.full((U,), s["sigma"], dtype=DT, device=dev)
        x0m = x0.reshape(1, -1).repeat(M, 1).contiguous()
        eps_full = None if eps is None else ops.NoiseSpec(eps=eps.repeat(1, K, 1).contiguous())

        def roll():
            return ops.mppi_rollout(pm, mp, w.cost, x0, a, cost_inputs=cin, noise=nz, particle_pred=s["sample"], traj_cost=traj, status=status)

        def update():
            return ops.mppi_update(mp, traj, a, noise=nz, a_new=a_new, out=out_buf, status=status)

        def fused():
            roll()
            return update()

        def composed():
            xi = torch.randn(H, K, U, dtype=DT, device=dev)
            xi[:, 0] = 0.0
            u = u_max * torch.tanh((a.unsqueeze(1) + sig * xi) / u_max)
            um = u.repeat_interleave(P, dim=1) if P > 1 else u
            states, _ = ops.rollout_open(pm, x0m, um[:H - 1].contiguous(), noise=eps_full, particle_pred=s["sample"])
            _, costs, _ = ops.cost_moments(w.cost, states, inputs=None if cin is None else um.contiguous(), cost_inputs=cin)
            S = costs.sum(0).reshape(K, P).mean(1)
            wts = torch.softmax(-(S - S.min()) / s["lam"], 0)
            return a + sig * torch.einsum("k,hku->hu", wts, xi), S

        cost_obj = (cf.Input_penalty(cf.Cart_pole_cost(c["cost_target"], c["cost_ls"], c["cost_angle_index"], c["cost_pos_index"]),
                                     lengthscales=[4.0 * u_max] * U)
                    if cin is not None else cf.Expected_saturated_distance_from_trajectory(w.problem["target_traj"], c["cost_ls"]))

        def control_step():
            return mppi.plan(pm, x0, a, cost_obj, K=K, P=P, iterations=args.iterations, sigma=s["sigma"], lam=s["lam"], u_max=u_max,
                             particle_pred=s["sample"], noise=nz)

        got, ref = fused(), composed()  # warm-up of both forms; the nominal is candidate 0 of both
        info = control_step()[1]
        torch.cuda.synchronize()
        nominal = [float(out_buf[0][0]), float(ref[1][0])]
        ms = dict(roll=[], update=[], fused=[], composed=[], step=[])
        for _ in range(args.blocks):
            ms["roll"].append(block_ms(roll, args.reps))
            ms["update"].append(block_ms(update, args.reps))
            ms["fused"].append(block_ms(fused, args.reps))
            ms["composed"].append(block_ms(composed, args.reps))
            ms["step"].append(block_ms(control_step, 1))
        out = dict(shape=name, N=w.problem["N"], G=pm.G, D=pm.D, H=H, K=K, P=P, status=int(status.item()), nominal_cost_fused_composed=nominal,
                   rollout_cost_ms=stat(ms["roll"]), update_ms=stat(ms["update"]), a_fused_iteration_ms=stat(ms["fused"]),
                   b_composed_iteration_ms=stat(ms["composed"]), control_step_ms=stat(ms["step"]), iterations=args.iterations,
                   plan_nominal_cost=[round(v, 6) for v in info["nominal_cost"]], plan_ess=[round(v, 2) for v in info["ess"]])
        out["ratio_b_over_a"] = round(out["b_composed_iteration_ms"][0] / out["a_fused_iteration_ms"][0], 2)
        out["fused_not_slower"] = out["a_fused_iteration_ms"][0] <= out["b_composed_iteration_ms"][0]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
