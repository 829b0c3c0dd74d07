"""Times the open-loop rollout: the fused mean chain (ops.rollout_open, M = 1) against the step-wise form it replaces, and the sampled
ensemble against the closed-loop forward launch at the same M and T.

    python tools/time_open_rollout.py [--blocks 7] [--reps 5] [--particles 400] [--runs 5] [--grad]

Events around the call, `reps` calls per block, median over the blocks.  Two step-wise figures: the RESTATED step loop
(the loop of MC_PILCO.rollout over Model_learning.get_next_state written out on the packed GPs: per step the feature map, one ops.posterior
launch per GP, the integration -- a lower bound of the class path, available at every shape) and, at the cart-pole shape, the class path
itself: MC_PILCO.rollout() on the drop-in object of workloads.dropin_c1 with fused_open_loop False (the code of the commit before the fused
kernel, line for line) and True, host tensor construction and the copy back included.  One JSON line per shape.

--grad: the gradient leg instead -- per shape (mean chain M = 1; sampled, M = --particles, cart-pole 400 / UR5 shape 200) the plain launch,
the recording launch (ops.rollout_open_diff, forward only), recording launch + reverse sweep (L = sum of the states), and torch autograd
through the restated step loop (forward + backward), which is what differentiating a rollout of given inputs took before.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcp_boot  # noqa: E402,F401

from mc_pilco_amd import ops, workloads  # noqa: E402

DT = torch.float64


def median_ms(fn, blocks, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def stepwise_mean(w, x0, u):
    c = w.problem["cfg"]
    ang, nang, vel, nvel, Ts = list(c["angle"]), list(c["not_angle"]), list(c["vel"]), list(c["not_vel"]), float(c["Ts"])
    T = u.shape[0] + 1
    traj = torch.zeros(T, x0.shape[1], dtype=DT, device=x0.device)
    traj[0:1] = x0
    for t in range(1, T):
        x = traj[t - 1:t]
        z = torch.cat([x[:, nang], torch.sin(x[:, ang]), torch.cos(x[:, ang]), u[t - 1:t]], 1)
        dv = torch.cat([ops.posterior(gp, z)[0].reshape(-1, 1) for gp in w.model.gps], 1)
        nxt = torch.zeros_like(x)
        nxt[:, vel] = x[:, vel] + dv
        nxt[:, nvel] = x[:, nvel] + Ts * x[:, vel] + Ts / 2 * dv
        traj[t:t + 1] = nxt
    return traj


def stepwise_diff(w, x0, u, eps):
    """The restated step loop with autograd (ops.posterior is differentiable), sampled when ``eps`` is given: forward + backward of sum(states)."""
    c = w.problem["cfg"]
    ang, nang, vel, nvel, Ts = list(c["angle"]), list(c["not_angle"]), list(c["vel"]), list(c["not_vel"]), float(c["Ts"])
    x0, u = x0.detach().requires_grad_(True), u.detach().requires_grad_(True)
    xs = [x0]
    for t in range(u.shape[0]):
        x = xs[-1]
        z = torch.cat([x[:, nang], torch.sin(x[:, ang]), torch.cos(x[:, ang]), u[t].expand(x.shape[0], -1)], 1)
        mv = [ops.posterior(gp, z) for gp in w.model.gps]
        dv = torch.cat([m.reshape(-1, 1) for m, _ in mv], 1)
        if eps is not None:
            dv = dv + torch.sqrt(torch.cat([v.reshape(-1, 1) for _, v in mv], 1)) * eps[t]
        nxt = torch.zeros_like(x)
        nxt[:, vel] = x[:, vel] + dv
        nxt[:, nvel] = x[:, nvel] + Ts * x[:, vel] + Ts / 2 * dv
        xs.append(nxt)
    torch.stack(xs).sum().backward()
    return x0.grad, u.grad


def grad_leg(args, dev):
    for name, T, M in (("c1", 150, args.particles), ("ur5_script", 200, max(1, args.particles // 2))):
        w = workloads.build(name, device=dev, M=M, T=T)
        torch.manual_seed(1)
        x1 = w.sample_x0(1)
        with torch.no_grad():
            u1 = ops.rollout_forward_raw(w.model, w.policy, ops.NoiseSpec(seed=1), x1, T, 0.0, False, need_jac=False)[1][:-1, 0:1].contiguous()
        out = dict(shape=name, N=w.problem["N"], G=w.model.G, D=w.model.D, T=T, M_sampled=M)
        for tag, x0, u, sample in (("mean_M1", x1, u1, False), ("sampled", x1.repeat(M, 1).contiguous(), u1.repeat(1, M, 1).contiguous(), True)):
            eps = torch.randn(T - 1, x0.shape[0], w.model.G, dtype=DT, device=dev) if sample else None
            nz = ops.NoiseSpec(eps=eps) if sample else None
            xg, ug = x0.clone().requires_grad_(True), u.clone().requires_grad_(True)

            def both():
                st, _ = ops.rollout_open_diff(w.model, xg, ug, noise=nz, particle_pred=sample)
                return torch.autograd.grad(st.sum(), [xg, ug])

            with torch.no_grad():
                out[tag + "_plain_ms"] = median_ms(lambda: ops.rollout_open(w.model, x0, u, noise=nz, particle_pred=sample), args.blocks, args.reps)
            out[tag + "_record_ms"] = median_ms(lambda: ops.rollout_open_diff(w.model, xg, ug, noise=nz, particle_pred=sample), args.blocks, args.reps)
            out[tag + "_record_and_sweep_ms"] = median_ms(both, args.blocks, args.reps)
            out[tag + "_autograd_step_loop_ms"] = median_ms(lambda: stepwise_diff(w, x0, u, eps), 3, 1)
            ga, gb = both(), stepwise_diff(w, x0, u, eps)
            out[tag + "_g_u_vs_step_loop_rel"] = float((ga[1] - gb[1]).abs().max() / gb[1].abs().max())
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--particles", type=int, default=400)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--grad", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.grad:
        return grad_leg(args, dev)
    for name, T in (("c1", 150), ("ur5_script", 200)):
        w = workloads.build(name, device=dev, M=args.particles, T=T)
        torch.manual_seed(1)
        x1 = w.sample_x0(1)
        with torch.no_grad():
            # inputs a policy would have produced: bounded, smooth enough to keep the state inside the data
            u = ops.rollout_forward_raw(w.model, w.policy, ops.NoiseSpec(seed=1), x1, T, 0.0, False, need_jac=False)[1][:-1, 0].contiguous()
            fused = median_ms(lambda: ops.rollout_open(w.model, x1, u), args.blocks, args.reps)
            step = median_ms(lambda: stepwise_mean(w, x1, u), max(3, args.blocks // 2), 1)
            gap = float((ops.rollout_open(w.model, x1, u)[0][:, 0] - stepwise_mean(w, x1, u)).abs().max())
            M = args.particles * args.runs
            xe = x1.repeat(M, 1).contiguous()
            lens = torch.as_tensor(np.repeat(np.linspace(T // 2, T, args.runs).astype(np.int32), args.particles)).to(dev)  # (on the device once)
            ens = median_ms(lambda: ops.rollout_open(w.model, xe, u, lengths=lens, noise=ops.NoiseSpec(seed=3), particle_pred=True), args.blocks, args.reps)
            full = median_ms(lambda: ops.rollout_open(w.model, xe, u, noise=ops.NoiseSpec(seed=3), particle_pred=True), args.blocks, args.reps)
            closed = median_ms(lambda: ops.rollout_forward_raw(w.model, w.policy, ops.NoiseSpec(seed=3), xe, T, 0.0, True, need_jac=False), args.blocks,
                               args.reps)
        cls = {}
        if name == "c1":  # the class path: MC_PILCO.rollout() on one recorded run of T samples
            obj, _ = workloads.dropin_c1(dev)
            with torch.no_grad():
                rec = ops.rollout_forward_raw(obj.model_learning.packed(), obj.control_policy.packed(), ops.NoiseSpec(seed=1), x1, T, 0.0, False,
                                              need_jac=False)
            obj.state_samples_history = [rec[0][:, 0].cpu().numpy()]
            obj.input_samples_history = [rec[1][:, 0].cpu().numpy()]
            with torch.no_grad():
                obj.fused_open_loop = True
                cls["class_rollout_fused_ms"] = median_ms(lambda: obj.rollout(0), args.blocks, args.reps)
                a = obj.rollout(0)
                obj.fused_open_loop = False
                cls["class_rollout_stepwise_ms"] = median_ms(lambda: obj.rollout(0), max(3, args.blocks // 2), 1)
                cls["class_fused_vs_stepwise_max_abs"] = float(np.abs(a - obj.rollout(0)).max())
        print(json.dumps(dict(cls, shape=name, N=w.problem["N"], G=w.model.G, D=w.model.D, T=T, mean_fused_ms=fused, mean_restated_step_loop_ms=step,
                              mean_fused_us_per_step=1e3 * fused[0] / (T - 1), fused_vs_restated_max_abs=gap, ensemble_M=M,
                              ensemble_ragged_ms=ens, ensemble_full_length_ms=full, closed_loop_fwd_same_M_T_ms=closed)), flush=True)


if __name__ == "__main__":
    main()
