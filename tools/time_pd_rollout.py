"""Times one optimizer step under the trainable PD controller through the class path -- MC_PILCO.apply_policy + a weighted-sum cost +
backward -- fused (ops.rollout_pd: one launch, one sweep) and with ``fused_feedback = False`` (the step loop on get_next_state with autograd
through it: the code before the fused form, line for line), in the same run.

    python tools/time_pd_rollout.py [--blocks 5] [--reps 3] [--step-blocks 3] [--pms]

Shapes: the UR5 script shape (6 GPs, D = 24, N = 400, M = 200, T = 200) and a two-joint arm (2 GPs, D = 8, N = 300, M = 400, T = 150).
Events around the step, `reps` steps per block, median over the blocks; the step path runs one step per block.  Also
counts the device launches of one step of either path (torch profiler), times the two fused launches alone, and -- for comparison --
``mcp_rollout_fwd`` with the shape's Sum_of_gaussians policy at the same M and T where the workload table has one.  One JSON line per shape.

``--pms``: the same two steps through MC_PILCO4PMS.apply_policy (every joint's position measured with noise, velocities by backward
differences through the first-order filter, fc = 0.3): the fused launch and sweep with the measurement model (ops.rollout_pd(meas=...))
against ``fused_feedback = False`` -- the step loop with the filter as torch ops -- in the same run; the step and launch counts only, plus
``fused_not_slower`` (the medians compared; the tool fails when it is false).
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcp_boot  # noqa: E402,F401

from mc_pilco_amd import ops, workloads  # noqa: E402
from mc_pilco_amd import synthetic as sy  # noqa: E402
from mc_pilco_amd.model_learning import Model_learning as ML  # noqa: E402
from mc_pilco_amd.policy_learning import MC_PILCO, Cost_function, Policy  # noqa: E402

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


def launches(fn):
    """Device kernels and copies one call enqueues (torch profiler); None where the profiler gives no device events."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
    return n or None


def rbf_dict(D, ls, sigma_n, dev):
    return dict(active_dims=np.arange(D), lengthscales_init=np.asarray(ls, dtype=float), flg_train_lengthscales=True, lambda_init=np.ones(1),
                flg_train_lambda=False, sigma_n_init=sigma_n * np.ones(1), sigma_n_num=None, flg_train_sigma_n=True, dtype=DT, device=dev)


def arm2_data(n, Ts, seed=3):
    rs = np.random.RandomState(seed)
    tt = Ts * np.arange(n + 1).reshape(-1, 1)
    u = 0.8 * np.sin(2 * np.pi * (0.2 + 0.5 * rs.rand(1, 2)) * tt + 6.28 * rs.rand(1, 2)) + 0.4 * np.sin(2 * np.pi * (1.0 + rs.rand(1, 2)) * tt)
    x = np.zeros((n + 1, 4))
    x[0] = [0.3, -0.2, 0.0, 0.0]
    for i in range(n):
        q, qd = x[i, :2], x[i, 2:]
        qdd = -4.0 * np.sin(q) - 0.4 * qd + 3.0 * u[i]
        x[i + 1, 2:] = qd + Ts * qdd
        x[i + 1, :2] = q + Ts * qd + 0.5 * Ts * Ts * qdd
    return x + 1e-3 * rs.randn(n + 1, 4), u


def build_object(shape, dev, pms=False):
    if shape == "ur5_script":
        c, N, M, T = sy.UR5, 400, 200, 200
        rolls = sy.ur5_rollouts(n_roll=2, seed=1)
        x = np.concatenate([r[0] for r in rolls], 0)[: N + 1]
        u = np.concatenate([r[1] for r in rolls], 0)[: N + 1]
        ls, sig = c["lengthscales"], c["sigma_n"]
        target = sy.ur5_target_traj(T=T, Ts=c["Ts"])
        u_max = 1.0
    else:
        c = dict(S=4, U=2, G=2, D=8, Ts=0.05, angle=[0, 1], not_angle=[2, 3], vel=[2, 3], not_vel=[0, 1])
        N, M, T = 300, 400, 150
        x, u = arm2_data(N, c["Ts"])
        ls, sig = 2.0 * np.ones(8), 0.05
        t = c["Ts"] * np.arange(T).reshape(-1, 1)
        om = np.array([0.6, 0.9]).reshape(1, -1)
        target = np.concatenate([0.4 * np.sin(om * t), 0.4 * om * np.cos(om * t)], 1)
        u_max = 1.5
    S, U, G, D = c["S"], c["U"], c["G"], c["D"]
    with contextlib.redirect_stdout(io.StringIO()):
        ml = ML.Speed_Model_learning_RBF_angle_state(num_gp=G, init_dict_list=[rbf_dict(D, ls, sig, dev)] * G, T_sampling=c["Ts"],
                                                     angle_indeces=c["angle"], not_angle_indeces=c["not_angle"], vel_indeces=c["vel"],
                                                     not_vel_indeces=c["not_vel"], dtype=DT, device=dev)
        ml.add_data(x, u)
        with torch.no_grad():
            for g in range(G):
                ml.pretrain_gp(g)
        ml.set_eval_mode()
        tg = torch.as_tensor(target, dtype=DT).to(dev).contiguous()
        ppar = dict(state_dim=S, input_dim=U, sqrt_Kp_gains=1.0 * np.ones(U), sqrt_Kd_gains=0.5 * np.ones(U), target_traj=tg, flg_squash=True,
                    u_max=u_max, flg_trainable=True, dtype=DT, device=dev)
        common = dict(T_sampling=c["Ts"], state_dim=S, input_dim=U, f_sim=lambda y, t, u: None, f_model_learning=lambda **kw: ml,
                      model_learning_par={}, f_rand_exploration_policy=Policy.Random_exploration,
                      rand_exploration_policy_par=dict(state_dim=S, input_dim=U, u_max=1.0, dtype=DT),
                      f_control_policy=Policy.PD_controller, control_policy_par=ppar,
                      f_cost_function=Cost_function.Expected_saturated_distance,
                      cost_function_par=dict(target_state=torch.zeros(S, dtype=DT, device=dev), lengthscales=torch.ones(S, dtype=DT, device=dev),
                                             active_dims=np.arange(S)),
                      log_path=None, dtype=DT, device=dev)
        if pms:  # positions 0..U-1 measured with 1e-3 of noise, their velocities S/2.. derived
            obj = MC_PILCO.MC_PILCO4PMS(pos_indeces=list(range(U)), vel_indeces=list(range(S // 2, S // 2 + U)), std_meas_noise=1e-3 * np.ones(S),
                                        filtering_dict={"fc": 0.3}, **common)
        else:
            obj = MC_PILCO.MC_PILCO(**common)
    sim = dict(particles_initial_state_mean=tg[0].clone(), particles_initial_state_var=1e-4 * torch.ones(S, dtype=DT, device=dev),
               flg_particles_init_uniform=False, particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
               num_particles=M, T_control=T)
    return obj, sim, N, M, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-blocks", type=int, default=3)
    ap.add_argument("--shapes", default="ur5_script,arm2")
    ap.add_argument("--pms", action="store_true", help="time MC_PILCO4PMS (the PD law on a simulated measurement) instead of MC_PILCO")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        obj, sim, N, M, T = build_object(shape, dev, pms=args.pms)
        pol, pm = obj.control_policy, obj.model_learning.packed()
        gen = torch.Generator(device=dev).manual_seed(1)
        w = torch.randn(T, M, pm.S, dtype=DT, device=dev, generator=gen)
        wu = torch.randn(T, M, pm.U, dtype=DT, device=dev, generator=gen)

        def step():
            for q in pol.parameters():
                q.grad = None
            st, inp = obj.apply_policy(**sim)
            ((w * st).sum() + (wu * inp).sum()).backward()
            return st

        out = dict(shape=shape, N=N, G=pm.G, D=pm.D, M=M, T=T)
        obj.fused_feedback = True
        out["fused_step_ms"] = median_ms(step, args.blocks, args.reps)
        assert obj.last_feedback_fused and int(obj.last_status.item()) == 0
        out["fused_launches"] = launches(step)
        if args.pms:
            out["class"] = "MC_PILCO4PMS"
            obj.fused_feedback = False
            out["step_path_step_ms"] = median_ms(step, args.step_blocks, 1)
            assert not obj.last_feedback_fused
            out["step_path_launches"] = launches(step)
            out["fused_not_slower"] = out["fused_step_ms"][0] <= out["step_path_step_ms"][0]  # medians of the same run
            print(json.dumps(out), flush=True)
            assert out["fused_not_slower"], "the fused step is slower than the step loop timed in the same run"
            continue
        x0 = obj.sample_initial_particles(sim["particles_initial_state_mean"], sim["particles_initial_state_var"], False, None, None, False, M)
        with torch.no_grad():
            out["fused_fwd_plain_ms"] = median_ms(lambda: ops.rollout_pd(pm, pol.packed(), ops.NoiseSpec(seed=1, call=1), x0, T), args.blocks, args.reps)
        out["fused_fwd_record_ms"] = median_ms(lambda: ops.rollout_pd(pm, pol.packed(), ops.NoiseSpec(seed=1, call=1), x0, T), args.blocks, args.reps)

        def fwd_bwd():
            st, inp, _ = ops.rollout_pd(pm, pol.packed(), ops.NoiseSpec(seed=1, call=1), x0, T)
            torch.autograd.grad((w * st).sum() + (wu * inp).sum(), [pol.sqrt_Kp_gains, pol.sqrt_Kd_gains])

        out["fused_fwd_record_and_sweep_ms"] = median_ms(fwd_bwd, args.blocks, args.reps)
        obj.fused_feedback = False
        out["step_path_step_ms"] = median_ms(step, args.step_blocks, 1)
        assert not obj.last_feedback_fused
        out["step_path_launches"] = launches(step)
        if shape == "ur5_script":  # the closed-loop forward launch with the shape's Sum_of_gaussians policy at the same M, T
            wl = workloads.build(shape, device=dev, M=M, T=T)
            with torch.no_grad():
                out["mcp_rollout_fwd_same_M_T_ms"] = median_ms(
                    lambda: ops.rollout_forward_raw(wl.model, wl.policy, ops.NoiseSpec(seed=3), x0, T, 0.0, True, need_jac=True), args.blocks, args.reps)
        else:
            wl = workloads.build("c1", device=dev, M=M, T=T)  # (no arm workload in the table: the cart-pole shape, N = 300, same M and T)
            with torch.no_grad():
                out["mcp_rollout_fwd_cartpole_same_M_T_ms"] = median_ms(
                    lambda: ops.rollout_forward_raw(wl.model, wl.policy, ops.NoiseSpec(seed=3), wl.sample_x0(M), T, 0.0, True, need_jac=True),
                    args.blocks, args.reps)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
