"""Times one optimizer step under ``Policy.PID_controller`` -- the PD law with a clamped integral of the position error -- through the class
path (MC_PILCO.apply_policy + a weighted-sum cost + backward) on three legs in the same run:

    a  fused                  ops.rollout_pd on the integral entries (mcp_rollout_pid): one launch, one sweep
    b  fused_feedback = False, fused_step = True    the same object on the step loop with one model launch per step: the best path for this
                              law before the integral form, the yardstick
    c  PD_controller, fused   the same gains and target without the integral (mcp_rollout_pd): what the term costs

    python tools/time_pid.py [--blocks 5] [--reps 3] [--step-blocks 3] [--shapes ur5_script,arm2] [--i-max 0.05]

Shapes, objects and the timing method are tools/time_pd_rollout.py's (the UR5 script shape: 6 GPs, D = 24, N = 400, M = 200, T = 200; a
two-joint arm: 2 GPs, D = 8, N = 300, M = 400, T = 150); the gains and the target are those of the PD controller the object was built with,
sqrt_ki = 0.7, dt = the object's T_sampling.  Legs a and c alternate block by block, so a drift of the machine reaches both.  Also times,
for a and c, the recording launch and recording + sweep alone (the sweep: their difference).  One JSON line per shape;
``fused_faster_than_fused_step``: the medians of legs a and b compared (the tool fails when it is false); ``record_ratio`` /
``sweep_ratio``: leg a over leg c, the figures DESIGN 4.10's rule of 1.5 is about."""
import argparse
import json

import numpy as np
import torch

from time_pd_rollout import DT, build_object, median_ms  # (puts the repository on sys.path and registers the package)

from mc_pilco_amd import ops  # noqa: E402
from mc_pilco_amd.policy_learning import Policy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-blocks", type=int, default=3)
    ap.add_argument("--shapes", default="ur5_script,arm2")
    ap.add_argument("--i-max", type=float, default=0.05)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    slower = []
    for shape in args.shapes.split(","):
        obj, sim, N, M, T = build_object(shape, dev)
        pm = obj.model_learning.packed()
        gen = torch.Generator(device=dev).manual_seed(1)
        w = torch.randn(T, M, pm.S, dtype=DT, device=dev, generator=gen)
        wu = torch.randn(T, M, pm.U, dtype=DT, device=dev, generator=gen)
        x0 = obj.sample_initial_particles(sim["particles_initial_state_mean"], sim["particles_initial_state_var"], False, None, None, False, M)
        out = dict(shape=shape, N=N, G=pm.G, D=pm.D, M=M, T=T, i_max=args.i_max)
        pd = obj.control_policy
        pid = Policy.PID_controller(state_dim=pm.S, input_dim=pm.U, sqrt_Kp_gains=pd.sqrt_Kp_gains.detach().cpu().numpy(),
                                    sqrt_Kd_gains=pd.sqrt_Kd_gains.detach().cpu().numpy(), sqrt_Ki_gains=0.7 * np.ones(pm.U),
                                    T_sampling=float(obj.T_sampling), i_max=args.i_max, target_traj=pd.target_traj, flg_squash=True, u_max=pd.u_max,
                                    flg_trainable=True, dtype=DT, device=dev)
        pols = dict(a=pid, c=pd)

        def step():
            for q in obj.control_policy.parameters():
                q.grad = None
            st, inp = obj.apply_policy(**sim)
            ((w * st).sum() + (wu * inp).sum()).backward()
            return st

        def one_block(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                step()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / reps

        obj.fused_feedback = True
        for leg in ("a", "c"):  # warm-up: every form's code objects, and its status
            obj.control_policy = pols[leg]
            step()
            assert obj.last_feedback_fused and int(obj.last_status.item()) == 0, leg
            step()
        torch.cuda.synchronize()
        integ = pid.packed().integ
        out["clamped_share"] = round(float((integ.abs() == args.i_max).to(DT).mean()), 3)
        ms = dict(a=[], c=[])
        for _ in range(args.blocks):  # a and c alternate inside every block
            for leg in ("a", "c"):
                obj.control_policy = pols[leg]
                ms[leg].append(one_block(args.reps))
        stat = lambda v: [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]
        out["a_fused_step_ms"], out["c_pd_fused_step_ms"] = stat(ms["a"]), stat(ms["c"])

        for leg in ("a", "c"):  # the launches alone: recording, recording + sweep
            pol = pols[leg]
            roll = lambda: ops.rollout_pd(pm, pol.packed(), ops.NoiseSpec(seed=1, call=1), x0, T)
            params = [q for q in pol.parameters() if q.requires_grad]
            out[leg + "_fwd_record_ms"] = median_ms(roll, args.blocks, args.reps)

            def fwd_bwd():
                st, inp, _ = roll()
                torch.autograd.grad((w * st).sum() + (wu * inp).sum(), params)

            out[leg + "_fwd_record_and_sweep_ms"] = median_ms(fwd_bwd, args.blocks, args.reps)
            out[leg + "_sweep_ms"] = round(out[leg + "_fwd_record_and_sweep_ms"][0] - out[leg + "_fwd_record_ms"][0], 4)
        out["record_ratio"] = round(out["a_fwd_record_ms"][0] / out["c_fwd_record_ms"][0], 4)
        out["sweep_ratio"] = round(out["a_sweep_ms"] / out["c_sweep_ms"], 4)

        obj.control_policy = pid
        obj.fused_feedback, obj.fused_step = False, True
        out["b_fused_step_path_step_ms"] = median_ms(step, args.step_blocks, 1)
        assert not obj.last_feedback_fused and obj.last_step_fused
        out["ratio_b_over_a"] = out["b_fused_step_path_step_ms"][0] / out["a_fused_step_ms"][0]
        out["a_minus_c_ms"] = round(out["a_fused_step_ms"][0] - out["c_pd_fused_step_ms"][0], 4)
        out["c_spread_ms"] = round(out["c_pd_fused_step_ms"][2] - out["c_pd_fused_step_ms"][1], 4)
        out["fused_faster_than_fused_step"] = out["a_fused_step_ms"][0] < out["b_fused_step_path_step_ms"][0]
        print(json.dumps(out), flush=True)
        slower += [] if out["fused_faster_than_fused_step"] else [shape]
    assert not slower, "the fused step is not faster than the fused-step loop timed in the same run: " + ", ".join(slower)


if __name__ == "__main__":
    main()
