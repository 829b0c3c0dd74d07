"""Times one optimizer step under ``Policy.TV_linear_controller`` -- a feedforward sequence plus time-varying dense linear feedback around
the target -- through the class path (apply_policy + a weighted-sum cost + backward) on three legs in the same run:

    a  fused                  ops.rollout_tvl (mcp_rollout_tvl): one launch, one sweep with a partial of the gradient per row
    b  fused_feedback = False, fused_step = True    the same object on the step loop with one model launch per step: the best path this
                              policy has without the fused form, the yardstick
    c  PD_controller, fused   the PD twin the law was built from (mcp_rollout_pd): what the dense rows cost

    python tools/time_tvl.py [--blocks 5] [--reps 3] [--step-blocks 3] [--shapes ur5_script,arm2] [--pms]

Shapes, objects and the timing method are tools/time_pd_rollout.py's (the UR5 script shape: 6 GPs, D = 24, N = 400, M = 200, T = 200; a
two-joint arm: 2 GPs, D = 8, N = 300, M = 400, T = 150); ``--pms``: MC_PILCO4PMS, the law on the simulated measurement.  The law is
``from_pd`` of the object's PD controller plus 0.05 randn on every gain entry and a 0.1 randn feedforward, so the dense dot and the
squashing work on values of the PD twin's size.  Legs a and c alternate block by block, so a drift of the machine reaches both.  Also
times, for a and c, the recording launch alone (apply_policy with gradients enabled) and recording + sweep (the step); the sweep is their
difference.  One JSON line per shape; ``fused_faster_than_fused_step``: the medians of legs a and b compared (reported, not asserted: the
PD twin does not reliably beat the step loop at the UR5 shape either, profiles/NOTES.md part AC); ``record_ratio`` / ``sweep_ratio``: leg
a over leg c, the figures DESIGN 4.10's rule of 1.5 is about."""
import argparse
import json

import numpy as np
import torch

from time_pd_rollout import DT, build_object, median_ms  # (puts the repository on sys.path and registers the package)

from mc_pilco_amd.policy_learning import Policy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-blocks", type=int, default=3)
    ap.add_argument("--shapes", default="ur5_script,arm2")
    ap.add_argument("--pms", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        obj, sim, N, M, T = build_object(shape, dev, pms=args.pms)
        pm = obj.model_learning.packed()
        gen = torch.Generator(device=dev).manual_seed(1)
        w = torch.randn(T, M, pm.S, dtype=DT, device=dev, generator=gen)
        wu = torch.randn(T, M, pm.U, dtype=DT, device=dev, generator=gen)
        out = dict(shape=shape, pms=args.pms, N=N, G=pm.G, D=pm.D, M=M, T=T)
        pd = obj.control_policy
        tvl = Policy.TV_linear_controller.from_pd(pd, T)
        with torch.no_grad():
            tvl.gain.add_(0.05 * torch.randn(tvl.gain.shape, dtype=DT, device=dev, generator=gen))
            tvl.ff.add_(0.1 * torch.randn(tvl.ff.shape, dtype=DT, device=dev, generator=gen))
        pols = dict(a=tvl, c=pd)

        def roll():
            return obj.apply_policy(**sim)

        def step():
            for q in obj.control_policy.parameters():
                q.grad = None
            st, inp = roll()
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
        ms = dict(a=[], c=[])
        for _ in range(args.blocks):  # a and c alternate inside every block
            for leg in ("a", "c"):
                obj.control_policy = pols[leg]
                ms[leg].append(one_block(args.reps))
        stat = lambda v: [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]
        out["a_fused_step_ms"], out["c_pd_fused_step_ms"] = stat(ms["a"]), stat(ms["c"])

        for leg in ("a", "c"):  # the launches alone: recording, recording + sweep
            obj.control_policy = pols[leg]
            out[leg + "_fwd_record_ms"] = [round(v, 4) for v in median_ms(roll, args.blocks, args.reps)]
            out[leg + "_fwd_record_and_sweep_ms"] = [round(v, 4) for v in median_ms(step, args.blocks, args.reps)]
            out[leg + "_sweep_ms"] = round(out[leg + "_fwd_record_and_sweep_ms"][0] - out[leg + "_fwd_record_ms"][0], 4)
        out["record_ratio"] = round(out["a_fwd_record_ms"][0] / out["c_fwd_record_ms"][0], 4)
        out["sweep_ratio"] = round(out["a_sweep_ms"] / out["c_sweep_ms"], 4)

        obj.control_policy = tvl
        obj.fused_feedback, obj.fused_step = False, True
        out["b_fused_step_path_step_ms"] = [round(v, 4) for v in median_ms(step, args.step_blocks, 1)]
        assert not obj.last_feedback_fused
        out["b_ran_the_fused_model_step"] = bool(obj.last_step_fused)
        out["ratio_b_over_a"] = round(out["b_fused_step_path_step_ms"][0] / out["a_fused_step_ms"][0], 4)
        out["a_minus_c_ms"] = round(out["a_fused_step_ms"][0] - out["c_pd_fused_step_ms"][0], 4)
        out["c_spread_ms"] = round(out["c_pd_fused_step_ms"][2] - out["c_pd_fused_step_ms"][1], 4)
        out["fused_faster_than_fused_step"] = out["a_fused_step_ms"][0] < out["b_fused_step_path_step_ms"][0]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
