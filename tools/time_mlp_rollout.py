"""Times one optimizer step under ``Policy.MLP_policy(hidden_sizes=[32])`` through the class path -- MC_PILCO.apply_policy + a weighted-sum
cost + backward -- on three legs in the same run, and counts the device launches of each:

    1  fused                  ops.rollout_mlp: one launch, one sweep
    2  fused_feedback = False, fused_step = True    the step loop with one model launch per step: the best path before the fused form
    3  both off               the step loop on get_next_state

    python tools/time_mlp_rollout.py [--blocks 5] [--reps 3] [--step-blocks 3] [--shapes ur5_script,arm2] [--pms]

Shapes, objects and the timing method are tools/time_pd_rollout.py's (the UR5 script shape: 6 GPs, D = 24, N = 400, M = 200, T = 200; a
two-joint arm: 2 GPs, D = 8, N = 300, M = 400, T = 150).  Also times the plain launch, the recording launch and recording + sweep alone, and --
as context, on the same objects in the same run -- the same three under the trainable PD controller (ops.rollout_pd) and its fused step.
One JSON line per shape; ``fused_faster_than_fused_step``: the medians of legs 1 and 2 compared (the tool fails when it is false).

``--pms``: legs 1 and 2 through MC_PILCO4PMS.apply_policy (tools/time_pd_rollout.py's object: every joint's position measured with noise,
velocities by backward differences through the first-order filter, fc = 0.3) -- the fused launch and sweep with the measurement model
(ops.rollout_mlp(meas=...)) against ``fused_feedback = False`` with ``fused_step = True``, the best path before the measured form, in the same
run, with the launch counts; the plain / recording / recording + sweep times are those of the measured launches.  Leg 3 is left out.
"""
import argparse
import json

import torch

from time_pd_rollout import DT, build_object, launches, median_ms  # (puts the repository on sys.path and registers the package)

from mc_pilco_amd import ops  # noqa: E402
from mc_pilco_amd.policy_learning import Policy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-blocks", type=int, default=3)
    ap.add_argument("--shapes", default="ur5_script,arm2")
    ap.add_argument("--hidden", default="32")
    ap.add_argument("--pms", action="store_true", help="time MC_PILCO4PMS (the network on a simulated measurement) instead of MC_PILCO")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hidden = [int(h) for h in args.hidden.split(",")]
    slower = []
    for shape in args.shapes.split(","):
        obj, sim, N, M, T = build_object(shape, dev, pms=args.pms)
        pm = obj._measured_model() if args.pms else obj.model_learning.packed()
        gen = torch.Generator(device=dev).manual_seed(1)
        w = torch.randn(T, M, pm.S, dtype=DT, device=dev, generator=gen)
        wu = torch.randn(T, M, pm.U, dtype=DT, device=dev, generator=gen)
        x0 = obj.sample_initial_particles(sim["particles_initial_state_mean"], sim["particles_initial_state_var"], False, None, None, False, M)
        out = dict(shape=shape, N=N, G=pm.G, D=pm.D, M=M, T=T, hidden=hidden)
        meas = lambda: None  # (a fresh MeasSpec per launch: the launch leaves its measured states there)
        if args.pms:
            from scipy import signal

            out["class"] = "MC_PILCO4PMS"
            b, a = signal.butter(1, obj.filtering_dict["fc"])
            meas = lambda: obj._meas_spec(b, a, None)

        def step():
            for q in obj.control_policy.parameters():
                q.grad = None
            st, inp = obj.apply_policy(**sim)
            ((w * st).sum() + (wu * inp).sum()).backward()
            return st

        def op_times(tag, roll, params):
            with torch.no_grad():
                out[tag + "_fwd_plain_ms"] = median_ms(roll, args.blocks, args.reps)
            out[tag + "_fwd_record_ms"] = median_ms(roll, args.blocks, args.reps)

            def fwd_bwd():
                st, inp, _ = roll()
                torch.autograd.grad((w * st).sum() + (wu * inp).sum(), params)

            out[tag + "_fwd_record_and_sweep_ms"] = median_ms(fwd_bwd, args.blocks, args.reps)

        # context: the PD controller the object was built with
        pd = obj.control_policy
        obj.fused_feedback = True
        out["pd_fused_step_ms"] = median_ms(step, args.blocks, args.reps)
        assert obj.last_feedback_fused
        op_times("pd", lambda: ops.rollout_pd(pm, pd.packed(), ops.NoiseSpec(seed=1, call=1), x0, T, meas=meas()), [pd.sqrt_Kp_gains, pd.sqrt_Kd_gains])

        torch.manual_seed(2)
        mdl = obj.model_learning
        pol = Policy.MLP_policy(state_dim=pm.S, input_dim=pm.U, hidden_sizes=hidden, angle_indices=[int(i) for i in mdl.angle_indeces],
                                non_angle_indices=[int(i) for i in mdl.not_angle_indeces], u_max=pd.u_max, flg_squash=True, dtype=DT, device=dev)
        obj.control_policy = pol
        out["n_param"] = pol.packed().n_param
        out["fused_step_ms"] = median_ms(step, args.blocks, args.reps)
        assert obj.last_feedback_fused and int(obj.last_status.item()) == 0
        out["fused_launches"] = launches(step)
        op_times("fused", lambda: ops.rollout_mlp(pm, pol.packed(), ops.NoiseSpec(seed=1, call=1), x0, T, meas=meas()), pol.mlp_parameters())
        obj.fused_feedback, obj.fused_step = False, True
        out["fused_step_path_step_ms"] = median_ms(step, args.step_blocks, 1)
        assert not obj.last_feedback_fused and obj.last_step_fused
        out["fused_step_path_launches"] = launches(step)
        if not args.pms:
            obj.fused_step = False
            out["step_path_step_ms"] = median_ms(step, args.step_blocks, 1)
            assert not obj.last_feedback_fused and not obj.last_step_fused
            out["step_path_launches"] = launches(step)
        out["ratio_fused_step_over_fused"] = out["fused_step_path_step_ms"][0] / out["fused_step_ms"][0]
        out["fused_faster_than_fused_step"] = out["fused_step_ms"][0] < out["fused_step_path_step_ms"][0]
        print(json.dumps(out), flush=True)
        slower += [] if out["fused_faster_than_fused_step"] else [shape]
    assert not slower, "the fused step is not faster than the fused-step loop timed in the same run: " + ", ".join(slower)


if __name__ == "__main__":
    main()
