"""Times ``Policy.MLP_policy(hidden_sizes=[32], history=H)`` -- the network that reads the last H rows -- on the shapes and objects of
tools/time_mlp_rollout.py (a two-joint arm: 2 GPs, D = 8, N = 300, M = 400, T = 150, the model's feature lists, P0 = 6; the UR5 script shape:
6 GPs, D = 24, N = 400, M = 200, T = 200, positions-only features, P0 = 6), every leg of a group timed in ALTERNATING blocks of the same run:

    step      one optimizer step through the class path (apply_policy + a weighted-sum cost + backward), fused, for H = 1, 2, 4; and for
              H = 2, 4 the same object on ``fused_feedback = False`` with ``fused_step = True`` -- a stateful module on the step loop with one
              model launch per step, the best path such a policy has without the fused form -- with the ratio
    launch    ops.rollout_mlp alone for H = 1, 2, 4: the plain launch, the recording launch, recording + sweep; the sweep alone is the
              difference of the last two

    python tools/time_mlp_hist.py [--blocks 9] [--reps 3] [--shapes arm2,ur5_script] [--only-h1 [--pms]]

One JSON line per shape: medians [min, max] in ms.  ``--only-h1``: the H = 1 legs alone, built WITHOUT the ``history`` keyword -- the form of
this tool that also runs on a tree from before the keyword, for the comparison of the unchanged kernels across two commits.  ``--pms``
(with ``--only-h1`` alone: a policy with memory has no fused form on a simulated measurement): those legs through MC_PILCO4PMS.  The tool
fails when a fused step with memory is not faster than its step loop.
"""
import argparse
import json

import numpy as np
import torch

from time_pd_rollout import DT, build_object  # (puts the repository on sys.path and registers the package)

from mc_pilco_amd import ops  # noqa: E402
from mc_pilco_amd.policy_learning import Policy  # noqa: E402


def alternating_ms(legs, blocks, reps):
    """{name: (median, min, max)} of the callables ``legs``, one block of ``reps`` calls each in turn, ``blocks`` times over."""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(blocks):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / reps)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="arm2,ur5_script")
    ap.add_argument("--hidden", default="32")
    ap.add_argument("--pms", action="store_true")
    ap.add_argument("--only-h1", action="store_true")
    args = ap.parse_args()
    if args.pms and not args.only_h1:
        ap.error("--pms needs --only-h1: a policy with memory has no fused form on a simulated measurement")
    dev = torch.device("cuda", 0)
    hidden = [int(h) for h in args.hidden.split(",")]
    depths = (1,) if args.only_h1 else (1, 2, 4)
    slower = []
    for shape in args.shapes.split(","):
        obj, sim, N, M, T = build_object(shape, dev, pms=args.pms)
        pm = obj._measured_model() if args.pms else obj.model_learning.packed()
        gen = torch.Generator(device=dev).manual_seed(1)
        w = torch.randn(T, M, pm.S, dtype=DT, device=dev, generator=gen)
        wu = torch.randn(T, M, pm.U, dtype=DT, device=dev, generator=gen)
        x0 = obj.sample_initial_particles(sim["particles_initial_state_mean"], sim["particles_initial_state_var"], False, None, None, False, M)
        meas = lambda: None
        if args.pms:
            from scipy import signal

            b, a = signal.butter(1, obj.filtering_dict["fc"])
            meas = lambda: obj._meas_spec(b, a, None)
        mdl, u_max = obj.model_learning, obj.control_policy.u_max
        if shape == "ur5_script":  # positions only: what the controller of a partially measurable arm is given
            lists = dict(angle_indices=None, non_angle_indices=list(range(pm.S // 2)))
        else:
            lists = dict(angle_indices=[int(i) for i in mdl.angle_indeces], non_angle_indices=[int(i) for i in mdl.not_angle_indeces])
        pols = {}
        for H in depths:
            torch.manual_seed(2)
            kw = {} if H == 1 else dict(history=H)
            pols[H] = Policy.MLP_policy(state_dim=pm.S, input_dim=pm.U, hidden_sizes=hidden, u_max=u_max, flg_squash=True, dtype=DT, device=dev, **lists, **kw)
        out = dict(shape=shape, cls="MC_PILCO4PMS" if args.pms else "MC_PILCO", N=N, G=pm.G, D=pm.D, M=M, T=T, hidden=hidden,
                   feature_dim={H: p.feature_dim for H, p in pols.items()})

        def step_of(H, fused):
            def step():
                obj.control_policy, obj.fused_feedback, obj.fused_step = pols[H], fused, True
                for q in pols[H].parameters():
                    q.grad = None
                st, inp = obj.apply_policy(**sim)
                ((w * st).sum() + (wu * inp).sum()).backward()
                assert obj.last_feedback_fused is fused
            return step

        legs = {"fused_H%d" % H: step_of(H, True) for H in depths}
        legs.update({"step_loop_H%d" % H: step_of(H, False) for H in depths if H > 1})
        out["step_ms"] = alternating_ms(legs, args.blocks, 1)
        for H in depths:
            if H > 1:
                r = out["step_ms"]["step_loop_H%d" % H][0] / out["step_ms"]["fused_H%d" % H][0]
                out["ratio_step_loop_over_fused_H%d" % H] = r
                slower += [] if r > 1.0 else ["%s H=%d" % (shape, H)]

        def roll_of(H):
            return lambda: ops.rollout_mlp(pm, pols[H].packed(), ops.NoiseSpec(seed=1, call=1), x0, T, meas=meas())

        def plain_of(H):
            def plain():
                with torch.no_grad():
                    roll_of(H)()
            return plain

        def sweep_of(H):
            def fwd_bwd():
                st, inp, _ = roll_of(H)()
                torch.autograd.grad((w * st).sum() + (wu * inp).sum(), pols[H].mlp_parameters())
            return fwd_bwd

        out["fwd_plain_ms"] = alternating_ms({"H%d" % H: plain_of(H) for H in depths}, args.blocks, args.reps)
        out["fwd_record_ms"] = alternating_ms({"H%d" % H: roll_of(H) for H in depths}, args.blocks, args.reps)
        out["fwd_record_and_sweep_ms"] = alternating_ms({"H%d" % H: sweep_of(H) for H in depths}, args.blocks, args.reps)
        out["sweep_ms"] = {k: out["fwd_record_and_sweep_ms"][k][0] - out["fwd_record_ms"][k][0] for k in out["fwd_record_ms"]}
        print(json.dumps(out), flush=True)
    assert not slower, "the fused step with memory is not faster than its step loop timed in the same run: " + ", ".join(slower)


if __name__ == "__main__":
    main()
