"""Times what the target-trajectory features cost in the fused tanh-MLP rollout: the recording launch plus the sweep (ops.rollout_mlp +
backward) on the UR5 launch script's workload (workloads "ur5_script": 6 GPs, D = 24, SE + polynomial(1), N = 400, M = 200, T = 200), hidden
(64, 64), in two forms of the same call, alternating inside every block:

    none     f = x, P = 12: a policy without a target (mcp_rollout_mlp + mcp_rollout_mlp_bwd, the code before the tracking form)
    track    f = [x, x*_t - x], P = 24: Policy.MLP_policy(target_traj=...) with all twelve errors (mcp_rollout_mlp_track + its sweep)

    python tools/time_mlp_track.py [--blocks 9] [--reps 5] [--forms none,track]

Events on the launch stream around ``reps`` calls, after a warm-up of every form; per form the median, minimum and maximum over the blocks
(ms per call), and the same for the plain forward launch alone (no gradients: nothing recorded).  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcp_boot  # noqa: E402,F401

from mc_pilco_amd import ops, workloads  # noqa: E402
from mc_pilco_amd.policy_learning import Policy  # noqa: E402

DT = torch.float64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hidden", default="64,64")
    ap.add_argument("--forms", default="none,track")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hidden = [int(h) for h in args.hidden.split(",")]
    wl = workloads.build("ur5_script", device=dev)
    pm, M, T = wl.model, wl.M, wl.T
    x0 = wl.sample_x0(M)
    t = torch.arange(T, dtype=DT, device=dev).reshape(-1, 1)
    target = x0.mean(0).reshape(1, -1) + 0.3 * torch.sin(0.02 * t + torch.arange(pm.S, dtype=DT, device=dev).reshape(1, -1))
    pols = {}
    for form, kw in (("none", {}), ("track", dict(target_traj=target))):
        torch.manual_seed(1)
        pols[form] = Policy.MLP_policy(state_dim=pm.S, input_dim=pm.U, hidden_sizes=hidden, u_max=1.0, dtype=DT, device=dev, **kw)
    gen = torch.Generator(device=dev).manual_seed(1)
    w = torch.randn(T, M, pm.S, dtype=DT, device=dev, generator=gen)
    wu = torch.randn(T, M, pm.U, dtype=DT, device=dev, generator=gen)
    forms = args.forms.split(",")
    call = lambda form: ops.rollout_mlp(pm, pols[form].packed(), ops.NoiseSpec(seed=1, call=1), x0, T)

    def fwd_bwd(form):
        st, inp, status = call(form)
        torch.autograd.grad((w * st).sum() + (wu * inp).sum(), list(pols[form].mlp_parameters()))
        return status

    def fwd_plain(form):
        with torch.no_grad():
            return call(form)[2]

    for f in forms:  # warm-up: every form's code objects, and its status
        assert int(fwd_bwd(f).item()) == 0 and int(fwd_plain(f).item()) == 0, f
        fwd_bwd(f)
    torch.cuda.synchronize()
    ms, ms_fwd = {f: [] for f in forms}, {f: [] for f in forms}
    for _ in range(args.blocks):
        for fn, acc in ((fwd_bwd, ms), (fwd_plain, ms_fwd)):
            for f in forms:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    fn(f)
                b.record()
                torch.cuda.synchronize()
                acc[f].append(a.elapsed_time(b) / args.reps)
    out = dict(workload="ur5_script", N=int(wl.problem["N"]), G=pm.G, D=pm.D, M=M, T=T, hidden=hidden, P={f: pols[f].feature_dim for f in forms},
               n_param={f: pols[f].packed().n_param for f in forms}, blocks=args.blocks, reps=args.reps)
    for f in forms:
        for key, acc in (("_fwd_record_and_sweep_ms", ms), ("_fwd_plain_ms", ms_fwd)):
            out[f + key] = [round(float(np.median(acc[f])), 4), round(float(np.min(acc[f])), 4), round(float(np.max(acc[f])), 4)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
