"""Times what dropout costs in the fused tanh-MLP rollout: the recording launch plus the sweep (ops.rollout_mlp + backward) at the cart-pole
size -- the headline workload's model (workloads "c1": SE kernel, N = 300), M = 400, T = 150, hidden (64, 64), f = x -- in three forms of the
same call, alternating inside every block:

    none     p_drop = 0: the call without the keyword (mcp_rollout_mlp + mcp_rollout_mlp_bwd, the code before dropout)
    philox   p_drop = 0.25, masks drawn in the kernels
    buffer   p_drop = 0.25, masks [T, M, 128] uint8 read from a buffer

    python tools/time_mlp_dropout.py [--blocks 9] [--reps 5] [--p 0.25] [--forms none,philox,buffer]

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
    ap.add_argument("--p", type=float, default=0.25)
    ap.add_argument("--hidden", default="64,64")
    ap.add_argument("--forms", default="none,philox,buffer")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hidden = [int(h) for h in args.hidden.split(",")]
    wl = workloads.build("c1", device=dev)
    pm, M, T = wl.model, wl.M, wl.T
    torch.manual_seed(1)
    pol = Policy.MLP_policy(state_dim=pm.S, input_dim=pm.U, hidden_sizes=hidden, u_max=10.0, dtype=DT, device=dev)
    x0 = wl.sample_x0(M)
    gen = torch.Generator(device=dev).manual_seed(1)
    w = torch.randn(T, M, pm.S, dtype=DT, device=dev, generator=gen)
    wu = torch.randn(T, M, pm.U, dtype=DT, device=dev, generator=gen)
    masks = torch.empty(T, M, sum(hidden), dtype=DT, device=dev).bernoulli_(1 - args.p, generator=gen).to(torch.uint8)
    params = list(pol.mlp_parameters())
    calls = {
        "none": lambda: ops.rollout_mlp(pm, pol.packed(), ops.NoiseSpec(seed=1, call=1), x0, T),
        "philox": lambda: ops.rollout_mlp(pm, pol.packed(), ops.NoiseSpec(seed=1, call=1), x0, T, p_drop=args.p),
        "buffer": lambda: ops.rollout_mlp(pm, pol.packed(), ops.NoiseSpec(seed=1, call=1, masks=masks), x0, T, p_drop=args.p),
    }
    forms = args.forms.split(",")

    def fwd_bwd(form):
        st, inp, status = calls[form]()
        torch.autograd.grad((w * st).sum() + (wu * inp).sum(), params)
        return status

    def fwd_plain(form):
        with torch.no_grad():
            return calls[form]()[2]

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
    out = dict(workload="c1", N=int(wl.problem["N"]), G=pm.G, D=pm.D, M=M, T=T, hidden=hidden, p=args.p,
               blocks=args.blocks, reps=args.reps)
    for f in forms:
        for key, acc in (("_fwd_record_and_sweep_ms", ms), ("_fwd_plain_ms", ms_fwd)):
            out[f + key] = [round(float(np.median(acc[f])), 4), round(float(np.min(acc[f])), 4), round(float(np.max(acc[f])), 4)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
