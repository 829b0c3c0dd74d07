"""Times a target-state expected cost with its gradient at the cart-pole script shape (T = 60, M = 400, S = 4):
Expected_saturated_distance on two state indices, ``cost, std = cf(states, None, 0); cost.backward()``.

    python tools/time_target_cost.py [--other CHECKOUT] [--blocks 9] [--reps 50] [--timeout 180]

The same call is timed on this checkout and, with ``--other``, on another checkout of the project (the commit before the cost ran on the HIP
kernels: there the class evaluates its torch formula and autograd differentiates it).  Each leg is a child process of its own under
``timeout`` and imports the package of ITS checkout; a leg that fails or runs out of time ends the tool.  Events around ``reps`` calls per
block, median over the blocks; the launches of one call are counted with torch.profiler (device kernels and memsets /
copies).  One JSON line per leg.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(root, blocks, reps):
    sys.path.insert(0, root)
    import mcp_boot  # noqa: F401
    import numpy as np
    import torch

    from mc_pilco_amd.policy_learning import Cost_function

    dev = torch.device("cuda", 0)
    T, M, S = 60, 400, 4
    G = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device=dev)
    rs = np.random.RandomState(1)
    x = rs.randn(T, M, S)
    x[:, :, 2] = np.pi + 3.0 * rs.uniform(-1, 1, (T, M))  # (pole angle / cart position within two lengthscales of the set point)
    x[:, :, 0] = 1.0 * rs.uniform(-1, 1, (T, M))
    states = G(x).requires_grad_(True)
    cf = Cost_function.Expected_saturated_distance(target_state=G([[np.pi, 0.0]]), lengthscales=G([3.0, 1.0]), active_dims=[2, 0])

    def call():
        states.grad = None
        cost, std = cf(states, None, 0)
        cost.backward()
        return cost.detach(), std.detach()

    cost, std = call()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(1e3 * a.elapsed_time(b) / reps)
    launches, names = None, []
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        launches = len(names)
    except Exception as e:  # noqa: BLE001  (the count is a by-product; the timing stands without it)
        names = ["profiler: %r" % (e,)]
    on_kernels = getattr(cf, "_packed", None) is not None
    print(json.dumps(dict(root=root, path="hip" if on_kernels else "torch", T=T, M=M, S=S, cost=float(cost), std=float(std),
                          grad_abs_sum=float(states.grad.abs().sum()), us_per_call_median=float(np.median(out)), us_min=float(np.min(out)),
                          us_max=float(np.max(out)), blocks=blocks, reps=reps, device_launches_per_call=launches,
                          kernels=sorted(set(n[:60] for n in names)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None, help="another checkout of the project (built) to time the same call on")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per leg")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        leg(os.path.abspath(args.leg), args.blocks, args.reps)
        return 0
    for root in [HERE] + ([os.path.abspath(args.other)] if args.other else []):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", root, "--blocks", str(args.blocks),
               "--reps", str(args.reps)]
        rc = subprocess.call(cmd)
        if rc != 0:  # (a fault, an abort or the time limit: nothing more is started on the device)
            print("leg %s ended with status %d" % (root, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
