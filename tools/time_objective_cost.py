"""Times the time-weighted, risk-sensitive objective on the HIP cost kernels against the same wrapped cost unshaped, alternating the two forms
inside every block:

    shaped  Cost_shaping(Input_penalty(state cost, effort and rate terms), discount=0.99, risk=0.5): mcp_cost_u_fwd / mcp_cost_rows /
            mcp_cost_bwd_shaped
    plain   the Input_penalty itself: mcp_cost_u_fwd / mcp_cost_finalize / mcp_cost_u_bwd

at the two shapes of tools/time_input_cost.py (cart-pole headline shape, M = 400, T = 150; arm2 under MLP_policy(hidden_sizes=[32])), two ways:
``cost`` = the cost and ``backward()`` on the states and inputs of one rollout (leaf tensors), ``step`` = ``apply_policy`` (Philox noise),
``_cost_backward`` and ``Adam.step()``.

    python tools/time_objective_cost.py [--blocks 9] [--reps 5] [--shapes cartpole,arm2]

Events on the launch stream around ``reps`` runs per form, after a warm-up of both; per form the median, minimum and maximum over the blocks
(ms) and the device launches of one run (torch.profiler: kernels, memsets and copies).  One JSON line per shape.  The condition from the design:
the shaped form makes no more device launches than the plain one; the time carries no pass mark -- read the shaped median against the plain
form's own min-max spread."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import time_input_cost as tic  # noqa: E402  (puts the repository and tests/ on the path, registers the package)

from mc_pilco_amd.policy_learning import Cost_function as CF  # noqa: E402


def launches(run):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            run()
            torch.cuda.synchronize()
        return len([e for e in prof.events() if str(e.device_type).endswith("CUDA")])
    except Exception as e:  # noqa: BLE001  (the count is a by-product; the timing stands without it)
        return "profiler: %r" % (e,)


def time_shape(build, dev, blocks, reps):
    obj, sim, plain, out = build(dev)
    obj.noise_mode = "philox"
    forms = {"shaped": CF.Cost_shaping(plain, discount=0.99, risk=0.5), "plain": plain}
    params = [q for q in obj.control_policy.parameters() if q.requires_grad]
    opt = torch.optim.Adam(params, 1e-4)
    last = {}
    with torch.no_grad():
        st0, in0 = obj.apply_policy(**sim)
    st0, in0 = st0.detach().clone().requires_grad_(True), in0.detach().clone().requires_grad_(True)

    def cost(form):
        st0.grad = in0.grad = None
        J, _ = forms[form](st0, in0, 0)
        J.backward()

    def step(form):
        obj.cost_function = forms[form]
        opt.zero_grad(set_to_none=True)
        st, inp = obj.apply_policy(**sim)
        J, _, _ = obj._cost_backward(st, inp, 0)
        opt.step()
        last[form] = J.detach()

    for what, run in (("cost", cost), ("step", step)):
        for f in forms:
            run(f)
            run(f)
        torch.cuda.synchronize()
        ms = {f: [] for f in forms}
        for _ in range(blocks):
            for f in forms:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    run(f)
                b.record()
                torch.cuda.synchronize()
                ms[f].append(a.elapsed_time(b) / reps)
        for f in forms:
            out["%s_%s_ms" % (f, what)] = [round(float(np.median(ms[f])), 4), round(float(np.min(ms[f])), 4), round(float(np.max(ms[f])), 4)]
            out["%s_%s_device_launches" % (f, what)] = launches(lambda: run(f))
        out["%s_shaped_minus_plain_ms" % what] = round(out["shaped_%s_ms" % what][0] - out["plain_%s_ms" % what][0], 4)
    shaped = forms["shaped"]
    assert shaped._packed is not None and shaped._objectives and plain._in_packs, "the shaped form did not run on the kernels"
    assert all(bool(torch.isfinite(v)) for v in last.values())
    out.update({f + "_last_cost": float(last[f]) for f in forms})
    out.update(blocks=blocks, reps=reps, costs_read_bytes=8 * st0.shape[0] * st0.shape[1])
    print(json.dumps(out), flush=True)
    for what in ("cost", "step"):
        a, b = out["shaped_%s_device_launches" % what], out["plain_%s_device_launches" % what]
        assert not (isinstance(a, int) and isinstance(b, int)) or a <= b, "the shaped %s makes %s device launches, the plain one %s" % (what, a, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="cartpole,arm2")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in args.shapes.split(","):
        time_shape(dict(cartpole=tic.cartpole, arm2=tic.arm2)[name], dev, args.blocks, args.reps)


if __name__ == "__main__":
    main()
