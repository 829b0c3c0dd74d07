"""Times one optimizer step through the class path with a cost that reads the inputs -- Input_penalty(state cost, effort and rate terms, ADD)
-- in its two forms, alternating inside every block:

    hip     the Input_penalty object itself: mcp_cost_u_fwd / mcp_cost_finalize / mcp_cost_u_bwd
    torch   the same formula as ordinary torch ops, Expected_cost(cf.cost_function): the only form there was before the kernels took the
            input terms, hence the yardstick

at two shapes: the cart-pole headline shape (workloads.dropin_c1: Sum_of_gaussians_with_angles, N = 300, M = 400, T = 150, Cart_pole_cost)
and the arm2 object of the closed-loop test family (tests/closed_loop_family.arm_object) under MLP_policy(hidden_sizes=[32]), M = 400,
T = 150, Expected_saturated_distance.  A step is ``apply_policy`` (Philox noise), ``_cost_backward`` and ``Adam.step()``.

    python tools/time_input_cost.py [--blocks 9] [--reps 5] [--shapes cartpole,arm2]

Events on the launch stream around ``reps`` steps per form, after a warm-up of both forms; per form the median, minimum and maximum over the
blocks (ms per step) and the device launches of one step (torch.profiler: kernels, memsets and copies).  One JSON line per shape; the ratio
carries no pass mark."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mcp_boot  # noqa: E402,F401

from mc_pilco_amd import workloads  # noqa: E402
from mc_pilco_amd.policy_learning import Cost_function as CF  # noqa: E402
from mc_pilco_amd.policy_learning import Policy  # noqa: E402


def cartpole(dev):
    obj, args = workloads.dropin_c1(dev)
    sim = {k: args[k] for k in ("particles_initial_state_mean", "particles_initial_state_var", "flg_particles_init_uniform", "particles_init_up_bound",
                                "particles_init_low_bound", "flg_particles_init_multi_gauss", "num_particles")}
    sim.update(T_control=150, p_dropout=0.25)
    cf = CF.Input_penalty(obj.cost_function, lengthscales=[10.0], rate_lengthscales=[5.0])
    return obj, sim, cf, dict(shape="cartpole", policy="Sum_of_gaussians_with_angles", N=300, M=400, T=150, state_cost="Cart_pole_cost")


def arm2(dev):
    import conftest  # noqa: F401
    import closed_loop_family as clf
    from mlp_models import SHAPES, network

    c = SHAPES["arm2"]
    obj = clf.arm_object(Policy.MLP_policy, clf.arm_mlp_par(network(c, (32,), c["angle"], c["not_angle"], 40), (32,)))
    cf = CF.Input_penalty(obj.cost_function, lengthscales=[1.5, 1.5], rate_lengthscales=[0.5, 0.5])
    return obj, clf.sim_args(400, 150), cf, dict(shape="arm2", policy="MLP_policy(hidden_sizes=[32])", N=int(obj.model_learning.gp_inputs.shape[0]),
                                                  M=400, T=150, state_cost="Expected_saturated_distance")


def time_shape(build, dev, blocks, reps):
    obj, sim, cf, out = build(dev)
    obj.noise_mode = "philox"
    forms = {"hip": cf, "torch": CF.Expected_cost(cf.cost_function)}
    params = [q for q in obj.control_policy.parameters() if q.requires_grad]
    opt = torch.optim.Adam(params, 1e-4)
    last = {}

    def step(form):
        obj.cost_function = forms[form]
        opt.zero_grad(set_to_none=True)
        st, inp = obj.apply_policy(**sim)
        cost, std, _ = obj._cost_backward(st, inp, 0)
        opt.step()
        last[form] = cost.detach()

    for f in forms:  # warm-up: both forms' code objects and descriptors
        step(f)
        step(f)
    torch.cuda.synchronize()
    assert cf._packed is not None and cf._in_packs, "the hip form did not run on the kernels"
    assert all(bool(torch.isfinite(v)) for v in last.values())
    ms = {f: [] for f in forms}
    for _ in range(blocks):
        for f in forms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                step(f)
            b.record()
            torch.cuda.synchronize()
            ms[f].append(a.elapsed_time(b) / reps)
    for f in forms:
        out[f + "_ms_per_step"] = [round(float(np.median(ms[f])), 4), round(float(np.min(ms[f])), 4), round(float(np.max(ms[f])), 4)]
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                step(f)
                torch.cuda.synchronize()
            out[f + "_device_launches_per_step"] = len([e for e in prof.events() if str(e.device_type).endswith("CUDA")])
        except Exception as e:  # noqa: BLE001  (the count is a by-product; the timing stands without it)
            out[f + "_device_launches_per_step"] = "profiler: %r" % (e,)
    torch.cuda.synchronize()
    out.update({f + "_last_cost": float(last[f]) for f in forms})
    out.update(blocks=blocks, reps=reps,ratio_torch_over_hip=round(out["torch_ms_per_step"][0] / out["hip_ms_per_step"][0], 4))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="cartpole,arm2")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in args.shapes.split(","):
        time_shape(dict(cartpole=cartpole, arm2=arm2)[name], dev, args.blocks, args.reps)


if __name__ == "__main__":
    main()
