"""Times one optimizer step under a policy the fused rollouts do not know -- a two-layer tanh torch.nn module -- through the class path:
MC_PILCO.apply_policy + a weighted-sum cost + backward, with ``fused_step = True`` (one mcp_model_step launch per time step, one
mcp_model_step_bwd in backward) and with ``fused_step = False`` (the step loop on get_next_state with autograd through it: the code before
the fused step, line for line), in the same run.

    python tools/time_model_step.py [--blocks 5] [--reps 3] [--step-blocks 3] [--shapes ur5_script,arm2] [--kernels-only]

Shapes (tools/time_pd_rollout.py builds them): the UR5 script shape (6 GPs, D = 24, N = 400, M = 200, T = 200) and a two-joint arm (2 GPs,
D = 8, N = 300, M = 400, T = 150).  Events around the step, `reps` steps per block, median over the blocks; the unfused
path runs one step per block.  Also counts the device launches of one step of either path (torch profiler) and times the step kernel and
the reverse kernel alone (sampled, recording; per launch).  One JSON line per shape; the tool fails when the fused step is the slower one.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_pd_rollout import DT, build_object, launches, median_ms  # noqa: E402  (also puts the package on the path)

from mc_pilco_amd import ops  # noqa: E402


class TanhPolicy(torch.nn.Module):
    """u = u_max tanh(W2 tanh(W1 x + b1) + b2), called as the package's policies are."""

    def __init__(self, S, U, H=32, u_max=1.0, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.l1, self.l2, self.u_max = torch.nn.Linear(S, H).double(), torch.nn.Linear(H, U).double(), u_max
        with torch.no_grad():
            for q in self.parameters():
                q.copy_(0.3 * torch.randn(q.shape, dtype=DT, generator=g))

    def forward(self, x, t=None, p_dropout=0.0):
        return self.u_max * torch.tanh(self.l2(torch.tanh(self.l1(x))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-blocks", type=int, default=3)
    ap.add_argument("--shapes", default="ur5_script,arm2")
    ap.add_argument("--kernels-only", action="store_true", help="only the step / reverse-step calls, 50 each per shape: the run to put under "
                    "`rocprofv3 --kernel-trace --stats` for the kernels' own times")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        obj, sim, N, M, T = build_object(shape, dev)
        pm = obj.model_learning.packed()
        pol = obj.control_policy = TanhPolicy(pm.S, pm.U).to(dev)
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
        if args.kernels_only:
            x = obj.sample_initial_particles(sim["particles_initial_state_mean"], sim["particles_initial_state_var"], False, None, None, False, M)
            xr, u = x.clone().requires_grad_(True), torch.zeros(M, pm.U, dtype=DT, device=dev)
            for _ in range(50):
                with torch.no_grad():
                    ops.model_step(pm, x, u, 0, noise=ops.NoiseSpec(seed=1, call=1))
                nx, _ = ops.model_step(pm, xr, u, 0, noise=ops.NoiseSpec(seed=1, call=1))
                torch.autograd.grad(nx.sum(), xr)
            torch.cuda.synchronize()
            continue
        obj.fused_step = True
        out["fused_step_ms"] = median_ms(step, args.blocks, args.reps)
        assert obj.last_step_fused and int(obj.last_status.item()) == 0
        out["fused_launches"] = launches(step)
        obj.fused_step = False
        out["unfused_step_ms"] = median_ms(step, args.step_blocks, 1)
        assert not obj.last_step_fused
        out["unfused_launches"] = launches(step)
        # the two kernels alone: a sampled recording step, and the reverse step over its record
        x = obj.sample_initial_particles(sim["particles_initial_state_mean"], sim["particles_initial_state_var"], False, None, None, False, M)
        u = torch.zeros(M, pm.U, dtype=DT, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        nz = ops.NoiseSpec(seed=1, call=1)
        with torch.no_grad():
            out["step_kernel_plain_ms"] = median_ms(lambda: ops.model_step(pm, x, u, 0, noise=nz, status=status), args.blocks, 20)
        xr = x.clone().requires_grad_(True)
        out["step_kernel_record_ms"] = median_ms(lambda: ops.model_step(pm, xr, u, 0, noise=nz, status=status), args.blocks, 20)
        nx, _ = ops.model_step(pm, xr, u, 0, noise=nz, status=status)
        g = torch.ones_like(nx)
        out["reverse_kernel_ms"] = median_ms(lambda: torch.autograd.grad(nx, xr, g, retain_graph=True), args.blocks, 20)
        out["fused_not_slower"] = out["fused_step_ms"][0] <= out["unfused_step_ms"][0]  # medians of the same run
        print(json.dumps(out), flush=True)
        assert out["fused_not_slower"], "the fused step is slower than the step loop timed in the same run"


if __name__ == "__main__":
    main()
