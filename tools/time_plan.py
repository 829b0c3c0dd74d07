"""Times the planner's extension (mcp_plan_ext) against the plain planner's entries, the forms alternating block by block in one visit:

    rollout-cost   a  ops.mppi_rollout                           the plain entry (with --base-lib: also the same entry of ANOTHER build of the
                                                                 library, e.g. the parent commit's, through its own handle)
                   b  ops.plan_rollout, default ext              the same launch through the new entry
                   c  ops.plan_rollout, sigma_rows + beta = 0.5  the extended form: a std per row from LDS, the AR(1) fma, one row ahead
                   d  c with u_prev
    update         e  ops.mppi_update                            the plain update
                   f  ops.mppi_update_ext, sigma_rows + beta     weights, white sums per row, the filter over H U sums
                   g  ops.cem_update, n_elite = K // 8           select + sort in one workgroup, the fit per input
                   h  the CEM update composed in torch           mean over particles, topk, gather from a [H][K][U] buffer of coloured
                                                                 perturbations (the colouring itself is NOT timed: the buffer is given), mean / var

    python tools/time_plan.py [--blocks 9] [--reps 5] [--shapes cartpole_mean,cartpole_sampled,ur5_mean] [--base-lib PATH]

Shapes and costs: tools/time_mppi.py's three (H = 30).  Events around the calls, `reps` calls per block; median [min, max] of the blocks; one
JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcp_boot  # noqa: E402,F401

from mc_pilco_amd import hipabi as abi  # noqa: E402
from mc_pilco_amd import ops, workloads  # noqa: E402
from time_mppi import DT, SHAPES, H, block_ms, stat  # noqa: E402


def base_rollout(path, pm, mp, cost, cin, nz, sample, x0, a, traj, status):
    """mcp_mppi_rollout of the library at ``path`` on the same descriptors (the entry and its structs are the same in both builds)."""
    h = C.CDLL(path)
    fn = h.mcp_mppi_rollout
    fn.restype, fn.argtypes = abi._SIGS["mcp_mppi_rollout"]
    mc, nc = mp.to_c(a, None, None, 0), nz.to_c()

    def call():
        abi.check(fn(ops._mc(pm), C.byref(mc), C.byref(cost.c), None if cin is None else C.byref(cin.c), C.byref(nc), int(sample), abi.ptr(x0),
                     abi.ptr(traj), None, None, abi.ptr(status), abi.stream()), "base mcp_mppi_rollout")

    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--base-lib", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in args.shapes.split(","):
        s = SHAPES[name]
        w = workloads.build(s["workload"], dev, T=H)
        pm, c = w.model, w.problem["cfg"]
        U, K, P, M = pm.U, s["K"], s["P"], s["K"] * s["P"]
        E = K // 8
        u_max = float(np.max(c["u_max"]))
        cin = ops.PackedCostInputs(U, dev, lengthscales=[4.0 * u_max] * U) if w.problem["system"] == "cartpole" else None
        mp = ops.PackedMPPI(K, P, H, U, s["sigma"], s["lam"], u_max=u_max)
        rows = np.full((H, U), s["sigma"]) * np.linspace(1.0, 0.5, H).reshape(-1, 1)
        e_def = ops.PackedPlanExt(H, U)
        e_col = ops.PackedPlanExt(H, U, beta=0.5, sigma_rows=rows, n_elite=E, alpha=0.1, sigma_min=0.05)
        x0 = w.x0_mean.reshape(-1).contiguous()
        a = torch.zeros(H, U, dtype=DT, device=dev)
        u_prev = torch.zeros(U, dtype=DT, device=dev)
        eps = torch.randn(H - 1, P, pm.G, dtype=DT, device=dev) if s["sample"] else None
        nz = ops.NoiseSpec(eps=eps, seed=1, call=0)
        new = lambda *sh: torch.empty(*sh, dtype=DT, device=dev)
        traj, a_new, s_new = new(M), new(H, U), new(H, U)
        out_m = (new(K), new(K), new(4))
        out_c = (new(K), torch.empty(E, dtype=torch.int32, device=dev), new(4))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        kw = dict(cost_inputs=cin, noise=nz, particle_pred=s["sample"], traj_cost=traj, status=status)
        xi_col = torch.randn(H, K, U, dtype=DT, device=dev)  # (h reads a buffer of perturbations)
        rows_d = e_col.rows_on(dev)

        def torch_cem():
            S = traj.reshape(K, P).mean(1)
            idx = torch.topk(S, E, largest=False).indices
            el = xi_col[:, idx]
            m, v = el.mean(1), el.var(1, unbiased=False)
            return 0.1 * a + 0.9 * (a + rows_d * m), torch.clamp(torch.sqrt(0.1 * rows_d ** 2 + 0.9 * rows_d ** 2 * v), min=0.05)

        forms = dict(
            a_mppi_rollout=lambda: ops.mppi_rollout(pm, mp, w.cost, x0, a, **kw),
            b_plan_rollout_default=lambda: ops.plan_rollout(pm, mp, e_def, w.cost, x0, a, **kw),
            c_plan_rollout_coloured_rows=lambda: ops.plan_rollout(pm, mp, e_col, w.cost, x0, a, **kw),
            d_plan_rollout_coloured_rows_u_prev=lambda: ops.plan_rollout(pm, mp, e_col, w.cost, x0, a, u_prev=u_prev, **kw),
            e_mppi_update=lambda: ops.mppi_update(mp, traj, a, noise=nz, a_new=a_new, out=out_m, status=status),
            f_mppi_update_ext=lambda: ops.mppi_update_ext(mp, e_col, traj, a, noise=nz, a_new=a_new, out=out_m, status=status),
            g_cem_update=lambda: ops.cem_update(mp, e_col, traj, a, noise=nz, a_new=a_new, sigma_new=s_new, out=out_c, status=status),
            h_cem_update_torch=torch_cem,
        )
        if args.base_lib:
            forms["a0_base_lib_mppi_rollout"] = base_rollout(args.base_lib, pm, mp, w.cost, cin, nz, s["sample"], x0, a, traj, status)
        for fn in forms.values():  # warm-up of every form
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(args.blocks):
            for k in sorted(forms):
                ms[k].append(block_ms(forms[k], args.reps))
        out = dict(shape=name, N=w.problem["N"], G=pm.G, D=pm.D, H=H, K=K, P=P, n_elite=E, status=int(status.item()))
        out.update({k + "_ms": stat(v) for k, v in sorted(ms.items())})
        base = out.get("a0_base_lib_mppi_rollout_ms", out["a_mppi_rollout_ms"])
        out["ratio_default_over_base"] = round(out["b_plan_rollout_default_ms"][0] / base[0], 4)
        out["ratio_coloured_over_base"] = round(out["c_plan_rollout_coloured_rows_ms"][0] / base[0], 4)
        out["ratio_cem_over_mppi_update"] = round(out["g_cem_update_ms"][0] / out["e_mppi_update_ms"][0], 3)
        out["ratio_torch_cem_over_cem"] = round(out["h_cem_update_torch_ms"][0] / out["g_cem_update_ms"][0], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
