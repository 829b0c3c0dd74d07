"""Records what the rollout dispatch decides on the device it runs on: tests/dispatch_table_mi355x.json.

    python tools/record_dispatch_table.py [--out tests/dispatch_table_mi355x.json]

One three-step (or the case's own T) rollout plus backward per case, through ``ops.rollout``; the two ``_ex`` entry points are wrapped on the
host so that every entry holds exactly what the library was given -- the descriptor scalars the dispatch reads, M, T, the flags, the
workspace bytes, the eleven request words of ``hipabi.DISPATCH`` -- and what it answered: the two return codes and the six ``ran_*`` words.
tests/test_dispatch_plan_cpu.py replays the table against the plan queries (mcp_rollout_fwd_plan / mcp_rollout_bwd_plan) without a GPU.

Cases: every workload of ``workloads.CONFIGS`` but the duplicate ``c4`` at T = 3 over the swarm sizes at which a dispatch rule changes; the 18
width cases of tests/width_models.py at their own T; forced requests only as existing GPU tests issue them (tests/test_gpu_width_classes.py's
variants, test_gpu_parity.py's lean-sweep and two-launch cases).  Descriptors are stored once and referenced by index.  The run stops at the
first error that is not a host-side refusal (MCP_ERR_ARG / LIMIT / WORKSPACE)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mcp_boot  # noqa: E402,F401  (makes the package importable as mc_pilco_amd)
from mc_pilco_amd import hipabi as abi  # noqa: E402
from mc_pilco_amd import ops, workloads  # noqa: E402

M_LIST = [1, 4, 16, 64, 200, 256, 257, 400, 512, 513, 1024, 1025, 1280, 2048, 2049, 2816, 2817, 4000]
REQUEST = ["fwd_particles", "gp_sharding", "fwd_lean", "policy_split", "row_split", "cluster_map", "fwd_no_xlds", "fwd_gb", "bwd_particles", "bwd_lean",
           "bwd_pipe"]
RAN = ["ran_particles", "ran_gp_sharded", "ran_fwd_lean", "ran_bwd_lean", "ran_row_split", "ran_bwd_pipe"]
HOST_ERRORS = (-1, -2, -3)


def model_scalars(m):
    if m is None:
        return None
    G = int(m.G)
    return dict(S=int(m.S), U=int(m.U), G=G, D=int(m.D), angle=[int(m.angle[i]) for i in range(m.n_angle)],
                not_angle=[int(m.not_angle[i]) for i in range(m.n_not_angle)], vel=[int(m.vel[g]) for g in range(G)],
                not_vel=[int(m.not_vel[g]) for g in range(G)], N=[int(m.gp[g].N) for g in range(G)], Npad=[int(m.gp[g].Npad) for g in range(G)],
                poly_deg=[int(m.gp[g].kern.poly_deg) for g in range(G)])


def policy_scalars(p):
    ms = p.meas
    return dict(kind=int(p.kind), S=int(p.S), P=int(p.P), B=int(p.B), U=int(p.U), angle=[int(p.angle[i]) for i in range(p.n_angle)],
                non_angle=[int(p.non_angle[i]) for i in range(p.n_non_angle)], traj_len=int(p.traj_len), p_drop=float(p.p_drop),
                meas=dict(n=int(ms.n), pos=[int(ms.pos[i]) for i in range(ms.n)], vel=[int(ms.vel[i]) for i in range(ms.n)]), bias=bool(p.bias))


class Recorder:
    """Wraps the two `_ex` entry points of the loaded library: what each call was given and what it returned."""

    def __init__(self):
        self.L = abi.lib()
        self.fwd = self.bwd = None
        for name in ("mcp_rollout_fwd_ex", "mcp_rollout_bwd_ex"):
            setattr(self.L, name, self._wrap(name, getattr(self.L._h, name)))

    def _wrap(self, name, fn):
        def call(*a):
            model = None if a[0] is None else a[0]._obj
            rec = dict(model=model_scalars(model), policy=policy_scalars(a[1]._obj), M=int(a[3]), T=int(a[4]),
                       request={k: int(getattr(abi.DISPATCH, k)) for k in REQUEST})
            if name == "mcp_rollout_fwd_ex":
                rec.update(flags=int(a[5]), workspace_bytes=int(a[12]))
            else:
                rec.update(workspace_bytes=int(a[15]))
            rec["rc"] = int(fn(*a))
            rec["ran"] = {k: int(getattr(abi.DISPATCH, k)) for k in RAN}
            if name == "mcp_rollout_fwd_ex":
                self.fwd = rec
            else:
                self.bwd = rec
            return rec["rc"]

        return call


def set_request(req):
    for k in REQUEST:
        setattr(abi.DISPATCH, k, int(req.get(k, 0)))


def intern(pool, obj):
    key = json.dumps(obj, sort_keys=True)
    if key not in pool:
        pool[key] = len(pool)
    return pool[key]


def run_case(rec, table, name, model, policy, cost, noise, meas, x0, T, p_drop, req):
    """One forward + backward under the request ``req``; appends the entry.  Returns False when the run has to stop."""
    set_request(req)
    rec.fwd = rec.bwd = None
    for q in (policy.log_ls, policy.centers, policy.weight) + (() if policy.bias is None else (policy.bias,)):
        q.grad = None
    try:
        st, _inp, status = ops.rollout(model, policy, noise, x0, T, p_drop, meas=meas)
        c, _ = ops.expected_cost(cost, st)
        c.backward()
        torch.cuda.synchronize()
        bad = int(status.item())
    except RuntimeError as e:  # (abi.check: a refused call)
        bad = 0
        print("  %s: %s" % (name, e), flush=True)
    finally:
        set_request({})
    f, b = rec.fwd, rec.bwd
    if f is None:
        print("no forward call was recorded for %s" % name)
        return False
    assert b is None or (b["model"] == f["model"] and b["policy"] == f["policy"] and b["M"] == f["M"] and b["T"] == f["T"])
    entry = dict(name=name, model=intern(table["_models"], f["model"]), policy=intern(table["_policies"], f["policy"]), M=f["M"], T=f["T"],
                 flags=f["flags"], fwd_workspace_bytes=f["workspace_bytes"], bwd_workspace_bytes=None if b is None else b["workspace_bytes"],
                 request=[f["request"][k] for k in REQUEST], rc_fwd=f["rc"], rc_bwd=None if b is None else b["rc"],
                 ran=[(b or f)["ran"][k] for k in RAN])
    table["entries"].append(entry)
    for r in (f, b):
        if r is not None and r["rc"] != 0 and r["rc"] not in HOST_ERRORS:
            print("stopping: %s returned %d" % (name, r["rc"]))
            return False
    if bad:
        print("stopping: %s left status %d" % (name, bad))
        return False
    return True


def workload_cases(rec, table, dev):
    for name in workloads.CONFIGS:
        if name == "c4":
            continue
        w = workloads.build(name, device=dev, T=3)
        for M in M_LIST:
            x0 = w.sample_x0(M)
            if not run_case(rec, table, "%s-M%d" % (name, M), w.model, w.policy, w.cost, ops.NoiseSpec(seed=5, call=1), w.meas, x0, 3, w.p_drop, {}):
                return False
        print(name, "done", flush=True)
    return True


def code_request(code, pb, pipe):
    """The request words of tests/gpu_helpers.forced_variant(code, bwd_particles=pb) plus the pipe switch of the width tests."""
    from gpu_helpers import forced_variant

    v = forced_variant(code, bwd_particles=pb)
    req = dict(fwd_particles=v.ppw, bwd_particles=v.pb, gp_sharding=2 if v.sharded else (0 if code == 0 else 1),
               fwd_lean=0 if (v.lean or code == 0) else 1)
    if pipe is not None:
        req["bwd_pipe"] = 1 if pipe == 0 else 0
    return req


def width_cases(rec, table):
    import width_models as wm
    from test_gpu_width_classes import ALL

    for c in wm.CASES:
        for M in (3, 16, 40):
            model, pol, cost, nz, meas, x0 = wm.packed(c, M)
            if not run_case(rec, table, "%s-M%d" % (c.name, M), model, pol, cost, nz, meas, x0, c.T, wm.P_DROP, {}):
                return False
    for c, (code, pb, pipe, M) in ALL:  # the forced variants exactly as test_rollout_cost_and_gradients_vs_oracle issues them
        if code == 0:
            continue
        model, pol, cost, nz, meas, x0 = wm.packed(c, M)
        nm = "%s-f%d-b%s%s-M%d" % (c.name, code, "a" if pb is None else pb, "" if pipe is None else "-pipe%d" % pipe, M)
        if not run_case(rec, table, nm, model, pol, cost, nz, meas, x0, c.T, wm.P_DROP, code_request(code, pb, pipe)):
            return False
    print("width cases done", flush=True)
    return True


def parity_cases(rec, table, dev):
    """test_gpu_parity.py: the general sweep forced beside the lean one, the two-launch sharded form and its unsharded twin."""
    for name, M, T, p in [("c1", 37, 2, 0.25), ("c1", 64, 9, 0.0), ("c3", 96, 20, 0.25), ("c1", 1333, 7, 0.25), ("pms_script", 37, 2, 0.25),
                          ("pms_script", 515, 6, 0.25)]:
        w = workloads.build(name, device=dev, M=M, T=T, p_drop=p)
        if not run_case(rec, table, "%s-M%d-T%d-nolean" % (name, M, T), w.model, w.policy, w.cost, ops.NoiseSpec(seed=21, call=4), w.meas,
                        w.sample_x0(), T, p, dict(bwd_lean=1)):
            return False
    w = workloads.build("c1", device=dev, M=700, T=10)
    for tag, req in [("sharded4", dict(gp_sharding=2, fwd_particles=4)), ("unsharded", dict(gp_sharding=1))]:
        if not run_case(rec, table, "c1-M700-T10-%s" % tag, w.model, w.policy, w.cost, ops.NoiseSpec(seed=3, call=1), w.meas, w.sample_x0(), 10,
                        w.p_drop, req):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "dispatch_table_mi355x.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    table = dict(device=torch.cuda.get_device_name(dev), cus=int(torch.cuda.get_device_properties(dev).multi_processor_count), request_words=REQUEST,
                 ran_words=RAN, _models={}, _policies={}, entries=[])
    rec = Recorder()
    ok = workload_cases(rec, table, dev) and width_cases(rec, table) and parity_cases(rec, table, dev)
    table["models"] = [json.loads(k) for k in table.pop("_models")]
    table["policies"] = [json.loads(k) for k in table.pop("_policies")]
    table["complete"] = bool(ok)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print("%d entries, %d models, %d policies -> %s%s" % (len(table["entries"]), len(table["models"]), len(table["policies"]), a.out,
                                                         "" if ok else "  (INCOMPLETE)"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
