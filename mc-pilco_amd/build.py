"""Builds libmcpilco_hip.so (gfx950) in-tree with hipcc.  No GPU is needed to compile.

    python mc-pilco_amd/build.py [--force]
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SOURCES = ["gp_pretrain.hip", "gp_linalg.hip", "gp_sod.hip", "gp_nll.hip", "rollout_fwd.hip", "rollout_fwd_lean.hip", "rollout_fwd_tile.hip", "rollout_open.hip", "rollout_mlp.hip", "rollout_mlp_hist.hip", "model_step.hip", "lqr.hip", "mppi.hip", "rollout_bwd.hip", "cost.hip", "policy_opt.hip", "comm.hip"]
HEADERS = [os.path.join(CSRC, "mcp_device.h"), os.path.join(CSRC, "gp_launch.h"), os.path.join(CSRC, "rollout_common.h"), os.path.join(CSRC, "rollout_fwd_shared.h"), os.path.join(CSRC, "rollout_plan.h"),
           os.path.join(CSRC, "rollout_open_phases.h"), os.path.join(CSRC, "rollout_mlp_kernels.h"), os.path.join(CSRC, "cost_point.h"),
           os.path.join(os.path.dirname(HERE), "include", "mcpilco_hip.h"),
           os.path.join(os.path.dirname(HERE), "include", "mcpilco_hip_debug.h")]  # (mcp_dispatch: every translation unit must see the same layout)
LIB = os.path.join(HERE, "libmcpilco_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -disable-machine-licm: the machine-level loop-invariant hoisting pulls the ~60 double-precision literals of exp / sincos / log /
# tanh out of the time-step loop into VGPRs, which then spill to scratch and are reloaded (global-latency) in every phase
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
         "-mllvm", "-disable-machine-licm"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile_all(jobs, verbose):
    """Runs the hipcc commands of the stale sources side by side (one process each, at most the CPU count)."""
    from concurrent.futures import ThreadPoolExecutor

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    if jobs:
        with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), os.cpu_count() or 1, int(os.environ.get("MCP_BUILD_JOBS", "8"))))) as ex:
            list(ex.map(run, jobs))


def _sources_digest():
    """Identity of what the library is built from: every source, header and the flags."""
    import hashlib

    h = hashlib.sha256(" ".join(FLAGS).encode())
    for f in [os.path.join(CSRC, s) for s in SOURCES] + HEADERS:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


STAMP = LIB + ".stamp"


def build(force=False, verbose=True):
    """Compiles what is stale and links.  A library whose stamp (libmcpilco_hip.so.stamp: a digest of sources, headers and flags) matches is
    up to date whatever the file times say and whether or not the objects are there -- a snapshot of the tree (gpurun, the driver's GPU box)
    carries the library and its stamp, not the objects (.gpurunignore), and must not spend minutes rebuilding them."""
    digest = _sources_digest()
    if not force and os.path.exists(LIB) and os.path.exists(STAMP) and open(STAMP).read().strip() == digest:
        return LIB
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        if force or _stale(o, [s] + HEADERS):
            jobs.append([HIPCC] + FLAGS + ["-c", s, "-o", o])
        objs.append(o)
    _compile_all(jobs, verbose)
    if force or jobs or _stale(LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-ldl", "-o", LIB]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    with open(STAMP, "w") as f:
        f.write(digest + "\n")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
