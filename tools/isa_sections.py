#!/usr/bin/env python3
"""Static instruction counts of one gfx950 kernel, per barrier-separated section, from hipcc -S (device-only compile, no GPU needed):
lane spills (v_readlane / v_writelane), vector, LDS, global and clock-read instructions between consecutive s_barrier's, in the order
of the listing.  Static counts, not executed counts: a section with a loop is listed once.

    python tools/isa_sections.py [file.hip] [kernel substring]      default: rollout_fwd_lean.hip 'rollout_fwd_lat_kernel<4, 3, 0, false, false>'
    python tools/isa_sections.py --list [file.hip]                  the kernels of the file
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mc-pilco_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-mllvm", "-disable-machine-licm", "--cuda-device-only", "-S"]
COLUMNS = ["v_readlane", "v_writelane", "vector", "LDS", "global", "clock"]


def listing(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + [src, "-o", out])
        return open(out).read()


def kernels(asm):
    """{demangled name: [instruction lines]} of every function of the listing."""
    res = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().replace("void ", "")
        res[re.sub(r"\(.*", "", name)] = [l.strip() for l in m.group(2).split("\n")]
    return res


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_readlane"):
        return "v_readlane"
    if op.startswith("v_writelane"):
        return "v_writelane"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "global"
    if op.startswith(("s_memtime", "s_memrealtime")):
        return "clock"
    if op.startswith("v_"):
        return "vector"
    return None


def sections(lines):
    rows, cur = [], dict.fromkeys(COLUMNS, 0)
    for l in lines:
        if not l or l.startswith((";", ".", "//")) or l.endswith(":"):
            continue
        if l.startswith("s_barrier"):
            rows.append(cur)
            cur = dict.fromkeys(COLUMNS, 0)
            continue
        k = classify(l)
        if k:
            cur[k] += 1
    rows.append(cur)
    return rows


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    f = args[0] if args else "rollout_fwd_lean.hip"
    src = f if os.path.exists(f) else os.path.join(CSRC, f)
    ks = kernels(listing(src))
    if "--list" in sys.argv:
        print("\n".join(ks))
        sys.exit(0)
    want = args[1] if len(args) > 1 else "rollout_fwd_lat_kernel<4, 3, 0, false, false>"
    hits = [k for k in ks if want in k]
    if len(hits) != 1:
        sys.exit("%d kernels match %r:\n%s" % (len(hits), want, "\n".join(hits or ks)))
    rows = sections(ks[hits[0]])
    print(hits[0])
    print("| section | " + " | ".join(COLUMNS) + " |\n|---|" + "---|" * len(COLUMNS))
    for i, r in enumerate(rows):
        name = "entry -> barrier 1" if i == 0 else ("barrier %d -> end" % i if i == len(rows) - 1 else "barrier %d -> %d" % (i, i + 1))
        print("| %s | " % name + " | ".join(str(r[c]) for c in COLUMNS) + " |")
    print("| total | " + " | ".join(str(sum(r[c] for r in rows)) for c in COLUMNS) + " |")
