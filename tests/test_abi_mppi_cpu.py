"""CPU: the layout of mcp_mppi through gcc on include/mcpilco_hip.h against the ctypes mirror (mc_pilco_amd.hipabi.MPPI) -- as
tests/test_abi_tvl_cpu.py does for mcp_tvl_policy --, the two planner entries (mcp_mppi_rollout, mcp_mppi_update) declared in the header,
bound with the declaration's argument list and exported by the library -- as tests/test_abi_lqr_cpu.py does for the trajectory-optimisation
entries --, the header and the binding naming the same set of entries, the limits restated in the binding, the Philox stream restated in
the header's comment, and the ABI version, which this struct and these entries leave at 7."""
import ctypes as C
import os
import re
import subprocess

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcpilco_hip.h")
DEVICE_HEADER = os.path.join(ROOT, "mc-pilco_amd", "csrc", "mcp_device.h")
FIELDS = ["K", "P", "H", "U", "squash", "u_max", "sigma", "lam", "kappa", "t0", "a", "xi", "w"]
C_NAME = {"lam": "lambda"}  # (a Python keyword on this side)
PTRS = {"const mcp_model*": "Model", "const mcp_mppi*": "MPPI", "const mcp_cost*": "Cost", "const mcp_cost_inputs*": "CostInputs",
        "const mcp_noise*": "Noise"}
CTYPE = {"int": C.c_int, "const double*": C.c_void_p, "double*": C.c_void_p, "uint32_t*": C.c_void_p, "void*": C.c_void_p}


def test_struct_layout_against_the_header(tmp_path):
    from mc_pilco_amd import hipabi

    names = [n for n, _ in hipabi.MPPI._fields_]
    assert names == FIELDS
    cn = [C_NAME.get(n, n) for n in names]
    src = tmp_path / "mp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(void){printf("%zu", sizeof(mcp_mppi));'
                   + "".join('printf(" %%zu %%zu", offsetof(mcp_mppi, %s), sizeof(((mcp_mppi*)0)->%s));' % (n, n) for n in cn)
                   + 'printf(" %d %d %d %d", MCP_MAX_INPUT, MCP_MPPI_MAX_K, MCP_MPPI_MAX_M, MCP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "mp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    # five ints (+ 4 bytes of padding), two arrays of MCP_MAX_INPUT doubles, two doubles, one int (+ 4), three pointers
    assert out[0] == C.sizeof(hipabi.MPPI) == 24 + 2 * 8 * 8 + 2 * 8 + 8 + 3 * 8
    for i, n in enumerate(names):
        f = getattr(hipabi.MPPI, n)
        assert out[1 + 2 * i:3 + 2 * i] == [f.offset, f.size], n
    assert out[-4:] == [hipabi.MAX_INPUT, hipabi.MPPI_MAX_K, hipabi.MPPI_MAX_M, hipabi.ABI_VERSION] == [8, 65536, 1 << 30, 7]


def test_the_entries_are_declared_bound_and_exported():
    from mc_pilco_amd import hipabi

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = hipabi.lib()
    for name, n_args, first in (("mcp_mppi_rollout", 12, "const mcp_model*"), ("mcp_mppi_update", 9, "const mcp_mppi*")):
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, txt).group(1)
        types = [re.sub(r"\s*\w+$", "", a.strip()) for a in decl.split(",")]
        assert len(types) == n_args and types[0] == first and types[-1] == "void*" and types[-2] == "uint32_t*"
        res, sig = hipabi._SIGS[name]
        assert res is C.c_int and len(sig) == n_args
        for t, s in zip(types, sig):
            assert s is (C.POINTER(getattr(hipabi, PTRS[t])) if t in PTRS else CTYPE[t]), (name, t)
        assert name in hipabi.EXPORTED and name in declared_symbols() and hasattr(lib, name)
    assert hipabi._SIGS["mcp_mppi_rollout"][1][5] is C.c_int  # particle_pred, by value


def test_header_and_binding_name_the_same_entries_and_the_version_stays():
    from mc_pilco_amd import hipabi

    assert set(hipabi.EXPORTED) == set(declared_symbols())
    assert hipabi.lib().mcp_abi_version() == hipabi.ABI_VERSION == 7
    txt = open(HEADER).read()
    assert re.search(r"#define MCP_ABI_VERSION 7\b", txt)
    assert int(re.search(r"#define MCP_MPPI_MAX_K (\d+)", txt).group(1)) == hipabi.MPPI_MAX_K


def test_the_planner_has_the_last_philox_stream():
    """Streams 0..2 were taken; the field is two bits wide.  The header's comment restates the device header's number."""
    dev = open(DEVICE_HEADER).read()
    streams = {n: int(v) for n, v in re.findall(r"#define MCP_STREAM_(\w+) (\d+)u", dev)}
    assert streams == {"EPS": 0, "MASK": 1, "POS": 2, "PLAN": 3}
    assert re.search(r"MCP_STREAM_PLAN = 3\b", open(HEADER).read())
