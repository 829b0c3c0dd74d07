"""CPU: the layout of mcp_tvl_policy through gcc on include/mcpilco_hip.h against the ctypes mirror (mc_pilco_amd.hipabi.TVLPolicy) -- as
tests/test_abi_hist_cpu.py does for mcp_mlp_hist -- the two entries' declarations against their bindings, the header and the binding naming
the same set of entries, and the ABI version, which this struct and these entries leave at 7."""
import ctypes as C
import os
import re
import subprocess

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcpilco_hip.h")
FIELDS = ["U", "S", "squash", "gain_rows", "ff_rows", "target_rows", "u_max", "gain", "ff", "target_traj"]


def test_struct_layout_against_the_header(tmp_path):
    from mc_pilco_amd import hipabi

    names = [n for n, _ in hipabi.TVLPolicy._fields_]
    assert names == FIELDS
    src = tmp_path / "tv.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(void){printf("%zu", sizeof(mcp_tvl_policy));'
                   + "".join('printf(" %%zu %%zu", offsetof(mcp_tvl_policy, %s), sizeof(((mcp_tvl_policy*)0)->%s));' % (n, n) for n in names)
                   + 'printf(" %d %d %d", MCP_MAX_INPUT, MCP_MAX_STATE, MCP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "tv"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(hipabi.TVLPolicy) == 6 * 4 + 8 * 8 + 3 * 8
    for i, n in enumerate(names):
        f = getattr(hipabi.TVLPolicy, n)
        assert out[1 + 2 * i:3 + 2 * i] == [f.offset, f.size], n
    assert out[-3:] == [hipabi.MAX_INPUT, hipabi.MAX_STATE, hipabi.ABI_VERSION] == [8, 16, 7]


def test_the_entries_are_declared_bound_and_exported():
    """The forward entry is mcp_rollout_pd_meas's argument list with the descriptor exchanged, the sweep mcp_rollout_pd_meas_bwd's."""
    from mc_pilco_amd import hipabi

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = hipabi.lib()
    types = lambda d: [re.sub(r"\s*\w+$", "", a.strip()) for a in d.split(",")]
    for name, twin in (("mcp_rollout_tvl", "mcp_rollout_pd_meas"), ("mcp_rollout_tvl_bwd", "mcp_rollout_pd_meas_bwd")):
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, txt).group(1)
        old = re.search(r"\bint %s\s*\(([^;]*)\);" % twin, txt).group(1)
        assert types(decl) == [types(old)[0], "const mcp_tvl_policy*"] + types(old)[2:]
        assert name in hipabi.EXPORTED and hasattr(lib, name)
        sig, sig_old = hipabi._SIGS[name][1], hipabi._SIGS[twin][1]
        assert sig[0] == sig_old[0] and sig[1] is C.POINTER(hipabi.TVLPolicy) and sig[2:] == sig_old[2:]


def test_header_and_binding_name_the_same_entries_and_the_version_stays():
    from mc_pilco_amd import hipabi

    assert set(hipabi.EXPORTED) == set(declared_symbols())
    assert hipabi.lib().mcp_abi_version() == hipabi.ABI_VERSION == 7
    txt = open(HEADER).read()
    assert re.search(r"#define MCP_ABI_VERSION 7\b", txt)
