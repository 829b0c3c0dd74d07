"""CPU: the layout of mcp_mlp_hist and the value of MCP_MAX_HIST, through gcc on include/mcpilco_hip.h, against the ctypes mirror
(mc_pilco_amd.hipabi.MLPHist, MAX_HIST) -- as tests/test_abi_cpu.py does for the other structs -- and the two entries' declarations."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcpilco_hip.h")


def test_struct_layout_and_limit_against_the_header(tmp_path):
    from mc_pilco_amd import hipabi

    names = [n for n, _ in hipabi.MLPHist._fields_]
    assert names == ["h"]
    src = tmp_path / "hz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(void){printf("%zu", sizeof(mcp_mlp_hist));'
                   + "".join('printf(" %%zu %%zu", offsetof(mcp_mlp_hist, %s), sizeof(((mcp_mlp_hist*)0)->%s));' % (n, n) for n in names)
                   + 'printf(" %d %d %d", MCP_MAX_HIST, MCP_MAX_PFEAT, MCP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "hz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(hipabi.MLPHist) == 4
    assert out[1:3] == [hipabi.MLPHist.h.offset, C.sizeof(C.c_int32)]
    assert out[3:] == [hipabi.MAX_HIST, hipabi.MAX_PFEAT, hipabi.ABI_VERSION] == [4, 32, 7]


def test_the_entries_are_declared_bound_and_exported():
    from mc_pilco_amd import hipabi

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = hipabi.lib()
    for name, behind in (("mcp_rollout_mlp_hist", "mcp_rollout_mlp_res"), ("mcp_rollout_mlp_hist_bwd", "mcp_rollout_mlp_res_bwd")):
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, txt).group(1)
        old = re.search(r"\bint %s\s*\(([^;]*)\);" % behind, txt).group(1)
        types = lambda d: [re.sub(r"\s*\w+$", "", a.strip()) for a in d.split(",")]
        assert types(decl) == types(old)[:2] + ["const mcp_mlp_hist*"] + types(old)[2:]  # the residual entry's arguments with `hist` behind `mlp`
        assert name in hipabi.EXPORTED and hasattr(lib, name)
        sig, sig_old = hipabi._SIGS[name][1], hipabi._SIGS[behind][1]
        assert sig[:2] == sig_old[:2] and sig[2] is C.POINTER(hipabi.MLPHist) and sig[3:] == sig_old[2:]
