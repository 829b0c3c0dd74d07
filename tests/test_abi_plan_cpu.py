"""CPU: the layout of mcp_plan_ext through gcc on include/mcpilco_hip.h against the ctypes mirror (mc_pilco_amd.hipabi.PlanExt), as
tests/test_abi_mppi_cpu.py does for mcp_mppi; the three entries of the planner's extension (mcp_plan_rollout, mcp_mppi_update_ext,
mcp_cem_update) declared in the header, bound with the declaration's argument list and exported by the library; the new limit restated in
the binding; the ABI version, which this struct and these entries leave at 7; and mcp_mppi, which they leave alone."""
import ctypes as C
import os
import re
import subprocess

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcpilco_hip.h")
FIELDS = ["sigma_rows", "u_prev", "beta", "alpha", "sigma_min", "n_elite"]
PTRS = {"const mcp_model*": "Model", "const mcp_mppi*": "MPPI", "const mcp_plan_ext*": "PlanExt", "const mcp_cost*": "Cost",
        "const mcp_cost_inputs*": "CostInputs", "const mcp_noise*": "Noise"}
CTYPE = {"int": C.c_int, "const double*": C.c_void_p, "double*": C.c_void_p, "int32_t*": C.c_void_p, "uint32_t*": C.c_void_p, "void*": C.c_void_p}
ENTRIES = (("mcp_plan_rollout", 13, "const mcp_model*"), ("mcp_mppi_update_ext", 10, "const mcp_mppi*"), ("mcp_cem_update", 11, "const mcp_mppi*"))


def test_struct_layout_against_the_header(tmp_path):
    from mc_pilco_amd import hipabi

    names = [n for n, _ in hipabi.PlanExt._fields_]
    assert names == FIELDS
    src = tmp_path / "pe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(void){printf("%zu", sizeof(mcp_plan_ext));'
                   + "".join('printf(" %%zu %%zu", offsetof(mcp_plan_ext, %s), sizeof(((mcp_plan_ext*)0)->%s));' % (n, n) for n in names)
                   + 'printf(" %zu %d %d %d", sizeof(mcp_mppi), MCP_MAX_INPUT, MCP_CEM_MAX_ELITE, MCP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "pe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    # two pointers, two doubles, one array of MCP_MAX_INPUT doubles, one int (+ 4 bytes of padding)
    assert out[0] == C.sizeof(hipabi.PlanExt) == 2 * 8 + 2 * 8 + 8 * 8 + 8
    for i, n in enumerate(names):
        f = getattr(hipabi.PlanExt, n)
        assert out[1 + 2 * i:3 + 2 * i] == [f.offset, f.size], n
    assert out[-4:] == [C.sizeof(hipabi.MPPI), hipabi.MAX_INPUT, hipabi.CEM_MAX_ELITE, hipabi.ABI_VERSION] == [200, 8, 1024, 7]


def test_the_entries_are_declared_bound_and_exported():
    from mc_pilco_amd import hipabi

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = hipabi.lib()
    for name, n_args, first in ENTRIES:
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, txt).group(1)
        types = [re.sub(r"\s*\w+$", "", a.strip()) for a in decl.split(",")]
        assert len(types) == n_args and types[0] == first and types[-1] == "void*" and types[-2] == "uint32_t*"
        res, sig = hipabi._SIGS[name]
        assert res is C.c_int and len(sig) == n_args
        for t, s in zip(types, sig):
            assert s is (C.POINTER(getattr(hipabi, PTRS[t])) if t in PTRS else CTYPE[t]), (name, t)
        assert name in hipabi.EXPORTED and name in declared_symbols() and hasattr(lib, name)
    # the extension sits behind the plan in every entry; the rollout's further arguments are mcp_mppi_rollout's
    assert all(hipabi._SIGS[name][1][2 if name == "mcp_plan_rollout" else 1] is C.POINTER(hipabi.PlanExt) for name, _, _ in ENTRIES)
    old, new = hipabi._SIGS["mcp_mppi_rollout"][1], hipabi._SIGS["mcp_plan_rollout"][1]
    assert new[:2] + new[3:] == old
    old, new = hipabi._SIGS["mcp_mppi_update"][1], hipabi._SIGS["mcp_mppi_update_ext"][1]
    assert new[:1] + new[2:] == old


def test_header_and_binding_name_the_same_entries_and_the_version_stays():
    from mc_pilco_amd import hipabi

    assert set(hipabi.EXPORTED) == set(declared_symbols())
    assert hipabi.lib().mcp_abi_version() == hipabi.ABI_VERSION == 7
    txt = open(HEADER).read()
    assert re.search(r"#define MCP_ABI_VERSION 7\b", txt)
    assert int(re.search(r"#define MCP_CEM_MAX_ELITE (\d+)", txt).group(1)) == hipabi.CEM_MAX_ELITE == 1024
