"""CPU: the two trajectory-optimisation entries (mcp_linearize, mcp_lqr_pass) are declared in include/mcpilco_hip.h, bound in
mc_pilco_amd.hipabi with the declaration's argument list and exported by the library; the header and the binding name the same set of
entries; the ABI version stays 7 (the change is additive) -- as tests/test_abi_tvl_cpu.py does for the entries of mcp_tvl_policy."""
import ctypes as C
import os
import re

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcpilco_hip.h")
CTYPE = {"const mcp_model*": "model", "int": C.c_int, "double": C.c_double, "const double*": C.c_void_p, "double*": C.c_void_p,
         "uint32_t*": C.c_void_p, "void*": C.c_void_p}


def test_the_entries_are_declared_bound_and_exported():
    from mc_pilco_amd import hipabi

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = hipabi.lib()
    for name, n_args in (("mcp_linearize", 9), ("mcp_lqr_pass", 16)):
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, txt).group(1)
        types = [re.sub(r"\s*\w+$", "", a.strip()) for a in decl.split(",")]
        assert len(types) == n_args and types[0] == "const mcp_model*" and types[-1] == "void*"
        res, sig = hipabi._SIGS[name]
        assert res is C.c_int and len(sig) == n_args
        for t, s in zip(types, sig):
            assert s is (C.POINTER(hipabi.Model) if CTYPE[t] == "model" else CTYPE[t]), (name, t)
        assert name in hipabi.EXPORTED and name in declared_symbols() and hasattr(lib, name)
    assert hipabi._SIGS["mcp_lqr_pass"][1][10] is C.c_double  # reg, by value


def test_header_and_binding_name_the_same_entries_and_the_version_stays():
    from mc_pilco_amd import hipabi

    assert set(hipabi.EXPORTED) == set(declared_symbols())
    assert hipabi.lib().mcp_abi_version() == hipabi.ABI_VERSION == 7
    txt = open(HEADER).read()
    assert re.search(r"#define MCP_ABI_VERSION 7\b", txt)
    assert int(re.search(r"#define MCP_LQR_MAX_T (\d+)", txt).group(1)) == hipabi.LQR_MAX_T
