"""The training epoch's plan without a GPU: `mcp_nll_epoch_plan` (include/mcpilco_hip_debug.h) -- the workspace map `mcp_nll_epoch` fills and
the gradient form it launches.  mcp_nll_epoch takes both from the same host function, so tests/test_gpu_nll_grad.py reads the epoch's own
operands at these offsets and asserts the form from this plan."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_HEADER = os.path.join(ROOT, "include", "mcpilco_hip_debug.h")
ORDER = ("K", "Uinv", "Kinv", "alpha", "r", "slab", "grad", "inv_ls", "w1", "w20", "w21", "scal", "logdet")  # the documented order


def plan(G, N, D):
    from mc_pilco_amd import hipabi

    p = hipabi.NllPlan()
    rc = hipabi.lib().mcp_nll_epoch_plan(G, N, D, C.byref(p))
    return rc, p


def test_plan_struct_layout_matches_the_debug_header(tmp_path):
    from mc_pilco_amd import hipabi

    hdr = open(DEBUG_HEADER).read()
    body = hdr[hdr.index("typedef struct mcp_nll_plan {"):hdr.index("} mcp_nll_plan;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = re.findall(r"^\s*(\w+)\s+([\w\s,]+);", body, re.M)
    assert decls and all(t == "int64_t" for t, _ in decls)
    names = [n.strip() for _, group in decls for n in group.split(",")]
    assert names == [f[0] for f in hipabi.NllPlan._fields_]
    src = tmp_path / "nz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip_debug.h"\nint main(){printf("%zu %d %d", sizeof(mcp_nll_plan), '
                   "MCP_NLL_GRAD_ROWS, MCP_NLL_GRAD_ROW_PER_WG);"
                   + "".join('printf(" %%zu", offsetof(mcp_nll_plan, %s));' % n for n in names) + "return 0;}\n")
    exe = tmp_path / "nz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(hipabi.NllPlan), hipabi.NLL_GRAD_ROWS, hipabi.NLL_GRAD_ROW_PER_WG] + [getattr(hipabi.NllPlan, n).offset for n in names]


@pytest.mark.parametrize("G,N,D", [(1, 17, 1), (1, 129, 6), (3, 530, 32), (6, 400, 24), (8, 1152, 13), (2, 257, 7)])
def test_workspace_map_is_the_documented_one(G, N, D):
    """Descriptors first (G mcp_kernel of 72 bytes, rounded up to 16), then G equal blocks; inside a block the documented order, every
    region rounded up to an even number of doubles; the end is mcp_nll_epoch_workspace_bytes."""
    from mc_pilco_amd import hipabi

    rc, p = plan(G, N, D)
    assert rc == 0
    assert C.sizeof(hipabi.Kernel) == 72
    assert p.first_gp == (G * 72 + 15) // 16 * 2
    NP = 4 * D + 3
    sizes = dict(K=N * N, Uinv=N * N, Kinv=N * N, alpha=N, r=N, slab=N * NP, grad=NP, inv_ls=D, w1=D + 1, w20=D, w21=D, scal=4, logdet=2)
    o = 0
    for name in ORDER:
        assert getattr(p, name) == o, name
        o += (sizes[name] + 1) // 2 * 2
    assert p.per_gp == o
    assert p.total == p.first_gp + G * p.per_gp
    assert 8 * p.total == hipabi.lib().mcp_nll_epoch_workspace_bytes(G, N, D)


def lds_rows(N, D):  # nll_grad_rows_lds (csrc/gp_nll.hip): four [N] row buffers, the weights, the inputs transposed at an odd pitch
    return 8 * (4 * N + 4 * D + 2 + D * (N | 1))


@pytest.mark.parametrize("N,D,form", [(681, 24, 1), (682, 24, 2), (529, 32, 1), (530, 32, 2), (1152, 12, 1), (1152, 13, 2), (129, 6, 1), (257, 8, 1),
                                      (1025, 6, 1), (1152, 15, 2), (17, 32, 1), (1152, 32, 2)])
def test_gradient_form_flips_where_the_rows_no_longer_fit_the_lds(N, D, form):
    from mc_pilco_amd import hipabi

    for G in (1, 3):
        rc, p = plan(G, N, D)
        assert rc == 0
        assert p.grad_form == form == (hipabi.NLL_GRAD_ROWS if lds_rows(N, D) <= 150 * 1024 else hipabi.NLL_GRAD_ROW_PER_WG)
        if form == hipabi.NLL_GRAD_ROWS:
            assert p.rows_per_wg == (N + 127) // 128 and p.slab_rows == (N + p.rows_per_wg - 1) // p.rows_per_wg
            assert p.lds_bytes == lds_rows(N, D)
        else:
            assert p.rows_per_wg == 1 and p.slab_rows == N and p.lds_bytes == 8 * (4 * N + 256)
        assert p.slab_rows <= N and p.lds_bytes <= 160 * 1024  # (the slab has N rows; the LDS of a gfx950 workgroup)


def test_plan_refuses_what_the_epoch_refuses():
    from mc_pilco_amd import hipabi

    assert hipabi.lib().mcp_nll_epoch_plan(1, 129, 6, None) == -1
    for (G, N, D), want in {(0, 129, 6): -1, (1, 0, 6): -1, (1, 129, 0): -1, (9, 129, 6): -2, (1, 16, 6): -2, (1, 1153, 6): -2, (1, 129, 33): -2}.items():
        assert plan(G, N, D)[0] == want, (G, N, D)
        # the epoch itself, asked the same: the sizes are validated before anything is launched (dummy non-null pointers, never followed)
        gps = (hipabi.NllGP * 8)()
        d = C.c_void_p(0x1000)
        assert hipabi.lib().mcp_nll_epoch(G, C.cast(gps, C.c_void_p), N, D, 0, 1, d, d, d, 1 << 40, None) == want, (G, N, D)
