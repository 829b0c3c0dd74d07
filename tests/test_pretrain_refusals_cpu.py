"""CPU: what the thirteen pretrain / training entry points refuse, and with which code (mcp_cov_build, mcp_cov_diag, mcp_gp_alpha, mcp_gp_pack;
mcp_chol_factor, mcp_chol_inverse, mcp_sym_sandwich; mcp_sod_workspace_bytes, mcp_sod_select; mcp_nll_workspace_bytes, mcp_nll_grad,
mcp_nll_epoch_workspace_bytes, mcp_nll_epoch).  A refused call returns before any HIP call, so the library answers without a GPU; the device
pointers are dummy non-NULL addresses that nothing reads, the stream is always NULL.

Every expected code is written out: -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT, -3 MCP_ERR_WORKSPACE.  NOTHING here passes validation: without a
device that would be a launch attempt.  Left out for that reason: mcp_nll_epoch's MCP_ERR_LIMIT for a Gram stage whose LDS need exceeds
150 KiB (it is tested after the first launch, and no D <= MCP_MAX_GPDIM reaches it), and launch_chol_blocked's own MCP_ERR_LIMIT (no N that
mcp_chol_factor sends there meets it).  The byte counts of the three size queries are literals."""
import ctypes as C

import pytest

PTR, PTR2, PTR3, PTR4 = 0x1000, 0x2000, 0x3000, 0x4000  # stand for device memory: never dereferenced by a refused call
N, D = 20, 6
BIG = 1 << 40  # a workspace size that is never the reason

# argument names of each entry, in call order ("stream" is always NULL and not listed)
SIGS = {
    "cov_build": ("kern", "N1", "X1", "N2", "X2", "add_noise", "K", "ldk"),
    "cov_diag": ("kern", "N", "X", "add_noise", "diag"),
    "chol_factor": ("N", "A", "lda", "logdet", "status"),
    "chol_inverse": ("N", "U", "ldu", "Uinv", "ldi", "Kinv", "ldk"),
    "sym_sandwich": ("N", "A", "lda", "G", "ldg", "out", "ldo", "scratch"),
    "gp_alpha": ("N", "Kinv", "ldk", "Y", "mean", "alpha"),
    "gp_pack": ("N", "D", "X", "alpha", "Kinv", "ldk", "Npad", "Xt_out", "X_out", "alpha_out", "Kinv_out", "aX_out"),
    "sod_select": ("kern", "N", "X", "threshold", "idx_out", "n_out", "workspace", "workspace_bytes"),
    "nll_grad": ("kern", "N", "X", "Kinv", "ldk", "alpha", "grad", "workspace", "workspace_bytes"),
    "nll_epoch": ("n_gp", "gps", "N", "D", "poly_deg", "ard", "X", "status", "workspace", "workspace_bytes"),
}
POINTERS = {
    "cov_build": ("kern", "X1", "X2", "K"),
    "cov_diag": ("kern", "X", "diag"),
    "chol_factor": ("A", "logdet", "status"),
    "chol_inverse": ("U", "Uinv", "Kinv"),
    "sym_sandwich": ("A", "G", "out", "scratch"),
    "gp_alpha": ("Kinv", "Y", "alpha"),
    "gp_pack": ("X", "alpha", "Kinv", "Xt_out", "X_out", "alpha_out", "Kinv_out", "aX_out"),
    "sod_select": ("kern", "X", "idx_out", "n_out", "workspace"),
    "nll_grad": ("kern", "X", "Kinv", "alpha", "grad", "workspace"),
    "nll_epoch": ("gps", "X", "status", "workspace"),
}
SIZES = ("N", "N1", "N2", "lda", "ldu", "ldi", "ldk", "ldg", "ldo")  # every one of them N by default
WITH_KERNEL = ("cov_build", "cov_diag", "sod_select", "nll_grad")
DISTINCT = {"A": PTR, "G": PTR2, "out": PTR3, "scratch": PTR4}  # mcp_sym_sandwich refuses aliased buffers


def abi():
    from mc_pilco_amd import hipabi

    return hipabi


def kernel(**edit):
    """A valid descriptor of degree 0 over D inputs; ``edit``: field = value."""
    k = abi().Kernel()
    k.D, k.poly_deg, k.lam, k.inv_ls = D, 0, 1.0, PTR
    for name, v in edit.items():
        setattr(k, name, v)
    return k


def nll_gps(G=2, **edit):
    """G valid raw-parameter descriptors of degree 0 (host memory: the entry copies them); ``edit`` goes into the LAST one."""
    gps = (abi().NllGP * max(G, 1))()
    for gp in gps:
        gp.log_ls, gp.log_lambda, gp.Y = PTR, PTR, PTR
    for name, v in edit.items():
        setattr(gps[max(G, 1) - 1], name, v)
    return gps


def call(entry, **over):
    """The entry on valid arguments (N 20, D 6, two GPs, every buffer a dummy address, a workspace that is large enough) with ``over`` put in."""
    args = dict(kern=kernel(), D=D, n_gp=2, gps=nll_gps(), poly_deg=0, ard=1, add_noise=1, mean=0.0, threshold=0.5, Npad=32, workspace_bytes=BIG)
    args.update(over)
    n = args.get("N", N)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else C.addressof(v) if isinstance(v, C.Array) else v)
        elif name in SIZES:
            vals.append(n)
        else:
            vals.append(DISTINCT.get(name, PTR))
    return getattr(abi().lib(), "mcp_" + entry)(*vals, None)


@pytest.mark.parametrize("entry", sorted(SIGS))
def test_null_pointers(entry):
    for name in POINTERS[entry]:
        assert call(entry, **{name: None}) == -1, name


def test_sizes():
    for bad in (0, -3):
        assert call("cov_build", N1=bad) == -1
        assert call("cov_build", N2=bad) == -1
        for entry in ("cov_diag", "chol_factor", "chol_inverse", "sym_sandwich", "gp_alpha", "gp_pack", "sod_select", "nll_grad", "nll_epoch"):
            assert call(entry, N=bad) == -1, entry
    assert call("cov_build", ldk=N - 1) == -1  # ldk against N2, not N1
    assert call("chol_factor", lda=N - 1) == -1
    for ld in ("ldu", "ldi", "ldk"):
        assert call("chol_inverse", **{ld: N - 1}) == -1, ld
    for ld in ("lda", "ldg", "ldo"):
        assert call("sym_sandwich", **{ld: N - 1}) == -1, ld
    assert call("gp_alpha", ldk=N - 1) == -1
    assert call("nll_grad", ldk=N - 1) == -1
    assert call("gp_pack", ldk=N - 1) == -1
    assert call("gp_pack", D=0) == -1
    assert call("gp_pack", D=33) == -1  # over MCP_MAX_GPDIM: an argument error here, not a limit
    assert call("gp_pack", Npad=16) == -1  # Npad < N
    assert call("gp_pack", Npad=24) == -1  # not a multiple of 16
    assert call("nll_epoch", n_gp=0) == -1
    assert call("nll_epoch", n_gp=-1) == -1
    assert call("nll_epoch", D=0) == -1


@pytest.mark.parametrize("edit", [dict(D=0), dict(D=-1), dict(D=33), dict(poly_deg=3), dict(poly_deg=-1), dict(inv_ls=None), dict(poly_deg=1),
                                  dict(poly_deg=2, w1=PTR, w20=PTR), dict(poly_deg=2, w1=PTR, w21=PTR), dict(poly_deg=2, w20=PTR, w21=PTR)], ids=str)
def test_kernel_descriptor(edit):
    """D = 0 and MCP_MAX_GPDIM + 1, a degree outside 0..2, no lengthscales, degree 1 without w1, degree 2 without w21 / w20 / w1."""
    assert {e: call(e, kern=kernel(**edit)) for e in WITH_KERNEL} == {"cov_build": -1, "cov_diag": -1, "sod_select": -1, "nll_grad": -1}


def test_limits():
    assert call("chol_factor", N=8193) == -2
    assert call("chol_inverse", N=16385) == -2
    assert call("sym_sandwich", N=16385) == -2
    assert call("sod_select", N=16385) == -2
    assert call("nll_grad", N=4097) == -2
    assert call("nll_epoch", N=1153) == -2  # the one-workgroup factorisation's last size is 1152
    assert call("nll_epoch", N=16) == -2  # the MFMA-blocked forms start at 17
    assert call("nll_epoch", N=1) == -2
    assert call("nll_epoch", n_gp=9, gps=nll_gps(9)) == -2  # MCP_MAX_GP + 1
    assert call("nll_epoch", D=33) == -2  # MCP_MAX_GPDIM + 1


def test_aliasing_of_sym_sandwich():
    assert call("sym_sandwich", out=PTR) == -1  # out == A
    assert call("sym_sandwich", out=PTR2) == -1  # out == G
    assert call("sym_sandwich", scratch=PTR) == -1  # scratch == A
    assert call("sym_sandwich", scratch=PTR2) == -1  # scratch == G
    assert call("sym_sandwich", scratch=PTR3) == -1  # scratch == out
    assert call("sym_sandwich", N=16385, out=PTR) == -2  # the limit is tested before the aliasing


def test_workspace_one_byte_short():
    lib = abi().lib()
    # SOD: the one-workgroup kernel's part is what is required (8 (N^2 + 2 N)); the multi-workgroup kernel's part is optional
    assert call("sod_select", workspace_bytes=8 * (20 * 20 + 40) - 1) == -3
    assert call("sod_select", N=300, workspace_bytes=8 * (300 * 300 + 600) - 1) == -3
    assert call("sod_select", workspace_bytes=0) == -3
    assert call("nll_grad", workspace_bytes=lib.mcp_nll_workspace_bytes(N, D) - 1) == -3
    assert call("nll_grad", workspace_bytes=4319) == -3  # 8 * 20 * 27 - 1
    assert call("nll_epoch", workspace_bytes=lib.mcp_nll_epoch_workspace_bytes(2, N, D) - 1) == -3
    assert call("nll_epoch", workspace_bytes=0) == -3


def test_order_of_the_checks():
    # mcp_sod_select: workspace before the limit
    assert call("sod_select", N=16385, workspace_bytes=100) == -3
    assert call("sod_select", N=0, workspace_bytes=0) == -1  # arguments before the workspace
    # mcp_nll_grad: arguments, limit, workspace
    assert call("nll_grad", N=4097, workspace_bytes=0) == -2
    assert call("nll_grad", N=4097, ldk=4096) == -1
    assert call("nll_grad", kern=kernel(D=33), workspace_bytes=0) == -1
    # mcp_nll_epoch: NULL / non-positive sizes, limits, degree, workspace, the descriptors' own pointers
    assert call("nll_epoch", N=1153, X=None) == -1
    assert call("nll_epoch", N=1153, poly_deg=3) == -2
    assert call("nll_epoch", poly_deg=3, workspace_bytes=0) == -1
    assert call("nll_epoch", poly_deg=-1) == -1
    assert call("nll_epoch", gps=nll_gps(log_ls=None), workspace_bytes=0) == -3
    # mcp_chol_factor / mcp_chol_inverse: arguments before the limit
    assert call("chol_factor", N=8193, lda=8192) == -1
    assert call("chol_inverse", N=16385, ldi=16384) == -1
    assert call("sym_sandwich", N=16385, scratch=None) == -1


def test_raw_parameter_descriptors_of_the_epoch():
    """Looked at after the workspace; every one of the G descriptors, not the first alone (the edits go into the last)."""
    for name in ("log_ls", "log_lambda", "Y"):
        assert call("nll_epoch", gps=nll_gps(**{name: None})) == -1, name
    assert call("nll_epoch", poly_deg=2, gps=nll_gps(mpk1=PTR)) == -1  # degree 2 without mpk2
    assert call("nll_epoch", poly_deg=2, gps=nll_gps(3, mpk2=None), n_gp=3) == -1


SIZES_N = (0, 255, 256, 4096, 4097)
SOD_BYTES = [0, 524280, 1085696, 276893696, 134348824]  # (from 256 to 4096 points the multi-workgroup kernel's granules and Gram matrix ride along)
NLL_BYTES = [0, 55080, 55296, 884736, 884952]  # D = 6: 8 N (4 D + 3)
EPOCH_BYTES = [0, 3240720, 3265616, 807208016, 807601840]  # G = 2, D = 6
EPOCH_BYTES_G8_D32 = 264768  # N = 20


def test_size_queries():
    lib = abi().lib()
    assert [lib.mcp_sod_workspace_bytes(n) for n in SIZES_N] == SOD_BYTES
    assert [lib.mcp_nll_workspace_bytes(n, D) for n in SIZES_N] == NLL_BYTES
    assert [lib.mcp_nll_epoch_workspace_bytes(2, n, D) for n in SIZES_N] == EPOCH_BYTES
    assert lib.mcp_sod_workspace_bytes(-1) == 0
    assert lib.mcp_nll_workspace_bytes(N, 0) == 0
    assert lib.mcp_nll_workspace_bytes(-1, D) == 0
    assert [lib.mcp_nll_epoch_workspace_bytes(*a) for a in ((0, N, D), (9, N, D), (2, N, 0), (2, N, 33), (2, -1, D))] == [0, 0, 0, 0, 0]
    assert lib.mcp_nll_epoch_workspace_bytes(8, N, 32) == EPOCH_BYTES_G8_D32
