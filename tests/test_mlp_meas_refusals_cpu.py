"""CPU: the C ABI of the fused closed loop under the tanh-MLP policy on a simulated measurement (mcp_rollout_mlp_meas,
mcp_rollout_mlp_meas_bwd): the exports, and what the two entries refuse, with which code.  A refused call returns before any HIP call, so
the library answers without a GPU; device pointers are dummy non-NULL addresses that nothing reads (tests/test_mlp_refusals_cpu.py).  The
status word is host memory here: a refused call leaves it alone.

Every expected code is written out: 0 MCP_OK, -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  Order of the checks: NULL pointers (meas NULL included) and
M / T (-1), the model's compiled limits (-2), the model (-1), the descriptor (its limits -2, then -1), the measurement (-1), then, the sweep
only, "nothing asked for" (0, no launch).  meas->n == 0: the plain entry's own checks on the same arguments."""
import ctypes as C

import pytest

from test_mlp_refusals_cpu import mlp_desc
from test_open_refusals_cpu import PTR, M, T, abi, model

SIGS = {
    "mlp_meas": ("model", "mlp", "meas", "noise", "M", "T", "particle_pred", "x0", "states", "inputs", "mu", "var", "jac", "status"),
    "mlp_meas_bwd": ("model", "mlp", "meas", "M", "T", "states", "inputs", "jac", "g_states", "g_inputs", "g_params", "g_x0"),
}
REQUIRED = {"mlp_meas": ("model", "mlp", "meas", "noise", "x0", "states", "inputs", "status"),
            "mlp_meas_bwd": ("model", "mlp", "meas", "states", "inputs", "jac", "g_states")}
OPTIONAL = ("mu", "var", "g_inputs", "g_params", "g_x0")
BOTH = ("mlp_meas", "mlp_meas_bwd")
STATUS = (C.c_uint32 * 1)(0xABCD)


def meas_desc(n=1, **edit):
    """A valid measurement model over model(U): U = 1 measures (0, 1), n = 2 on model(2) measures (0, 2) and (1, 3)."""
    ms = abi().Meas()
    ms.n = n
    pairs = ((0, 1),) if n == 1 else ((0, 2), (1, 3))
    for i, (p, v) in enumerate(pairs[:max(n, 0)]):
        ms.pos[i], ms.vel[i], ms.std_pos[i] = p, v, 0.1
    ms.b0, ms.b1, ms.a0, ms.a1 = 0.42, 0.31, 1.25, -0.38
    ms.meas = PTR
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(ms, k)[v[0]] = v[1]
        else:
            setattr(ms, k, v)
    return ms


def call(entry, **over):
    a = abi()
    args = dict(model=model(), mlp=mlp_desc(), meas=meas_desc(), noise=a.Noise(), M=M, T=T, particle_pred=1, status=C.cast(STATUS, C.c_void_p))
    args.update(over)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL or (name == "jac" and entry == "mlp_meas") else PTR)
    return getattr(a.lib(), "mcp_rollout_" + entry)(*vals, None)


def codes(**over):
    return {e: call(e, **over) for e in BOTH}


def both(code):
    return {e: code for e in BOTH}


def two(**edit):
    """model(U = 2), its descriptor and both pairs measured, the measurement edited."""
    return dict(model=model(U=2), mlp=mlp_desc(U=2, hidden=(7, 3)), meas=meas_desc(2, **edit))


def test_exports_and_binding():
    a = abi()
    assert "mcp_rollout_mlp_meas" in a.EXPORTED and "mcp_rollout_mlp_meas_bwd" in a.EXPORTED
    lib = a.lib()
    assert hasattr(lib, "mcp_rollout_mlp_meas") and hasattr(lib, "mcp_rollout_mlp_meas_bwd")
    assert lib.mcp_abi_version() == a.ABI_VERSION == 7
    # the argument lists are the plain entries' with the measurement behind the policy descriptor
    for name in ("mcp_rollout_mlp", "mcp_rollout_mlp_bwd"):
        plain, meas = a._SIGS[name][1], a._SIGS[name.replace("mlp", "mlp_meas")][1]
        assert meas[:2] == plain[:2] and meas[2] is C.POINTER(a.Meas) and meas[3:] == plain[2:]


def test_the_sweep_accepts_valid_arguments_with_nothing_asked_for():
    assert call("mlp_meas_bwd") == 0
    assert call("mlp_meas_bwd", **two()) == 0
    assert call("mlp_meas_bwd", T=1, jac=None) == 0
    assert call("mlp_meas_bwd", T=2, jac=None) == -1
    assert STATUS[0] == 0xABCD


@pytest.mark.parametrize("entry", BOTH)
def test_null_pointers(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
    assert STATUS[0] == 0xABCD


def test_measurement_errors():
    assert codes(meas=meas_desc(pos=(0, 4))) == both(-1)  # a pair index out of range
    assert codes(meas=meas_desc(vel=(0, -1))) == both(-1)
    assert codes(**two(pos=(1, 0))) == both(-1)  # a position in two pairs
    assert codes(**two(vel=(1, 2))) == both(-1)  # a velocity in two pairs
    assert codes(**two(vel=(1, 0))) == both(-1)  # a component listed as both
    assert codes(meas=meas_desc(meas=None)) == both(-1)
    assert codes(meas=meas_desc(a0=0.0)) == both(-1)
    assert codes(meas=meas_desc(a0=float("nan"))) == both(-1)
    assert codes(model=model(Ts=0.0)) == both(-1)
    assert codes(model=model(Ts=float("nan"))) == both(-1)
    assert codes(meas=meas_desc(n=-1)) == both(-1)
    assert codes(meas=meas_desc(n=3)) == both(-1)  # more pairs than S / 2
    assert STATUS[0] == 0xABCD


def test_precedence():
    assert codes(meas=None, model=model(S=17)) == both(-1)  # NULL pointers before limits
    assert codes(model=model(S=17), meas=meas_desc(a0=0.0)) == both(-2)  # limits before arguments
    assert codes(mlp=mlp_desc(hidden=(65,)), meas=meas_desc(a0=0.0)) == both(-2)  # MCP_MAX_HIDDEN before the measurement
    assert codes(model=model(angle=(0, 9)), mlp=mlp_desc(hidden=(65,))) == both(-1)  # the model before the descriptor
    assert codes(mlp=mlp_desc(n_hidden=3), meas=meas_desc(pos=(0, 4))) == both(-1)
    assert call("mlp_meas_bwd", meas=meas_desc(a0=0.0)) == -1  # a bad measurement is refused even when nothing is asked for
    assert STATUS[0] == 0xABCD


def test_no_pairs_reaches_the_plain_entrys_own_checks():
    """meas->n == 0: nothing of the measurement is looked at (no buffer, a zeroed filter, Ts = 0 are no errors), and the refusals are
    mcp_rollout_mlp's and mcp_rollout_mlp_bwd's with their codes."""
    from test_mlp_refusals_cpu import call as plain

    none = abi().Meas()
    assert call("mlp_meas_bwd", meas=none) == 0
    assert call("mlp_meas_bwd", meas=none, model=model(Ts=0.0)) == 0
    for over in (dict(mlp=mlp_desc(hidden=(65,))), dict(mlp=mlp_desc(U=2)), dict(model=model(S=17)), dict(mlp=mlp_desc(u_max=(0, 0.0))), dict(M=0),
                 dict(model=model(gp_N=4097, gp_Npad=4112))):
        assert codes(meas=none, **over) == {"mlp_meas": plain("mlp", **over), "mlp_meas_bwd": plain("mlp_bwd", **over)}, over
    assert STATUS[0] == 0xABCD
