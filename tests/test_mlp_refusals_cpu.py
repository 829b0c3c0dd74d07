"""CPU: the C ABI of the fused closed loop under the tanh-MLP policy (mcp_rollout_mlp, mcp_rollout_mlp_bwd): the exports, the layout of
mcp_mlp_policy against the ctypes mirror, and what the two entries refuse, with which code.  A refused call returns before any HIP call, so
the library answers without a GPU; device pointers are dummy non-NULL addresses that nothing reads (tests/test_open_refusals_cpu.py).

Every expected code is written out: 0 MCP_OK, -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  Order of the checks: NULL pointers and M / T (-1), the
model's compiled limits (-2), the model (-1), the descriptor -- its compiled limits (-2: U, S, P, then after n_hidden (-1) the widths), then
everything else (-1) --, then, the sweep only, "nothing asked for" (0, no launch).  The forward entry launches whenever it accepts, so
every forward call here is a refusal."""
import ctypes as C
import os
import subprocess

import pytest

from test_open_refusals_cpu import PTR, REPEATED_INDEX, M, T, abi, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = {
    "mlp": ("model", "mlp", "noise", "M", "T", "particle_pred", "x0", "states", "inputs", "mu", "var", "jac", "status"),
    "mlp_bwd": ("model", "mlp", "M", "T", "states", "inputs", "jac", "g_states", "g_inputs", "g_params", "g_x0"),
}
REQUIRED = {"mlp": ("model", "mlp", "noise", "x0", "states", "inputs", "status"), "mlp_bwd": ("model", "mlp", "states", "inputs", "jac", "g_states")}
OPTIONAL = ("mu", "var", "g_inputs", "g_params", "g_x0")
BOTH = ("mlp", "mlp_bwd")


def mlp_desc(U=1, hidden=(5,), lists=True, **edit):
    """A valid descriptor over model(U): the model's own feature lists (or none), squashed at 1."""
    p = abi().MLPPolicy()
    ang, nang = ([2], [0, 1, 3]) if U == 1 else ([0, 1], [2, 3])
    p.S, p.U, p.n_hidden, p.squash = 4, U, len(hidden), 1
    for l, h in enumerate(hidden):
        p.h[l] = h
    if lists:
        p.n_angle, p.n_non_angle = len(ang), len(nang)
        for i, v in enumerate(ang):
            p.angle[i] = v
        for i, v in enumerate(nang):
            p.non_angle[i] = v
    p.P = len(nang) + 2 * len(ang) if lists else 4
    for k in range(min(U, abi().MAX_INPUT)):
        p.u_max[k] = 1.0
    for sl in ((0, 2) if len(hidden) == 1 else (0, 1, 2)):
        p.W[sl], p.b[sl] = PTR, PTR
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def call(entry, **over):
    a = abi()
    args = dict(model=model(), mlp=mlp_desc(), noise=a.Noise(), M=M, T=T, particle_pred=1)
    args.update(over)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL or (name == "jac" and entry == "mlp") else PTR)
    return getattr(a.lib(), "mcp_rollout_" + entry)(*vals, None)


def codes(**over):
    return {e: call(e, **over) for e in BOTH}


def both(code):
    return {e: code for e in BOTH}


def test_exports_and_version():
    a = abi()
    assert "mcp_rollout_mlp" in a.EXPORTED and "mcp_rollout_mlp_bwd" in a.EXPORTED
    lib = a.lib()
    assert hasattr(lib, "mcp_rollout_mlp") and hasattr(lib, "mcp_rollout_mlp_bwd")
    assert lib.mcp_abi_version() == a.ABI_VERSION == 7


def test_struct_layout_against_the_header(tmp_path):
    a = abi()
    names = [n for n, _ in a.MLPPolicy._fields_]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(void){printf("%zu", sizeof(mcp_mlp_policy));'
                   + "".join('printf(" %%zu", offsetof(mcp_mlp_policy, %s));' % n for n in names)
                   + 'printf(" %d %d", MCP_MAX_HIDDEN, MCP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(a.MLPPolicy)
    assert out[1:1 + len(names)] == [getattr(a.MLPPolicy, n).offset for n in names]
    assert out[-2:] == [a.MAX_HIDDEN, a.ABI_VERSION] == [64, 7]


def test_the_sweep_accepts_valid_arguments_with_nothing_asked_for():
    assert call("mlp_bwd") == 0
    assert call("mlp_bwd", mlp=mlp_desc(hidden=(64, 64))) == 0
    assert call("mlp_bwd", mlp=mlp_desc(lists=False)) == 0  # f = x
    assert call("mlp_bwd", model=model(U=2), mlp=mlp_desc(U=2, hidden=(7, 3))) == 0
    assert call("mlp_bwd", T=1, jac=None) == 0  # the policy alone has no record
    assert call("mlp_bwd", T=2, jac=None) == -1


@pytest.mark.parametrize("entry", BOTH)
def test_null_pointers(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
    # a missing layer pointer: the two the widths name (one hidden layer: slots 0 and 2; the middle slot is not looked at)
    for sl in (0, 2):
        assert call(entry, mlp=mlp_desc(W=(sl, None))) == -1
        assert call(entry, mlp=mlp_desc(b=(sl, None))) == -1
    assert call(entry, mlp=mlp_desc(hidden=(5, 5), W=(1, None))) == -1
    assert call(entry, mlp=mlp_desc(hidden=(5, 5), b=(1, None))) == -1
    assert call("mlp_bwd", mlp=mlp_desc(W=(1, None), b=(1, None))) == 0


def test_sizes():
    assert codes(M=0) == both(-1)
    assert codes(M=-2) == both(-1)
    assert codes(T=0) == both(-1)


def test_compiled_limits():
    for edit in (dict(S=17), dict(U=9), dict(G=9), dict(D=33)):
        assert codes(model=model(**edit)) == both(-2), edit
    assert codes(model=model(gp_N=4097, gp_Npad=4112)) == {"mlp": -2, "mlp_bwd": 0}  # the sweep never reads a GP descriptor
    assert codes(mlp=mlp_desc(U=9)) == both(-2)
    assert codes(mlp=mlp_desc(S=17)) == both(-2)
    assert codes(mlp=mlp_desc(P=33)) == both(-2)
    assert codes(mlp=mlp_desc(hidden=(65,))) == both(-2)
    assert codes(mlp=mlp_desc(hidden=(5, 65))) == both(-2)
    assert call("mlp_bwd", mlp=mlp_desc(hidden=(5,), h=(1, 65))) == 0  # h[1] is not read with one hidden layer
    assert codes(mlp=mlp_desc(n_angle=17)) == both(-2)
    assert codes(mlp=mlp_desc(n_non_angle=17)) == both(-2)


def test_descriptor_errors():
    assert codes(mlp=mlp_desc(U=2)) == both(-1)  # not the model's U
    assert codes(mlp=mlp_desc(U=0)) == both(-1)
    assert codes(mlp=mlp_desc(S=3)) == both(-1)  # not the model's S
    assert codes(mlp=mlp_desc(n_hidden=0)) == both(-1)
    assert codes(mlp=mlp_desc(n_hidden=3)) == both(-1)
    assert codes(mlp=mlp_desc(hidden=(0,))) == both(-1)
    assert codes(mlp=mlp_desc(hidden=(5, 0))) == both(-1)
    assert codes(mlp=mlp_desc(hidden=(-4,))) == both(-1)
    assert codes(mlp=mlp_desc(angle=(0, 4))) == both(-1)  # out of range
    assert codes(mlp=mlp_desc(non_angle=(1, -1))) == both(-1)
    assert codes(mlp=mlp_desc(non_angle=(1, 0))) == both(-1)  # listed twice among the non-angles
    assert codes(mlp=mlp_desc(angle=(0, 3))) == both(-1)  # listed as an angle and as a non-angle
    assert codes(mlp=mlp_desc(P=4)) == both(-1)  # P is n_non_angle + 2 n_angle
    assert codes(mlp=mlp_desc(lists=False, P=5)) == both(-1)  # without lists P is S
    assert codes(mlp=mlp_desc(n_angle=-1)) == both(-1)
    assert codes(mlp=mlp_desc(u_max=(0, 0.0))) == both(-1)  # squash needs u_max > 0
    assert codes(mlp=mlp_desc(u_max=(0, float("nan")))) == both(-1)
    assert call("mlp_bwd", mlp=mlp_desc(u_max=(0, 0.0), squash=0)) == 0  # without squashing u_max is not read


@pytest.mark.parametrize("edit", REPEATED_INDEX, ids=str)
def test_a_model_index_listed_twice(edit):
    """The model's lists name a component once per role (tests/test_open_refusals_cpu.py), as the policy's do above; a policy without
    lists of its own changes nothing about that."""
    assert codes(model=model(**edit)) == both(-1)
    assert codes(model=model(**edit), mlp=mlp_desc(lists=False)) == both(-1)


def test_precedence():
    assert codes(M=0, model=model(S=17)) == both(-1)  # sizes before limits
    assert codes(model=model(S=17, angle=(0, 9))) == both(-2)  # the model's limits before its lists
    assert codes(model=model(angle=(0, 9)), mlp=mlp_desc(U=9)) == both(-1)  # the model before the descriptor
    assert codes(mlp=mlp_desc(U=9, angle=(0, 4))) == both(-2)  # the descriptor's limits before its other errors
    assert codes(mlp=mlp_desc(hidden=(65,), u_max=(0, 0.0))) == both(-2)
    assert codes(mlp=mlp_desc(hidden=(65,), n_hidden=3)) == both(-1)  # n_hidden says which widths count: looked at before them
    assert call("mlp_bwd", mlp=mlp_desc(u_max=(0, 0.0))) == -1  # a bad descriptor is refused even when nothing is asked for
