"""CPU: what mcp_rollout_tvl and mcp_rollout_tvl_bwd refuse, with which code, on the pattern of tests/test_open_refusals_cpu.py: a refused
call returns before any HIP call, so the library answers without a GPU; device pointers are dummy non-NULL addresses that nothing reads.

Every expected code is written out: 0 MCP_OK, -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  Order of the checks: NULL pointers and M / T (-1), the
model's compiled limits (-2), the model (-1), the descriptor -- its compiled limits first (-2: U > MCP_MAX_INPUT, S > MCP_MAX_STATE), then
everything else (-1) --, the measurement (-1), then, the sweep only, "nothing asked for" (0, no launch).  The forward entry launches whenever
it accepts, so every forward call here is a refusal."""
import ctypes as C

import pytest

from test_mlp_meas_refusals_cpu import meas_desc
from test_open_refusals_cpu import PTR, REPEATED_INDEX, M, T, abi, model

SIGS = {
    "tvl": ("model", "tvl", "meas", "noise", "M", "T", "particle_pred", "x0", "states", "inputs", "jac", "mu", "var", "status"),
    "tvl_bwd": ("model", "tvl", "meas", "M", "T", "states", "inputs", "jac", "g_states", "g_inputs", "g_part", "g_x0"),
}
REQUIRED = {"tvl": ("model", "tvl", "noise", "x0", "states", "inputs", "status"), "tvl_bwd": ("model", "tvl", "states", "inputs", "jac", "g_states")}
OPTIONAL = ("meas", "mu", "var", "g_inputs", "g_part", "g_x0")
BOTH = ("tvl", "tvl_bwd")


def tvl_desc(U=1, S=4, **edit):
    """A valid descriptor over model(U): time-varying gains and a feedforward of T + 1 rows, squashed at 1."""
    p = abi().TVLPolicy()
    p.U, p.S, p.squash, p.gain_rows, p.ff_rows, p.target_rows = U, S, 1, T + 1, T + 1, T + 2
    p.gain, p.ff, p.target_traj = PTR, PTR, PTR
    for k in range(abi().MAX_INPUT):
        p.u_max[k] = 1.0
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def call(entry, **over):
    a = abi()
    args = dict(model=model(), tvl=tvl_desc(), noise=a.Noise(), M=M, T=T, particle_pred=1)
    args.update(over)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL or (name == "jac" and entry == "tvl") else PTR)
    return getattr(a.lib(), "mcp_rollout_" + entry)(*vals, None)


def codes(**over):
    return {e: call(e, **over) for e in BOTH}


def both(code):
    return {e: code for e in BOTH}


def test_the_sweep_accepts_valid_arguments_with_nothing_asked_for():
    assert call("tvl_bwd") == 0
    assert call("tvl_bwd", tvl=tvl_desc(gain_rows=1)) == 0  # a shared gain
    assert call("tvl_bwd", tvl=tvl_desc(ff_rows=0, ff=None)) == 0  # no feedforward
    assert call("tvl_bwd", tvl=tvl_desc(gain_rows=T, ff_rows=T, target_rows=T)) == 0  # exactly T rows
    assert call("tvl_bwd", tvl=tvl_desc(squash=0, u_max=(0, 0.0))) == 0  # the bound is not read without squashing
    assert call("tvl_bwd", model=model(2), tvl=tvl_desc(2)) == 0
    assert call("tvl_bwd", meas=meas_desc()) == 0 and call("tvl_bwd", meas=meas_desc(n=0)) == 0
    assert call("tvl_bwd", T=1, jac=None, tvl=tvl_desc(gain_rows=1, ff_rows=1, target_rows=1)) == 0  # the policy alone has no record
    assert call("tvl_bwd", T=2, jac=None) == -1


@pytest.mark.parametrize("entry", BOTH)
def test_null_pointers_and_sizes(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
    assert call(entry, M=0) == -1 and call(entry, M=-3) == -1
    assert call(entry, T=0) == -1


def test_the_descriptor():
    assert codes(tvl=tvl_desc(U=9)) == both(-2)  # beyond MCP_MAX_INPUT
    assert codes(tvl=tvl_desc(S=17)) == both(-2)  # beyond MCP_MAX_STATE
    assert codes(tvl=tvl_desc(U=2)) == both(-1)  # not the model's
    assert codes(tvl=tvl_desc(U=0)) == both(-1)
    assert codes(tvl=tvl_desc(S=3)) == both(-1) and codes(tvl=tvl_desc(S=5)) == both(-1)
    assert codes(tvl=tvl_desc(target_rows=T - 1)) == both(-1)
    assert codes(tvl=tvl_desc(gain_rows=T - 1)) == both(-1)  # neither 1 nor >= T
    assert codes(tvl=tvl_desc(gain_rows=0)) == both(-1)
    assert codes(tvl=tvl_desc(ff_rows=T - 1)) == both(-1)  # neither 0 nor >= T
    assert codes(tvl=tvl_desc(ff_rows=1)) == both(-1)
    assert codes(tvl=tvl_desc(ff_rows=-1)) == both(-1)
    assert codes(tvl=tvl_desc(ff=None)) == both(-1)  # ff_rows > 0 with ff NULL
    assert codes(tvl=tvl_desc(gain=None)) == both(-1)
    assert codes(tvl=tvl_desc(target_traj=None)) == both(-1)
    assert codes(tvl=tvl_desc(u_max=(0, 0.0))) == both(-1)  # with squash
    assert codes(tvl=tvl_desc(u_max=(0, -1.0))) == both(-1)
    assert codes(tvl=tvl_desc(u_max=(0, float("nan")))) == both(-1)
    assert codes(model=model(2), tvl=tvl_desc(2, u_max=(1, 0.0))) == both(-1)  # every input's bound
    assert call("tvl_bwd", tvl=tvl_desc(u_max=(1, 0.0))) == 0  # (beyond U: not read)


@pytest.mark.parametrize("edit", REPEATED_INDEX, ids=str)
def test_a_model_index_listed_twice(edit):
    """The model's lists name a component once per role (tests/test_open_refusals_cpu.py): the sweep refuses with nothing asked for."""
    assert codes(model=model(**edit)) == both(-1)
    assert codes(model=model(**edit), meas=meas_desc()) == both(-1)


def test_precedence():
    assert codes(M=0, tvl=tvl_desc(U=9)) == both(-1)  # sizes before limits
    assert codes(model=model(S=17), tvl=tvl_desc(target_rows=0)) == both(-2)  # the model's limits before the descriptor
    assert codes(model=model(angle=(0, 9)), tvl=tvl_desc(U=9)) == both(-1)  # the model before the descriptor
    assert codes(tvl=tvl_desc(U=9, target_rows=0)) == both(-2)  # the descriptor's limits before its other errors
    assert codes(tvl=tvl_desc(S=17, gain=None)) == both(-2)
    assert codes(tvl=tvl_desc(ff_rows=1), meas=meas_desc(a0=0.0)) == both(-1)
    assert call("tvl_bwd", tvl=tvl_desc(gain_rows=2)) == -1  # a bad descriptor is refused even when nothing is asked for


def test_the_measurement_checks_of_the_pd_entry():
    """meas NULL and n == 0: the true state.  Else every check of mcp_rollout_pd_meas, behind the descriptor's."""
    refused = [meas_desc(n=-1), meas_desc(n=3), meas_desc(meas=None), meas_desc(a0=0.0), meas_desc(pos=(0, 4)), meas_desc(vel=(0, -1)),
               meas_desc(pos=(0, 1))]  # (the last: component 1 listed as a position and as a velocity)
    for ms in refused:
        assert codes(meas=ms) == both(-1)
    assert codes(model=model(2), tvl=tvl_desc(2), meas=meas_desc(n=2, pos=(1, 0))) == both(-1)  # a repeated position
    assert codes(model=model(Ts=0.0), meas=meas_desc()) == both(-1)
    assert call("tvl_bwd", model=model(Ts=0.0), meas=meas_desc(n=0)) == 0  # (nothing is measured: Ts is not asked about)
