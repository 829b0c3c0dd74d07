"""CPU: what mcp_rollout_mlp_hist and mcp_rollout_mlp_hist_bwd refuse, with which code, on the pattern of tests/test_mlp_refusals_cpu.py: a
refused call returns before any HIP call, so the library answers without a GPU; device pointers are dummy non-NULL addresses that nothing
reads.

Every expected code is written out: 0 MCP_OK, -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  Order of the checks: NULL pointers, p_drop and M / T (-1),
the model's compiled limits (-2), the model (-1), the descriptor WITH the memory -- its compiled limits first (-2: U, S, P > MCP_MAX_PFEAT,
track->n, h > MCP_MAX_HIST, then after n_hidden (-1) the widths), then everything else (-1: h < 1 with the sizes, P != h P0 + n with the
lists) --, the track's own errors (-1), the PD term's (-1), the measurement's, then, the sweep only, "nothing asked for" (0, no launch).
hist NULL and h == 1 reach exactly the checks of mcp_rollout_mlp_res / _res_bwd.  The forward entry launches whenever it accepts, so every
forward call here is a refusal."""
import ctypes as C

import pytest

from test_mlp_refusals_cpu import mlp_desc
from test_open_refusals_cpu import PTR, M, T, abi, model

SIGS = {
    "mlp_hist": ("model", "mlp", "hist", "track", "res", "meas", "noise", "p_drop", "M", "T", "particle_pred", "x0", "states", "inputs", "mu", "var", "jac",
                 "status"),
    "mlp_hist_bwd": ("model", "mlp", "hist", "track", "res", "meas", "noise", "p_drop", "M", "T", "states", "inputs", "jac", "g_states", "g_inputs",
                     "g_params", "g_x0"),
    "mlp_res": ("model", "mlp", "track", "res", "meas", "noise", "p_drop", "M", "T", "particle_pred", "x0", "states", "inputs", "mu", "var", "jac", "status"),
    "mlp_res_bwd": ("model", "mlp", "track", "res", "meas", "noise", "p_drop", "M", "T", "states", "inputs", "jac", "g_states", "g_inputs", "g_params",
                    "g_x0"),
}
OPTIONAL = ("mu", "var", "g_inputs", "g_params", "g_x0", "hist", "track", "res", "meas")
BOTH = ("mlp_hist", "mlp_hist_bwd")


def hist(h):
    s = abi().MLPHist()
    s.h = h
    return s


def hist_desc(h, n=0, **kw):
    """mlp_desc over model(U = 1) (P0 = 5: three plain features, one angle) with P = h P0 + n."""
    return mlp_desc(**dict(dict(P=5 * h + n), **kw))


def track(n=2, rows=T, idx=(3, 0), target=PTR):
    t = abi().MLPTrack()
    t.n, t.rows, t.target = n, rows, target
    for i, v in enumerate(idx):
        t.idx[i] = v
    return t


def pd_term(**edit):
    r = abi().MLPResidual()
    r.on, r.rows, r.target, r.sqrt_kp, r.sqrt_kd = 1, T, PTR, PTR, PTR
    r.pos[0], r.vel[0] = 0, 1
    for k, v in edit.items():
        setattr(r, k, v)
    return r


def call(entry, **over):
    a = abi()
    args = dict(model=model(), mlp=mlp_desc(), noise=a.Noise(), p_drop=0.0, M=M, T=T, particle_pred=1)
    args.update(over)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL or (name == "jac" and not entry.endswith("bwd")) else PTR)
    return getattr(a.lib(), "mcp_rollout_" + entry)(*vals, None)


def codes(**over):
    return {e: call(e, **over) for e in BOTH}


def both(code):
    return {e: code for e in BOTH}


def test_exports_and_version():
    a = abi()
    lib = a.lib()
    for name in ("mcp_rollout_mlp_hist", "mcp_rollout_mlp_hist_bwd"):
        assert name in a.EXPORTED and hasattr(lib, name)
    assert lib.mcp_abi_version() == a.ABI_VERSION == 7 and a.MAX_HIST == 4


def test_the_sweep_accepts_valid_arguments_with_nothing_asked_for():
    for h in (1, 2, 3, 4):
        assert call("mlp_hist_bwd", mlp=hist_desc(h), hist=hist(h)) == 0
    assert call("mlp_hist_bwd", mlp=hist_desc(4, 2), hist=hist(4), track=track()) == 0  # P = 22
    assert call("mlp_hist_bwd", mlp=hist_desc(2), hist=hist(2), res=pd_term()) == 0
    assert call("mlp_hist_bwd", mlp=mlp_desc(lists=False, P=8), hist=hist(2)) == 0  # f = x: P0 = S
    assert call("mlp_hist_bwd", mlp=hist_desc(6, 2), hist=hist(6)) == -2  # P = 32 is within the limit, h is not
    assert call("mlp_hist_bwd", mlp=hist_desc(3), hist=hist(3), T=1, jac=None) == 0  # the policy alone has no record
    assert call("mlp_hist_bwd", mlp=hist_desc(3), hist=hist(3), T=2, jac=None) == -1


@pytest.mark.parametrize("entry", BOTH)
def test_null_pointers_and_sizes(entry):
    req = ("model", "mlp", "noise", "x0", "states", "inputs", "status") if entry == "mlp_hist" else ("model", "mlp", "states", "inputs", "jac", "g_states")
    for name in req:
        assert call(entry, **dict(dict(mlp=hist_desc(2), hist=hist(2)), **{name: None})) == -1, name
    assert call(entry, mlp=hist_desc(2), hist=hist(2), M=0) == -1
    assert call(entry, mlp=hist_desc(2), hist=hist(2), T=0) == -1
    assert call(entry, mlp=hist_desc(2), hist=hist(2), p_drop=1.0) == -1
    assert call(entry, mlp=hist_desc(2), hist=hist(2), p_drop=float("nan")) == -1


def test_the_depth_of_the_window():
    assert codes(mlp=hist_desc(1), hist=hist(0)) == both(-1)  # h < 1
    assert codes(mlp=hist_desc(1), hist=hist(-3)) == both(-1)
    assert codes(mlp=hist_desc(5), hist=hist(5)) == both(-2)  # h > MCP_MAX_HIST (P = 25 is within its limit)
    assert codes(mlp=hist_desc(4), hist=hist(5)) == both(-2)  # the limit before the width rule
    assert codes(mlp=hist_desc(7), hist=hist(4)) == both(-2)  # P = 35 > MCP_MAX_PFEAT
    assert codes(mlp=hist_desc(7), hist=hist(0)) == both(-2)  # limits first: P = 35 before h < 1
    assert codes(mlp=hist_desc(5), hist=hist(0)) == both(-1)


def test_the_width_rule():
    assert codes(mlp=hist_desc(2), hist=hist(3)) == both(-1)  # P = 10, h P0 = 15
    assert codes(mlp=hist_desc(3), hist=hist(2)) == both(-1)
    assert codes(mlp=hist_desc(2)) == both(-1)  # hist NULL: h = 1, P must be P0
    assert codes(mlp=hist_desc(2), hist=hist(1)) == both(-1)
    assert codes(mlp=hist_desc(2, 2), hist=hist(2)) == both(-1)  # two more columns and no track
    assert codes(mlp=hist_desc(2), hist=hist(2), track=track()) == both(-1)  # a track and no columns for it
    assert codes(mlp=hist_desc(2, 2), hist=hist(2), track=track(n=0)) == both(-1)
    assert codes(mlp=mlp_desc(lists=False, P=12), hist=hist(2)) == both(-1)  # f = x: h S = 8


def test_precedence():
    assert codes(M=0, mlp=hist_desc(5), hist=hist(5)) == both(-1)  # sizes before limits
    assert codes(model=model(S=17), mlp=hist_desc(2), hist=hist(0)) == both(-2)  # the model's limits before the descriptor
    assert codes(model=model(angle=(0, 9)), mlp=hist_desc(5), hist=hist(5)) == both(-1)  # the model before the descriptor
    assert codes(mlp=hist_desc(5, n_hidden=3), hist=hist(5)) == both(-2)  # h's limit with the first limits, ahead of n_hidden
    assert codes(mlp=hist_desc(2, hidden=(65,)), hist=hist(0)) == both(-2)  # the widths' limit before h < 1
    assert codes(mlp=hist_desc(2, n_hidden=3), hist=hist(0)) == both(-1)
    assert codes(mlp=hist_desc(2, 2), hist=hist(2), track=track(rows=T - 1)) == both(-1)  # the track's own errors behind the descriptor's
    assert codes(mlp=hist_desc(2, 2), hist=hist(2), track=track(idx=(3, 3))) == both(-1)
    assert codes(mlp=hist_desc(2), hist=hist(2), res=pd_term(rows=T - 1)) == both(-1)  # then the PD term's
    assert codes(mlp=hist_desc(2), hist=hist(2), res=pd_term(sqrt_kp=None)) == both(-1)
    assert codes(mlp=hist_desc(3), hist=hist(2), res=pd_term(rows=T - 1)) == both(-1)
    assert call("mlp_hist_bwd", mlp=hist_desc(2), hist=hist(3)) == -1  # a bad depth is refused even when nothing is asked for


@pytest.mark.parametrize("h", [None, 1])
def test_no_memory_reaches_the_residual_entries_checks(h):
    """hist NULL and h == 1: every code of mcp_rollout_mlp_res / _res_bwd on the same arguments."""
    hs = {} if h is None else dict(hist=hist(h))
    refused = [(dict(M=0), -1), (dict(T=0), -1), (dict(p_drop=1.0), -1), (dict(model=model(S=17)), -2), (dict(mlp=mlp_desc(P=33)), -2),
               (dict(mlp=mlp_desc(P=4)), -1), (dict(mlp=mlp_desc(hidden=(65,))), -2), (dict(mlp=mlp_desc(n_hidden=0)), -1),
               (dict(mlp=mlp_desc(P=7), track=track(rows=T - 1)), -1), (dict(mlp=mlp_desc(P=7), track=track(idx=(0, 4))), -1),
               (dict(track=track(n=17)), -2), (dict(track=track()), -1), (dict(res=pd_term(rows=T - 1)), -1), (dict(res=pd_term(target=None)), -1),
               (dict(mlp=mlp_desc(u_max=(0, 0.0))), -1)]
    for kw, code in refused:
        old = {e: call(o, **kw) for e, o in zip(BOTH, ("mlp_res", "mlp_res_bwd"))}
        assert old == both(code) and codes(**kw, **hs) == old, kw
    # (an accepted forward call would launch: of valid arguments the sweeps alone are asked, with nothing asked for)
    for kw in (dict(), dict(mlp=mlp_desc(P=7), track=track()), dict(res=pd_term())):
        assert call("mlp_res_bwd", **kw) == 0 and call("mlp_hist_bwd", **kw, **hs) == 0, kw


def test_memory_with_a_measurement_model_is_refused():
    """The history forms are built on the true state only: hist with h > 1 and an active measurement model is MCP_ERR_ARG, behind every other
    check of the descriptor; h == 1 with one reaches the residual entry (the sweep, nothing asked for: accepted)."""
    from test_mlp_meas_refusals_cpu import meas_desc as meas

    assert codes(mlp=hist_desc(2), hist=hist(2), meas=meas()) == both(-1)
    assert codes(mlp=hist_desc(5), hist=hist(5), meas=meas()) == both(-2)  # the limits first
    assert call("mlp_hist_bwd", hist=hist(1), meas=meas()) == 0

