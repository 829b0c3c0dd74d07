"""CPU: target-trajectory features of the tanh-MLP policy.  The exports and the layout of mcp_mlp_track against the ctypes mirror; what
mcp_rollout_mlp_track / mcp_rollout_mlp_track_bwd refuse, with which code (a refused call returns before any HIP call, so the library
answers without a GPU; device pointers are dummy non-NULL addresses that nothing reads, as in tests/test_mlp_refusals_cpu.py);
Policy.MLP_policy(target_traj=...) against the law written out in tests/mlp_track_models.py; and the conditions that keep
tests/test_gpu_mlp_track.py from passing vacuously, on the cases of its table.

Every expected code is written out: 0 MCP_OK, -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  Order of the checks: NULL pointers, M / T and p_drop (-1), the
model's compiled limits (-2), the model (-1), the descriptor's limits -- track->n > MCP_MAX_STATE and P > MCP_MAX_PFEAT among them -- (-2),
the descriptor's other errors, then the track's (-1), the measurement model (-1), then, the sweep only, "nothing asked for" (0, no launch)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import mlp_drop_models as mdm
from mlp_models import SHAPES
from mlp_track_models import CASES, DEFECTS, case_id, case_inputs, case_truth, network, target_for, track_law, truth_of
from test_mlp_drop_cpu import meas_desc
from test_mlp_refusals_cpu import call as old_call
from test_mlp_refusals_cpu import mlp_desc
from test_open_refusals_cpu import PTR, M, T, abi, model

DT = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = {
    "mlp_track": ("model", "mlp", "track", "meas", "noise", "p_drop", "M", "T", "particle_pred", "x0", "states", "inputs", "mu", "var", "jac", "status"),
    "mlp_track_bwd": ("model", "mlp", "track", "meas", "noise", "p_drop", "M", "T", "states", "inputs", "jac", "g_states", "g_inputs", "g_params",
                      "g_x0"),
}
REQUIRED = {"mlp_track": ("model", "mlp", "noise", "x0", "states", "inputs", "status"), "mlp_track_bwd": ("model", "mlp", "states", "inputs", "jac", "g_states")}
OPTIONAL = ("mu", "var", "g_inputs", "g_params", "g_x0")
BOTH = ("mlp_track", "mlp_track_bwd")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def track_desc(idx=(3, 0), rows=T, **edit):
    """A valid track over model(): errors on components 3 and 0 (not ascending), as many rows as the launch reads."""
    t = abi().MLPTrack()
    t.n, t.rows, t.target = len(idx), rows, PTR
    for i, v in enumerate(idx):
        t.idx[i] = v
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(t, k)[v[0]] = v[1]
        else:
            setattr(t, k, v)
    return t


def tracked(n=2, **kw):
    """mlp_desc whose P counts ``n`` error features behind the lists' (or the state's) own."""
    base = mlp_desc(**{k: v for k, v in kw.items() if k in ("U", "hidden", "lists")}).P
    return mlp_desc(**dict(dict(P=base + n), **kw))


def call(entry, **over):
    a = abi()
    args = dict(model=model(), mlp=tracked(), track=track_desc(), meas=None, noise=a.Noise(), p_drop=0.0, M=M, T=T, particle_pred=1)
    args.update(over)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL or (name == "jac" and entry == "mlp_track") else PTR)
    return getattr(a.lib(), "mcp_rollout_" + entry)(*vals, None)


def codes(**over):
    return {e: call(e, **over) for e in BOTH}


def both(code):
    return {e: code for e in BOTH}


def test_exports_and_version():
    from test_abi_cpu import declared_symbols

    a = abi()
    assert "mcp_rollout_mlp_track" in a.EXPORTED and "mcp_rollout_mlp_track_bwd" in a.EXPORTED
    lib = a.lib()
    assert hasattr(lib, "mcp_rollout_mlp_track") and hasattr(lib, "mcp_rollout_mlp_track_bwd")
    assert lib.mcp_abi_version() == a.ABI_VERSION == 7  # the additions are additive
    assert set(declared_symbols()) == set(a.EXPORTED)  # the header and the binding stay the same set


def test_struct_layout_against_the_header(tmp_path):
    a = abi()
    names = [n for n, _ in a.MLPTrack._fields_]
    assert names == ["n", "idx", "rows", "target"]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(void){printf("%zu", sizeof(mcp_mlp_track));'
                   + "".join('printf(" %%zu", offsetof(mcp_mlp_track, %s));' % n for n in names)
                   + 'printf(" %zu %d %d %d", sizeof(mcp_mlp_policy), MCP_MAX_STATE, MCP_MAX_PFEAT, MCP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(a.MLPTrack)
    assert out[1:1 + len(names)] == [getattr(a.MLPTrack, n).offset for n in names]
    assert out[-4:] == [C.sizeof(a.MLPPolicy), a.MAX_STATE, a.MAX_PFEAT, a.ABI_VERSION] == [C.sizeof(a.MLPPolicy), 16, 32, 7]  # mcp_mlp_policy did not move


def test_the_sweep_accepts_valid_arguments_with_nothing_asked_for():
    assert call("mlp_track_bwd") == 0
    assert call("mlp_track_bwd", noise=None) == 0  # without dropout the sweep needs no noise
    assert call("mlp_track_bwd", p_drop=0.25) == 0
    assert call("mlp_track_bwd", p_drop=0.25, noise=None) == -1
    assert call("mlp_track_bwd", track=None, mlp=mlp_desc()) == 0  # no track: the dropout entry's arguments
    assert call("mlp_track_bwd", track=track_desc(idx=()), mlp=mlp_desc()) == 0  # n == 0: the same
    assert call("mlp_track_bwd", track=track_desc(idx=(), target=None, rows=0), mlp=mlp_desc()) == 0  # (nothing of an empty track is read)
    assert call("mlp_track_bwd", mlp=tracked(lists=False)) == 0  # f = [x, errors]: P = S + n
    assert call("mlp_track_bwd", track=track_desc(idx=(3, 2, 1, 0)), mlp=tracked(4, hidden=(64, 64))) == 0
    assert call("mlp_track_bwd", track=track_desc(rows=T + 2)) == 0
    assert call("mlp_track_bwd", meas=meas_desc()) == 0
    assert call("mlp_track_bwd", T=1, jac=None, track=track_desc(rows=1)) == 0
    assert call("mlp_track_bwd", T=2, jac=None) == -1


@pytest.mark.parametrize("entry", BOTH)
def test_null_pointers_sizes_and_the_probability(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
    assert call(entry, M=0) == -1 and call(entry, T=0) == -1
    for p in (-0.1, 1.0, float("nan")):
        assert call(entry, p_drop=p) == -1, p
    assert call(entry, mlp=tracked(W=(0, None))) == -1


def test_the_limits():
    assert codes(track=track_desc(n=17)) == both(-2)  # track->n > MCP_MAX_STATE
    assert codes(track=track_desc(n=17), mlp=tracked(17)) == both(-2)
    assert codes(mlp=tracked(28)) == both(-2)  # P = 33 > MCP_MAX_PFEAT
    assert codes(mlp=tracked(hidden=(65,))) == both(-2)
    assert codes(model=model(S=17)) == both(-2)


def test_the_track_errors():
    assert codes(track=track_desc(n=-1)) == both(-1)
    assert codes(track=track_desc(n=-1), mlp=mlp_desc()) == both(-1)
    assert codes(track=track_desc(idx=(3, 4))) == both(-1)  # out of range
    assert codes(track=track_desc(idx=(-1, 0))) == both(-1)
    assert codes(track=track_desc(idx=(3, 3))) == both(-1)  # repeated
    assert codes(track=track_desc(rows=T - 1)) == both(-1)  # rows < T
    assert codes(track=track_desc(target=None)) == both(-1)  # n > 0 without a target
    assert codes(mlp=mlp_desc()) == both(-1)  # P does not count the error features
    assert codes(mlp=tracked(3)) == both(-1)  # P counts one too many
    assert codes(track=None) == both(-1)  # P counts error features there are none of
    assert codes(track=track_desc(idx=())) == both(-1)
    assert codes(mlp=tracked(lists=False, P=5)) == both(-1)  # without lists P is S + n


def test_the_old_entries_still_refuse_a_width_that_counts_error_features():
    for e in ("mlp", "mlp_bwd"):
        assert old_call(e, mlp=tracked()) == -1
        assert old_call(e, mlp=tracked(lists=False)) == -1
    from test_mlp_drop_cpu import call as drop_call

    for e in ("mlp_drop", "mlp_drop_bwd"):
        assert drop_call(e, mlp=tracked()) == -1


def test_precedence():
    assert codes(M=0, model=model(S=17)) == both(-1)  # sizes before limits
    assert codes(p_drop=1.0, track=track_desc(n=17)) == both(-1)
    assert codes(model=model(angle=(0, 9)), track=track_desc(n=17)) == both(-1)  # the model before the descriptor and the track's limit
    assert codes(model=model(angle=(0, 9)), mlp=tracked(U=9)) == both(-1)
    assert codes(mlp=tracked(U=9, angle=(0, 4))) == both(-2)  # the descriptor's limits before its other errors
    assert codes(track=track_desc(n=17, rows=0)) == both(-2)  # the track's limit before the track's errors
    assert codes(track=track_desc(n=17), mlp=tracked(angle=(0, 4))) == both(-2)  # ... and before the descriptor's errors
    assert codes(mlp=tracked(28), track=track_desc(idx=(3, 3))) == both(-2)
    assert codes(mlp=tracked(hidden=(65,)), track=track_desc(rows=0)) == both(-2)  # the descriptor before the track
    assert codes(track=track_desc(idx=(3, 3)), meas=meas_desc(a0=0.0)) == both(-1)  # the track before the measurement: both -1 ...
    assert codes(track=track_desc(n=17), meas=meas_desc(a0=0.0)) == both(-2)  # ... so with the track's limit code
    assert codes(meas=meas_desc(a0=0.0)) == both(-1)
    assert codes(model=model(gp_N=4097, gp_Npad=4112)) == {"mlp_track": -2, "mlp_track_bwd": 0}  # the sweep never reads a GP descriptor
    assert call("mlp_track_bwd", track=track_desc(idx=(3, 3))) == -1  # a bad track is refused even when nothing is asked for


# ---- the class ------------------------------------------------------------------------------------------------------------------------------
def _policy(c, hidden, params, target, idx=None, lists=True, **kw):
    from mc_pilco_amd.policy_learning import Policy

    return Policy.MLP_policy(state_dim=c["S"], input_dim=c["U"], hidden_sizes=list(hidden), angle_indices=c["angle"] if lists else None,
                             non_angle_indices=c["not_angle"] if lists else None, u_max=1.3, weight_init=params, dtype=DT, device=torch.device("cpu"),
                             target_traj=target, error_indices=idx, **kw)


@pytest.mark.parametrize("hidden,idx,lists", [((5,), None, True), ((7, 3), [3, 0], True), ((5,), None, False), ((7, 3), [2], False)])
def test_forward_matches_the_written_out_law(hidden, idx, lists):
    c = SHAPES["arm2"]
    angle, non_angle = (c["angle"], c["not_angle"]) if lists else ([], [])
    n = c["S"] if idx is None else len(idx)
    x = torch.randn(9, c["S"], dtype=DT, generator=torch.Generator().manual_seed(4))
    target = target_for(c, 6, x)
    params = network(c, hidden, angle, non_angle, n, 11)
    pol = _policy(c, hidden, params, target, idx, lists)
    P = (len(non_angle) + 2 * len(angle) if lists else c["S"]) + n
    assert pol.feature_dim == P and pol.error_indices == (list(range(c["S"])) if idx is None else idx)
    assert [tuple(q.shape) for q in pol.mlp_parameters()][:2] == [(hidden[0], P), (hidden[0],)]
    for t in (0, 3, 7):
        ref = track_law(x, t, params, angle, non_angle, 1.3, True, target, pol.error_indices)
        assert float((pol(x, t=t).detach() - ref).abs().max()) < 1e-15
        assert tuple(pol.features(x, t).shape) == (9, P)
        if not lists and idx is None:  # the reference's map (policy_learning/Policy.py:389-403): cat(x, x*_t - x)
            assert torch.equal(pol.features(x, t), torch.cat([x, target[t].reshape(1, -1) - x], dim=1))
    assert float((pol(x, t=0) - pol(x, t=3)).detach().abs().max()) > 1e-3  # (the row is read)
    for f in (lambda: pol(x), lambda: pol.features(x), lambda: pol(x, t=None)):
        with pytest.raises(ValueError):
            f()
    u = pol.forward_np(x[0].numpy(), 3)  # the real system's call (get_data_from_system passes t)
    assert float(abs(u - track_law(x[:1], 3, params, angle, non_angle, 1.3, True, target, pol.error_indices).numpy()).max()) < 1e-15
    pol.reinit()
    assert tuple(pol.W0.shape) == (hidden[0], P) and float(pol.W0[:, -n:].abs().min()) > 0


def test_fusable():
    from mc_pilco_amd import hipabi

    c = SHAPES["arm2"]
    model_like = type("M", (), dict(S=c["S"], U=c["U"]))()
    x = torch.zeros(1, c["S"], dtype=DT)
    mk = lambda target, idx=None, hidden=(5,), **kw: _policy(c, hidden, network(c, hidden, c["angle"], c["not_angle"], c["S"] if idx is None else len(idx), 1),
                                                              target, idx, **kw)
    target = target_for(c, 6, x)  # 8 rows
    # (fusable() asks for GPU parameters first; _fus answers that for it, so the track's conditions are looked at on their own here)
    assert _fus(mk(target), model_like, 8) is True and _fus(mk(target), model_like, 1) is True
    assert _fus(mk(target), model_like, 9) is False  # rows < T
    assert _fus(mk(target, [3, 3]), model_like, 4) is False  # a repeated index
    assert _fus(mk(target, [3, 4]), model_like, 4) is False  # out of range
    assert _fus(mk(target.to(torch.float32)), model_like, 4) is False  # a float32 target
    assert _fus(mk(target[:, :3]), model_like, 4) is False  # not [rows, S]
    assert _fus(mk(target, [3, 0]), model_like, 4) is True
    wide = SHAPES["limits"]  # S = 16: its own lists (P = 24) plus nine errors: feature_dim = 33
    lim = type("M", (), dict(S=16, U=8))()
    tw = target_for(wide, 6, torch.zeros(1, 16, dtype=DT))
    mkw = lambda n: _policy(wide, (5,), network(wide, (5,), wide["angle"], wide["not_angle"], n, 1), tw, list(range(n)))
    assert mkw(9).feature_dim == 33 > hipabi.MAX_PFEAT and _fus(mkw(9), lim, 4) is False
    assert mkw(8).feature_dim == 32 and _fus(mkw(8), lim, 4) is True


class _GpuView:
    """Stands for a parameter on a GPU: fusable() reads its dtype and ``is_cuda`` alone."""

    def __init__(self, q):
        self.dtype, self.is_cuda = q.dtype, True


def _fus(pol, model_like, T):
    """MLP_policy.fusable on ``pol``'s settings with its parameters taken for GPU tensors: what the answer turns on without a GPU."""
    view = type("V", (), {})()
    view.__dict__.update({k: v for k, v in pol.__dict__.items() if not k.startswith("_") or k == "_lists"})
    view.mlp_parameters = lambda: [_GpuView(q) for q in pol.mlp_parameters()]
    view._u_max_values = pol._u_max_values
    return type(pol).fusable(view, model_like, T)


def test_without_a_target_the_object_is_the_one_it_was():
    """Same parameter shapes, the same forward bits on a seeded input (the expression of the class before the keywords, written out), t or not."""
    from mc_pilco_amd.policy_learning import Policy

    c = SHAPES["arm2"]
    for hidden, lists in (((5,), True), ((7, 3), False)):
        angle, non_angle = (c["angle"], c["not_angle"]) if lists else ([], [])
        params = network(c, hidden, angle, non_angle, 0, 11)
        pol = Policy.MLP_policy(state_dim=c["S"], input_dim=c["U"], hidden_sizes=list(hidden), angle_indices=angle or None, non_angle_indices=non_angle or None,
                                u_max=1.3, weight_init=params, dtype=DT, device=torch.device("cpu"))
        assert pol.target_traj is None and pol.error_indices == [] and pol.feature_dim == (6 if lists else 4)
        assert [tuple(q.shape) for q in pol.mlp_parameters()] == [tuple(q.shape) for q in params]
        x = torch.randn(9, c["S"], dtype=DT, generator=torch.Generator().manual_seed(4))
        h = torch.cat([x[:, non_angle], torch.sin(x[:, angle]), torch.cos(x[:, angle])], dim=1) if lists else x
        assert torch.equal(pol.features(x), h) and torch.equal(pol.features(x, 3), h)
        for l in range(len(hidden)):
            h = torch.tanh(h @ params[2 * l].t() + params[2 * l + 1])
        ref = pol.f_squash(h @ params[-2].t() + params[-1])
        assert torch.equal(pol(x).detach(), ref) and torch.equal(pol(x, t=5).detach(), ref)
    with pytest.raises(ValueError):
        Policy.MLP_policy(state_dim=4, input_dim=2, hidden_sizes=[5], error_indices=[0], device=torch.device("cpu"))


# ---- the truth's conditioning ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_truth_is_conditioned(case):
    """On every case: the variances stay positive, everything is finite, every tensor has a gradient to compare, and the gradient with
    respect to the error columns of W0 is at least 1e-3 of the largest gradient entry -- the errors reach the loss."""
    mode, shape, deg, N, Tc, Mc, hidden, opt = case
    c, m, ins, (st, inp, ym, grads, gx0, vmin) = case_truth(case)
    if Tc > 1:
        assert vmin > 0.0
    n = len(ins["idx"])
    assert tuple(ins["target"].shape) == (Tc + opt.get("rows_extra", 0), c["S"]) and tuple(grads[0].shape)[1] == tuple(ins["params"][0].shape)[1]
    assert bool(torch.isfinite(st).all()) and bool(torch.isfinite(inp).all()) and all(bool(torch.isfinite(g).all()) for g in grads + [gx0])
    assert all(float(g.abs().max()) > 0 for g in grads) and float(gx0.abs().max()) > 0
    big = max(float(g.abs().max()) for g in grads)
    ecol = float(grads[0][:, -n:].abs().max())
    print("%s: min var %.3e, |g W0 error columns| %.3e of %.3e" % (case_id(case), vmin, ecol, big))
    assert ecol >= 1e-3 * big
    assert (ym is None) == ("meas" not in opt)
    if ins["masks"] is not None:
        assert mdm.masks_mixed(ins["masks"], hidden)


def test_the_table_covers_what_it_names():
    opts = [c[7] for c in CASES]
    assert {c[4] for c in CASES} == {1, 2, 3, 12} and {1, 5, 17, 1041} <= {c[5] for c in CASES}
    assert sum(c[5] == 1041 for c in CASES) == 1
    assert {"arm2", "arm2_delta", "ur5", "limits"} == {c[1] for c in CASES} and {"mean", "sampled"} == {c[0] for c in CASES}
    assert {len(c[6]) for c in CASES} == {1, 2} and ("ur5", (64, 64)) in {(c[1], c[6]) for c in CASES} and ("limits", (64, 64)) in {(c[1], c[6]) for c in CASES}
    for case in CASES:
        if case[1] == "limits":  # its own lists plus eight errors: P = 32 exactly
            ins = case_inputs(case)[2]
            assert tuple(ins["params"][0].shape) == (64, 32) and len(ins["idx"]) == 8 and ins["angle"] and ins["non_angle"]
    assert any(o.get("features") == "state" for o in opts)
    assert any("idx" in o and list(o["idx"]) != sorted(o["idx"]) for o in opts)  # a proper subset, not ascending
    assert any(o.get("rows_extra") == 2 for o in opts) and any("rows_extra" not in o for o in opts)
    for key in ("squash", "no_g_inputs"):
        assert sum(key in o for o in opts) == 1
    assert [o["only_grad"] for o in opts if "only_grad" in o] == [0]  # W0
    assert sum("meas" in o and "p" not in o for o in opts) == 1 and sum("p" in o and "meas" not in o for o in opts) == 1
    assert sum("meas" in o and "p" in o for o in opts) == 1 and {o["p"] for o in opts if "p" in o} == {0.25}


@pytest.mark.parametrize("case", [c for c in CASES if c[4] == 12], ids=case_id)
def test_near_misses_are_far_from_the_truth(case):
    """A rollout that reads the target a row early or late, flips the error's sign, reads row 0 throughout or (measured) takes the error on the
    true state differs from the truth in the states by at least 1e-6 -- 1000 times the GPU test's state bound -- and leaves row 0 equal."""
    c, m, ins, truth = case_truth(case)
    for defect in DEFECTS:
        if defect == "true_state" and ins["ms"] is None:
            continue
        st = truth_of(m, ins, defect=defect)[0]
        d = float((st - truth[0]).abs().max())
        print("%s, %s: |states - truth| %.3e" % (case_id(case), defect, d))
        assert d >= 1e-6 and torch.equal(st[0], truth[0][0])
