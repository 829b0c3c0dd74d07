"""CPU: the residual policy, PD law plus tanh-MLP correction under one squashing.  The exports and the layout of mcp_mlp_pd against the
ctypes mirror; what mcp_rollout_mlp_res / mcp_rollout_mlp_res_bwd refuse, with which code (a refused call returns before any HIP call, so
the library answers without a GPU; device pointers are dummy non-NULL addresses that nothing reads, as in tests/test_mlp_refusals_cpu.py);
Policy.Residual_MLP_policy against the law written out in tests/mlp_res_models.py; and the conditions that keep tests/test_gpu_mlp_res.py
from passing vacuously, on the cases of its table.

Every expected code is written out: 0 MCP_OK, -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  Order of the checks: those of mcp_rollout_mlp_track up to
and including the track's (tests/test_mlp_track_cpu.py), then the residual's (-1), the measurement model (-1), then, the sweep only,
"nothing asked for" (0, no launch)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import mlp_drop_models as mdm
from mlp_models import SHAPES
from mlp_res_models import CASES, DEFECTS, case_id, case_inputs, case_truth, default_lists, gains_for, pd_target_for, res_law, truth_of
from mlp_track_models import network, target_for
from test_mlp_drop_cpu import meas_desc
from test_mlp_refusals_cpu import mlp_desc
from test_mlp_track_cpu import _GpuView, track_desc, tracked
from test_open_refusals_cpu import PTR, M, T, abi, model

DT = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = {
    "mlp_res": ("model", "mlp", "track", "res", "meas", "noise", "p_drop", "M", "T", "particle_pred", "x0", "states", "inputs", "mu", "var", "jac",
                "status"),
    "mlp_res_bwd": ("model", "mlp", "track", "res", "meas", "noise", "p_drop", "M", "T", "states", "inputs", "jac", "g_states", "g_inputs", "g_params",
                    "g_x0"),
}
REQUIRED = {"mlp_res": ("model", "mlp", "noise", "x0", "states", "inputs", "status"), "mlp_res_bwd": ("model", "mlp", "states", "inputs", "jac", "g_states")}
OPTIONAL = ("mu", "var", "g_inputs", "g_params", "g_x0")
BOTH = ("mlp_res", "mlp_res_bwd")
U2 = dict(U=2)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def res_desc(pos=(1, 0), vel=(3, 2), rows=T, **edit):
    """A valid PD term over model(U=2): positions 1, 0 and velocities 3, 2 (not ascending), as many rows as the launch reads."""
    r = abi().MLPResidual()
    r.on, r.rows, r.target, r.sqrt_kp, r.sqrt_kd = 1, rows, PTR, PTR, PTR
    for k, v in enumerate(pos):
        r.pos[k] = v
    for k, v in enumerate(vel):
        r.vel[k] = v
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(r, k)[v[0]] = v[1]
        else:
            setattr(r, k, v)
    return r


def call(entry, **over):
    a = abi()
    args = dict(model=model(**U2), mlp=tracked(**U2), track=track_desc(), res=res_desc(), meas=None, noise=a.Noise(), p_drop=0.0, M=M, T=T, particle_pred=1)
    args.update(over)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL or (name == "jac" and entry == "mlp_res") else PTR)
    return getattr(a.lib(), "mcp_rollout_" + entry)(*vals, None)


def codes(**over):
    return {e: call(e, **over) for e in BOTH}


def both(code):
    return {e: code for e in BOTH}


def test_exports_and_version():
    from test_abi_cpu import declared_symbols

    a = abi()
    assert "mcp_rollout_mlp_res" in a.EXPORTED and "mcp_rollout_mlp_res_bwd" in a.EXPORTED
    lib = a.lib()
    assert hasattr(lib, "mcp_rollout_mlp_res") and hasattr(lib, "mcp_rollout_mlp_res_bwd")
    assert lib.mcp_abi_version() == a.ABI_VERSION == 7  # the additions are additive
    assert set(declared_symbols()) == set(a.EXPORTED)  # the header and the binding stay the same set


def test_struct_layout_against_the_header(tmp_path):
    a = abi()
    names = [n for n, _ in a.MLPResidual._fields_]
    assert names == ["on", "pos", "vel", "sqrt_kp", "sqrt_kd", "target", "rows"]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(void){printf("%zu", sizeof(mcp_mlp_pd));'
                   + "".join('printf(" %%zu", offsetof(mcp_mlp_pd, %s));' % n for n in names)
                   + 'printf(" %zu %zu %d %d", sizeof(mcp_mlp_policy), sizeof(mcp_mlp_track), MCP_MAX_INPUT, MCP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(a.MLPResidual)
    assert out[1:1 + len(names)] == [getattr(a.MLPResidual, n).offset for n in names]
    assert out[-4:] == [C.sizeof(a.MLPPolicy), C.sizeof(a.MLPTrack), a.MAX_INPUT, a.ABI_VERSION]  # the older descriptors did not move
    assert out[-2:] == [8, 7]


def test_the_sweep_accepts_valid_arguments_with_nothing_asked_for():
    assert call("mlp_res_bwd") == 0
    assert call("mlp_res_bwd", noise=None) == 0  # without dropout the sweep needs no noise
    assert call("mlp_res_bwd", p_drop=0.25) == 0
    assert call("mlp_res_bwd", p_drop=0.25, noise=None) == -1
    assert call("mlp_res_bwd", res=None) == 0 and call("mlp_res_bwd", res=res_desc(on=0)) == 0  # no term: the track entry's arguments
    assert call("mlp_res_bwd", res=res_desc(on=0, target=None, sqrt_kp=None, sqrt_kd=None, rows=0, pos=(0, 99))) == 0  # (nothing of it is read)
    assert call("mlp_res_bwd", track=None, mlp=mlp_desc(**U2)) == 0  # the term without a track ...
    assert call("mlp_res_bwd", track=track_desc(idx=()), mlp=mlp_desc(**U2)) == 0  # ... and with an empty one
    assert call("mlp_res_bwd", res=res_desc(pos=(0, 1), vel=(0, 1))) == 0  # a component may serve as a position and as a velocity
    assert call("mlp_res_bwd", res=res_desc(rows=T + 2)) == 0
    assert call("mlp_res_bwd", meas=meas_desc()) == 0
    assert call("mlp_res_bwd", T=1, jac=None, track=track_desc(rows=1), res=res_desc(rows=1)) == 0
    assert call("mlp_res_bwd", T=2, jac=None) == -1
    assert call("mlp_res_bwd", model=model(), mlp=tracked(), res=res_desc(pos=(1, 99), vel=(3, 99))) == 0  # U = 1: only entry 0 is read


@pytest.mark.parametrize("entry", BOTH)
def test_null_pointers_sizes_and_the_probability(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
    assert call(entry, M=0) == -1 and call(entry, T=0) == -1
    for p in (-0.1, 1.0, float("nan")):
        assert call(entry, p_drop=p) == -1, p
    assert call(entry, mlp=tracked(W=(0, None), **U2)) == -1


def test_the_residual_errors():
    assert codes(res=res_desc(pos=(1, 4))) == both(-1)  # out of range
    assert codes(res=res_desc(pos=(-1, 0))) == both(-1)
    assert codes(res=res_desc(vel=(3, 4))) == both(-1)
    assert codes(res=res_desc(vel=(-1, 2))) == both(-1)
    assert codes(res=res_desc(pos=(1, 1))) == both(-1)  # repeated within pos
    assert codes(res=res_desc(vel=(2, 2))) == both(-1)  # repeated within vel
    for name in ("sqrt_kp", "sqrt_kd", "target"):
        assert codes(res=res_desc(**{name: None})) == both(-1), name
    assert codes(res=res_desc(rows=T - 1)) == both(-1)  # rows < T
    assert codes(res=res_desc(rows=T - 1), track=track_desc(rows=T + 2)) == both(-1)  # its own rows, not the track's
    assert call("mlp_res_bwd", res=res_desc(on=2, pos=(1, 1))) == -1 and call("mlp_res_bwd", res=res_desc(on=2)) == 0  # any non-zero `on` is the term


def test_the_track_entries_checks_come_first():
    assert codes(track=track_desc(n=17)) == both(-2)
    assert codes(mlp=tracked(28, **U2)) == both(-2)  # P = 33 > MCP_MAX_PFEAT
    assert codes(model=model(S=17, **U2)) == both(-2)
    assert codes(model=model(U=9), mlp=tracked(U=9)) == both(-2)  # more than MCP_MAX_INPUT inputs: a limit of the model
    assert codes(track=track_desc(idx=(3, 3))) == both(-1)
    assert codes(mlp=mlp_desc(**U2)) == both(-1)  # P does not count the error features


def test_precedence():
    assert codes(M=0, res=res_desc(pos=(1, 1))) == both(-1)
    assert codes(track=track_desc(n=17), res=res_desc(pos=(1, 1))) == both(-2)  # the track's limit before the residual's errors
    assert codes(mlp=tracked(hidden=(65,), **U2), res=res_desc(rows=0)) == both(-2)  # the descriptor's limits too
    assert codes(model=model(S=17, **U2), res=res_desc(target=None)) == both(-2)
    assert codes(track=track_desc(idx=(3, 3)), res=res_desc(pos=(1, 1))) == both(-1)  # both -1 ...
    assert codes(res=res_desc(pos=(1, 1)), meas=meas_desc(a0=0.0)) == both(-1)  # the residual before the measurement: both -1
    assert codes(meas=meas_desc(a0=0.0)) == both(-1)
    assert codes(res=None, meas=meas_desc(a0=0.0)) == both(-1)
    assert call("mlp_res_bwd", res=res_desc(pos=(1, 1))) == -1  # a bad term is refused even when nothing is asked for
    assert codes(model=model(gp_N=4097, gp_Npad=4112, **U2)) == {"mlp_res": -2, "mlp_res_bwd": 0}  # the sweep never reads a GP descriptor


# ---- the class ------------------------------------------------------------------------------------------------------------------------------
def _policy(c, hidden, params, kp, kd, target, idx=None, lists=True, **kw):
    from mc_pilco_amd.policy_learning import Policy

    return Policy.Residual_MLP_policy(state_dim=c["S"], input_dim=c["U"], hidden_sizes=list(hidden), angle_indices=c["angle"] if lists else None,
                                      non_angle_indices=c["not_angle"] if lists else None, u_max=1.3, weight_init=params, dtype=DT,
                                      device=torch.device("cpu"), target_traj=target, error_indices=idx, sqrt_Kp_gains=kp, sqrt_Kd_gains=kd, **kw)


@pytest.mark.parametrize("hidden,idx,lists,scalar,other,explicit", [((5,), None, True, False, False, False), ((7, 3), [3, 0], True, True, True, True),
                                                                     ((5,), [], False, False, True, False), ((7, 3), [2], False, False, False, True)])
def test_forward_matches_the_written_out_law(hidden, idx, lists, scalar, other, explicit):
    c = SHAPES["arm2"]
    angle, non_angle = (c["angle"], c["not_angle"]) if lists else ([], [])
    n = c["S"] if idx is None else len(idx)
    x = torch.randn(9, c["S"], dtype=DT, generator=torch.Generator().manual_seed(4))
    target = target_for(c, 6, x)
    pd_target = pd_target_for(c, 6, x) if other else target
    params = network(c, hidden, angle, non_angle, n, 11)
    kp, kd = gains_for(c["U"], 11, scalar)
    pos, vel = ([1, 0], [3, 2]) if explicit else default_lists(c)
    kw = dict(pd_pos_indices=pos, pd_vel_indices=vel) if explicit else {}
    pol = _policy(c, hidden, params, kp, kd, target, idx, lists, pd_target_traj=pd_target if other else None, **kw)
    assert pol.pd_pos_indices == pos and pol.pd_vel_indices == vel and pol.error_indices == (list(range(c["S"])) if idx is None else idx)
    assert (pol.pd_target_traj is pol.target_traj) is (not other)
    assert tuple(pol.sqrt_Kp_gains.shape) == tuple(kp.shape) and not pol.sqrt_Kp_gains.requires_grad and not pol.sqrt_Kd_gains.requires_grad
    assert [tuple(q.shape) for q in pol.mlp_parameters()] == [tuple(q.shape) for q in params]  # the network's tensors alone
    wide = lambda g: g.expand(c["U"]) if g.numel() == 1 else g
    for t in (0, 3, 7):
        ref = res_law(x, t, params, wide(kp), wide(kd), angle, non_angle, 1.3, True, target, pol.error_indices, pd_target, pos, vel)
        assert float((pol(x, t=t).detach() - ref).abs().max()) < 1e-15
    assert float((pol(x, t=0) - pol(x, t=3)).detach().abs().max()) > 1e-3  # (the row is read)
    with pytest.raises(ValueError):
        pol(x)
    u = pol.forward_np(x[0].numpy(), 3)  # the real system's call (get_data_from_system passes t)
    ref = res_law(x[:1], 3, params, wide(kp), wide(kd), angle, non_angle, 1.3, True, target, pol.error_indices, pd_target, pos, vel)
    assert float(abs(u - ref.numpy()).max()) < 1e-15


def test_the_constructor():
    from mc_pilco_amd.policy_learning import Policy

    c = SHAPES["arm2"]
    x = torch.zeros(1, 4, dtype=DT)
    target, (kp, kd) = target_for(c, 6, x), gains_for(2, 1)
    params = network(c, (5,), c["angle"], c["not_angle"], 4, 1)
    pol = _policy(c, (5,), params, kp, kd, target, flg_train_gains=True)
    assert pol.sqrt_Kp_gains.requires_grad and pol.sqrt_Kd_gains.requires_grad
    assert {n for n, _ in pol.named_parameters()} == {"W0", "b0", "Wout", "bout", "sqrt_Kp_gains", "sqrt_Kd_gains"}
    zero = _policy(c, (5,), params, kp, kd, target, zero_output=True)  # from the PD law itself: the network's output layer is zero
    assert float(zero.Wout.detach().abs().max()) == 0 and float(zero.bout.detach().abs().max()) == 0 and float(zero.W0.detach().abs().max()) > 0
    from pd_models import pd_law

    xs = torch.randn(5, 4, dtype=DT, generator=torch.Generator().manual_seed(2))
    assert float((zero(xs, t=2).detach() - pd_law(xs, 2, kp, kd, target, 1.3, True, [0, 1], [2, 3])).abs().max()) < 1e-15
    zero.reinit()
    assert float(zero.Wout.detach().abs().max()) == 0 and float(zero.bout.detach().abs().max()) == 0 and float(zero.W0.detach().abs().max()) > 0
    pol.reinit()
    assert float(pol.Wout.detach().abs().max()) > 0
    bare = network(c, (5,), c["angle"], c["not_angle"], 0, 1)
    net_only = _policy(c, (5,), bare, kp, kd, None, pd_target_traj=target)  # no feature target
    assert net_only.target_traj is None and net_only.error_indices == [] and net_only.feature_dim == 6
    with pytest.raises(ValueError):  # neither target
        _policy(c, (5,), bare, kp, kd, None)
    with pytest.raises(ValueError):  # one list without the other
        _policy(c, (5,), params, kp, kd, target, pd_pos_indices=[0, 1])
    with pytest.raises(ValueError):  # one entry per input
        _policy(c, (5,), params, kp, kd, target, pd_pos_indices=[0], pd_vel_indices=[2])
    with pytest.raises(ValueError):  # three gains for two inputs
        _policy(c, (5,), params, torch.ones(3, dtype=DT), kd, target)
    with pytest.raises(ValueError):  # S = 4, U = 1: the default layout does not apply
        Policy.Residual_MLP_policy(state_dim=4, input_dim=1, hidden_sizes=[5], device=torch.device("cpu"), target_traj=target, sqrt_Kp_gains=[1.0],
                                   sqrt_Kd_gains=[1.0])
    one = Policy.Residual_MLP_policy(state_dim=4, input_dim=1, hidden_sizes=[5], device=torch.device("cpu"), target_traj=target, sqrt_Kp_gains=[1.0],
                                     sqrt_Kd_gains=[1.0], pd_pos_indices=[1], pd_vel_indices=[3])
    assert tuple(one(xs, t=0).shape) == (5, 1)
    with pytest.raises(TypeError):  # the gains are required
        Policy.Residual_MLP_policy(state_dim=4, input_dim=2, hidden_sizes=[5], device=torch.device("cpu"), target_traj=target)


def _fus(pol, model_like, T_):
    """Residual_MLP_policy.fusable on ``pol``'s settings with its parameters taken for GPU tensors (tests/test_mlp_track_cpu.py::_fus)."""
    view = type("V", (type(pol),), {"__init__": lambda self: None})()  # (an instance of the class: its fusable() asks its parent's first)
    view.__dict__.update({k: v for k, v in pol.__dict__.items() if not k.startswith("_") or k == "_lists"})
    view.__dict__.update(mlp_parameters=lambda: [_GpuView(q) for q in pol.mlp_parameters()], sqrt_Kp_gains=_GpuView(pol.sqrt_Kp_gains),
                         sqrt_Kd_gains=_GpuView(pol.sqrt_Kd_gains))
    return view.fusable(model_like, T_)


def test_fusable():
    c = SHAPES["arm2"]
    model_like = type("M", (), dict(S=c["S"], U=c["U"]))()
    x = torch.zeros(1, c["S"], dtype=DT)
    kp, kd = gains_for(2, 1)
    target = target_for(c, 6, x)  # 8 rows
    mk = lambda tgt=target, idx=None, **kw: _policy(c, (5,), network(c, (5,), c["angle"], c["not_angle"], c["S"] if idx is None else len(idx), 1), kp, kd,
                                                    tgt, idx, **kw)
    assert _fus(mk(), model_like, 8) is True and _fus(mk(), model_like, 1) is True
    assert _fus(mk(), model_like, 9) is False  # rows < T (the parent's answer)
    assert _fus(mk(idx=[]), model_like, 8) is True  # no error features, the PD term keeps its target
    assert _fus(mk(pd_target_traj=target[:5]), model_like, 6) is False  # the PD target's own rows < T
    assert _fus(mk(pd_target_traj=target[:5]), model_like, 5) is True
    assert _fus(mk(pd_target_traj=target.to(torch.float32)), model_like, 4) is False
    assert _fus(mk(pd_target_traj=target[:, :3]), model_like, 4) is False  # not [rows, S]
    assert _fus(mk(pd_pos_indices=[1, 1], pd_vel_indices=[2, 3]), model_like, 4) is False  # repeated within pos
    assert _fus(mk(pd_pos_indices=[1, 0], pd_vel_indices=[2, 4]), model_like, 4) is False  # out of range
    assert _fus(mk(pd_pos_indices=[1, 0], pd_vel_indices=[1, 0]), model_like, 4) is True  # across the two lists a component may repeat
    assert _fus(mk(idx=[3, 3]), model_like, 4) is False  # (the parent's refusals stand)
    cpu = mk()
    assert cpu.fusable(model_like, 4) is False  # CPU parameters


def test_without_gains_the_parent_class_is_untouched():
    """MLP_policy's forward is the expression it was (tests/test_mlp_track_cpu.py checks the bits); the object has nothing of the term."""
    from mc_pilco_amd.policy_learning import Policy

    c = SHAPES["arm2"]
    params = network(c, (5,), c["angle"], c["not_angle"], 0, 11)
    pol = Policy.MLP_policy(state_dim=4, input_dim=2, hidden_sizes=[5], angle_indices=c["angle"], non_angle_indices=c["not_angle"], u_max=1.3,
                            weight_init=params, dtype=DT, device=torch.device("cpu"))
    assert not hasattr(pol, "sqrt_Kp_gains") and not hasattr(pol, "pd_target_traj") and pol._packed_key_extra() == ()
    assert {n for n, _ in pol.named_parameters()} == {"W0", "b0", "Wout", "bout"}
    x = torch.randn(9, 4, dtype=DT, generator=torch.Generator().manual_seed(4))
    h = torch.tanh(torch.cat([x[:, c["not_angle"]], torch.sin(x[:, c["angle"]]), torch.cos(x[:, c["angle"]])], dim=1) @ params[0].t() + params[1])
    assert torch.equal(pol(x).detach(), pol.f_squash(h @ params[2].t() + params[3]))
    assert torch.equal(pol.network(x).detach(), h @ params[2].t() + params[3])


# ---- the truth's conditioning ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_truth_is_conditioned(case):
    """On every case: the variances stay positive, everything is finite, every differentiated tensor has a nonzero gradient, and each of
    g_sqrt_kp, g_sqrt_kd has a largest entry of at least 1e-3 of the largest gradient entry -- the project's rule for the error columns."""
    mode, shape, deg, N, Tc, Mc, hidden, opt = case
    c, m, ins, (st, inp, ym, grads, gx0, vmin) = case_truth(case)
    if Tc > 1:
        assert vmin > 0.0
    rows = Tc + opt.get("rows_extra", 0)
    assert tuple(ins["target"].shape) == (rows, c["S"]) and tuple(ins["pd_target"].shape) == (rows, c["S"])
    assert (ins["pd_target"] is ins["target"]) is (opt.get("pd_target") != "other")
    assert len(grads) == len(ins["params"]) + 2 and tuple(grads[-2].shape) == tuple(ins["kp"].shape) == ((1,) if opt.get("scalar_gain") else (c["U"],))
    assert bool(torch.isfinite(st).all()) and bool(torch.isfinite(inp).all()) and all(bool(torch.isfinite(g).all()) for g in grads + [gx0])
    assert all(float(g.abs().max()) > 0 for g in grads) and float(gx0.abs().max()) > 0
    big = max(float(g.abs().max()) for g in grads)
    gkp, gkd = float(grads[-2].abs().max()), float(grads[-1].abs().max())
    print("%s: min var %.3e, |g sqrt_kp| %.3e |g sqrt_kd| %.3e of %.3e" % (case_id(case), vmin, gkp, gkd, big))
    assert gkp >= 1e-3 * big and gkd >= 1e-3 * big
    assert (ym is None) == ("meas" not in opt)
    if ins["masks"] is not None:
        assert mdm.masks_mixed(ins["masks"], hidden)


def test_the_table_covers_what_it_names():
    opts = [c[7] for c in CASES]
    assert {c[4] for c in CASES} == {1, 2, 3, 12} and {1, 5, 17, 1041} <= {c[5] for c in CASES}
    assert sum(c[5] == 1041 for c in CASES) == 1
    assert {"arm2", "arm2_delta", "ur5", "limits"} == {c[1] for c in CASES} and {"mean", "sampled"} == {c[0] for c in CASES}
    assert {c[3] for c in CASES if c[1] == "ur5"} == {48} and {c[3] for c in CASES if c[1] != "ur5"} == {37}
    assert {len(c[6]) for c in CASES} == {1, 2} and ("limits", (64, 64)) in {(c[1], c[6]) for c in CASES}
    for case in CASES:
        c, _, ins = case_inputs(case) if case[1] == "limits" or "pos" in case[7] else (SHAPES[case[1]], None, None)
        if case[1] == "limits":
            assert (c["S"], c["U"]) == (16, 8) and tuple(ins["params"][0].shape) == (64, 32)
        if ins is not None:  # explicit lists: not the default layout, not ascending, each without a repeat and in range
            assert (ins["pos"], ins["vel"]) != default_lists(c) and ins["pos"] != sorted(ins["pos"]) and len(ins["pos"]) == len(ins["vel"]) == c["U"]
            assert len(set(ins["pos"])) == c["U"] == len(set(ins["vel"])) and all(0 <= i < c["S"] for i in ins["pos"] + ins["vel"])
    assert sum("pos" in o for o in opts) >= 2 and any("pos" in o and "meas" in o for o in opts)
    assert any(o.get("idx") == [] for o in opts) and any("idx" in o and o["idx"] and list(o["idx"]) != sorted(o["idx"]) for o in opts)
    assert any(o.get("features") == "state" for o in opts)
    for key in ("squash", "no_g_inputs", "fixed_gains", "scalar_gain"):
        assert sum(key in o for o in opts) == 1, key
    assert [o["only_grad"] for o in opts if "only_grad" in o] == ["kp"]
    assert sum(o.get("pd_target") == "other" for o in opts) >= 1 and any("pd_target" not in o for o in opts)
    assert sum("meas" in o and "p" not in o for o in opts) == 1 and sum("p" in o and "meas" not in o for o in opts) == 1
    assert sum("meas" in o and "p" in o for o in opts) == 1 and {o["p"] for o in opts if "p" in o} == {0.25}


@pytest.mark.parametrize("case", [c for c in CASES if c[4] == 12], ids=case_id)
def test_near_misses_are_far_from_the_truth(case):
    """A rollout whose PD term leaves the gains unsquared, flips the error's sign, sits outside the squashing, reads the target a row early or
    late or row 0 throughout, swaps pos and vel or (measured) takes the error on the true state differs from the truth in the states by at
    least 1e-6 -- 1000 times the GPU test's state bound -- and leaves row 0 equal."""
    c, m, ins, truth = case_truth(case)
    for defect in DEFECTS:
        if defect == "true_state" and ins["ms"] is None:
            continue
        if defect == "outside_squash" and not ins["squash"]:
            continue
        st = truth_of(m, ins, defect=defect)[0]
        d = float((st - truth[0]).abs().max())
        print("%s, %s: |states - truth| %.3e" % (case_id(case), defect, d))
        assert d >= 1e-6 and torch.equal(st[0], truth[0][0])
