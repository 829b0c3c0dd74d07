"""CPU-only checks around the fused closed loop under the PID controller: the truth the GPU tests compare with (tests/pid_models.pid_truth)
against the PD truth it extends and against its own central differences, the two clamp conditions every GPU case is held to (asserted here
on the truth alone, so the GPU test cannot hide a flipped clamp), Policy.PID_controller's torch formula, the mcp_pid_term layout, and the
library's two entries with their host-side argument checks in the documented order."""
import ctypes as C
import functools
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import noise_truth
import pid_models as pm
from pd_models import SHAPES, build_pair, inputs_for, pd_truth
from test_pd_rollout_cpu import _fusable_but_for_the_device, _valid_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
INF = pm.INF


@functools.lru_cache(maxsize=None)
def _pair(shape, N, deg):
    return build_pair(shape, N, deg, seed=N + deg)


def relmax(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---- the truth ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [False, True])
def test_truth_without_integral_gain_is_the_pd_truth(sample):
    """sqrt_ki = 0 (a finite bound, so the clamp is live): states and inputs are pd_truth's, the gradients agree to 1e-14 relative."""
    torch.set_num_threads(1)
    c, m, _ = _pair("arm2", 37, 1)
    x0, kp, kd, target, eps, w, wu = inputs_for(c, 5, 12, seed=1205)
    t = pm.pid_truth("arm2", m, x0, kp, kd, torch.zeros(2, dtype=DT), target, eps, w, wu, sample, i_max=0.05)
    st, inp, gkp, gkd, gx, _ = pd_truth("arm2", m, x0, kp, kd, target, eps, w, wu, sample)
    assert torch.equal(t.states, st) and torch.equal(t.inputs, inp)
    assert relmax(t.grads[0], gkp) < 1e-14 and relmax(t.grads[1], gkd) < 1e-14 and relmax(t.g_x0, gx) < 1e-14
    assert float(t.grads[2].abs().max()) == 0.0 and 0.1 < pm.clamp_figures(t, 0.05)[0] < 0.9


def _fd_truth():
    F = pm.FD_CASE
    c, m, _ = _pair(F["shape"], F["N"], F["deg"])
    x0, kp, kd, ki, target, w, wu = pm.fd_inputs()
    eps = torch.as_tensor(noise_truth.eps_table(F["philox"][0], F["philox"][1], F["T"], F["M"], c["G"]), dtype=DT)
    args = lambda ts: (F["shape"], m, ts[3], ts[0], ts[1], ts[2], target, eps, w, wu, True)
    return F, [kp, kd, ki, x0], args


@pytest.mark.parametrize("measured", [False, True])
def test_truth_gradients_against_central_differences(measured):
    """On the central-difference case (margin >= 1e-3 against a step of 1e-6: no clamp changes side): every gain, first and last entry, and
    two entries of x0, to 1e-6 relative with floor 1e-3 (the difference's own truncation and rounding at this step)."""
    torch.set_num_threads(1)
    F, tensors, args = _fd_truth()
    kw = dict(i_max=F["i_max"])
    if measured:
        ms = pm.meas_model(F["shape"], "all")
        kw.update(ms=ms, pos_noise=pm.pos_noise_for(F["T"], F["M"], len(ms["pos"]), 5))
    t = pm.pid_truth(*args(tensors), **kw)
    share, margin = pm.clamp_figures(t, F["i_max"])
    assert margin >= pm.FD_MARGIN and pm.SHARE[0] <= share <= pm.SHARE[1]
    grads = t.grads + [t.g_x0]
    for i, e in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 1), (3, 2 * 4 + 1)):
        plus, minus = [q.clone() for q in tensors], [q.clone() for q in tensors]
        plus[i].reshape(-1)[e] += 1e-6
        minus[i].reshape(-1)[e] -= 1e-6
        fd = (pm.loss_of(*args(plus), **kw) - pm.loss_of(*args(minus), **kw)) / 2e-6
        g = float(grads[i].reshape(-1)[e])
        print("tensor %d entry %d: fd %.9e autograd %.9e" % (i, e, fd, g))
        assert abs(fd - g) < 1e-6 * max(abs(g), 1e-3)


def test_clamp_conditions_hold_on_every_case():
    """Over the finite-i_max cases the truth has clamped and unclamped (t, m, k) entries in the same case, each share within [0.1, 0.9];
    every case keeps min | |q| - i_max | >= 1e-7, the central-difference case >= 1e-3; every sampled case keeps its variances positive."""
    torch.set_num_threads(1)
    finite = 0
    for case in pm.CASES:
        mode, shape, deg, N, T, M, variant, opt = case
        c, m, _ = _pair(shape, N, deg)
        t, inp = pm.case_truth(case, m)
        share, margin = pm.clamp_figures(t, inp[-1]["i_max"])
        print("%s: clamped share %.2f margin %.3e" % (pm.case_id(case), share, margin))
        assert margin >= pm.MARGIN, pm.case_id(case)
        if "i_max" in opt:
            finite += 1
            assert pm.SHARE[0] <= share <= pm.SHARE[1], pm.case_id(case)
        else:
            assert share == 0.0
        assert mode != "sampled" or T == 1 or t.vmin > 0, pm.case_id(case)
        assert torch.equal(t.integ, torch.clamp(t.q, -pm.bounds(inp[-1]["i_max"], c["U"]), pm.bounds(inp[-1]["i_max"], c["U"])))
    assert finite >= 20
    F, tensors, args = _fd_truth()
    share, margin = pm.clamp_figures(pm.pid_truth(*args(tensors), i_max=F["i_max"]), F["i_max"])
    print("central-difference case: clamped share %.2f margin %.3e" % (share, margin))
    assert margin >= pm.FD_MARGIN and pm.SHARE[0] <= share <= pm.SHARE[1]


# ---- the class ------------------------------------------------------------------------------------------------------------------------------------
def _policy(S=4, U=2, rows=10, dtype=DT, ki=(0.7, 0.9), i_max=None, Ts=0.05, target=None, **kw):
    from mc_pilco_amd.policy_learning import Policy

    return Policy.PID_controller(state_dim=S, input_dim=U, sqrt_Kp_gains=np.asarray((1.0, 1.2)[:U]), sqrt_Kd_gains=np.asarray((0.5, 0.4)[:U]),
                                 sqrt_Ki_gains=np.asarray(ki), T_sampling=Ts, i_max=i_max,
                                 target_traj=torch.zeros(rows, S, dtype=dtype) if target is None else target, flg_trainable=True, dtype=dtype,
                                 device=torch.device("cpu"), **kw)


@pytest.mark.parametrize("i_max", [None, 0.02, [0.02, INF]])
def test_class_forward_is_the_truth_law(i_max):
    """PID_controller.forward on CPU tensors, row after row on given states, against pid_models.pid_law; the gradients of a loss through
    the held integral against the law's; t == 0 resets; a call out of order or on another particle count raises ValueError."""
    c = SHAPES["arm2"]
    M, T = 5, 8
    x0, kp, kd, target, eps, w, wu = inputs_for(c, M, T, seed=77)
    gen = torch.Generator().manual_seed(9)
    xs = 0.8 * (torch.rand(T, M, 4, dtype=DT, generator=gen) - 0.5)
    ki = pm.ki_for(c, 77)
    pol = _policy(ki=ki.numpy(), i_max=i_max, target=target, u_max=[0.4, 1.7])
    with torch.no_grad():
        pol.sqrt_Kp_gains.copy_(kp), pol.sqrt_Kd_gains.copy_(kd)
    assert [n for n, _ in pol.named_parameters()] == ["sqrt_Kp_gains", "sqrt_Kd_gains", "sqrt_Ki_gains"] and all(q.requires_grad for q in pol.parameters())
    tk = [g.clone().requires_grad_(True) for g in (kp, kd, ki)]
    for rounds in range(2):  # (the second pass starts at t == 0 again: the integral is reset)
        integ, us, ut = torch.zeros(M, 2, dtype=DT), [], []
        for t in range(T):
            us.append(pol(xs[t], t))
            u, integ, _ = pm.pid_law(xs[t], t, integ, tk[0], tk[1], tk[2], target, 0.05, INF if i_max is None else i_max, [0.4, 1.7], True, [0, 1], [2, 3])
            ut.append(u)
        us, ut = torch.stack(us), torch.stack(ut)
        assert float((us - ut).detach().abs().max()) < 1e-15
        if i_max is not None:
            assert 0.1 < float((integ.abs() >= 0.02).to(DT).mean()) < 0.9  # (the last row: both sides of the clamp)
    g = torch.autograd.grad((wu * us).sum(), list(pol.parameters()))
    gt = torch.autograd.grad((wu * ut).sum(), tk)
    assert all(relmax(a, b) < 1e-13 for a, b in zip(g, gt))
    with pytest.raises(ValueError):
        pol(xs[0], 3)  # after t = T - 1
    pol(xs[0], 0)
    with pytest.raises(ValueError):
        pol(xs[1][:3], 1)  # another particle count
    with pytest.raises(ValueError):
        _policy()(xs[0], 1)  # never reset


def test_fusable_truth_table():
    from mc_pilco_amd import ops

    model = types.SimpleNamespace(S=4, U=2)
    names = ("sqrt_Kp_gains", "sqrt_Kd_gains", "sqrt_Ki_gains")
    on_gpu = lambda pol, mdl=model, Tn=8: _fusable_with(pol, mdl, Tn, names)
    assert _policy().fusable(model, 8) is False  # CPU parameters
    assert _fusable_but_for_the_device(_policy(), model, 8) is False  # the third gain is looked at too
    assert on_gpu(_policy()) is True and on_gpu(_policy(i_max=0.05)) is True and on_gpu(_policy(i_max=[0.05, INF])) is True
    assert on_gpu(_policy(ki=(0.7,))) is True  # one value for all
    for pol in (_policy(rows=7), _policy(dtype=torch.float32), _policy(Ts=0.0), _policy(Ts=float("nan")), _policy(i_max=0.0), _policy(i_max=[0.05, -1.0]),
                _policy(i_max=[0.05, 0.05, 0.05]), _policy(i_max=float("nan"))):
        assert on_gpu(pol) is False
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rollout_pd(model, _policy().packed(), None, torch.zeros(3, 4, dtype=DT), 4)
    assert issubclass(ops.PackedPID, ops.PackedPD) and ops.PackedPID.fwd_pid == "mcp_rollout_pid" and ops.PackedPID.bwd_pid == "mcp_rollout_pid_bwd"


def _fusable_with(pol, model, Tn, names):
    """``fusable`` with the device condition taken out of the named gains (tests/test_pd_rollout_cpu.py's device stand-in, for three)."""

    class OnGpu:
        def __init__(self, t):
            self.t, self.is_cuda, self.dtype = t, True, t.dtype

        def numel(self):
            return self.t.numel()

    saved = dict(pol._parameters)
    try:
        for n in names:
            del pol._parameters[n]
            object.__setattr__(pol, n, OnGpu(saved[n]))
        return pol.fusable(model, Tn)
    finally:
        for n in names:
            object.__delattr__(pol, n)
        pol._parameters.update(saved)


# ---- the descriptor and the entries -----------------------------------------------------------------------------------------------------------------
def test_pid_term_struct_layout_matches_header(tmp_path):
    """mcp_pid_term against hipabi.PIDTerm through gcc; the ABI version is still 7 and mcp_pd_policy did not move."""
    from mc_pilco_amd import hipabi

    names = [f[0] for f in hipabi.PIDTerm._fields_]
    assert names == ["on", "sqrt_ki", "i_max", "dt", "integ"]
    pd_names = [f[0] for f in hipabi.PDPolicy._fields_]
    src = tmp_path / "pid.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(){printf("%zu", sizeof(mcp_pid_term));'
                   + "".join('printf(" %%zu", offsetof(mcp_pid_term, %s));' % n for n in names) + 'printf(" %d", MCP_ABI_VERSION);'
                   + 'printf(" %zu", sizeof(mcp_pd_policy));' + "".join('printf(" %%zu", offsetof(mcp_pd_policy, %s));' % n for n in pd_names)
                   + "return 0;}\n")
    exe = tmp_path / "pid"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == ([C.sizeof(hipabi.PIDTerm)] + [getattr(hipabi.PIDTerm, n).offset for n in names] + [7] + [C.sizeof(hipabi.PDPolicy)]
                   + [getattr(hipabi.PDPolicy, n).offset for n in pd_names])
    # the figures of the commit before the term: 8-byte alignment, MCP_MAX_INPUT == 8
    assert C.sizeof(hipabi.PDPolicy) == 168 and [getattr(hipabi.PDPolicy, n).offset for n in pd_names] == [0, 4, 8, 40, 72, 136, 144, 152, 160]
    assert hipabi.lib().mcp_abi_version() == 7


def _term(on=1):
    from mc_pilco_amd import hipabi

    t = hipabi.PIDTerm()
    t.on, t.dt = on, 0.05
    t.sqrt_ki = t.integ = 0x1000  # (never followed)
    for k in range(hipabi.MAX_INPUT):
        t.i_max[k] = 0.05 if k else INF
    return t


def test_library_exports_and_argument_checks_without_gpu():
    """Every refusal of both entries, without a launch: those of the PD entries in their order, then the term's own."""
    from mc_pilco_amd import hipabi

    lib = hipabi.lib()
    assert "mcp_rollout_pid" in hipabi.EXPORTED and "mcp_rollout_pid_bwd" in hipabi.EXPORTED
    ARG, LIMIT = -1, -2
    n = hipabi.Noise()
    one = C.c_void_p(0x1000)  # a non-NULL pointer the checks never follow
    ref = lambda s: None if s is None else C.byref(s)
    fwd = lambda m_, p_, t_, ms=None, M=4, Tn=8, x0=one: lib.mcp_rollout_pid(ref(m_), ref(p_), ref(t_), ref(ms), C.byref(n), M, Tn, 1, x0, one, one, None,
                                                                              None, None, one, None)
    bwd = lambda m_, p_, t_, ms=None, M=4, Tn=8, gs=one, jac=one: lib.mcp_rollout_pid_bwd(ref(m_), ref(p_), ref(t_), ref(ms), M, Tn, one, one, jac, gs, None,
                                                                                         None, None, None)
    m, p = _valid_descriptors()
    t = _term()
    assert bwd(m, p, t) == 0  # every check passes and nothing is asked for: no launch
    assert bwd(m, p, None) == 0 and bwd(m, p, _term(on=0)) == 0  # pid NULL / on == 0: the PD sweep's checks, accepted
    ms0 = hipabi.Meas()  # n == 0: the true state
    assert bwd(m, p, t, ms0) == 0 and bwd(m, p, None, ms0) == 0
    for call in (fwd, bwd):
        # the PD entries' refusals, in their order, with a valid term, with none, and ahead of a bad one
        for term in (t, None, _bad_term("dt", 0.0)):
            assert call(None, p, term) == ARG and call(m, None, term) == ARG
            assert call(m, p, term, Tn=0) == ARG and call(m, p, term, M=0) == ARG
            assert call(m, p, term, Tn=9) == ARG  # target_rows < T
            for field, bad in (("pos", 4), ("vel", -1), ("pos", 1)):  # out of range, negative, repeated
                m2, p2 = _valid_descriptors()
                getattr(p2, field)[0] = bad
                assert call(m2, p2, term) == ARG
            m2, p2 = _valid_descriptors()
            p2.U = 1
            assert call(m2, p2, term) == ARG  # U != model->U
            p2.U = hipabi.MAX_INPUT + 1
            assert call(m2, p2, term) == LIMIT  # (a limit ahead of the bad term's MCP_ERR_ARG)
            m2, p2 = _valid_descriptors()
            m2.S = hipabi.MAX_STATE + 1
            assert call(m2, p2, term) == LIMIT
            m2, p2 = _valid_descriptors()
            p2.sqrt_kp = None
            assert call(m2, p2, term) == ARG
            msb = hipabi.Meas()
            msb.n = 3  # 2 n > S: the measurement's refusal
            assert call(m, p, term, msb) == ARG
        # the term's own: a NULL pointer, dt, a bound
        for field in ("sqrt_ki", "integ"):
            assert call(m, p, _bad_term(field, None)) == ARG
        for dt in (0.0, -0.05, float("nan")):
            assert call(m, p, _bad_term("dt", dt)) == ARG
        for v in (0.0, -1.0, float("nan")):
            bad = _term()
            bad.i_max[1] = v
            assert call(m, p, bad) == ARG
    # (accepted descriptors go to the sweep alone, which asks for nothing here and so launches nothing)
    bad = _term()
    bad.i_max[2] = -1.0  # beyond U: not looked at
    assert bwd(m, p, bad) == 0
    off = _bad_term("dt", -1.0)  # on == 0: nothing of the term is looked at
    off.on, off.sqrt_ki = 0, None
    assert bwd(m, p, off) == 0
    assert fwd(m, p, t, x0=None) == ARG and bwd(m, p, t, gs=None) == ARG
    assert bwd(m, p, t, jac=None) == ARG and bwd(m, p, t, Tn=1, jac=None) == 0  # T == 1: the policy alone, no record
    m2, p2 = _valid_descriptors()
    p2.u_max[1] = 0.0
    assert fwd(m2, p2, t) == ARG


def _bad_term(field, value):
    t = _term()
    setattr(t, field, value)
    return t
