"""CPU-only checks around the fused closed loop under the PD controller: the truth the GPU tests compare with (tests/pd_models.pd_truth)
pinned to the reference's own run (tests/golden/rollout_pd.npz, made by tests/golden/make_golden_pd.py), the mcp_pd_policy layout, the
library's two entries and their host-side argument checks, and the host-side choice of the path."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from pd_models import CASES, build_pair, case_id, golden_model, inputs_for, pd_truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64


def T(a):
    return torch.as_tensor(np.asarray(a), dtype=DT)


def relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


@pytest.mark.parametrize("kind", ["speed", "delta"])
def test_truth_is_pinned_to_the_reference(golden, kind):
    """pd_truth on the reference's alpha / Kinv and replayed noise against the reference's MC_PILCO.apply_policy with
    PD_controller(flg_trainable=True) and backward(): the bounds tests/test_oracle_golden_delta.py holds rollout_delta.npz to (SE models:
    states and inputs 1e-12 absolute, gradients 1e-10 relative to the gradient's largest magnitude)."""
    fx = golden("rollout_pd")
    k = lambda n: fx[kind + "_" + n]
    m = golden_model(fx, kind)
    x0 = T(k("x0_mean")).reshape(1, -1) + torch.sqrt(T(k("x0_var"))).reshape(1, -1) * T(k("eps0"))
    assert np.array_equal(x0.numpy(), k("states")[0])  # bit-exact x0
    torch.set_num_threads(1)
    shape = "arm2" if kind == "speed" else "arm2_delta"
    st, inp, gkp, gkd, _, vmin = pd_truth(shape, m, x0, T(k("sqrt_kp")), T(k("sqrt_kd")), T(k("target")), T(k("eps")), T(k("w")), T(k("wu")), True,
                                          u_max=float(k("u_max")))
    es, ei = np.max(np.abs(st.numpy() - k("states"))), np.max(np.abs(inp.numpy() - k("inputs")))
    ep, ed = relerr(gkp.numpy(), k("g_sqrt_kp")), relerr(gkd.numpy(), k("g_sqrt_kd"))
    print("%s: states %.3e inputs %.3e g_sqrt_kp %.3e g_sqrt_kd %.3e (min var %.3e)" % (kind, es, ei, ep, ed, vmin))
    assert vmin > 0
    assert es < 1e-12 and ei < 1e-12
    assert ep < 1e-10 and ed < 1e-10
    assert k("states").shape == (8, 6, 4) and k("inputs").shape == (8, 6, 2) and float(np.abs(k("g_sqrt_kp")).max()) > 0


def test_sampled_cases_keep_their_variance_positive():
    """The condition of the GPU parity test, checked where it costs no GPU time: in every sampled case the truth's smallest variance is
    positive (a case that violated it would get other gains, target or seed -- never another bound)."""
    torch.set_num_threads(1)
    for case in CASES:
        mode, shape, deg, N, Tn, M, opt = case
        if mode != "sampled" or N > 48 or shape == "ur5":  # (the larger models are checked by the GPU test itself, on its own truth)
            continue
        c, m, _ = build_pair(shape, N, deg, seed=N + deg)
        x0, kp, kd, target, eps, w, wu = inputs_for(c, M, Tn, seed=Tn * 100 + M)
        *_, vmin = pd_truth(shape, m, x0, kp, kd, target, eps, w, wu, True, u_max=opt.get("u_max", 1.0), squash=opt.get("squash", True),
                            var_scale=opt.get("var_scale"))
        assert Tn == 1 or vmin > 0, case_id(case)


def test_pd_policy_struct_layout_matches_header(tmp_path):
    from mc_pilco_amd import hipabi

    names = [f[0] for f in hipabi.PDPolicy._fields_]
    assert names == ["U", "squash", "pos", "vel", "u_max", "sqrt_kp", "sqrt_kd", "target_traj", "target_rows"]
    src = tmp_path / "pd.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(){printf("%zu", sizeof(mcp_pd_policy));'
                   + "".join('printf(" %%zu", offsetof(mcp_pd_policy, %s));' % n for n in names) + 'printf(" %d", MCP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "pd"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(hipabi.PDPolicy)] + [getattr(hipabi.PDPolicy, n).offset for n in names] + [7]


def _valid_descriptors():
    """A model and a PD descriptor that pass every host-side check (their device pointers are never followed: each call below is refused
    before a launch)."""
    from mc_pilco_amd import hipabi

    m = hipabi.Model()
    m.S, m.U, m.G, m.D, m.n_angle, m.n_not_angle = 4, 2, 2, 8, 2, 2
    for i, v in enumerate([0, 1]):
        m.angle[i] = v
    for i, v in enumerate([2, 3]):
        m.not_angle[i] = v
    for g, (v, q) in enumerate([(2, 0), (3, 1)]):
        m.vel[g], m.not_vel[g] = v, q
        gp = m.gp[g]
        gp.kern.D, gp.N, gp.Npad = 8, 37, 48
        gp.Xt = gp.X = gp.alpha = gp.Kinv = gp.kern.inv_ls = 0x1000  # (never read)
    p = hipabi.PDPolicy()
    p.U, p.squash, p.target_rows = 2, 1, 8
    for k in range(2):
        p.pos[k], p.vel[k], p.u_max[k] = k, 2 + k, 1.0
    p.sqrt_kp = p.sqrt_kd = p.target_traj = 0x1000
    return m, p


def test_library_exports_and_argument_checks_without_gpu():
    from mc_pilco_amd import hipabi

    lib = hipabi.lib()
    assert hasattr(lib, "mcp_rollout_pd") and hasattr(lib, "mcp_rollout_pd_bwd")
    assert "mcp_rollout_pd" in hipabi.EXPORTED and "mcp_rollout_pd_bwd" in hipabi.EXPORTED
    ARG, LIMIT = -1, -2
    n = hipabi.Noise()
    one = C.c_void_p(0x1000)  # a non-NULL pointer the checks never follow
    m, p = _valid_descriptors()
    fwd = lambda m_, p_, M=4, Tn=8, x0=one: lib.mcp_rollout_pd(None if m_ is None else C.byref(m_), None if p_ is None else C.byref(p_), C.byref(n), M, Tn, 1, x0,
                                                               one, one, None, None, None, one, None)
    bwd = lambda m_, p_, M=4, Tn=8, gs=one, jac=one: lib.mcp_rollout_pd_bwd(None if m_ is None else C.byref(m_), None if p_ is None else C.byref(p_), M, Tn, one,
                                                                           one, jac, gs, None, None, None, None)
    assert bwd(m, p) == 0  # every check passes and nothing is asked for: no launch
    for call in (fwd, bwd):
        assert call(None, p) == ARG and call(m, None) == ARG
        assert call(m, p, Tn=0) == ARG and call(m, p, M=0) == ARG
        assert call(m, p, Tn=9) == ARG  # target_rows < T
        for field, bad in (("pos", 4), ("vel", -1), ("pos", 1)):  # out of range, negative, repeated
            m2, p2 = _valid_descriptors()
            getattr(p2, field)[0] = bad
            assert call(m2, p2) == ARG
        m2, p2 = _valid_descriptors()
        p2.U = 1
        assert call(m2, p2) == ARG  # U != model->U
        p2.U = hipabi.MAX_INPUT + 1
        assert call(m2, p2) == LIMIT
        m2, p2 = _valid_descriptors()
        m2.S = hipabi.MAX_STATE + 1
        assert call(m2, p2) == LIMIT
        m2, p2 = _valid_descriptors()
        p2.sqrt_kp = None
        assert call(m2, p2) == ARG
    assert fwd(m, p, x0=None) == ARG and bwd(m, p, gs=None) == ARG
    assert bwd(m, p, jac=None) == ARG and bwd(m, p, Tn=1, jac=None) == 0  # T == 1: the policy alone, no record
    m2, p2 = _valid_descriptors()
    p2.u_max[1] = 0.0
    assert fwd(m2, p2) == ARG


def _policy(S=4, U=2, rows=10, dtype=DT, kp=(1.0, 1.2), kd=(0.5, 0.4)):
    from mc_pilco_amd.policy_learning import Policy

    return Policy.PD_controller(state_dim=S, input_dim=U, sqrt_Kp_gains=np.asarray(kp), sqrt_Kd_gains=np.asarray(kd),
                                target_traj=torch.zeros(rows, S, dtype=dtype), flg_trainable=True, dtype=dtype, device=torch.device("cpu"))


def test_host_side_path_choice():
    from mc_pilco_amd import ops

    model = types.SimpleNamespace(S=4, U=2)
    ok = _policy()
    assert ok.fusable(model, 8) is False  # CPU parameters
    # the other conditions, each with everything else in order
    for pol, mdl, Tn in ((_policy(S=5, U=2, kp=(1.0, 1.0), kd=(1.0, 1.0)), types.SimpleNamespace(S=5, U=2), 8),   # odd S
                         (_policy(S=4, U=1, kp=(1.0,), kd=(1.0,)), types.SimpleNamespace(S=4, U=1), 8),             # input_dim != S / 2
                         (_policy(rows=7), model, 8),                                                                 # short target
                         (_policy(dtype=torch.float32), model, 8)):                                                   # float32
        assert _fusable_but_for_the_device(pol, mdl, Tn) is False
    assert _fusable_but_for_the_device(ok, model, 8) is True and _fusable_but_for_the_device(ok, model, 10) is True
    assert _fusable_but_for_the_device(ok, model, 11) is False
    x0 = torch.zeros(3, 4, dtype=DT)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rollout_pd(model, types.SimpleNamespace(sqrt_kp=ok.sqrt_Kp_gains, sqrt_kd=ok.sqrt_Kd_gains), None, x0, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rollout_pd(model, ok.packed(), None, x0, 4)


def _fusable_but_for_the_device(pol, model, Tn):
    """``fusable`` with the device condition taken out: the gains report ``is_cuda`` (nothing else of them is touched on this path)."""

    class OnGpu:
        def __init__(self, t):
            self.t = t
            self.is_cuda = True
            self.dtype = t.dtype

        def numel(self):
            return self.t.numel()

    saved = dict(pol._parameters)
    try:
        for n in ("sqrt_Kp_gains", "sqrt_Kd_gains"):
            del pol._parameters[n]
            object.__setattr__(pol, n, OnGpu(saved[n]))
        return pol.fusable(model, Tn)
    finally:
        for n in ("sqrt_Kp_gains", "sqrt_Kd_gains"):
            object.__delattr__(pol, n)
        pol._parameters.update(saved)
