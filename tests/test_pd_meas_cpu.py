"""CPU-only checks around the fused closed loop under the PD controller on a simulated measurement (mcp_rollout_pd_meas /
mcp_rollout_pd_meas_bwd): the truth the GPU tests compare with (tests/pd_meas_models.pd_meas_truth) pinned to the reference's own
MC_PILCO4PMS.apply_policy run (tests/golden/rollout_pd_pms.npz, made by tests/golden/make_golden_pd_pms.py), its gradients against central
differences, the fixture's power to tell the measurement formulas from their near misses, and the two entries' host-side argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from pd_meas_models import loss_of, pd_meas_truth
from pd_models import golden_model

DT = torch.float64


def T(a):
    return torch.as_tensor(np.asarray(a), dtype=DT)


def relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def fixture_run(fx, kind, defect=None):
    """pd_meas_truth on the reference's alpha / Kinv and replayed draws.  Returns (k, truth tuple, eps0)."""
    k = lambda n: fx[kind + "_" + n]
    m = golden_model(fx, kind)
    x0 = T(k("x0_mean")).reshape(1, -1) + torch.sqrt(T(k("x0_var"))).reshape(1, -1) * T(k("eps0"))
    ms = dict(pos=[int(i) for i in k("pos_indeces")], vel=[int(i) for i in k("vel_indeces")],
              std=[float(v) for v in k("std_meas_noise")[k("pos_indeces")]], b=[float(v) for v in k("butter_b")],
              a=[float(v) for v in k("butter_a")], Ts=float(k("Ts")))
    shape = "arm2" if kind == "speed" else "arm2_delta"
    torch.set_num_threads(1)
    args = (shape, m, x0, T(k("sqrt_kp")), T(k("sqrt_kd")), T(k("target")), T(k("eps")), T(k("pos_noise")), T(k("w")), T(k("wu")), True, ms)
    return k, x0, args, pd_meas_truth(*args, u_max=float(k("u_max")), defect=defect)


@pytest.mark.parametrize("kind", ["speed", "delta"])
def test_truth_is_pinned_to_the_reference(golden, kind):
    """States, inputs and the three gradients to 1e-10 of the largest entry (the level tests/test_pd_rollout_cpu.py holds pd_truth to).  The
    reference's x0 is mean + sqrt(var) eps0 with a leaf mean and variance: its gradients are sum_m dL/dx0[m] and
    sum_m dL/dx0[m] eps0[m] / (2 sqrt(var)), two independent weightings of the truth's per-particle dL/dx0."""
    fx = golden("rollout_pd_pms")
    k, x0, _, (st, inp, ym, gkp, gkd, gx, vmin) = fixture_run(fx, kind)
    assert np.array_equal(x0.numpy(), k("states")[0])  # bit-exact x0
    gm = gx.sum(0).numpy()
    gv = (gx * T(k("eps0")) / (2.0 * torch.sqrt(T(k("x0_var"))).reshape(1, -1))).sum(0).numpy()
    es, ei = relerr(st.numpy(), k("states")), relerr(inp.numpy(), k("inputs"))
    ep, ed, em, ev = relerr(gkp.numpy(), k("g_sqrt_kp")), relerr(gkd.numpy(), k("g_sqrt_kd")), relerr(gm, k("g_x0_mean")), relerr(gv, k("g_x0_var"))
    print("%s: states %.3e inputs %.3e g_sqrt_kp %.3e g_sqrt_kd %.3e g_x0_mean %.3e g_x0_var %.3e (min var %.3e)" % (kind, es, ei, ep, ed, em, ev, vmin))
    assert vmin > 0
    assert es < 1e-10 and ei < 1e-10
    assert ep < 1e-10 and ed < 1e-10 and em < 1e-10 and ev < 1e-10
    assert k("states").shape == (6, 6, 4) and k("inputs").shape == (6, 6, 2) and k("pos_noise").shape == (5, 6, 2)
    assert float(np.abs(k("g_sqrt_kp")).max()) > 0 and float(k("butter_a")[1]) != 0.0
    # the measurement itself: row 0 is the true state, the measured positions are the true ones plus std * noise
    assert torch.equal(ym[0], st[0])
    pos = [int(i) for i in k("pos_indeces")]
    assert relerr((ym[1:, :, pos] - st[1:, :, pos]).numpy(), k("std_meas_noise")[pos] * k("pos_noise")) < 1e-12


@pytest.mark.parametrize("kind", ["speed", "delta"])
def test_gradients_against_central_differences(golden, kind):
    """Step 1e-6, bound 1e-5 relative with floor 1e-3 (tests/test_gpu_pd_rollout.py::test_philox_mode_against_central_differences)."""
    fx = golden("rollout_pd_pms")
    k, x0, args, (_, _, _, gkp, gkd, gx, _) = fixture_run(fx, kind)
    h = 1e-6

    def fd(which, idx):
        a = [t.clone() if isinstance(t, torch.Tensor) else t for t in args]
        b = [t.clone() if isinstance(t, torch.Tensor) else t for t in args]
        a[which][idx] += h
        b[which][idx] -= h
        return (loss_of(*a, u_max=float(k("u_max"))) - loss_of(*b, u_max=float(k("u_max")))) / (2 * h)

    for name, which, idx, g in (("sqrt_kp[1]", 3, (1,), gkp[1]), ("sqrt_kd[0]", 4, (0,), gkd[0]), ("x0[2,0]", 2, (2, 0), gx[2, 0]),
                                ("x0[4,3]", 2, (4, 3), gx[4, 3])):
        d, g = fd(which, idx), float(g)
        print("%s %s: fd %.9e autograd %.9e" % (kind, name, d, g))
        assert abs(d - g) < 1e-5 * max(abs(g), 1e-3)


@pytest.mark.parametrize("defect", ["no_b1", "no_a1", "row0_filtered", "swap_columns"])
def test_fixture_tells_the_measurement_from_its_near_misses(golden, defect):
    """On the truth alone: a dropped b1 term, a dropped -a1 term, row 0 treated like the other rows and swapped columns of the position
    noise each move the inputs and a gain gradient of the speed fixture by many orders of magnitude more than the pin's 1e-10."""
    fx = golden("rollout_pd_pms")
    k, _, _, (st, inp, _, gkp, gkd, _, _) = fixture_run(fx, "speed", defect=defect)
    ei, eg = relerr(inp.numpy(), k("inputs")), max(relerr(gkp.numpy(), k("g_sqrt_kp")), relerr(gkd.numpy(), k("g_sqrt_kd")))
    print("%s: inputs %.3e gain gradients %.3e" % (defect, ei, eg))
    assert ei > 1e-6 and eg > 1e-6


def _valid_descriptors():
    """A model, a PD descriptor and a measurement model that pass every host-side check (their device pointers are never followed)."""
    from mc_pilco_amd import hipabi
    from test_pd_rollout_cpu import _valid_descriptors as base

    m, p = base()
    m.Ts = 0.05
    ms = hipabi.Meas()
    ms.n = 2
    for i in range(2):
        ms.pos[i], ms.vel[i], ms.std_pos[i] = i, 2 + i, 0.1
    ms.b0, ms.b1, ms.a0, ms.a1 = 0.4, 0.3, 1.2, -0.4
    ms.meas = 0x1000
    return m, p, ms


def test_library_exports_and_argument_checks_without_gpu():
    """Every refusal comes back before a launch (no GPU here), with the status word -- host memory in this test -- untouched."""
    from mc_pilco_amd import hipabi

    lib = hipabi.lib()
    assert "mcp_rollout_pd_meas" in hipabi.EXPORTED and "mcp_rollout_pd_meas_bwd" in hipabi.EXPORTED
    assert hipabi.ABI_VERSION == lib.mcp_abi_version() == 7
    ARG = -1
    n = hipabi.Noise()
    one = C.c_void_p(0x1000)
    status = (C.c_uint32 * 1)(0xABCD)
    ref = lambda o: None if o is None else C.byref(o)
    fwd = lambda m_, p_, s_: lib.mcp_rollout_pd_meas(ref(m_), ref(p_), ref(s_), C.byref(n), 4, 8, 1, one, one, one, None, None, None,
                                                     C.cast(status, C.c_void_p), None)
    bwd = lambda m_, p_, s_, want=None: lib.mcp_rollout_pd_meas_bwd(ref(m_), ref(p_), ref(s_), 4, 8, one, one, one, one, None, want, None, None)
    m, p, ms = _valid_descriptors()
    assert bwd(m, p, ms) == 0  # every check passes and nothing is asked for: no launch
    ms0 = hipabi.Meas()
    assert bwd(m, p, ms0) == 0  # n == 0: mcp_rollout_pd_bwd's checks alone (a zeroed filter is no error there)
    m0 = _valid_descriptors()[0]
    m0.Ts = 0.0
    assert bwd(m0, p, ms0) == 0  # Ts <= 0 passes every check of the model: with pairs it is the measurement's own check that refuses it

    def broken(edit):
        m2, p2, s2 = _valid_descriptors()
        edit(m2, s2)
        return m2, p2, s2

    cases = {
        "meas NULL": lambda: _valid_descriptors()[:2] + (None,),
        "pos out of range": lambda: broken(lambda m2, s2: s2.pos.__setitem__(0, 4)),
        "vel negative": lambda: broken(lambda m2, s2: s2.vel.__setitem__(1, -1)),
        "pos repeated": lambda: broken(lambda m2, s2: s2.pos.__setitem__(1, 0)),
        "vel repeated": lambda: broken(lambda m2, s2: s2.vel.__setitem__(1, 2)),
        "listed as both": lambda: broken(lambda m2, s2: s2.vel.__setitem__(1, 0)),
        "no meas buffer": lambda: broken(lambda m2, s2: setattr(s2, "meas", None)),
        "a0 == 0": lambda: broken(lambda m2, s2: setattr(s2, "a0", 0.0)),
        "a0 NaN": lambda: broken(lambda m2, s2: setattr(s2, "a0", float("nan"))),
        "Ts <= 0": lambda: broken(lambda m2, s2: setattr(m2, "Ts", 0.0)),
        "n negative": lambda: broken(lambda m2, s2: setattr(s2, "n", -1)),
        "more pairs than S / 2": lambda: broken(lambda m2, s2: setattr(s2, "n", 3)),
    }
    for name, make in cases.items():
        for call in (fwd, bwd):
            assert call(*make()) == ARG, name
    assert status[0] == 0xABCD
    # the checks of mcp_rollout_pd still apply
    m2, p2, s2 = _valid_descriptors()
    p2.pos[0] = 1
    assert fwd(m2, p2, s2) == ARG and bwd(m2, p2, s2) == ARG


def test_ops_refuses_cpu_tensors_and_a_missing_buffer():
    import types

    from mc_pilco_amd import ops
    from test_pd_rollout_cpu import _policy

    model = types.SimpleNamespace(S=4, U=2)
    ms = ops.MeasSpec(pos=[0, 1], vel=[2, 3], std_pos=[0.1, 0.1], b=[0.5, 0.5], a=[1.0, 0.0])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rollout_pd(model, _policy().packed(), None, torch.zeros(3, 4, dtype=DT), 4, meas=ms)
    with pytest.raises(RuntimeError, match="pos_noise"):  # a CPU noise buffer
        ops.MeasSpec(pos=[0], vel=[2], std_pos=[0.1], b=[0.5, 0.5], a=[1.0, 0.0], pos_noise=torch.zeros(3, 3, 1, dtype=DT)).fill(
            ops.abi.Meas(), 4, 3, torch.zeros(1))
