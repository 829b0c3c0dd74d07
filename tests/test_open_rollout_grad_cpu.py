"""CPU-only checks of the differentiable open-loop rollout's boundary: the recording entry point and the reverse sweep are declared, bound
and exported by the cross-compiled library; both refuse bad arguments on the host with the documented codes before any launch; the operator
refuses CPU tensors; the oracle side of the GPU parity cases keeps every sampled variance positive (the seeds are checked here first)."""
import ctypes as C
import inspect
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_new_symbols_are_declared_and_exported():
    from mc_pilco_amd import build, hipabi

    lib = hipabi.lib()
    header = open(os.path.join(os.path.dirname(HERE), "include", "mcpilco_hip.h")).read()
    for name in ("mcp_rollout_open_rec", "mcp_rollout_open_bwd"):
        assert hasattr(lib, name)
        assert name in hipabi.EXPORTED and name not in hipabi.EXPORTED_DEBUG
        assert "int %s(" % name in header
    assert "rollout_open.hip" in build.SOURCES
    assert lib.mcp_abi_version() == 7  # purely additive


def _model(S=4, U=1, G=2, D=6):
    from mc_pilco_amd import hipabi

    m = hipabi.Model()
    m.S, m.U, m.G, m.D = S, U, G, D
    m.n_angle, m.n_not_angle = 1, 3
    m.angle[0] = 2
    m.not_angle[0], m.not_angle[1], m.not_angle[2] = 0, 1, 3
    m.vel[0], m.vel[1], m.not_vel[0], m.not_vel[1] = 1, 3, 0, 2
    return m


def test_recording_entry_validates_on_the_host():
    from mc_pilco_amd import hipabi

    lib = hipabi.lib()
    ARG, LIMIT = -1, -2
    n = hipabi.Noise()
    p = C.c_void_p(64)  # never dereferenced: every call below is refused on the host
    call = lambda model, noise, M, T, x0, u, Mu, states, jac, status: lib.mcp_rollout_open_rec(model, noise, M, T, 0, x0, u, Mu, None, states, None,
                                                                                               None, jac, status, None)
    m = _model()
    ok = (C.byref(m), C.byref(n), 4, 3, p, p, 4, p, p, p)
    for i in (0, 1, 4, 5, 7, 8, 9):  # model, noise, x0, u, states, jac, status
        args = list(ok)
        args[i] = None
        assert call(*args) == ARG, i
    assert call(C.byref(m), C.byref(n), 0, 3, p, p, 1, p, p, p) == ARG  # M < 1
    assert call(C.byref(m), C.byref(n), 4, 1, p, p, 4, p, p, p) == ARG  # T < 2
    assert call(C.byref(m), C.byref(n), 4, 3, p, p, 2, p, p, p) == ARG  # Mu not in {1, M}
    assert call(C.byref(_model(G=hipabi.MAX_GP + 1)), C.byref(n), 4, 3, p, p, 4, p, p, p) == LIMIT
    assert call(C.byref(_model(D=hipabi.MAX_GPDIM + 1)), C.byref(n), 4, 3, p, p, 4, p, p, p) == LIMIT
    assert call(C.byref(_model(S=hipabi.MAX_STATE + 1)), C.byref(n), 4, 3, p, p, 4, p, p, p) == LIMIT
    big = _model()
    big.gp[0].N = hipabi.MAX_TRAIN + 1
    assert call(C.byref(big), C.byref(n), 4, 3, p, p, 4, p, p, p) == LIMIT
    assert call(C.byref(m), C.byref(n), 4, 3, p, p, 4, p, p, p) == ARG  # no GP operands: refused, nothing launched


def test_reverse_sweep_validates_on_the_host():
    from mc_pilco_amd import hipabi

    lib = hipabi.lib()
    ARG, LIMIT = -1, -2
    p = C.c_void_p(64)
    call = lambda model, M, T, states, jac, g_states, g_x0, g_u: lib.mcp_rollout_open_bwd(model, M, T, states, None, jac, g_states, g_x0, g_u, None)
    m = _model()
    assert call(C.byref(m), 4, 3, p, p, None, p, p) == ARG  # NULL g_states
    assert call(None, 4, 3, p, p, p, p, p) == ARG
    assert call(C.byref(m), 4, 3, None, p, p, p, p) == ARG
    assert call(C.byref(m), 4, 3, p, None, p, p, p) == ARG
    assert call(C.byref(m), 0, 3, p, p, p, p, p) == ARG  # M < 1
    assert call(C.byref(m), 4, 1, p, p, p, p, p) == ARG  # T < 2
    assert call(C.byref(_model(G=hipabi.MAX_GP + 1)), 4, 3, p, p, p, p, p) == LIMIT
    assert call(C.byref(_model(D=hipabi.MAX_GPDIM + 1)), 4, 3, p, p, p, p, p) == LIMIT
    assert call(C.byref(_model(S=hipabi.MAX_STATE + 1)), 4, 3, p, p, p, p, p) == LIMIT
    assert call(C.byref(_model(U=hipabi.MAX_INPUT + 1)), 4, 3, p, p, p, p, p) == LIMIT
    assert call(C.byref(_model(D=7)), 4, 3, p, p, p, p, p) == ARG  # the feature map does not add up to D
    bad = _model()
    bad.vel[1] = 9
    assert call(C.byref(bad), 4, 3, p, p, p, p, p) == ARG
    assert call(C.byref(m), 4, 3, p, p, p, None, None) == 0  # nothing asked for: nothing launched


def test_operator_and_class_surface():
    import torch

    from mc_pilco_amd import ops
    from mc_pilco_amd.model_learning import Model_learning as ML

    x0, u = torch.zeros(3, 4, dtype=torch.float64, requires_grad=True), torch.zeros(5, 3, 1, dtype=torch.float64, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rollout_open_diff(None, x0, u)
    sig = inspect.signature(ML.Model_learning.open_loop_rollout).parameters
    assert list(sig)[-1] == "differentiable" and sig["differentiable"].default is False
    assert list(sig)[:7] == ["self", "initial_states", "inputs", "particle_pred", "lengths", "noise", "moments"]


def test_oracle_variances_stay_positive_on_the_parity_cases():
    """The sampled GPU cases assert status == 0; the oracle alone must already keep every variance positive on their seeds."""
    import torch

    from open_grad_models import CASES, build_pair, inputs_for, oracle_truth

    torch.set_num_threads(1)
    for (mode, shape, deg, N, T, M, vs) in CASES:
        if mode != "sampled" or N > 48:
            continue  # (the N = 300 cases check the same on the GPU test's own oracle run)
        c, m, _ = build_pair(shape, N, deg, seed=N + deg)
        x0, u, eps, w = inputs_for(c, M, T, seed=T * 100 + M)
        _, gx, gu, vmin = oracle_truth(shape, m, x0, u, eps, w, True, var_scale=vs)
        assert vmin > 0.0 and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gu).all()), (mode, shape, deg, N, T, M)
