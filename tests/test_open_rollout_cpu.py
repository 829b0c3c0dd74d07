"""CPU-only checks of the open-loop rollout's boundary: the library exports mcp_rollout_open and the binding lists it, the host-side
validation refuses bad arguments with the documented codes before any launch, and the class surface has the new entry points."""
import ctypes as C
import inspect

import pytest


def test_library_exports_the_open_loop_rollout():
    from mc_pilco_amd import build, hipabi

    lib = hipabi.lib()
    assert hasattr(lib, "mcp_rollout_open")
    assert "mcp_rollout_open" in hipabi.EXPORTED and "mcp_rollout_open" not in hipabi.EXPORTED_DEBUG
    assert "rollout_open.hip" in build.SOURCES
    assert lib.mcp_abi_version() == 7  # purely additive


def _model(S=4, U=1, G=2, D=6):
    from mc_pilco_amd import hipabi

    m = hipabi.Model()
    m.S, m.U, m.G, m.D = S, U, G, D
    m.n_angle, m.n_not_angle = 1, 3
    return m


def test_argument_validation_without_gpu():
    from mc_pilco_amd import hipabi

    lib = hipabi.lib()
    ARG, LIMIT = -1, -2
    n = hipabi.Noise()
    p = C.c_void_p(64)  # never dereferenced: every call below is refused on the host
    call = lambda model, noise, M, T, x0, u, Mu, states, status: lib.mcp_rollout_open(model, noise, M, T, 0, x0, u, Mu, None, states, None, None,
                                                                                      status, None)
    m = _model()
    ok = (C.byref(m), C.byref(n), 4, 3, p, p, 4, p, p)
    for i in (0, 1, 4, 5, 7, 8):  # model, noise, x0, u, states, status
        args = list(ok)
        args[i] = None
        assert call(*args) == ARG, i
    assert call(C.byref(m), C.byref(n), 0, 3, p, p, 1, p, p) == ARG  # M <= 0
    assert call(C.byref(m), C.byref(n), -2, 3, p, p, 1, p, p) == ARG
    assert call(C.byref(m), C.byref(n), 4, 1, p, p, 4, p, p) == ARG  # T < 2
    assert call(C.byref(m), C.byref(n), 4, 3, p, p, 2, p, p) == ARG  # Mu not in {1, M}
    assert call(C.byref(m), C.byref(n), 4, 3, p, p, 0, p, p) == ARG
    assert call(C.byref(_model(G=hipabi.MAX_GP + 1)), C.byref(n), 4, 3, p, p, 4, p, p) == LIMIT
    assert call(C.byref(_model(D=hipabi.MAX_GPDIM + 1)), C.byref(n), 4, 3, p, p, 4, p, p) == LIMIT
    assert call(C.byref(_model(S=hipabi.MAX_STATE + 1)), C.byref(n), 4, 3, p, p, 4, p, p) == LIMIT
    big = _model()
    big.gp[0].N = hipabi.MAX_TRAIN + 1
    assert call(C.byref(big), C.byref(n), 4, 3, p, p, 4, p, p) == LIMIT
    # an empty descriptor inside the limits (no GP operands) is a bad argument, and nothing was launched
    assert call(C.byref(m), C.byref(n), 4, 3, p, p, 4, p, p) == ARG


def test_class_surface():
    from mc_pilco_amd.model_learning import Model_learning as ML
    from mc_pilco_amd.policy_learning import MC_PILCO

    assert list(inspect.signature(MC_PILCO.MC_PILCO.rollout).parameters) == ["self", "data_collection_index", "T_rollout", "particle_pred"]
    sig = inspect.signature(MC_PILCO.MC_PILCO.rollout_ensemble).parameters
    assert list(sig) == ["self", "data_collection_index", "num_particles", "T_rollout", "seed"]
    assert sig["data_collection_index"].default is None
    assert MC_PILCO.MC_PILCO4PMS.rollout is MC_PILCO.MC_PILCO.rollout
    assert MC_PILCO.MC_PILCO4PMS.rollout_ensemble is MC_PILCO.MC_PILCO.rollout_ensemble
    assert callable(ML.Model_learning.open_loop_rollout)


def test_operator_refuses_cpu_tensors_and_gradients():
    import torch

    from mc_pilco_amd import ops

    x0, u = torch.zeros(3, 4, dtype=torch.float64), torch.zeros(5, 3, 1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rollout_open(None, x0, u)
