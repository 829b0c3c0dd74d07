"""CPU: the boundary of the fused model step (mcp_model_step, mcp_model_step_bwd): the library exports both and the binding lists them,
the ABI version stays 7, and what the two entries refuse, with which code.  A refused call returns before any HIP call, so the library
answers without a GPU (the style of tests/test_open_refusals_cpu.py, whose valid descriptor is used here); device pointers are dummy
non-NULL addresses that nothing reads.  Every expected code is written out: 0 MCP_OK, -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  The forward
entry launches whenever it accepts, so every forward call below is a refusal; the sweep is always called with no gradient asked for."""
import ctypes as C

import pytest
from test_open_refusals_cpu import PTR, REPEATED_INDEX, abi, model

M = 5
FWD = ("model", "noise", "M", "t", "particle_pred", "x", "u", "x_next", "mean", "var", "jac", "status")
BWD = ("model", "M", "x", "jac", "g_next", "g_x", "g_u")
FWD_REQUIRED = ("model", "noise", "x", "u", "x_next", "status")
BWD_REQUIRED = ("model", "x", "jac", "g_next")
OPTIONAL = ("mean", "var", "g_x", "g_u")  # NULL by default; the forward call's jac too ("no record")


def call(entry, **over):
    a = abi()
    args = dict(model=model(), noise=a.Noise(), M=M, t=0, particle_pred=1)
    args.update(over)
    vals = []
    for name in (FWD if entry == "step" else BWD):
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL or (name == "jac" and entry == "step") else PTR)
    return getattr(a.lib(), "mcp_model_step" if entry == "step" else "mcp_model_step_bwd")(*vals, None)


def both(**over):
    return call("step", **over), call("bwd", **over)


def test_symbols_and_version():
    a = abi()
    lib = a.lib()
    assert lib.mcp_abi_version() == 7 and a.ABI_VERSION == 7
    for name in ("mcp_model_step", "mcp_model_step_bwd"):
        assert hasattr(lib, name)
        assert name in a.EXPORTED and name not in a.EXPORTED_DEBUG


def test_the_sweep_with_nothing_asked_for_is_ok_without_a_launch():
    assert call("bwd") == 0
    assert call("bwd", model=model(not_vel=(0, -1))) == 0  # a delta-state GP


def test_null_pointers():
    for name in FWD_REQUIRED:
        assert call("step", **{name: None}) == -1, name
    for name in BWD_REQUIRED:
        assert call("bwd", **{name: None}) == -1, name


def test_sizes():
    assert both(M=0) == (-1, -1)
    assert both(M=-3) == (-1, -1)
    assert call("step", t=-1) == -1


def test_compiled_limits():
    a = abi()
    assert both(model=model(G=a.MAX_GP + 1)) == (-2, -2)
    assert both(model=model(D=a.MAX_GPDIM + 1)) == (-2, -2)
    assert both(model=model(S=a.MAX_STATE + 1)) == (-2, -2)
    assert both(model=model(U=a.MAX_INPUT + 1)) == (-2, -2)
    # more training points than MCP_MAX_TRAIN: the forward entry refuses; the sweep never reads a GP descriptor
    assert both(model=model(gp_N=4097, gp_Npad=4112)) == (-2, 0)


def test_precedence():
    assert both(M=0, model=model(S=17)) == (-1, -1)  # sizes before limits
    assert both(model=model(S=17, angle=(0, 9))) == (-2, -2)  # limits before the model's lists


@pytest.mark.parametrize("edit", [dict(angle=(0, 9)), dict(angle=(0, -1)), dict(not_angle=(0, 4)), dict(vel=(0, 4)), dict(vel=(1, -1)),
                                  dict(not_vel=(0, -2)), dict(not_vel=(1, 4)), dict(n_not_angle=2), dict(n_angle=-1), dict(S=0), dict(G=0)] + REPEATED_INDEX,
                         ids=str)
def test_broken_index_lists(edit):
    """Refused by both entries -- by the sweep even though nothing is asked for."""
    assert both(model=model(**edit)) == (-1, -1)


@pytest.mark.parametrize("edit", [dict(gp_Kinv=None), dict(gp_Xt=None), dict(gp_alpha=None), dict(kern_inv_ls=None), dict(gp_Npad=40), dict(gp_N=0),
                                  dict(kern_poly_deg=3), dict(kern_poly_deg=1), dict(kern_D=5)], ids=str)
def test_gp_operand_errors_are_the_forward_entry_alone(edit):
    assert both(model=model(**edit)) == (-1, 0)


def test_fused_next_state_refuses_a_model_that_overrides_its_step():
    """No GPU is touched: the refusal comes before the model is packed."""
    import torch

    from mc_pilco_amd.model_learning import Model_learning as ML

    class Mine(ML.Speed_Model_learning_RBF_angle_state):
        def get_next_state(self, current_state, current_input, particle_pred=True):
            return super().get_next_state(current_state, current_input, particle_pred)

    for cls, ok in ((ML.Speed_Model_learning_RBF_angle_state, True), (Mine, False)):
        ml = cls.__new__(cls)  # (the predicate looks at the class alone)
        assert ml.steps_like_the_packed_model() is ok
    with pytest.raises(NotImplementedError, match="get_next_state"):
        Mine.__new__(Mine).fused_next_state(torch.zeros(1, 4), torch.zeros(1, 1))
