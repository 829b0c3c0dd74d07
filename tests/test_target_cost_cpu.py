"""CPU-only checks of the target-state cost kinds (MCP_COST_TARGET / MCP_COST_TARGET_QUAD): the ABI did not move, the library's host-side
validation rejects bad descriptors before any launch, and ops.PackedCost("target") refuses inconsistent descriptors before it touches a device."""
import ctypes as C
import os
import re

import pytest
import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcpilco_hip.h")


def _cost(kind, S=4, used=(0, 2), target=8, ls=8):
    """A descriptor that passes validation as it stands (the pointers are never followed on the host: any non-null value serves)."""
    from mc_pilco_amd import hipabi

    c = hipabi.Cost()
    c.kind, c.S, c.n_used = kind, S, len(used)
    for i, u in enumerate(used):
        c.used[i] = u
    c.target_traj, c.lengthscales = target, ls
    return c


def test_abi_version_and_struct_did_not_move():
    from mc_pilco_amd import hipabi

    assert hipabi.lib().mcp_abi_version() == hipabi.ABI_VERSION == 7
    hdr = open(HEADER).read()
    assert int(re.search(r"#define MCP_COST_TARGET (\d+)", hdr).group(1)) == hipabi.COST_TARGET == 2
    assert int(re.search(r"#define MCP_COST_TARGET_QUAD (\d+)", hdr).group(1)) == hipabi.COST_TARGET_QUAD == 3
    # kind, S, 2 indices | 4 doubles | n_used + 16 indices (+ 4 bytes of padding) | 2 pointers: the layout of ABI 7
    assert C.sizeof(hipabi.Cost) == 16 + 32 + 4 + 64 + 4 + 16 == 136
    assert hipabi.Cost.target_traj.offset == 120 and hipabi.Cost.lengthscales.offset == 128


@pytest.mark.parametrize("kind", [2, 3])
def test_bad_target_descriptors_are_rejected_on_the_host(kind):
    """Every call here must return MCP_ERR_ARG from the host-side checks: each has at least one defect, so none may reach a launch."""
    from mc_pilco_amd import hipabi

    lib = hipabi.lib()
    p = C.c_void_p(8)  # (a non-null stand-in for the buffers; validation fails first, nothing dereferences it)

    def fwd(c, states=p, costs=p, moments=p, status=p):
        return lib.mcp_cost_fwd(C.byref(c), 3, 4, states, costs, moments, status, None)

    def bwd(c, states=p, g_states=p):
        return lib.mcp_cost_bwd(C.byref(c), 3, 4, states, None, 0.25, g_states, None)

    good = _cost(kind)
    # null buffers with an otherwise valid descriptor
    for kw in (dict(states=None), dict(costs=None), dict(moments=None), dict(status=None)):
        assert fwd(good, **kw) == -1
    for kw in (dict(states=None), dict(g_states=None)):
        assert bwd(good, **kw) == -1
    assert lib.mcp_cost_fwd(None, 3, 4, p, p, p, p, None) == -1 and lib.mcp_cost_bwd(None, 3, 4, p, None, 0.25, p, None) == -1
    # bad descriptors with valid-looking buffers
    bad = [_cost(kind, used=()), _cost(kind, S=4, used=(0, 4)), _cost(kind, used=(-1,)), _cost(kind, ls=None), _cost(kind, target=None)]
    too_many = _cost(kind, S=16, used=tuple(range(16)))
    too_many.n_used = 17
    bad.append(too_many)
    for c in bad:
        assert fwd(c) == -1 and bwd(c) == -1
    assert hipabi.ERRORS[-1] == "MCP_ERR_ARG"


def test_packed_target_cost_refuses_inconsistent_descriptors():
    """Mismatched counts and indices outside [0, S) raise ValueError from the host values alone (no device is touched before the checks)."""
    from mc_pilco_amd import ops

    ok = dict(target_state=[[0.3, -0.2]], lengthscales=[1.5, 0.7], active_dims=[0, 2])
    for change in (dict(lengthscales=[1.5, 0.7, 2.0]), dict(target_state=[[0.3, -0.2, 1.0]]), dict(active_dims=[0, 1, 2]),
                   dict(target_state=torch.zeros(2, 2, dtype=torch.float64)),  # two target rows are not one row
                   dict(active_dims=[0, 4]), dict(active_dims=[-1, 0]),
                   dict(active_dims=[], target_state=[], lengthscales=[])):
        for saturate in (True, False):
            with pytest.raises(ValueError):
                ops.PackedCost("target", 4, "cuda:0", saturate=saturate, **dict(ok, **change))
    with pytest.raises(ValueError):
        ops.PackedCost("target", 17, "cuda:0", target_state=[0.0] * 17, lengthscales=[1.0] * 17, active_dims=list(range(17)))


def test_classes_choose_their_path_per_instance_and_per_call():
    """One target row: a candidate for the kernels; several rows, a slice or trainable lengthscales: the torch path, and on CPU tensors every
    instance evaluates the torch formula -- bit for bit what Expected_cost(cost_function) gives."""
    from mc_pilco_amd.policy_learning import Cost_function as CF

    D = torch.float64
    st = torch.randn(3, 2, 4, dtype=D, generator=torch.Generator().manual_seed(3))
    ls = torch.tensor([1.5, 0.7], dtype=D)
    for cls, f in ((CF.Expected_distance, CF.distance_from_target), (CF.Expected_saturated_distance, CF.saturated_distance_from_target)):
        one = cls(torch.tensor([[0.3, -0.2]], dtype=D), ls, [0, 2])
        flat = cls(torch.tensor([0.3, -0.2], dtype=D), ls, [0, 2])
        two = cls(torch.tensor([[0.3, -0.2], [0.1, 0.4]], dtype=D), ls, [0, 2])
        sl = cls(torch.tensor([[0.3, -0.2]], dtype=D), ls, slice(0, 2))
        tr = cls(torch.tensor([[0.3, -0.2]], dtype=D), ls.clone().requires_grad_(True), [0, 2])
        assert isinstance(one, CF.Expected_cost) and isinstance(one, CF._HipExpectedCost)
        assert one.runs_on_kernels() and flat.runs_on_kernels()
        assert not two.runs_on_kernels() and not sl.runs_on_kernels() and not tr.runs_on_kernels()
        for cf in (one, flat, two, sl, tr):
            assert not cf.runs_on_kernels(st)  # CPU states
            x = st.clone().requires_grad_(True)
            c, s = cf(x, None, 0)
            c.backward()
            y = st.clone().requires_grad_(True)
            c0, s0 = CF.Expected_cost(cf.cost_function)(y, None, 0)
            c0.backward()
            assert torch.equal(c, c0) and torch.equal(s, s0) and torch.equal(x.grad, y.grad) and cf._packed is None
        ref = f(st, None, 0, torch.tensor([[0.3, -0.2]], dtype=D), ls, [0, 2])
        assert torch.equal(one.cost_function(st, None, 0), ref)
        # the sharded form on CPU tensors stays the torch one as well
        share, sums = one.local_moments(st, None, 0, 2)
        share0, sums0 = CF.Expected_cost(one.cost_function).local_moments(st, None, 0, 2)
        assert torch.equal(share, share0) and torch.equal(sums, sums0)
        for a, b in zip(one.from_sums(sums, 2), CF.Expected_cost.from_sums(sums0, 2)):
            assert torch.equal(a, b)
    assert CF.Cart_pole_cost([3.14, 0.0], [3.0, 1.0], 2, 0).runs_on_kernels()
