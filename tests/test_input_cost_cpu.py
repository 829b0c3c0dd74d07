"""CPU-only checks of the control-effort / input-rate cost terms (mcp_cost_inputs, mcp_cost_u_fwd / _bwd, ops.PackedCostInputs,
Cost_function.Input_penalty): the truth the GPU tests compare against feels every term, the hand gradient form the kernels implement is
autograd's, the ABI addition sits where the header puts it, the host-side checks refuse bad calls before any launch, and the class evaluates
its torch formula wherever the kernels do not apply."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import input_cost_models as icm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64
CASES = icm.gpu_cases()


# ---- the truth -----------------------------------------------------------------------------------------------------------------------------
def test_every_gpu_case_is_drawn_inside_the_margin_and_feels_every_term():
    """d_x + d_u + d_r <= 9 in every case, and the truth's cost moves by at least 1e-3 (relative) when the effort term is dropped, the rate
    term is dropped, u* is set to 0 or the mode is swapped (each where the case has that term): a kernel that ignores one cannot pass at
    1e-12."""
    assert len(CASES) == 5 * 2 * 2 * 3 + 4
    seen = set()
    for name, c in CASES:
        d = sum(icm.distances(c, icm._t(c["x"]), icm._t(c["u"])))
        assert float(d.max()) <= 9.0, name
        base = float(icm.truth(c)["cost"])
        for what, v in icm.variants(c):
            moved = abs(float(icm.truth(v)["cost"]) - base) / abs(base)
            assert moved >= 1e-3, "%s: %s moves the cost by %.2e only" % (name, what, moved)
            seen.add(what)
    assert seen == {"effort dropped", "rate dropped", "u* = 0", "mode swapped"}


@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_hand_gradient_form_is_autograds(name, c):
    """g_states = b_t d d_x/dx and g_inputs[t] = a_t (effort + rate into t) - a_{t+1} (rate into t + 1): within 1e-14 of each tensor's largest
    entry of what autograd gives for the torch formula (the T = 1 rate-only case has no input gradient at all: exactly zero)."""
    tr = icm.truth(c)
    gx, gu = icm.hand_gradients(c)
    for hand, auto in ((gx, tr["g_states"].numpy()), (gu, tr["g_inputs"].numpy())):
        top = np.abs(auto).max()
        if top == 0.0:
            assert np.abs(hand).max() == 0.0
        else:
            assert np.abs(hand - auto).max() <= 1e-14 * top


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_cost_inputs_layout_matches_the_header_and_the_abi_did_not_move(tmp_path):
    from mc_pilco_amd import hipabi

    names = [f[0] for f in hipabi.CostInputs._fields_]
    assert names == ["U", "mode", "n_used", "used", "target", "scales", "rate_scales"]
    src = tmp_path / "ci.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(){printf("%zu %zu %d %d %d", sizeof(mcp_cost_inputs),'
                   " sizeof(mcp_cost), MCP_COST_U_ADD, MCP_COST_U_JOINT, MCP_ABI_VERSION);"
                   + "".join('printf(" %%zu", offsetof(mcp_cost_inputs, %s));' % n for n in names) + "return 0;}\n")
    exe = tmp_path / "ci"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(hipabi.CostInputs), C.sizeof(hipabi.Cost), hipabi.COST_U_ADD, hipabi.COST_U_JOINT, hipabi.ABI_VERSION] \
        + [getattr(hipabi.CostInputs, n).offset for n in names]
    assert C.sizeof(hipabi.Cost) == 136 and C.sizeof(hipabi.CostInputs) == 12 + 4 * hipabi.MAX_INPUT + 4 + 24
    assert hipabi.lib().mcp_abi_version() == hipabi.ABI_VERSION == 7
    raw = C.CDLL(hipabi.LIB_PATH)
    for n in ("mcp_cost_u_fwd", "mcp_cost_u_bwd"):
        assert hasattr(raw, n) and n in hipabi.EXPORTED


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
P = C.c_void_p(8)  # (a non-null stand-in for buffers and arrays; the checks fail first, nothing dereferences it)


def _cost(kind=2, S=4, used=(0, 2)):
    from mc_pilco_amd import hipabi

    c = hipabi.Cost()
    c.kind, c.S, c.n_used = kind, S, len(used)
    for i, u in enumerate(used):
        c.used[i] = u
    c.target_traj, c.lengthscales = 8, 8
    return c


def _cin(U=3, used=(2, 0), mode=0, scales=8, rate=8, target=None):
    from mc_pilco_amd import hipabi

    c = hipabi.CostInputs()
    c.U, c.mode, c.n_used = U, mode, len(used)
    for i, u in enumerate(used):
        c.used[i] = u
    c.scales, c.rate_scales, c.target = scales, rate, target
    return c


def _fwd(c, ci, states=P, inputs=P, costs=P, moments=P, status=P):
    from mc_pilco_amd import hipabi

    return hipabi.lib().mcp_cost_u_fwd(None if c is None else C.byref(c), None if ci is None else C.byref(ci), 3, 4, states, inputs, costs,
                                       moments, status, None)


def _bwd(c, ci, states=P, inputs=P, g_states=P, g_inputs=P):
    from mc_pilco_amd import hipabi

    return hipabi.lib().mcp_cost_u_bwd(None if c is None else C.byref(c), None if ci is None else C.byref(ci), 3, 4, states, inputs, None,
                                       0.25, g_states, g_inputs, None)


def test_bad_calls_are_refused_on_the_host():
    """Every call here has at least one defect and must return MCP_ERR_ARG from the host-side checks: none may reach a launch."""
    from mc_pilco_amd import hipabi

    good, gin = _cost(), _cin()
    # the cost descriptor comes first
    for bad_cost in (None, _cost(used=()), _cost(used=(0, 4)), _cost(kind=7)):
        assert _fwd(bad_cost, gin) == -1 and _bwd(bad_cost, gin) == -1
    # then the inputs descriptor
    too_many = _cin(U=8, used=tuple(range(8)))
    too_many.n_used = hipabi.MAX_INPUT + 1
    negative = _cin()
    negative.n_used = -1
    for bad in (_cin(U=0), _cin(U=hipabi.MAX_INPUT + 1), too_many, negative, _cin(used=(0, 3)), _cin(used=(-1,)), _cin(used=(1, 1)),
                _cin(used=(0, 2, 0)), _cin(mode=2), _cin(mode=-1)):
        assert _fwd(good, bad) == -1 and _bwd(good, bad) == -1
    # a bad descriptor is refused even where it switches no term on
    assert _fwd(good, _cin(U=0, used=())) == -1 and _bwd(good, _cin(mode=2, scales=None, rate=None)) == -1
    # null buffers with valid descriptors
    for kw in (dict(states=None), dict(inputs=None), dict(costs=None), dict(moments=None), dict(status=None)):
        assert _fwd(good, gin, **kw) == -1
    for kw in (dict(states=None), dict(inputs=None), dict(g_states=None)):
        assert _bwd(good, gin, **kw) == -1
    # without a descriptor the width of g_inputs is unknown: it cannot be given
    assert _bwd(good, None, inputs=None) == -1
    assert hipabi.ERRORS[-1] == "MCP_ERR_ARG"


def test_descriptors_without_input_terms_do_not_need_the_inputs():
    """NULL descriptor, n_used == 0 or both scale pointers NULL: the entries take the path of mcp_cost_fwd / mcp_cost_bwd, and `inputs` may be
    NULL.  The descriptor checks do not refuse these calls -- with a device they run (on real buffers); without one the launch itself is what
    fails (MCP_ERR_LAUNCH), which is past every host-side check."""
    from mc_pilco_amd import hipabi

    none = [None, _cin(used=()), _cin(scales=None, rate=None)]
    if not torch.cuda.is_available():
        for ci in none:
            assert _fwd(_cost(), ci, inputs=None) == -4
            assert _bwd(_cost(), ci, inputs=None, g_inputs=None) == -4
        return
    dev = torch.device("cuda", 0)
    tg, ls = torch.zeros(2, dtype=D, device=dev), torch.ones(2, dtype=D, device=dev)
    cost = _cost()
    cost.target_traj, cost.lengthscales = tg.data_ptr(), ls.data_ptr()
    x = torch.zeros(3, 4, 4, dtype=D, device=dev)
    costs, mom, g = torch.empty(3, 4, dtype=D, device=dev), torch.empty(3, 2, dtype=D, device=dev), torch.empty_like(x)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    p = hipabi.ptr
    for ci in none:
        assert _fwd(cost, ci, states=p(x), inputs=None, costs=p(costs), moments=p(mom), status=p(status)) == 0
        assert _bwd(cost, ci, states=p(x), inputs=None, g_states=p(g), g_inputs=None) == 0
    torch.cuda.synchronize()


# ---- ops.PackedCostInputs --------------------------------------------------------------------------------------------------------------------
def test_packed_cost_inputs_refuses_inconsistent_descriptors():
    """Counts that disagree, indices out of range or repeated, a scale that is not finite and > 0, both scale arrays None: ValueError from the
    host values alone (no device is touched before the checks)."""
    from mc_pilco_amd import ops

    ok = dict(input_indices=[2, 0], lengthscales=[1.5, 0.7], rate_lengthscales=[0.5, 2.0], target_input=[0.1, -0.2])
    for change in (dict(lengthscales=[1.5]), dict(rate_lengthscales=[0.5, 2.0, 1.0]), dict(target_input=[0.1]), dict(input_indices=[0, 1, 2]),
                   dict(input_indices=[0, 3]), dict(input_indices=[-1, 0]), dict(input_indices=[1, 1]),
                   dict(input_indices=[], lengthscales=[], rate_lengthscales=[], target_input=[]),
                   dict(lengthscales=[1.5, 0.0]), dict(lengthscales=[1.5, -0.7]), dict(lengthscales=[float("nan"), 0.7]),
                   dict(rate_lengthscales=[float("inf"), 2.0]), dict(rate_lengthscales=torch.tensor([0.5, -2.0], dtype=D)),
                   dict(lengthscales=None, rate_lengthscales=None)):
        for joint in (False, True):
            with pytest.raises(ValueError):
                ops.PackedCostInputs(3, "cuda:0", joint=joint, **dict(ok, **change))
    for U in (0, 9):
        with pytest.raises(ValueError):
            ops.PackedCostInputs(U, "cuda:0", lengthscales=[1.0] * U)
    with pytest.raises(ValueError):  # (no indices given: every input, so the counts must be U)
        ops.PackedCostInputs(3, "cuda:0", lengthscales=[1.0, 2.0])


# ---- Cost_function.Input_penalty ---------------------------------------------------------------------------------------------------------------
def _state_costs():
    from mc_pilco_amd.policy_learning import Cost_function as CF

    tt = torch.randn(3, 4, dtype=D, generator=torch.Generator().manual_seed(5))
    return [CF.Cart_pole_cost([3.0, 0.1], [3.0, 1.0], 2, 0),
            CF.Expected_saturated_distance_from_trajectory(tt, [1.5, 0.7], used_indeces=[1, 3]),
            CF.Expected_distance(torch.tensor([[0.3, -0.2]], dtype=D), torch.tensor([1.5, 0.7], dtype=D), [0, 2]),
            CF.Expected_saturated_distance(torch.tensor([[0.3, -0.2]], dtype=D), torch.tensor([1.5, 0.7], dtype=D), [0, 2])]


def test_input_distance_is_the_difference_form():
    from mc_pilco_amd.policy_learning import Cost_function as CF

    u = torch.randn(4, 3, 3, dtype=D, generator=torch.Generator().manual_seed(2))
    d_u, d_r = CF.input_distance(u, [1.5, 0.7], [0.5, 2.0], [0.1, -0.2], [2, 0])
    c = dict(kind="quad", joint=False, used_x=[0], tg=np.zeros(1), ls=np.ones(1), used_u=[2, 0], l=np.array([1.5, 0.7]), r=np.array([0.5, 2.0]),
             ustar=np.array([0.1, -0.2]))
    _, tu, tr = icm.distances(c, torch.zeros(4, 3, 1, dtype=D), u)
    assert d_u.shape == d_r.shape == (4, 3) and torch.equal(d_u, tu) and torch.equal(d_r, tr) and float(d_r[0].abs().sum()) == 0.0
    z_u, _ = CF.input_distance(u, None, [0.5, 2.0, 1.0])
    _, z_r = CF.input_distance(u, [0.5, 2.0, 1.0], None)
    assert float(z_u.abs().sum()) == 0.0 and float(z_r.abs().sum()) == 0.0


@pytest.mark.parametrize("joint", [False, True])
def test_input_penalty_on_cpu_tensors_is_expected_cost_of_its_formula(joint):
    """On CPU tensors every instance evaluates its torch formula -- bit for bit what Expected_cost(cf.cost_function) gives: cost, std, both
    gradients, and the sharded form (local_moments / from_sums) -- and the formula is the truth's."""
    from mc_pilco_amd.policy_learning import Cost_function as CF

    g = torch.Generator().manual_seed(3)
    st, u = torch.randn(3, 5, 4, dtype=D, generator=g), torch.randn(3, 5, 3, dtype=D, generator=g)
    for sc in _state_costs():
        cf = CF.Input_penalty(sc, lengthscales=[1.5, 0.7], rate_lengthscales=[0.5, 2.0], target_input=[0.1, -0.2], input_indices=[2, 0], joint=joint)
        assert isinstance(cf, CF._HipExpectedCost) and cf.runs_on_kernels() and not cf.runs_on_kernels(st)
        x, v = st.clone().requires_grad_(True), u.clone().requires_grad_(True)
        c, s = cf(x, v, 0)
        c.backward()
        y, w = st.clone().requires_grad_(True), u.clone().requires_grad_(True)
        c0, s0 = CF.Expected_cost(cf.cost_function)(y, w, 0)
        c0.backward()
        assert torch.equal(c, c0) and torch.equal(s, s0) and torch.equal(x.grad, y.grad) and torch.equal(v.grad, w.grad) and cf._packed is None
        assert float(v.grad[:, :, 1].abs().sum()) == 0.0 and bool((v.grad[:, :, [0, 2]] != 0).all())
        share, sums = cf.local_moments(st, u, 0, 5)
        share0, sums0 = CF.Expected_cost(cf.cost_function).local_moments(st, u, 0, 5)
        assert torch.equal(share, share0) and torch.equal(sums, sums0)
        for a, b in zip(cf.from_sums(sums, 5), CF.Expected_cost.from_sums(sums0, 5)):
            assert torch.equal(a, b)
    # the formula against the truth's own (target kinds: the same difference form; 1e-14 covers the order of the additions)
    for kind, cls in (("quad", CF.Expected_distance), ("sat", CF.Expected_saturated_distance)):
        case = dict(kind=kind, joint=joint, x=st.numpy(), u=u.numpy(), used_x=[0, 2], tg=np.array([0.3, -0.2]), ls=np.array([1.5, 0.7]),
                    used_u=[2, 0], l=np.array([1.5, 0.7]), r=np.array([0.5, 2.0]), ustar=np.array([0.1, -0.2]))
        cf = CF.Input_penalty(cls(torch.tensor([[0.3, -0.2]], dtype=D), torch.tensor([1.5, 0.7], dtype=D), [0, 2]), lengthscales=[1.5, 0.7],
                              rate_lengthscales=[0.5, 2.0], target_input=[0.1, -0.2], input_indices=[2, 0], joint=joint)
        ref = icm.costs_of(case, st, u)
        assert float((cf.cost_function(st, u, 0) - ref).abs().max()) <= 1e-14 * float(ref.abs().max())


def test_input_penalty_keeps_the_torch_path_where_the_kernels_do_not_apply():
    from mc_pilco_amd.policy_learning import Cost_function as CF

    sc = _state_costs()
    ls = torch.tensor([1.5, 0.7, 1.0], dtype=D)
    assert CF.Input_penalty(sc[0], lengthscales=ls).runs_on_kernels()
    assert not CF.Input_penalty(sc[0], lengthscales=ls.clone().requires_grad_(True)).runs_on_kernels()
    assert not CF.Input_penalty(sc[0], rate_lengthscales=ls.clone().requires_grad_(True)).runs_on_kernels()
    two_rows = CF.Expected_saturated_distance(torch.tensor([[0.3, -0.2], [0.1, 0.4]], dtype=D), torch.tensor([1.5, 0.7], dtype=D), [0, 2])
    assert not two_rows.runs_on_kernels() and not CF.Input_penalty(two_rows, lengthscales=ls).runs_on_kernels()
    with pytest.raises(ValueError):
        CF.Input_penalty(sc[0])
    with pytest.raises(TypeError):
        CF.Input_penalty(CF.Expected_cost(lambda x, u, k: x.sum(2)), lengthscales=ls)
    # trainable scales: the torch path differentiates them
    tr = ls.clone().requires_grad_(True)
    cf = CF.Input_penalty(sc[3], lengthscales=tr)
    g = torch.Generator().manual_seed(4)
    c, _ = cf(torch.randn(3, 5, 4, dtype=D, generator=g), torch.randn(3, 5, 3, dtype=D, generator=g), 0)
    c.backward()
    assert tr.grad is not None and bool((tr.grad != 0).all())
