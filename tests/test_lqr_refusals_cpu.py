"""CPU: what mcp_linearize and mcp_lqr_pass refuse, with which code, on the pattern of tests/test_tvl_refusals_cpu.py (a refused call
returns before any HIP call, so the library answers without a GPU; device pointers are dummy non-NULL addresses that nothing reads); what
ops.linearize / ops.lqr_pass refuse with ValueError; and Quadratic_tracking_cost.expansion against torch autograd.

Every expected code is written out: 0 MCP_OK, -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  Order of the checks: NULL pointers, M / T and reg (-1),
the compiled limits (-2), the model's scalars and index lists (-1), then -- mcp_linearize only -- "nothing asked for" (0, no launch).
mcp_lqr_pass launches whenever it accepts, so every call of it here is a refusal."""
import ctypes as C
import types

import pytest
import torch

from test_open_refusals_cpu import PTR, REPEATED_INDEX, M, T, abi, model

SIGS = {
    "linearize": ("model", "M", "T", "states", "jac", "du_da", "A", "B"),
    "lqr_pass": ("model", "M", "T", "states", "jac", "du_da", "lx", "lu", "hxx", "huu", "reg", "gain", "kff", "dv", "status"),
}
REQUIRED = {"linearize": ("model", "states", "jac"), "lqr_pass": ("model", "states", "jac", "lx", "lu", "hxx", "huu", "gain", "kff", "dv", "status")}
OPTIONAL = ("du_da", "A", "B")
BOTH = ("linearize", "lqr_pass")


def call(entry, **over):
    args = dict(model=model(), M=M, T=T, reg=0.0)
    args.update(over)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL else PTR)
    return getattr(abi().lib(), "mcp_" + entry)(*vals, None)


def codes(**over):
    return {e: call(e, **over) for e in BOTH}


def both(code):
    return {e: code for e in BOTH}


def test_linearize_accepts_valid_arguments_with_nothing_asked_for():
    assert call("linearize") == 0
    assert call("linearize", du_da=PTR) == 0
    assert call("linearize", model=model(2)) == 0
    assert call("linearize", T=2, M=1) == 0
    assert call("linearize", T=abi().LQR_MAX_T) == 0
    assert call("linearize", model=model(gp_Kinv=None, gp_N=0)) == 0  # no GP operand is looked at: the entries run from the record


@pytest.mark.parametrize("entry", BOTH)
def test_null_pointers_and_sizes(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
    assert call(entry, M=0) == -1 and call(entry, M=-3) == -1
    assert call(entry, T=1) == -1 and call(entry, T=0) == -1 and call(entry, T=-2) == -1


def test_reg():
    for bad in (-1e-300, -1.0, float("inf"), float("-inf"), float("nan")):
        assert call("lqr_pass", reg=bad) == -1, bad


def test_limits_and_the_model():
    assert codes(model=model(S=17)) == both(-2)
    assert codes(model=model(U=9)) == both(-2)
    assert codes(model=model(G=9)) == both(-2)
    assert codes(model=model(D=33)) == both(-2)
    assert codes(T=abi().LQR_MAX_T + 1) == both(-2)
    assert codes(model=model(angle=(0, 9))) == both(-1)  # an index outside the state
    assert codes(model=model(not_angle=(1, -1))) == both(-1)
    assert codes(model=model(vel=(0, 4))) == both(-1)
    assert codes(model=model(not_vel=(1, -2))) == both(-1)
    assert codes(model=model(D=7)) == both(-1)  # D != n_not_angle + 2 n_angle + U
    assert codes(model=model(S=0)) == both(-1) and codes(model=model(G=0)) == both(-1) and codes(model=model(U=0)) == both(-1)


@pytest.mark.parametrize("edit", REPEATED_INDEX, ids=str)
def test_an_index_listed_twice(edit):
    """The model's lists name a component once per role (tests/test_open_refusals_cpu.py): linearize refuses with nothing asked for."""
    assert codes(model=model(**edit)) == both(-1)


def test_precedence():
    assert codes(M=0, model=model(S=17)) == both(-1)  # sizes before limits
    assert call("lqr_pass", reg=-1.0, model=model(S=17)) == -1  # reg is looked at with the sizes
    assert codes(T=abi().LQR_MAX_T + 1, model=model(angle=(0, 9))) == both(-2)  # limits before the model
    assert call("linearize", model=model(angle=(0, 9))) == -1  # a bad model is refused even when nothing is asked for


# ---- ops ------------------------------------------------------------------------------------------------------------------------------------
def _stub(device):
    return types.SimpleNamespace(S=4, U=2, G=2, D=8, device=torch.device(device), c=None)


def _operands(Tn=3, Mn=2, dtype=torch.float64):
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    return dict(states=z(Tn, Mn, 4), jac=z(Tn - 1, Mn, 2, 8), lx=z(Tn, Mn, 4), lu=z(Tn, Mn, 2), hxx=z(Tn, Mn, 4), huu=z(Tn, Mn, 2))


def test_ops_refuse_wrong_dtype_shape_and_device():
    """On this side of the ABI: ValueError, before anything is launched (CPU tensors are the wrong device)."""
    from mc_pilco_amd import ops

    mdl, o = _stub("cuda:0"), _operands()
    with pytest.raises(ValueError, match="device"):
        ops.linearize(mdl, o["states"], o["jac"])
    with pytest.raises(ValueError, match="device"):
        ops.lqr_pass(mdl, **o)
    with pytest.raises(ValueError, match="float64"):
        ops.linearize(mdl, o["states"].float(), o["jac"])
    with pytest.raises(ValueError, match="float64"):
        ops.lqr_pass(mdl, **dict(o, jac=o["jac"].float()))
    with pytest.raises(ValueError, match="shape"):
        ops.linearize(mdl, o["states"], o["jac"][:, :, :, :7])
    with pytest.raises(ValueError, match="shape"):
        ops.linearize(mdl, o["states"], o["jac"], du_da=torch.zeros(3, 2, 3, dtype=torch.float64))
    for name in ("lx", "lu", "hxx", "huu"):
        with pytest.raises(ValueError, match="%s must have the shape" % name):
            ops.lqr_pass(mdl, **dict(o, **{name: o[name][:2]}))
        with pytest.raises(ValueError, match="%s must be a float64" % name):
            ops.lqr_pass(mdl, **dict(o, **{name: o[name].double().float()}))
    with pytest.raises(ValueError, match="T >= 2"):
        ops.linearize(mdl, o["states"][:1], o["jac"][:0])
    with pytest.raises(ValueError, match="T >= 2"):
        ops.linearize(mdl, o["states"][0], o["jac"])
    with pytest.raises(ValueError, match="states"):
        ops.linearize(mdl, o["states"].numpy(), o["jac"])


# ---- the cost's expansion ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("squash", [True, False])
@pytest.mark.parametrize("variant", ["all", "subset", "no_inputs"])
def test_expansion_against_autograd(squash, variant):
    """T = 3, M = 2 on CPU tensors: J against the formula written out, lx / lu against autograd's gradient, hxx / huu against the diagonal of
    the Gauss-Newton Hessian -- J^T J of the residual vector r = [(x - x*) / l, (u - u*) / r] with respect to (x, a), by autograd."""
    from mc_pilco_amd.policy_learning.ilqr import Quadratic_tracking_cost

    gen = torch.Generator().manual_seed(4)
    Tn, Mn, S, U = 3, 2, 4, 2
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=gen)
    target, x, a = rnd(Tn + 1, S), rnd(Tn, Mn, S), rnd(Tn, Mn, U)
    u_max = [0.7, 1.6]
    idx = [0, 1, 2, 3] if variant != "subset" else [3, 1]
    ls = 0.5 + torch.rand(len(idx), dtype=torch.float64, generator=gen)
    r = None if variant == "no_inputs" else 0.5 + torch.rand(U, dtype=torch.float64, generator=gen)
    ut = None if variant == "no_inputs" else rnd(U)
    cost = Quadratic_tracking_cost(target, ls, state_indices=None if variant == "all" else idx, input_lengthscales=r, target_input=ut)
    J, lx, lu, hxx, huu, du_da = cost.expansion(x, a, u_max, squash)
    um = torch.tensor(u_max, dtype=torch.float64)

    def residuals(xv, av):
        uv = um * torch.tanh(av / um) if squash else av
        parts = [((xv[:, :, idx] - target[:Tn, idx].unsqueeze(1)) / ls).reshape(-1)]
        if r is not None:
            parts.append(((uv - ut) / r).reshape(-1))
        return torch.cat(parts)

    xg, ag = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    res = residuals(xg, ag)
    total = 0.5 * (res * res).sum()
    gx, ga = torch.autograd.grad(total, [xg, ag], allow_unused=True)
    ga = torch.zeros_like(a) if ga is None else ga
    Jx, Ja = torch.autograd.functional.jacobian(residuals, (x, a))
    gn_x, gn_a = (Jx * Jx).sum(0), (Ja * Ja).sum(0)
    per_m = 0.5 * ((x[:, :, idx] - target[:Tn, idx].unsqueeze(1)) / ls).pow(2).sum((0, 2))
    if r is not None:
        per_m = per_m + 0.5 * (((um * torch.tanh(a / um) if squash else a) - ut) / r).pow(2).sum((0, 2))
    close = lambda p, q: float((p - q).abs().max()) <= 1e-13 * max(1.0, float(q.abs().max()))
    assert close(J, per_m) and close(J.sum(), total.detach())
    assert close(lx, gx) and close(lu, ga) and close(hxx, gn_x) and close(huu, gn_a)
    s = 1.0 - torch.tanh(a / um) ** 2 if squash else torch.ones_like(a)
    assert close(du_da, s)
    assert all(t.is_contiguous() and t.dtype == torch.float64 for t in (lx, lu, hxx, huu, du_da))


def test_expansion_refuses_a_short_target():
    from mc_pilco_amd.policy_learning.ilqr import Quadratic_tracking_cost

    cost = Quadratic_tracking_cost(torch.zeros(2, 4), torch.ones(4))
    with pytest.raises(ValueError):
        cost.expansion(torch.zeros(3, 1, 4, dtype=torch.float64), torch.zeros(3, 1, 2, dtype=torch.float64))
