"""CPU: dropout in the tanh-MLP policy.  Policy.MLP_policy(flg_drop=True).forward against the law written out in tests/mlp_drop_models.py under a
fixed seed; the conditions that keep tests/test_gpu_mlp_drop.py from passing vacuously, on every case of its table; the exports; and what
mcp_rollout_mlp_drop / mcp_rollout_mlp_drop_bwd refuse, with which code (a refused call returns before any HIP call, so the library answers
without a GPU; device pointers are dummy non-NULL addresses that nothing reads, as in tests/test_mlp_refusals_cpu.py).

Every expected code is written out: 0 MCP_OK, -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  Order of the checks: NULL pointers, M / T and p_drop (-1), the
model's compiled limits (-2), the model (-1), the descriptor (its limits -2, then -1), the measurement model where there is one (-1), then,
the sweep only, "nothing asked for" (0, no launch)."""
import ctypes as C

import pytest
import torch

from mlp_drop_models import CASES, case_id, case_inputs, masks_mixed, mlp_law, truth_of
from mlp_models import SHAPES, network
from test_mlp_refusals_cpu import mlp_desc
from test_open_refusals_cpu import PTR, M, T, abi, model

DT = torch.float64
SIGS = {
    "mlp_drop": ("model", "mlp", "meas", "noise", "p_drop", "M", "T", "particle_pred", "x0", "states", "inputs", "mu", "var", "jac", "status"),
    "mlp_drop_bwd": ("model", "mlp", "meas", "noise", "p_drop", "M", "T", "states", "inputs", "jac", "g_states", "g_inputs", "g_params", "g_x0"),
}
REQUIRED = {"mlp_drop": ("model", "mlp", "noise", "x0", "states", "inputs", "status"), "mlp_drop_bwd": ("model", "mlp", "states", "inputs", "jac", "g_states")}
OPTIONAL = ("mu", "var", "g_inputs", "g_params", "g_x0")
BOTH = ("mlp_drop", "mlp_drop_bwd")


# ---- the class ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,p", [((5,), 0.25), ((7, 3), 0.5)])
def test_forward_matches_the_written_out_law(hidden, p):
    from mc_pilco_amd.policy_learning import Policy

    c = SHAPES["arm2"]
    params = network(c, hidden, c["angle"], c["not_angle"], 11)
    mk = lambda **kw: Policy.MLP_policy(state_dim=c["S"], input_dim=c["U"], hidden_sizes=list(hidden), angle_indices=c["angle"],
                                        non_angle_indices=c["not_angle"], u_max=1.3, weight_init=params, dtype=DT, device=torch.device("cpu"), **kw)
    pol = mk(flg_drop=True)
    H, Mx = sum(hidden), 9
    assert pol.flg_drop is True and pol.drop_width == H
    x = torch.randn(Mx, c["S"], dtype=DT, generator=torch.Generator().manual_seed(4))
    torch.manual_seed(123)
    got = pol(x, t=3, p_dropout=p).detach()
    torch.manual_seed(123)
    keep = torch.empty(Mx, 1, H, dtype=DT).bernoulli_(1 - p).reshape(Mx, H)  # the ONE draw of reference_draws' mask()
    ref = mlp_law(x, params, c["angle"], c["not_angle"], 1.3, True, keep, p)
    plain = mlp_law(x, params, c["angle"], c["not_angle"], 1.3, True)
    assert float((got - ref).abs().max()) < 1e-14
    assert float((got - plain).abs().max()) > 1e-3  # (the masks did something)
    assert bool(keep.min() == 0) and bool(keep.max() == 1)
    # one draw per call: the generator is where a second mask() of the same shape leaves it
    after = torch.get_rng_state()
    torch.manual_seed(123)
    torch.empty(Mx, 1, H, dtype=DT).bernoulli_(1 - p)
    assert torch.equal(after, torch.get_rng_state())
    # p_dropout = 0 draws nothing and is the plain law
    state = torch.get_rng_state()
    assert float((pol(x, t=0, p_dropout=0.0).detach() - plain).abs().max()) < 1e-14 and torch.equal(state, torch.get_rng_state())
    # the default construction ignores p_dropout, and draws nothing
    off = mk()
    assert off.flg_drop is False and off.drop_width == H
    assert float((off(x, t=0, p_dropout=p).detach() - plain).abs().max()) < 1e-14 and torch.equal(state, torch.get_rng_state())


# ---- the truth's conditioning ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_truth_is_conditioned(case):
    """On every case: the truth's variances stay positive; the mask buffer holds a kept and a dropped entry in every layer wider than one unit
    (and both values overall); states or inputs differ from the truth without dropout by more than 1e-3."""
    mode, shape, deg, N, T, Mc, hidden, p, opt = case
    c, m, ins = case_inputs(case)
    st, inp, grads, gx0, vmin = truth_of(m, ins)
    if T > 1:
        assert vmin > 0.0
    k = ins["masks"]
    assert tuple(k.shape) == (T, Mc, sum(hidden)) and k.dtype == torch.uint8 and masks_mixed(k, hidden)
    assert int(k.min()) == 0 and int(k.max()) == 1
    s0, i0, *_ = truth_of(m, ins, masks=None)
    d = max(float((st - s0).abs().max()), float((inp - i0).abs().max()))
    print("%s: min var %.3e, keep rate %.3f (mask seed %d), |dropout - none| %.3e" % (case_id(case), vmin, float(k.double().mean()), ins["mask_seed"], d))
    assert d > 1e-3
    assert bool(torch.isfinite(st).all()) and bool(torch.isfinite(inp).all()) and all(bool(torch.isfinite(g).all()) for g in grads + [gx0])
    assert all(float(g.abs().max()) > 0 for g in grads)  # (every tensor has a gradient to compare)


def test_the_table_covers_what_it_names():
    assert {c[4] for c in CASES} == {1, 2, 3, 12} and {1, 5, 17, 1041} <= {c[5] for c in CASES}
    assert {(1,), (5,), (7, 3), (33, 64), (64, 64)} == {c[6] for c in CASES} and {c[7] for c in CASES} == {0.25, 0.5}
    assert {"arm2", "arm2_delta", "ur5", "limits"} == {c[1] for c in CASES}
    assert sum("meas" in c[8] for c in CASES) == 2
    for key in ("squash", "no_g_inputs", "only_grad"):
        assert sum(key in c[8] for c in CASES) == 1


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def call(entry, **over):
    a = abi()
    args = dict(model=model(), mlp=mlp_desc(), meas=None, noise=a.Noise(), p_drop=0.25, M=M, T=T, particle_pred=1)
    args.update(over)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL or (name == "jac" and entry == "mlp_drop") else PTR)
    return getattr(a.lib(), "mcp_rollout_" + entry)(*vals, None)


def codes(**over):
    return {e: call(e, **over) for e in BOTH}


def both(code):
    return {e: code for e in BOTH}


def meas_desc(n=1, **edit):
    ms = abi().Meas()
    ms.n = n
    ms.pos[0], ms.vel[0], ms.std_pos[0] = 0, 2, 0.1
    ms.b0, ms.b1, ms.a0, ms.a1 = 0.42, 0.31, 1.25, -0.38
    ms.meas = PTR
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(ms, k)[v[0]] = v[1]
        else:
            setattr(ms, k, v)
    return ms


def test_exports():
    from test_abi_cpu import declared_symbols

    a = abi()
    assert "mcp_rollout_mlp_drop" in a.EXPORTED and "mcp_rollout_mlp_drop_bwd" in a.EXPORTED
    lib = a.lib()
    assert hasattr(lib, "mcp_rollout_mlp_drop") and hasattr(lib, "mcp_rollout_mlp_drop_bwd")
    assert lib.mcp_abi_version() == a.ABI_VERSION == 7  # the additions are additive
    assert set(declared_symbols()) == set(a.EXPORTED)  # the header and the binding stay the same set


def test_the_sweep_accepts_valid_arguments_with_nothing_asked_for():
    assert call("mlp_drop_bwd") == 0
    assert call("mlp_drop_bwd", p_drop=0.0) == 0
    assert call("mlp_drop_bwd", p_drop=0.0, noise=None) == 0  # without dropout the sweep needs no noise
    assert call("mlp_drop_bwd", mlp=mlp_desc(hidden=(64, 64)), p_drop=0.5) == 0
    assert call("mlp_drop_bwd", meas=meas_desc()) == 0
    assert call("mlp_drop_bwd", meas=meas_desc(n=0, meas=None)) == 0  # n == 0: the true state
    assert call("mlp_drop_bwd", T=1, jac=None) == 0
    assert call("mlp_drop_bwd", T=2, jac=None) == -1


def test_the_probability():
    for p in (-0.1, 1.0, float("nan"), 1.5, float("inf")):
        assert codes(p_drop=p) == both(-1), p
    assert call("mlp_drop_bwd", p_drop=0.999) == 0
    assert call("mlp_drop_bwd", p_drop=0.25, noise=None) == -1  # the sweep draws the forward's decisions again: it needs the noise
    assert call("mlp_drop_bwd", p_drop=1e-300, noise=None) == -1
    assert call("mlp_drop", p_drop=0.0, noise=None) == -1  # the forward entry needs it always, as mcp_rollout_mlp does


@pytest.mark.parametrize("entry", BOTH)
def test_null_pointers_and_sizes(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
    assert call(entry, M=0) == -1 and call(entry, T=0) == -1
    assert call(entry, mlp=mlp_desc(W=(0, None))) == -1


def test_the_measurement_model():
    assert codes(meas=meas_desc(pos=(0, 4))) == both(-1)  # out of range
    assert codes(meas=meas_desc(vel=(0, 0))) == both(-1)  # a component listed as both
    assert codes(meas=meas_desc(meas=None)) == both(-1)
    assert codes(meas=meas_desc(a0=0.0)) == both(-1)
    assert codes(meas=meas_desc(n=3)) == both(-1)  # 2 n > S


def test_precedence():
    assert codes(p_drop=1.0, model=model(S=17)) == both(-1)  # the probability is looked at with the sizes: before the limits
    assert codes(p_drop=-0.1, mlp=mlp_desc(hidden=(65,))) == both(-1)
    assert call("mlp_drop_bwd", noise=None, model=model(S=17)) == -1  # so is the sweep's missing noise
    assert codes(M=0, model=model(S=17)) == both(-1)  # sizes before limits
    assert codes(model=model(S=17, angle=(0, 9))) == both(-2)  # the model's limits before its lists
    assert codes(model=model(angle=(0, 9)), mlp=mlp_desc(U=9)) == both(-1)  # the model before the descriptor
    assert codes(mlp=mlp_desc(U=9, angle=(0, 4))) == both(-2)  # the descriptor's limits before its other errors
    assert codes(mlp=mlp_desc(hidden=(65,)), meas=meas_desc(a0=0.0)) == both(-2)  # the descriptor before the measurement model
    assert codes(mlp=mlp_desc(n_hidden=3), meas=meas_desc(a0=0.0)) == both(-1)
    assert codes(model=model(gp_N=4097, gp_Npad=4112)) == {"mlp_drop": -2, "mlp_drop_bwd": 0}  # the sweep never reads a GP descriptor
    assert call("mlp_drop_bwd", mlp=mlp_desc(u_max=(0, 0.0))) == -1  # a bad descriptor is refused even when nothing is asked for
