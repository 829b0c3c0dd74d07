"""CPU: what mcp_plan_rollout, mcp_mppi_update_ext and mcp_cem_update refuse, with which code, on the pattern of
tests/test_mppi_refusals_cpu.py (a refused call returns before any HIP call, so the library answers without a GPU; device pointers are dummy
non-NULL addresses that nothing reads); what ops.PackedPlanExt, ops.plan_rollout / mppi_update_ext / cem_update and policy_learning.mppi.plan
refuse on this side of the ABI.

Every expected code is written out: -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  The three entries keep the order of the two they extend -- NULL
pointers; sizes (-1; the CEM update: n_elite < 1 among them); limits (-2; the CEM update: n_elite > MCP_CEM_MAX_ELITE, n_elite > K); the
model (the rollout); values (-1; beta with them; the CEM update: alpha, sigma_min); the cost descriptors (the rollout) or the outputs'
aliasing (the updates); last, the rollout's LDS fit with the std's rows counted (-2).  Every entry launches whenever it accepts, so every call
here is a refusal: the rollout and the MPPI update are called under a non-default extension unless the refusal is one of mcp_mppi_rollout's /
mcp_mppi_update's own, which a default extension must return as well."""
import ctypes as C
import types

import pytest
import torch

from test_mppi_refusals_cpu import A_PTR, cin, cost, mppi
from test_open_refusals_cpu import PTR, abi, model

SIGS = {
    "plan_rollout": ("model", "mppi", "ext", "cost", "cin", "noise", "particle_pred", "x0", "traj_cost", "states", "inputs", "status"),
    "mppi_update_ext": ("mppi", "ext", "noise", "traj_cost", "a_new", "cand_cost", "weights", "stats", "status"),
    "cem_update": ("mppi", "ext", "noise", "traj_cost", "a_new", "sigma_new", "cand_cost", "elite", "stats", "status"),
}
REQUIRED = {"plan_rollout": ("model", "mppi", "cost", "noise", "x0", "traj_cost", "status"),
            "mppi_update_ext": ("mppi", "noise", "traj_cost", "a_new", "cand_cost", "weights", "stats", "status"),
            "cem_update": ("mppi", "ext", "noise", "traj_cost", "a_new", "sigma_new", "cand_cost", "elite", "stats", "status")}
OPTIONAL = ("cin", "states", "inputs")
ALL = tuple(SIGS)
S_PTR, OUT2 = 0x3000, 0x4000  # the std's rows; sigma_new (PTR stands for a_new among the rest)


def ext(**edit):
    """A valid, non-default extension: beta 0.5, 4 elites (of mppi()'s 8 candidates), alpha 0.1, floor 0.05."""
    e = abi().PlanExt()
    e.beta, e.alpha, e.n_elite = 0.5, 0.1, 4
    for k in range(abi().MAX_INPUT):
        e.sigma_min[k] = 0.05
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(e, k)[v[0]] = v[1]
        else:
            setattr(e, k, v)
    return e


def call(entry, **over):
    U = over.pop("U", 1)
    args = dict(model=model(U), mppi=mppi(U), ext=ext(), cost=cost(), noise=abi().Noise(), particle_pred=1, sigma_new=OUT2)
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
    return {e: call(e, **dict(over)) for e in ALL}


def every(code):
    return {e: code for e in ALL}


@pytest.mark.parametrize("entry", ALL)
def test_null_pointers(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
        if entry != "cem_update" and name != "mppi":  # a default extension, and none: the refusal of the entry underneath
            assert call(entry, **{name: None, "ext": abi().PlanExt()}) == -1 and call(entry, **{name: None, "ext": None}) == -1, name
    assert call(entry, mppi=mppi(a=None)) == -1


def test_sizes_and_limits_of_the_plan():
    for edit in (dict(K=0), dict(P=0), dict(H=1), dict(U=0), dict(t0=-1)):
        assert codes(mppi=mppi(**edit)) == every(-1), edit
        assert call("plan_rollout", mppi=mppi(**edit), ext=None) == -1 and call("mppi_update_ext", mppi=mppi(**edit), ext=abi().PlanExt()) == -1
    assert codes(mppi=mppi(U=abi().MAX_INPUT + 1)) == every(-2)
    assert codes(mppi=mppi(K=abi().MPPI_MAX_K + 1)) == every(-2)
    assert codes(mppi=mppi(K=1, P=abi().MPPI_MAX_M + 1), ext=ext(n_elite=1)) == every(-2)
    assert codes(mppi=mppi(H=20481)) == every(-2)
    for edit in (dict(S=17), dict(U=9), dict(G=9), dict(D=33), dict(gp_N=abi().MAX_TRAIN + 1)):
        assert call("plan_rollout", model=model(**edit)) == -2, edit
    assert call("plan_rollout", model=model(angle=(0, 9))) == -1 and call("plan_rollout", model=model(2)) == -1


def test_beta():
    for bad in (-1e-300, -0.5, 1.0, 1.5, float("inf"), float("nan")):
        assert codes(ext=ext(beta=bad)) == every(-1), bad
        assert call("plan_rollout", ext=ext(beta=bad, sigma_rows=S_PTR, u_prev=PTR)) == -1


def test_the_values_of_the_plan():
    for edit in (dict(lam=0.0), dict(lam=float("nan")), dict(sigma=(0, -0.5)), dict(sigma=(0, float("inf"))), dict(u_max=(0, 0.0)), dict(kappa=0.5, P=1),
                 dict(kappa=float("nan"))):
        assert codes(mppi=mppi(**edit)) == every(-1), edit
        assert codes(mppi=mppi(**edit), ext=ext(sigma_rows=S_PTR)) == every(-1), edit


def test_the_elites():
    for bad in (0, -1, -(2 ** 31)):
        assert call("cem_update", ext=ext(n_elite=bad)) == -1, bad
    assert call("cem_update", ext=ext(n_elite=9)) == -2  # more elites than the 8 candidates
    assert call("cem_update", mppi=mppi(K=2000), ext=ext(n_elite=abi().CEM_MAX_ELITE + 1)) == -2
    assert call("cem_update", mppi=mppi(K=abi().MPPI_MAX_K), ext=ext(n_elite=2 ** 31 - 1)) == -2
    # the rollout and the MPPI update do not read n_elite, alpha or sigma_min: with a bad one they are refused for something else alone
    for e in (ext(n_elite=0), ext(alpha=2.0), ext(sigma_min=(0, -1.0))):
        assert call("plan_rollout", ext=e, cost=cost(kind=7)) == -1 and call("mppi_update_ext", ext=e, a_new=A_PTR) == -1


def test_alpha_and_the_floor():
    for bad in (-1e-300, -0.5, 1.0, 2.0, float("inf"), float("nan")):
        assert call("cem_update", ext=ext(alpha=bad)) == -1, bad
    for bad in (-1e-300, -0.5, float("inf"), float("nan")):
        assert call("cem_update", ext=ext(sigma_min=(0, bad))) == -1, bad
        assert call("cem_update", U=2, ext=ext(sigma_min=(1, bad))) == -1, bad


def test_the_outputs_are_buffers_of_their_own():
    assert call("mppi_update_ext", a_new=A_PTR) == -1 and call("mppi_update_ext", a_new=A_PTR, ext=None) == -1
    assert call("mppi_update_ext", a_new=S_PTR, ext=ext(sigma_rows=S_PTR)) == -1
    for over in (dict(a_new=A_PTR), dict(sigma_new=A_PTR), dict(a_new=OUT2), dict(a_new=S_PTR, ext=ext(sigma_rows=S_PTR)),
                 dict(sigma_new=S_PTR, ext=ext(sigma_rows=S_PTR))):
        assert call("cem_update", **over) == -1, over


def test_the_cost_descriptors():
    for edit in (dict(kind=7), dict(S=3), dict(n_used=0), dict(target_traj=None)):
        assert call("plan_rollout", cost=cost(**edit)) == -1, edit
    for edit in (dict(U=2), dict(mode=2), dict(used=(0, 1))):
        assert call("plan_rollout", cin=cin(**edit)) == -1, edit


def test_the_std_rows_count_in_the_lds_fit():
    """H U = 10241 doubles of nominal fit beside this small model's operands, twice that (the std's rows) cannot: 20482 > 20480 doubles of
    LDS.  Both rungs of the sampled ladder and the mean form refuse; nothing is launched."""
    for e in (ext(), ext(beta=0.0, sigma_rows=S_PTR), ext(beta=0.0, u_prev=PTR)):
        assert call("plan_rollout", mppi=mppi(H=10241), ext=e) == -2
        assert call("plan_rollout", mppi=mppi(H=10241), ext=e, particle_pred=0) == -2
    assert call("plan_rollout", mppi=mppi(H=20480)) == -2


def test_precedence():
    assert codes(mppi=mppi(K=0, U=abi().MAX_INPUT + 1)) == every(-1)  # sizes before limits
    assert call("cem_update", mppi=mppi(K=abi().MPPI_MAX_K + 1), ext=ext(n_elite=0)) == -1  # n_elite < 1 is a size
    assert codes(mppi=mppi(K=abi().MPPI_MAX_K + 1), ext=ext(beta=2.0)) == every(-2)  # the plan's limits before beta
    assert call("cem_update", ext=ext(n_elite=9, alpha=2.0)) == -2 and call("cem_update", ext=ext(n_elite=9, beta=2.0)) == -2
    assert call("plan_rollout", model=model(S=17), ext=ext(beta=2.0)) == -2  # the model's limits before beta
    assert call("plan_rollout", mppi=mppi(H=10241), ext=ext(beta=2.0)) == -1  # beta before the fit
    assert call("plan_rollout", mppi=mppi(H=10241), cost=cost(kind=7)) == -1  # the cost before the fit


# ---- this side of the ABI -------------------------------------------------------------------------------------------------------------------
def test_packed_plan_ext_refuses_bad_host_values():
    from mc_pilco_amd import ops

    ok = dict(H=6, U=2)
    e = ops.PackedPlanExt(**ok)
    assert (e.beta, e.alpha, e.n_elite, e.sigma_min.tolist(), e.sigma_rows) == (0.0, 0.0, 1, [0.0, 0.0], None)
    rows = [[0.1, 0.2]] * 6
    assert ops.PackedPlanExt(sigma_rows=rows, beta=0.5, n_elite=4, alpha=0.3, sigma_min=[0.0, 0.1], **ok).sigma_rows.shape == (6, 2)
    bad_rows = [[0.1, 0.2]] * 5 + [[0.1, float("nan")]]
    for edit in (dict(H=1), dict(U=0), dict(U=9), dict(beta=-0.1), dict(beta=1.0), dict(beta=float("nan")), dict(alpha=1.0), dict(alpha=-0.1),
                 dict(alpha=float("nan")), dict(n_elite=0), dict(n_elite=ops.abi.CEM_MAX_ELITE + 1), dict(sigma_min=-0.1), dict(sigma_min=float("inf")),
                 dict(sigma_min=[0.1, 0.2, 0.3]), dict(sigma_rows=[[0.1, 0.2]] * 5), dict(sigma_rows=bad_rows), dict(sigma_rows=[[0.1, -0.2]] * 6),
                 dict(sigma_rows=[[0.1, float("inf")]] * 6)):
        with pytest.raises(ValueError):
            ops.PackedPlanExt(**dict(ok, **edit))


def _stub(device):
    return types.SimpleNamespace(S=4, U=2, G=2, D=8, device=torch.device(device), c=None)


def test_ops_refuse_wrong_operands():
    from mc_pilco_amd import ops

    mp = ops.PackedMPPI(K=8, P=2, H=6, U=2, sigma=0.3, lam=1.0)
    e = ops.PackedPlanExt(6, 2, beta=0.5, n_elite=4)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    pc = types.SimpleNamespace(kind="target", c=None)
    with pytest.raises(ValueError, match="made for"):
        ops.plan_rollout(_stub("cuda:0"), mp, ops.PackedPlanExt(7, 2), pc, z(4), z(6, 2))
    with pytest.raises(ValueError, match="sigma_rows must have the shape"):
        ops.plan_rollout(_stub("cuda:0"), mp, e, pc, z(4), z(6, 2), sigma_rows=z(5, 2))
    with pytest.raises(ValueError, match="u_prev must have the shape"):
        ops.plan_rollout(_stub("cuda:0"), mp, e, pc, z(4), z(6, 2), u_prev=z(3))
    with pytest.raises(ValueError, match="device"):
        ops.plan_rollout(_stub("cuda:0"), mp, None, pc, z(4), z(6, 2), u_prev=z(2))
    with pytest.raises(ValueError, match="device"):
        ops.mppi_update_ext(mp, e, z(16), z(6, 2))
    with pytest.raises(ValueError, match="shape"):
        ops.mppi_update_ext(mp, e, z(15), z(6, 2))
    with pytest.raises(ValueError, match="elites of"):
        ops.cem_update(mp, ops.PackedPlanExt(6, 2, n_elite=9), z(16), z(6, 2))
    with pytest.raises(ValueError, match="PackedPlanExt"):
        ops.cem_update(mp, None, z(16), z(6, 2))
    with pytest.raises(ValueError, match="device"):
        ops.cem_update(mp, e, z(16), z(6, 2))
    with pytest.raises(ValueError, match="traj_cost"):
        ops.cem_update(mp, e, [0.0] * 16, z(6, 2))


def test_plan_refuses_a_bad_method_and_bad_extension_values():
    from mc_pilco_amd.policy_learning import Cost_function as cf
    from mc_pilco_amd.policy_learning import mppi

    pm = types.SimpleNamespace(S=4, U=2, G=2, D=8, device=torch.device("cpu"))  # (every refusal comes before the model is looked at)
    cost_ = cf.Expected_saturated_distance([0.0, 0.0], [1.0, 1.0], [0, 1])
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    import mc_pilco_amd.policy_learning.mppi as mod

    keep = mod._packed_model
    mod._packed_model = lambda m: m
    try:
        for kw, msg in ((dict(method="softmax"), "method"), (dict(beta=1.0), "beta"), (dict(method="cem", alpha=1.0), "alpha"),
                        (dict(method="cem", n_elite=9), "elites"), (dict(method="cem", sigma_min=-1.0), "sigma_min"),
                        (dict(sigma_rows=[[0.1, -0.1]] * 6), "sigma_rows")):
            with pytest.raises(ValueError, match=msg):
                mppi.plan(pm, z(4), z(6, 2), cost_, K=8, **kw)
    finally:
        mod._packed_model = keep
