"""CPU: what mcp_mppi_rollout and mcp_mppi_update refuse, with which code, on the pattern of tests/test_lqr_refusals_cpu.py (a refused call
returns before any HIP call, so the library answers without a GPU; device pointers are dummy non-NULL addresses that nothing reads); what
ops.PackedMPPI / ops.mppi_rollout / ops.mppi_update and policy_learning.mppi refuse on this side of the ABI.

Every expected code is written out: -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  Order of the checks: NULL pointers; the plan's sizes (-1: K, P < 1,
H < 2, U < 1, t0 < 0, no nominal); the plan's limits (-2: U, K, K P); -- the rollout only -- the model's limits (-2), the model (-1), U
against the model (-1); the plan's values (-1: lambda, kappa, sigma, u_max); the cost descriptors (the rollout) or a_new == a (the update).
Both entries launch whenever they accept, so every call here is a refusal."""
import ctypes as C
import types

import pytest
import torch

from test_open_refusals_cpu import PTR, REPEATED_INDEX, abi, model

SIGS = {
    "mppi_rollout": ("model", "mppi", "cost", "cin", "noise", "particle_pred", "x0", "traj_cost", "states", "inputs", "status"),
    "mppi_update": ("mppi", "noise", "traj_cost", "a_new", "cand_cost", "weights", "stats", "status"),
}
REQUIRED = {"mppi_rollout": ("model", "mppi", "cost", "noise", "x0", "traj_cost", "status"),
            "mppi_update": ("mppi", "noise", "traj_cost", "a_new", "cand_cost", "weights", "stats", "status")}
OPTIONAL = ("cin", "states", "inputs")
BOTH = ("mppi_rollout", "mppi_update")
A_PTR = 0x2000  # the nominal: another address than PTR, which stands for a_new among the rest


def mppi(U=1, **edit):
    """A valid plan over model(U): K 8, P 2, H 6, squashed at 1, sigma 0.3, lambda 1."""
    p = abi().MPPI()
    p.K, p.P, p.H, p.U, p.squash, p.lam, p.kappa, p.t0, p.a = 8, 2, 6, U, 1, 1.0, 0.0, 0, A_PTR
    for k in range(abi().MAX_INPUT):
        p.u_max[k], p.sigma[k] = 1.0, 0.3
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def cost(**edit):
    """A valid target cost over the four state components of model()."""
    c = abi().Cost()
    c.kind, c.S, c.n_used, c.target_traj, c.lengthscales = abi().COST_TARGET, 4, 2, PTR, PTR
    c.used[0], c.used[1] = 0, 2
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


def cin(U=1, **edit):
    c = abi().CostInputs()
    c.U, c.mode, c.n_used, c.scales = U, abi().COST_U_ADD, 1, PTR
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


def call(entry, **over):
    U = over.pop("U", 1)
    args = dict(model=model(U), mppi=mppi(U), cost=cost(), noise=abi().Noise(), particle_pred=1)
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
    return {e: call(e, **dict(over)) for e in BOTH}


def both(code):
    return {e: code for e in BOTH}


@pytest.mark.parametrize("entry", BOTH)
def test_null_pointers(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
    assert call(entry, mppi=mppi(a=None)) == -1


def test_sizes():
    for edit in (dict(K=0), dict(K=-2), dict(P=0), dict(P=-1), dict(H=1), dict(H=0), dict(H=-3), dict(U=0), dict(t0=-1)):
        assert codes(mppi=mppi(**edit)) == both(-1), edit


def test_limits():
    assert codes(mppi=mppi(U=abi().MAX_INPUT + 1)) == both(-2)
    assert codes(mppi=mppi(K=abi().MPPI_MAX_K + 1)) == both(-2)
    assert codes(mppi=mppi(K=abi().MPPI_MAX_K, P=abi().MPPI_MAX_M // abi().MPPI_MAX_K + 1)) == both(-2)  # K P beyond the index arithmetic
    assert codes(mppi=mppi(K=1, P=abi().MPPI_MAX_M + 1)) == both(-2)
    assert codes(mppi=mppi(H=20481)) == both(-2) and codes(mppi=mppi(H=2 ** 31 - 1)) == both(-2)  # the nominal's H U doubles alone exceed the LDS
    assert codes(U=2, mppi=mppi(2, H=10241)) == both(-2)
    for edit in (dict(S=17), dict(U=9), dict(G=9), dict(D=33), dict(gp_N=abi().MAX_TRAIN + 1)):
        assert call("mppi_rollout", model=model(**edit)) == -2, edit


def test_the_model():
    assert call("mppi_rollout", model=model(angle=(0, 9))) == -1  # an index outside the state
    assert call("mppi_rollout", model=model(D=7)) == -1  # D != n_not_angle + 2 n_angle + U
    assert call("mppi_rollout", model=model(gp_Kinv=None)) == -1  # model_ok looks at the GP operands (the mean form is no exception)
    assert call("mppi_rollout", model=model(gp_Npad=20)) == -1
    assert call("mppi_rollout", model=model(2)) == -1  # U != model->U
    assert call("mppi_rollout", mppi=mppi(2)) == -1


@pytest.mark.parametrize("edit", REPEATED_INDEX, ids=str)
def test_an_index_listed_twice(edit):
    assert call("mppi_rollout", model=model(**edit)) == -1


def test_values():
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert codes(mppi=mppi(lam=bad)) == both(-1), bad
    for bad in (-1e-300, -0.5, float("inf"), float("nan")):
        assert codes(mppi=mppi(sigma=(0, bad))) == both(-1), bad
    for bad in (0.0, -1.0, float("nan")):
        assert codes(mppi=mppi(u_max=(0, bad))) == both(-1), bad
    assert codes(mppi=mppi(kappa=0.5, P=1)) == both(-1)  # the std of one particle
    assert codes(mppi=mppi(kappa=float("nan"))) == both(-1) and codes(mppi=mppi(kappa=float("inf"))) == both(-1)
    assert call("mppi_update", a_new=A_PTR) == -1  # a_new == a


def test_the_cost_descriptors():
    for edit in (dict(kind=7), dict(S=0), dict(S=17), dict(S=3), dict(n_used=0), dict(n_used=17), dict(used=(1, 4)), dict(used=(0, -1)),
                 dict(target_traj=None), dict(lengthscales=None)):
        assert call("mppi_rollout", cost=cost(**edit)) == -1, edit
    assert call("mppi_rollout", cost=cost(kind=abi().COST_CARTPOLE, angle_index=4)) == -1
    for edit in (dict(U=2), dict(U=0), dict(mode=2), dict(n_used=9), dict(used=(0, 1)), dict(used=(0, -1))):
        assert call("mppi_rollout", cin=cin(**edit)) == -1, edit
    assert call("mppi_rollout", U=2, cin=cin(2, n_used=2, used=(1, 0))) == -1  # an input index listed twice


def test_precedence():
    assert codes(mppi=mppi(K=0, U=abi().MAX_INPUT + 1)) == both(-1)  # sizes before limits
    assert codes(mppi=mppi(K=abi().MPPI_MAX_K + 1, lam=-1.0)) == both(-2)  # the plan's limits before its values
    assert call("mppi_rollout", mppi=mppi(K=abi().MPPI_MAX_K + 1), model=model(angle=(0, 9))) == -2  # limits before the model
    assert call("mppi_rollout", mppi=mppi(K=0), model=model(S=17)) == -1  # the plan's sizes before the model's limits
    assert call("mppi_rollout", model=model(S=17), mppi=mppi(lam=0.0)) == -2  # the model's limits before the plan's values
    assert call("mppi_rollout", mppi=mppi(lam=0.0), cost=cost(kind=7)) == -1


# ---- this side of the ABI -------------------------------------------------------------------------------------------------------------------
def test_packed_mppi_refuses_bad_host_values():
    from mc_pilco_amd import ops

    ok = dict(K=8, P=2, H=6, U=2, sigma=0.3, lam=1.0)
    mp = ops.PackedMPPI(**ok)
    assert (mp.M, mp.sigma.tolist(), mp.u_max.tolist(), mp.squash) == (16, [0.3, 0.3], [1.0, 1.0], True)
    for edit in (dict(K=0), dict(P=0), dict(H=1), dict(U=0), dict(U=9), dict(K=ops.abi.MPPI_MAX_K + 1), dict(sigma=-0.1), dict(sigma=[0.1, float("nan")]),
                 dict(sigma=[0.1, 0.2, 0.3]), dict(lam=0.0), dict(lam=float("inf")), dict(kappa=float("nan")), dict(kappa=0.5, P=1), dict(u_max=0.0),
                 dict(u_max=[1.0, -1.0])):
        with pytest.raises(ValueError):
            ops.PackedMPPI(**dict(ok, **edit))
    assert ops.PackedMPPI(**dict(ok, u_max=0.0, squash=False)).squash is False  # (the bound is not looked at without squashing)


def _stub(device):
    return types.SimpleNamespace(S=4, U=2, G=2, D=8, device=torch.device(device), c=None)


def test_ops_refuse_wrong_dtype_shape_and_device():
    from mc_pilco_amd import ops

    mp = ops.PackedMPPI(K=8, P=2, H=6, U=2, sigma=0.3, lam=1.0)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    pc = types.SimpleNamespace(kind="target", c=None)
    with pytest.raises(ValueError, match="device"):
        ops.mppi_rollout(_stub("cuda:0"), mp, pc, z(4), z(6, 2))
    with pytest.raises(ValueError, match="shape"):
        ops.mppi_rollout(_stub("cuda:0"), mp, pc, z(4), z(5, 2))
    with pytest.raises(ValueError, match="float64"):
        ops.mppi_rollout(_stub("cuda:0"), mp, pc, z(4), z(6, 2).float())
    with pytest.raises(ValueError, match="xi must have the shape"):
        ops.mppi_rollout(_stub("cuda:0"), mp, pc, z(4), z(6, 2), xi=z(6, 7, 2))
    with pytest.raises(ValueError, match="inputs"):
        ops.mppi_rollout(types.SimpleNamespace(S=4, U=1, device=torch.device("cuda:0")), mp, pc, z(4), z(6, 2))
    with pytest.raises(ValueError, match="device"):
        ops.mppi_update(mp, z(16), z(6, 2))
    with pytest.raises(ValueError, match="shape"):
        ops.mppi_update(mp, z(15), z(6, 2))
    with pytest.raises(ValueError, match="traj_cost"):
        ops.mppi_update(mp, [0.0] * 16, z(6, 2))


def test_plan_refuses_costs_the_kernels_do_not_evaluate():
    from mc_pilco_amd.policy_learning import Cost_function as cf
    from mc_pilco_amd.policy_learning import mppi

    dev = torch.device("cuda:0")
    generic = cf.Expected_cost(lambda x, u, k: (x * x).sum(2))
    with pytest.raises(NotImplementedError):
        mppi.kernel_cost(generic, 4, 2, 6, dev)
    many = cf.Expected_saturated_distance(torch.zeros(3, 2), torch.ones(2), [0, 1])  # three target rows: the torch path
    with pytest.raises(NotImplementedError):
        mppi.kernel_cost(many, 4, 2, 6, dev)
    risky = cf.Cost_shaping(cf.Expected_saturated_distance([0.0, 0.0], [1.0, 1.0], [0, 1]), risk=0.5)
    with pytest.raises(NotImplementedError, match="risk"):
        mppi.kernel_cost(risky, 4, 2, 6, dev)
    with pytest.raises(ValueError, match="rows"):
        mppi._check_rows(types.SimpleNamespace(kind="traj", traj_len=7), 2, 6)
    mppi._check_rows(types.SimpleNamespace(kind="traj", traj_len=8), 2, 6)
    mppi._check_rows(types.SimpleNamespace(kind="target"), 100, 6)
