"""GPU: which C entries the one closed-loop host path of ops (``_rollout_closed``: ops.rollout_pd, ops.rollout_mlp) calls.  The library is
wrapped by a recorder for the duration of a test; the names it hands out in forward, and then in ``backward()``, are compared with the
literal lists below -- per policy (PD law, tanh MLP with one and with two hidden layers), with and without a measurement model, with no
gradient asked for, the parameters' alone, or x0's alone.  The smallest model of tests/pd_models.py (the two-joint arm: S = 4, U = 2, N = 37),
M = 5, T = 3; T = 1 (no transition: nothing to record) once per policy."""
import pytest
import torch

from closed_loop_family import PD, controller
from closed_loop_family import policy as mlp_policy
from gpu_helpers import G
from mlp_models import network
from pd_models import inputs_for

pytestmark = pytest.mark.gpu
pair = PD.pair

# (policy kind, measured) -> (the mcp_rollout_* entries of forward, of backward)
ENTRIES = {
    ("pd", False): (["mcp_rollout_pd"], ["mcp_rollout_pd_bwd"]),
    ("pd", True): (["mcp_rollout_pd_meas"], ["mcp_rollout_pd_meas_bwd"]),
    ("mlp", False): (["mcp_rollout_mlp"], ["mcp_rollout_mlp_bwd"]),
    ("mlp", True): (["mcp_rollout_mlp_meas"], ["mcp_rollout_mlp_meas_bwd"]),
}
POLICIES = {"pd": None, "mlp3": (3,), "mlp3x2": (3, 2)}  # (the hidden widths of the networks)
M, SEED = 5, 41


@pytest.fixture
def calls(monkeypatch):
    """The names of the library's functions in the order ops asked for them (each one is called where it is asked for)."""
    from mc_pilco_amd import hipabi

    real, names = hipabi.lib(), []

    class Recorder:
        def __getattr__(self, name):
            names.append(name)
            return getattr(real, name)

    recorder = Recorder()
    monkeypatch.setattr(hipabi, "lib", lambda: recorder)
    return names


def rollout_entries(names):
    out = [n for n in names if n.startswith("mcp_rollout_")]
    del names[:]
    return out


def build(kind, T, trainable):
    """(ops function, policy module, its parameter tensors) on the arm model's shape."""
    from mc_pilco_amd import ops

    c, _, _ = pair("arm2", 37, 0)
    _, kp, kd, target, _, _, _ = inputs_for(c, M, T, seed=SEED)
    if kind == "pd":
        pol = controller(c, kp, kd, target, trainable=trainable)
        return ops.rollout_pd, pol, [pol.sqrt_Kp_gains, pol.sqrt_Kd_gains]
    hidden = POLICIES[kind]
    pol = mlp_policy(c, network(c, hidden, c["angle"], c["not_angle"], SEED), hidden, trainable=trainable)
    return ops.rollout_mlp, pol, list(pol.mlp_parameters())


def one_pair():
    from mc_pilco_amd import ops

    return ops.MeasSpec(pos=[0], vel=[2], std_pos=[0.01], b=[0.3375, 0.3375], a=[1.0, -0.3249])


def run(kind, T, measured, grads):
    """One call of the op with ``grads`` in ("off", "params", "x0"): (states, inputs, x0, parameter tensors, the MeasSpec or None)."""
    from mc_pilco_amd import ops

    c, _, pm = pair("arm2", 37, 0)
    op, pol, params = build(kind, T, trainable=grads == "params")
    x = G(inputs_for(c, M, T, seed=SEED)[0]).requires_grad_(grads == "x0")
    meas = one_pair() if measured else None
    st, inp, status = op(pm, pol.packed(), ops.NoiseSpec(seed=4, call=2), x, T, meas=meas)
    assert int(status.item()) == 0
    return st, inp, x, params, meas


@pytest.mark.parametrize("grads", ["off", "params", "x0"])
@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
@pytest.mark.parametrize("kind", list(POLICIES))
def test_entries_called(calls, kind, measured, grads):
    T = 3
    fwd, bwd = ENTRIES[("pd" if kind == "pd" else "mlp", measured)]
    st, inp, x, params, meas = run(kind, T, measured, grads)
    assert rollout_entries(calls) == fwd
    if measured:  # (without a MeasSpec there is nowhere to set one: the saved-tensor count below shows that none was allocated)
        assert tuple(meas.measured.shape) == (T, M, 4) and bool(torch.isfinite(meas.measured).all())
    if grads == "off":
        # nothing recorded: the forward entry alone, and the bits of the recording call
        assert not st.requires_grad and not inp.requires_grad and st.grad_fn is None
        rs, ri, _, _, _ = run(kind, T, measured, "x0")
        assert rollout_entries(calls) == fwd
        assert torch.equal(st, rs) and torch.equal(inp, ri)
        return
    # the record: states, inputs, the parameter tensors, jac, and the measured states of a measured launch
    assert len(st.grad_fn.saved_tensors) == 2 + len(params) + 1 + int(measured)
    (st.sum() + inp.sum()).backward()
    assert rollout_entries(calls) == bwd
    if grads == "params":
        assert x.grad is None and all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in params)
    else:
        assert all(q.grad is None for q in params) and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0


@pytest.mark.parametrize("kind", list(POLICIES))
def test_one_row_records_no_jac(calls, kind):
    """T = 1: the policy alone.  The forward entry is called, no jac is allocated or saved, and backward runs the sweep without one."""
    fwd, bwd = ENTRIES[("pd" if kind == "pd" else "mlp", False)]
    st, inp, x, params, _ = run(kind, 1, False, "params")
    assert rollout_entries(calls) == fwd and tuple(st.shape) == (1, M, 4)
    assert len(st.grad_fn.saved_tensors) == 2 + len(params)
    (st.sum() + inp.sum()).backward()
    assert rollout_entries(calls) == bwd
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in params)
    assert float(params[0].grad.abs().max()) > 0
