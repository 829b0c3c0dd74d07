"""The expected-cost kernels at their own edges.  cost_fwd_kernel strides the particles by 256 and reduces over four waves; cost_finalize_kernel,
cost_sums_kernel and cost_finalize_sums_kernel stride the time steps by 256: M around one wave, one workgroup and two, T on both sides of 256.
The truth is the oracle (cart-pole cost, trajectory cost over a ``used`` subset, torch autograd) or plain torch on the concatenated particles;
bounds 1e-12 relative, as in test_gpu_parity.py::test_costs."""
import functools

import numpy as np
import pytest
import torch

from helpers import T as TT
from oracle import mcpilco_oracle as orc

pytestmark = pytest.mark.gpu

S, USED = 5, [4, 0, 2]
MS, TS = [2, 63, 64, 65, 255, 256, 257, 513], [1, 2, 257]


@functools.lru_cache(maxsize=None)
def _truth(kind, T, M):
    """(states, target trajectory, lengthscales, cost, std, dJ/dstates): once per shape."""
    g = torch.Generator().manual_seed(100000 * (kind == "traj") + 1000 * T + M)
    st = torch.randn(T, M, S, dtype=torch.float64, generator=g)
    st[:, 0, 2] = 0.0  # theta exactly 0 (d|theta|/dtheta = 0 there, like torch.abs) beside negative and positive angles
    st[:, M - 1, 2] = -st[:, M - 1, 2].abs() - 0.1
    tgt = 0.5 * torch.randn(T, S, dtype=torch.float64, generator=g)
    ls = 1.0 + 2.0 * torch.rand(len(USED), dtype=torch.float64, generator=g)
    x = st.clone().requires_grad_(True)
    if kind == "cartpole":
        c = orc.cart_pole_cost(x, TT([np.pi, 0.0]), TT([3.0, 1.0]), 2, 0)
    else:
        c = orc.traj_cost(x, tgt, ls, USED)
    cost, std = orc.expected_cost(c)
    cost.backward()
    return st, tgt, ls, float(cost.detach()), float(std), x.grad.numpy(), c.detach()


def _packed_cost(kind, tgt, ls):
    from gpu_helpers import dev
    from mc_pilco_amd import ops

    if kind == "cartpole":
        return ops.PackedCost("cartpole", S, dev(), target_state=[np.pi, 0.0], lengthscales=[3.0, 1.0], angle_index=2, pos_index=0)
    return ops.PackedCost("traj", S, dev(), target_traj=tgt.numpy(), lengthscales=ls.numpy(), used=USED)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("kind", ["cartpole", "traj"])
def test_expected_cost_value_std_and_gradient(kind, M, T):
    from gpu_helpers import G
    from mc_pilco_amd import ops

    st, tgt, ls, oc, ostd, og, _ = _truth(kind, T, M)
    x = G(st.numpy()).requires_grad_(True)
    c, s = ops.expected_cost(_packed_cost(kind, tgt, ls), x)
    c.backward()
    errs = [_rel(float(c), oc), _rel(float(s), ostd), float(np.abs(x.grad.cpu().numpy() - og).max() / np.abs(og).max())]
    print("cost, std, gradient (rel):", " ".join("%.2e" % e for e in errs))
    assert float(x.grad[0, 0, 2]) == 0.0 or kind == "traj"  # (the |theta| subgradient at 0)
    assert max(errs) < 1e-12


def _moments(c):
    """[T,2] (mean, centred sum of squares) of the costs c [T,n] -- what mcp_cost_fwd leaves per rank."""
    m = c.mean(1)
    return torch.stack([m, ((c - m.reshape(-1, 1)) ** 2).sum(1)], 1)


@pytest.mark.parametrize("T", [1, 257])
@pytest.mark.parametrize("counts", [(7,), (1, 64, 5), tuple(1 + (3 * r) % 11 for r in range(64))], ids=["R1", "R3", "R64"])
def test_pooled_finalize_against_the_concatenated_particles(counts, T):
    """mcp_cost_finalize on hand-built per-rank moments with unequal counts (a rank of ONE particle among them) = mean and unbiased std over all the
    particles together."""
    from gpu_helpers import G
    from mc_pilco_amd import ops

    g = torch.Generator().manual_seed(len(counts) * 1000 + T)
    parts = [torch.rand(T, n, dtype=torch.float64, generator=g) for n in counts]
    allc = torch.cat(parts, 1)
    want = (float(allc.mean(1).sum()), float(allc.std(1).sum()))
    out = ops.cost_finalize(G(torch.stack([_moments(p) for p in parts]).numpy()), list(counts)).cpu()
    assert _rel(float(out[0]), want[0]) < 1e-12 and _rel(float(out[1]), want[1]) < 1e-12


def test_more_than_64_ranks_is_a_limit_error():
    from gpu_helpers import G
    from mc_pilco_amd import ops

    with pytest.raises(RuntimeError, match="MCP_ERR_LIMIT"):
        ops.cost_finalize(G(np.zeros((65, 2, 2))), [3] * 65)


@pytest.mark.parametrize("shifted", [False, True])
def test_summable_form_at_257_steps(shifted):
    """mcp_cost_sums per share + mcp_cost_finalize_sums on the added sums (what one all-reduce pools), T = 257 (two strides of the finalize kernel, two
    workgroups of the sums kernel), unequal shares, with and without a shift: the same truth as the one-process cost."""
    from gpu_helpers import G
    from mc_pilco_amd import ops

    T, M = 257, 65
    st, tgt, ls, oc, ostd, _, costs = _truth("traj", T, M)
    cost = _packed_cost("traj", tgt, ls)
    shift = G((costs.mean(1) + 0.01).numpy()) if shifted else None  # (any value near the mean: the previous step's pooled mean in the product)
    x = G(st.numpy())
    sums = None
    for lo, hi in ((0, 1), (1, 40), (40, M)):
        _, s = ops.local_cost(cost, x[:, lo:hi].contiguous(), M, shift=shift)
        sums = s.clone() if sums is None else sums + s
    mean_out = torch.empty(T, dtype=torch.float64, device=x.device)
    out = ops.cost_from_sums(sums, M, shift=shift, mean_out=mean_out).cpu()
    print("summable form (shift %s): cost %.2e std %.2e" % (shifted, _rel(float(out[0]), oc), _rel(float(out[1]), ostd)))
    assert _rel(float(out[0]), oc) < 1e-12 and _rel(float(out[1]), ostd) < 1e-12
    assert float((mean_out.cpu() - costs.mean(1)).abs().max()) < 1e-14
