"""The policy alone (T = 1, ``model=None``) at the feature, input and basis limits: inputs[0] against ``oracle.policy_forward`` with recorded dropout
masks (p = 0.25) and without, squashed and not, at 1e-12 relative (test_gpu_parity.py::test_policy_forward), and the gradient of a fixed random
linear functional of the inputs w.r.t. every parameter and x0 through ``rollout_backward_raw`` against autograd on the oracle at 1e-10 relative.
One case cannot meet that for a reason of conditioning, CONDITIONED = angles-P1-B65-U2-M1 on its squashed form: the single particle sits deep in the
tanh, 1 - tanh^2 cancels, and the oracle's fp64 autograd is itself 2.0e-10 (log_ls), 1.0e-10 (centers), 9.1e-11 (weight, bias), 5.3e-11 (x0) from the
same gradient in long double (``_longdouble_grads``: the policy written out with numpy, no project code).  There, and only there, the bound is 8 x the
level the test measures on the oracle (capped: the level must stay below 1e-9), as the optimizer-loop tests do.  Every other case measures <= 1.1e-13
against long double; the test asserts < 1e-12 there and keeps the 1e-10 bound (profiles/NOTES.md, part L).

Feature layouts: the three kinds at P in {1, 8, 9, 16, 17, 32} (plain: P = S <= 16; traj: P = 2 S, even; angles reach the odd and the largest
widths); B in {1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024}; U in {1, 2, 8} and M in {1, 5, 257} cycled beside them so that every B meets
every U and every M over the layouts.  A wide policy (P > 16 or U > 4) with B > 512 is refused where it is created (MCP_MAX_BASIS_WIDE): those
combinations assert the refusal."""
import itertools

import numpy as np
import pytest
import torch

from helpers import T as TT
from oracle import mcpilco_oracle as orc

pytestmark = pytest.mark.gpu

P_DROP = 0.25
CONDITIONED = "angles-P1-B65-U2-M1"
# (kind, S, angle, non_angle) -> P
LAYOUTS = [
    ("plain", 1, (), ()), ("plain", 8, (), ()), ("plain", 9, (), ()), ("plain", 16, (), ()),
    ("angles", 1, (), (0,)), ("angles", 5, (0, 1, 2), (3, 4)), ("angles", 5, (0, 1, 2, 3), (4,)), ("angles", 8, tuple(range(8)), ()),
    ("angles", 9, tuple(range(8)), (8,)), ("angles", 16, tuple(range(16)), ()),
    ("traj", 4, (), ()), ("traj", 8, (), ()), ("traj", 16, (), ()),
]
BS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024]
US, MS = [1, 2, 8], [1, 5, 257]
CASES = [(lay, B, US[(i + j) % 3], MS[(i + 2 * j + j // 3) % 3]) for (i, lay), (j, B) in itertools.product(enumerate(LAYOUTS), enumerate(BS))]


def _P(lay):
    kind, S, ang, non = lay
    return {"plain": S, "traj": 2 * S, "angles": len(non) + 2 * len(ang)}[kind]


def _id(case):
    lay, B, U, M = case
    return "%s-P%d-B%d-U%d-M%d" % (lay[0], _P(lay), B, U, M)


def _data(lay, B, U, M):
    kind, S, ang, non = lay
    P = _P(lay)
    rng = np.random.RandomState(1000 * P + 10 * B + U + M)
    return dict(ls=(1.0 + rng.rand(P)) * np.sqrt(max(P, 4) / 4.0), centers=0.7 * rng.randn(B, P), weight=rng.randn(U, B) * (0.5 if B > 1 else 2.0),
                bias=0.3 * rng.randn(U), u_max=list(0.5 + rng.rand(U)), traj=0.3 * rng.randn(1, S), x0=0.5 * rng.randn(M, S),
                mask=(rng.rand(1, M, B) >= P_DROP).astype(np.uint8), w=rng.randn(M, U))


def _longdouble_grads(lay, d, squash, masked):
    """dL/d(log_ls, centers, weight, bias, x0) of L = sum w * u in numpy long double, with the distances in their direct form: what measures the
    rounding level of the oracle's fp64 autograd on the same data."""
    LD = np.longdouble
    kind, S, ang, non = lay
    ang, non = list(ang), list(non)
    x, traj = d["x0"].astype(LD), d["traj"].astype(LD)
    if kind == "angles":
        s = np.concatenate([x[:, non], np.cos(x[:, ang]), np.sin(x[:, ang])], 1)
    elif kind == "traj":
        s = np.concatenate([x, traj[0:1] - x], 1)
    else:
        s = x
    ls = np.exp(np.log(d["ls"]).astype(LD))  # (the parameter is the fp64 logarithm)
    W, um, w = d["weight"].astype(LD), np.asarray(d["u_max"], LD), d["w"].astype(LD)
    diff = (s[:, None, :] - d["centers"].astype(LD)[None, :, :]) / ls
    phi = np.exp(-(diff ** 2).sum(2))
    if masked:
        phi = phi * (d["mask"][0].astype(LD) / (LD(1) - LD(P_DROP)))
    lin = phi @ W.T + d["bias"].astype(LD)
    g_lin = w * (1 - np.tanh(lin / um) ** 2) if squash else w
    g_dist = -phi * (g_lin @ W)
    g_s = (g_dist[:, :, None] * 2 * diff / ls).sum(1)
    if kind == "angles":
        g_x = np.zeros_like(x)
        n = len(non)
        np.add.at(g_x, (slice(None), non), g_s[:, :n])
        np.add.at(g_x, (slice(None), ang), -np.sin(x[:, ang]) * g_s[:, n:n + len(ang)] + np.cos(x[:, ang]) * g_s[:, n + len(ang):])
    elif kind == "traj":
        g_x = g_s[:, :S] - g_s[:, S:]
    else:
        g_x = g_s
    return ((g_dist[:, :, None] * -2 * diff ** 2).sum((0, 1)), (g_dist[:, :, None] * -2 * diff / ls).sum(0), g_lin.T @ phi, g_lin.sum(0), g_x)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_policy_alone_forward_and_gradient(case):
    from gpu_helpers import G, dev
    from mc_pilco_amd import ops

    lay, B, U, M = case
    kind, S, ang, non = lay
    P = _P(lay)
    d = _data(lay, B, U, M)

    def packed(squash):
        prm = [torch.log(G(d["ls"])).reshape(1, -1), G(d["centers"]), G(d["weight"]), G(d["bias"])]
        return ops.PackedPolicy(kind, S, prm[0], prm[1], prm[2], d["u_max"], squash, angle=list(ang), non_angle=list(non),
                                target_traj=d["traj"] if kind == "traj" else None, bias=prm[3])

    if (P > 16 or U > 4) and B > 512:
        with pytest.raises(ValueError, match="MCP_MAX_BASIS_WIDE"):
            packed(True)
        return
    x0 = G(d["x0"])
    for squash, masked in ((True, True), (False, False), (True, False), (False, True)):
        p = P_DROP if masked else 0.0
        prm = [torch.log(TT(d["ls"])).reshape(1, -1), TT(d["centers"]), TT(d["weight"]), TT(d["bias"])]
        xo = TT(d["x0"]).requires_grad_(True)
        for q in prm:
            q.requires_grad_(True)
        pp = orc.PolicyPar(prm[0], prm[1], prm[2], d["u_max"], kind, angle=list(ang), non_angle=list(non), target_traj=TT(d["traj"]) if kind == "traj" else None,
                           squash=squash, bias=prm[3])
        want = orc.policy_forward(pp, xo, 0, TT(d["mask"][0]) if masked else None, p)
        pol = packed(squash)
        nz = ops.NoiseSpec(masks=torch.as_tensor(d["mask"]).to(dev()).contiguous() if masked else None)
        states, inputs, _, status = ops.rollout_forward_raw(None, pol, nz, x0, 1, p, need_jac=False)
        assert int(status.item()) == 0 and torch.equal(states[0], x0)
        scale = float(want.detach().abs().max())
        err = float((inputs[0].cpu() - want.detach()).abs().max()) / scale
        assert err < 1e-12, (squash, masked, err)
        if squash != masked:
            continue  # (the gradient: on the squashed, masked form and on the plain one)
        (want * TT(d["w"])).sum().backward()
        g_ls, g_c, g_w, g_x0, g_b = ops.rollout_backward_raw(None, pol, nz, states, inputs, None, None, G(d["w"]).reshape(1, M, U), p, want_gx0=True)
        exact = _longdouble_grads(lay, d, squash, masked)
        for name, got, ref, ex in zip(("log_ls", "centers", "weight", "bias", "x0"), (g_ls, g_c, g_w, g_b, g_x0),
                                      (prm[0].grad, prm[1].grad, prm[2].grad, prm[3].grad, xo.grad), exact):
            ex = np.asarray(ex).reshape(tuple(ref.shape))
            level = float(np.abs(ref.numpy().astype(np.longdouble) - ex).max() / np.abs(ex).max())  # the oracle's own fp64 error
            if _id(case) == CONDITIONED and squash:
                assert level < 1e-9, (name, level)
                bound = max(1e-10, 8.0 * level)
            else:
                assert level < 1e-12, (name, squash, masked, level)  # (the restatement and the oracle agree: the 1e-10 bound is meaningful)
                bound = 1e-10
            gerr = float((got.cpu().reshape(ref.shape) - ref).abs().max() / ref.abs().max())
            if level > 1e-11:
                print("%s squash %s masked %s: oracle vs long double %.2e, bound %.2e, kernel vs oracle %.2e" % (name, squash, masked, level, bound, gerr))
            assert gerr < bound, (name, squash, masked, gerr, level)
