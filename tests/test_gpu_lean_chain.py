"""The lean forward kernel's serial chain at the smallest shapes where it can go wrong: the trajectory stores wave 0 issues behind its own
phase J (states, measurements, inputs of step t, Jacobian columns of step t - 1, and the tail of the last step, which has no phase J), the
words the Jacobian columns and the measurement wait in until then (every polynomial degree, with and without the measurement model), and
the u phase at one chunk of eight policy groups, a partial second group and a second chunk.

M = 5 at four particles per workgroup: one full cluster and one ragged one.  N = 30 / 44 -> Npad = 32 (two row tiles: only wave 0 owns
rows of Kinv) / 48.  The oracle consumes the same alpha and Kinv and the same recorded noise (eps, masks, position noise), so what is
compared is the evaluation alone: the bounds are those of the short recorded rollouts in test_gpu_parity.py (1e-9 absolute on states and
inputs, 1e-8 relative on the gradients, which every Jacobian column feeds).

T = 1 never reaches a GP-sharded launch (the library takes T > 1 for it: there is no hand-off to make), so that case checks the same call
on the kernel the library picks; T = 2, 3, 4 are the lean kernel's three tails (no Jacobian yet / the tail's Jacobian is the first / both)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from helpers import T as TT
from helpers import hyper
from oracle import mcpilco_oracle as orc

pytestmark = pytest.mark.gpu

S, M = 4, 5
ANGLE, NOT_ANGLE, VEL, NOT_VEL = [2], [0, 1, 3], [1, 3], [0, 2]
TS, U_MAX, SIGMA_N, P_DROP = 0.05, 2.0, 0.1, 0.25
POS, PVEL, STD_POS, FC = [0, 2], [1, 3], [0.01, 0.015], 0.5


@functools.lru_cache(maxsize=None)
def _model(N, U, deg):
    """Arrays of a two-GP speed-integration model on random training data: GP input [x0, x1, x3, sin x2, cos x2, u] (D = 5 + U)."""
    rng = np.random.RandomState(100 * N + 10 * U + deg)
    D = 5 + U
    Z = rng.randn(N, D)
    ls = 1.5 + rng.rand(D)
    poly = None
    if deg >= 1:
        poly = [[0.01 * (0.8 + 0.4 * rng.rand(D + 1))] + ([0.01 * (0.8 + 0.4 * rng.rand(2 * D))] if deg >= 2 else []) for _ in range(2)]
    hyp = [hyper(ls, SIGMA_N, 1.0, None if poly is None else poly[g]) for g in range(2)]
    Ys = [np.sin(Z @ rng.randn(D, 1)) * 0.3 for _ in range(2)]
    caches = [orc.pretrain_gp(hyp[g], TT(Z), TT(Ys[g])) for g in range(2)]
    return dict(ls=ls, poly=poly, hyp=hyp, caches=caches, om=orc.SpeedModel(hyp, caches, TS, ANGLE, NOT_ANGLE, VEL, NOT_VEL))


@functools.lru_cache(maxsize=None)
def _policy(B, U):
    rng = np.random.RandomState(7 * B + U)
    return dict(ls=1.0 + rng.rand(5), centers=rng.randn(B, 5), weight=rng.randn(U, B) * 0.5)


@functools.lru_cache(maxsize=None)
def _noise(T, B, U):
    g = torch.Generator().manual_seed(1000 * T + 10 * B + U)
    x0 = 0.3 * torch.randn(M, S, dtype=torch.float64, generator=g)
    eps = torch.randn(max(T - 1, 0), M, 2, dtype=torch.float64, generator=g)
    masks = (torch.rand(T, M, B, dtype=torch.float64, generator=g) >= P_DROP).to(torch.float64)
    pos_noise = torch.randn(max(T - 1, 0), M, len(POS), dtype=torch.float64, generator=g)
    return x0, eps, masks, pos_noise


@functools.lru_cache(maxsize=None)
def _oracle(T, N, B, U, deg, pms):
    """(states, inputs, cost, gradients) of the oracle: computed once per case, shared by the tests that compare against it."""
    md, pi = _model(N, U, deg), _policy(B, U)
    x0, eps, masks, pos_noise = _noise(T, B, U)
    pp = orc.PolicyPar(torch.log(TT(pi["ls"])).reshape(1, -1), TT(pi["centers"]), TT(pi["weight"]), U_MAX, "angles", angle=[2], non_angle=[0, 1, 3])
    prm = [pp.log_ls, pp.centers, pp.weight]
    for q in prm:
        q.requires_grad_(True)
    if pms:
        st, inp = orc.apply_policy_pms(md["om"], pp, x0, T, POS, PVEL, TT(STD_POS), FC, P_DROP, eps, masks, pos_noise)
    else:
        st, inp = orc.apply_policy(md["om"], pp, x0, T, P_DROP, eps, masks)
    cost, _ = orc.expected_cost(orc.cart_pole_cost(st, TT([np.pi, 0.0]), TT([3.0, 1.0]), 2, 0))
    if T == 1:  # (the cost of x0 alone: nothing to differentiate)
        return st.detach().numpy(), inp.detach().numpy(), float(cost.detach()), None
    cost.backward()
    return st.detach().numpy(), inp.detach().numpy(), float(cost.detach()), [q.grad.numpy().copy() for q in prm]


def _packed(T, N, B, U, deg, pms):
    from gpu_helpers import G, dev, spec_from
    from mc_pilco_amd import ops

    md, pi = _model(N, U, deg), _policy(B, U)
    x0, eps, masks, pos_noise = _noise(T, B, U)
    gps = [ops.PackedGP(spec_from(md["ls"], SIGMA_N, 1.0, None if md["poly"] is None else md["poly"][g]), G(md["caches"][g].X.numpy()),
                        G(md["caches"][g].alpha.numpy()), G(md["caches"][g].Kinv.numpy())) for g in range(2)]
    model = ops.PackedModel(gps, S, U, TS, ANGLE, NOT_ANGLE, VEL, NOT_VEL)
    pol = ops.PackedPolicy("angles", S, torch.log(G(pi["ls"])).reshape(1, -1).requires_grad_(True), G(pi["centers"]).requires_grad_(True),
                           G(pi["weight"]).requires_grad_(True), U_MAX, True, angle=[2], non_angle=[0, 1, 3])
    cost = ops.PackedCost("cartpole", S, dev(), target_state=[np.pi, 0.0], lengthscales=[3.0, 1.0], angle_index=2, pos_index=0)
    nz = ops.NoiseSpec(eps=G(eps.numpy()), masks=masks.to(torch.uint8).to(dev()).contiguous())
    meas = None
    if pms:
        b, a = orc.butter1(FC)
        meas = ops.MeasSpec(pos=POS, vel=PVEL, std_pos=STD_POS, b=b, a=a, pos_noise=G(pos_noise.numpy()))
    return model, pol, cost, nz, meas, G(x0.numpy())


def _cases():
    """Every (degree, measurement model, T) with Npad, B and U cycled through beside them, so that each value of each meets each degree and
    both measurement settings; then the remaining (Npad, B, U) combinations on the SE kernel."""
    out = []
    for i, (deg, pms, T) in enumerate(itertools.product((0, 1, 2), (False, True), (1, 2, 3, 4))):
        out.append((T, (30, 44)[(i + deg) % 2], (16, 17, 129)[(i + pms) % 3], 1 + (i // 2 + deg) % 2, deg, pms))
    for N, B, U in itertools.product((30, 44), (16, 17, 129), (1, 2)):
        out.append((4, N, B, U, 0, False))
    return sorted(set(out))


CASES = _cases()


def _abserr(a, b):
    return float(np.abs(a.detach().cpu().numpy() - np.asarray(b)).max())


def _relerr(a, b):
    b = np.asarray(b)
    return float(np.abs(a.detach().cpu().numpy() - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("T,N,B,U,deg,pms", CASES)
def test_lean_rollout_and_gradient_vs_oracle(T, N, B, U, deg, pms):
    from gpu_helpers import forced_variant
    from mc_pilco_amd import ops

    ost, oin, oc, og = _oracle(T, N, B, U, deg, pms)
    model, pol, cost, nz, meas, x0 = _packed(T, N, B, U, deg, pms)
    with forced_variant(204) as fv:
        st, inp, status = ops.rollout(model, pol, nz, x0, T, P_DROP, meas=meas)
        if T > 1:
            fv.check(lean_expected=True)
        c, _ = ops.expected_cost(cost, st)
        if T > 1:
            c.backward()
    assert int(status.item()) == 0
    errs = [_abserr(st, ost), _abserr(inp, oin), abs(float(c) - oc) / abs(oc)]
    if T > 1:
        errs += [_relerr(pol.log_ls.grad, og[0]), _relerr(pol.centers.grad, og[1]), _relerr(pol.weight.grad, og[2])]
    print("states, inputs (abs), cost, gradients (rel):", " ".join("%.2e" % e for e in errs))
    assert errs[0] < 1e-9 and errs[1] < 1e-9
    assert errs[2] < 1e-11
    assert max(errs[3:], default=0.0) < 1e-8


@pytest.mark.parametrize("T,N,B,U,deg,pms", [(2, 30, 17, 1, 0, False), (4, 44, 129, 2, 2, True), (4, 30, 16, 2, 1, False)])
def test_states_only_call(T, N, B, U, deg, pms):
    """`jac` absent: same trajectories as the call that stores the Jacobian columns, and the oracle's."""
    from gpu_helpers import forced_variant
    from mc_pilco_amd import hipabi, ops

    ost, oin, _, _ = _oracle(T, N, B, U, deg, pms)
    model, pol, _, nz, meas, x0 = _packed(T, N, B, U, deg, pms)
    with forced_variant(204):
        full = ops.rollout_forward_raw(model, pol, nz, x0, T, P_DROP, need_jac=True, meas=meas)
        only = ops.rollout_forward_raw(model, pol, nz, x0, T, P_DROP, need_jac=False, meas=meas)
        assert hipabi.lib().mcp_debug_last_fwd_lean() == 1
    assert only[2] is None and int(only[3].item()) == 0 and int(full[3].item()) == 0
    assert torch.equal(only[0], full[0]) and torch.equal(only[1], full[1])
    if pms:
        assert torch.equal(only[4], full[4])
    assert _abserr(only[0], ost) < 1e-9 and _abserr(only[1], oin) < 1e-9


@pytest.mark.parametrize("T,N,B,U,deg", [(2, 30, 16, 1, 0), (3, 44, 17, 2, 1), (4, 30, 129, 2, 2), (4, 44, 129, 1, 0)])
def test_every_output_element_is_written(monkeypatch, T, N, B, U, deg):
    """states, inputs, jac and meas start as NaN: none is left."""
    from gpu_helpers import forced_variant
    from mc_pilco_amd import hipabi, ops

    model, pol, _, nz, meas, x0 = _packed(T, N, B, U, deg, True)
    real_empty = torch.empty

    def nan_empty(*shape, **kw):  # (the output arrays are the call's only float tensors of three or more dimensions)
        t = real_empty(*shape, **kw)
        if t.dtype == torch.float64 and t.dim() >= 3:
            t.fill_(float("nan"))
        return t

    with forced_variant(204):
        monkeypatch.setattr(torch, "empty", nan_empty)
        states, inputs, jac, status, mbuf = ops.rollout_forward_raw(model, pol, nz, x0, T, P_DROP, need_jac=True, meas=meas)
        monkeypatch.undo()
        assert hipabi.lib().mcp_debug_last_fwd_lean() == 1
    assert int(status.item()) == 0
    assert tuple(jac.shape) == (T - 1, M, 2, 5 + U)
    for name, t in (("states", states), ("inputs", inputs), ("jac", jac), ("meas", mbuf)):
        assert not bool(torch.isnan(t).any()), name


@pytest.mark.parametrize("T,N,B,U,deg,pms", [(4, 44, 129, 2, 0, False), (4, 30, 17, 1, 2, True)])
def test_particles_per_workgroup_reproduce_each_other(T, N, B, U, deg, pms):
    """Forced P = 1, 2, 4 on the lean kernel: bit for bit the same trajectories, Jacobian columns and measurements."""
    from gpu_helpers import forced_variant
    from mc_pilco_amd import hipabi, ops

    model, pol, _, nz, meas, x0 = _packed(T, N, B, U, deg, pms)
    ref = None
    for code in (204, 202, 201):
        with forced_variant(code):
            out = ops.rollout_forward_raw(model, pol, nz, x0, T, P_DROP, need_jac=True, meas=meas)
            assert hipabi.lib().mcp_debug_last_fwd_lean() == 1 and hipabi.lib().mcp_debug_last_particles_per_wg() == code % 100
        assert int(out[3].item()) == 0
        got = [out[0], out[1], out[2]] + ([out[4]] if pms else [])
        if ref is None:
            ref = got
            continue
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
