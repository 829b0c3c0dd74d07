"""GPU: the fused differentiable model step (mcp_model_step + mcp_model_step_bwd, ops.model_step, Model_learning.fused_next_state,
MC_PILCO.fused_step) -- bit for bit against the open-loop rollout it shares its phases with, against the oracle's step and torch autograd
through it, and through the class path under a policy the fused rollouts do not know (a two-layer tanh torch.nn module).

Models: the seeded generators of tests/width_models.py (random training data, the oracle's own pretrain; the packed side consumes the oracle's
X, alpha and Kinv), N in {17, 33, 48} (Npad 32 / 48 / 48), T = 6, M in {1, 5, 16, 17, 37}: one tile, the tile edge, a ragged last tile, three
tiles.  The rungs of the ladder (4 and 1 particles per workgroup) need N = 640 / 2600: the pairs of tests/test_gpu_open_rollout_grad.py.

Bounds (the ones the open-loop and closed-loop kernels are held to on the oracle's own Kinv / alpha): states, means and
variances 1e-9 absolute; gradients 1e-9 relative to the gradient's largest magnitude."""
import copy
import functools

import numpy as np
import pytest
import torch

import width_models as wm
from closed_loop_family import open_pair, zero_variance_model
from gpu_helpers import G, dev, relmax
from oracle import mcpilco_oracle as orc

pytestmark = pytest.mark.gpu
DT = torch.float64
T = 6
MS = (1, 5, 16, 17, 37)
TOL = 1e-9


def _case(name, S, U, angle, not_angle, vel, not_vel, N, deg=0, vs=None):
    return wm.Case("step_" + name, S, U, tuple(angle), tuple(not_angle), tuple(vel), tuple(not_vel), tuple(N), "plain", 1, T, deg=deg, var_scale=vs)


CASES = {
    # speed models S = 4, U = 1, G = 2 (D = 6): SE, and SE + polynomial(2) with var_scale != 1
    "speed_se": _case("speed_se", 4, 1, (2,), (0, 1, 3), (1, 3), (0, 2), (17, 33)),
    "speed_poly2": _case("speed_poly2", 4, 1, (2,), (0, 1, 3), (1, 3), (0, 2), (33, 48), deg=2, vs=(0.49, 2.25)),
    # delta-state model with an angle, G = S = 3 (D = 5)
    "delta_angle": _case("delta_angle", 3, 1, (1,), (0, 2), (0, 1, 2), (-1, -1, -1), (17, 33, 48)),
    # G = 1 (degree 1) and G = 8 (a delta-state model at S = 8, D = 10)
    "g1": _case("g1", 2, 1, (), (0, 1), (1,), (0,), (33,), deg=1),
    "g8": _case("g8", 8, 1, (0,), range(1, 8), range(8), (-1,) * 8, (17, 33, 48, 17, 33, 48, 17, 33)),
    # the wide class: D = 24, G = 6, degree 1 (two row blocks of [X^T; 1] in phase J)
    "wide": _case("wide", 12, 6, range(6), range(6, 12), range(6, 12), range(6), (33, 17, 48, 33, 48, 17), deg=1),
}


@functools.lru_cache(maxsize=None)
def packed(name):
    """PackedModel on the oracle's own X / alpha / Kinv; built once per process and shared, never modified."""
    from gpu_helpers import spec_from
    from mc_pilco_amd import ops

    c = CASES[name]
    gps = [ops.PackedGP(spec_from(q["ls"], wm.SIGMA_N, 1.0, q["poly"]), G(q["cache"].X.numpy()), G(q["cache"].alpha.numpy()), G(q["cache"].Kinv.numpy()))
           for q in wm.model(c)["gps"]]
    return ops.PackedModel(gps, c.S, c.U, wm.TS, list(c.angle), list(c.not_angle), list(c.vel), list(c.not_vel), var_scale=c.var_scale)


@functools.lru_cache(maxsize=None)
def inputs(name, M):
    """(x0 [M,S], u [T-1,M,U], eps [T-1,M,G], w [T,M,S], wu [T,M,U]) on the CPU from a seeded generator."""
    c = CASES[name]
    g = torch.Generator().manual_seed(7000 + c.seed + M)
    r = lambda *s: torch.randn(*s, dtype=DT, generator=g)  # noqa: E731
    return 0.3 * r(M, c.S), torch.rand(T - 1, M, c.U, dtype=DT, generator=g) * 2 - 1, r(T - 1, M, c.G), r(T, M, c.S), r(T, M, c.U)


def oracle_step(name, x, u, e, sample):
    c = CASES[name]
    return orc.mixed_next_state(wm.model(c)["om"], x, u, e, sample, c.var_scale)


class TanhPolicy(torch.nn.Module):
    """u = u_max tanh(W2 tanh(W1 x + b1) + b2): a policy the fused rollouts do not know, with the step interface of the package's policies."""

    def __init__(self, S, U, seed, H=8, u_max=2.0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.l1, self.l2, self.u_max = torch.nn.Linear(S, H).double(), torch.nn.Linear(H, U).double(), u_max
        with torch.no_grad():
            for q in self.parameters():
                q.copy_(0.5 * torch.randn(q.shape, dtype=DT, generator=g))

    def forward(self, x, t=None, p_dropout=0.0):
        return self.u_max * torch.tanh(self.l2(torch.tanh(self.l1(x))))


def step_noise(mode, eps, t, off=0):
    from mc_pilco_amd import ops

    return None if mode == "mean" else (ops.NoiseSpec(eps=eps[t].contiguous()) if mode == "eps" else ops.NoiseSpec(seed=11, call=3, particle_offset=off))


def chain(pm, x0, u, eps, mode, moments=False, off=0, record=False):
    """T - 1 successive ops.model_step calls fed the inputs u; returns (states [T,M,S], means, variances [T-1,M,G] or None, status word)."""
    from mc_pilco_amd import ops

    status = torch.zeros(1, dtype=torch.int32, device=dev())
    xs, mus, vrs = [x0], [], []
    for t in range(u.shape[0]):
        x = xs[-1].clone().requires_grad_(True) if record else xs[-1]
        out = ops.model_step(pm, x, u[t], t, noise=step_noise(mode, eps, t, off), particle_pred=mode != "mean", moments=moments, status=status)
        assert out[-1] is status and out[0].requires_grad == record
        xs.append(out[0].detach())
        if moments:
            mus.append(out[1])
            vrs.append(out[2])
    return torch.stack(xs), (torch.stack(mus) if moments else None), (torch.stack(vrs) if moments else None), int(status.item())


# ---- 1. chain identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "eps", "philox"])
@pytest.mark.parametrize("name", list(CASES))
def test_a_chain_of_steps_carries_the_bits_of_the_open_loop_rollout(name, mode):
    from mc_pilco_amd import ops

    pm = packed(name)
    for M in MS:
        x0, u, eps, _, _ = (G(a) for a in inputs(name, M))
        sample = mode != "mean"
        nz = None if mode == "mean" else (ops.NoiseSpec(eps=eps) if mode == "eps" else ops.NoiseSpec(seed=11, call=3))
        st, mu, var, status = ops.rollout_open(pm, x0, u, noise=nz, particle_pred=sample, moments=True)
        assert int(status.item()) == 0
        cs, cmu, cvar, cstatus = chain(pm, x0, u, eps, mode, moments=True)
        assert cstatus == 0
        assert torch.equal(cs, st) and torch.equal(cmu, mu) and torch.equal(cvar, var), (name, mode, M)
        # without the moments (the mean step then reads no Kinv: one particle per workgroup, as the rollout's mean chain)
        sp, _ = ops.rollout_open(pm, x0, u, noise=nz, particle_pred=sample)
        plain, _, _, pstatus = chain(pm, x0, u, eps, mode)
        assert pstatus == 0 and torch.equal(plain, sp), (name, mode, M)
        # the recording launch (an input requires grad) and the plain launch agree bitwise
        rec, rmu, rvar, rstatus = chain(pm, x0, u, eps, mode, moments=True, record=True)
        assert rstatus == 0 and torch.equal(rec, cs) and torch.equal(rmu, cmu) and torch.equal(rvar, cvar), (name, mode, M)
        rec2, _, _, _ = chain(pm, x0, u, eps, mode, record=True)
        assert torch.equal(rec2, plain), (name, mode, M)


@pytest.mark.parametrize("name", ["speed_poly2", "g8"])
def test_philox_by_global_particle(name):
    """particle_offset != 0 against the rollout with the same offset; M split over two calls against one call (shard invariance)."""
    from mc_pilco_amd import ops

    pm, M, off = packed(name), 37, 1000
    x0, u, eps, _, _ = (G(a) for a in inputs(name, M))
    st, _ = ops.rollout_open(pm, x0, u, noise=ops.NoiseSpec(seed=11, call=3, particle_offset=off), particle_pred=True)
    whole, _, _, status = chain(pm, x0, u, eps, "philox", off=off)
    assert status == 0 and torch.equal(whole, st)
    a, _, _, _ = chain(pm, x0[:20].contiguous(), u[:, :20].contiguous(), eps, "philox", off=off)
    b, _, _, _ = chain(pm, x0[20:].contiguous(), u[:, 20:].contiguous(), eps, "philox", off=off + 20)
    assert torch.equal(torch.cat([a, b], 1), whole)
    other, _, _, _ = chain(pm, x0, u, eps, "philox", off=off + 1)
    assert not torch.equal(other[1], whole[1])


# ---- 2. one step against the oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_one_step_and_its_gradients_against_the_oracle(name, sample):
    from mc_pilco_amd import ops

    M = 17
    x0, u, eps, w, _ = inputs(name, M)
    torch.set_num_threads(1)
    xo, uo = x0.clone().requires_grad_(True), u[0].clone().requires_grad_(True)
    onx, omu, ovar = oracle_step(name, xo, uo, eps[0], sample)
    assert float(ovar.detach().min()) > 0.0
    ogx, ogu = torch.autograd.grad((w[1] * onx).sum(), [xo, uo])
    xg, ug = G(x0).requires_grad_(True), G(u[0]).requires_grad_(True)
    nx, mu, var, status = ops.model_step(packed(name), xg, ug, 0, noise=ops.NoiseSpec(eps=G(eps[0])) if sample else None, particle_pred=sample,
                                         moments=True)
    assert nx.requires_grad and not mu.requires_grad and not var.requires_grad
    (G(w[1]) * nx).sum().backward()
    ex, em, ev = (float((a.detach().cpu() - b.detach()).abs().max()) for a, b in ((nx, onx), (mu, omu), (var, ovar)))
    egx, egu = relmax(xg.grad, ogx), relmax(ug.grad, ogu)
    print("%s sample %d: x_next %.3e mean %.3e var %.3e g_x %.3e g_u %.3e" % (name, sample, ex, em, ev, egx, egu))
    assert int(status.item()) == 0
    assert ex < TOL and em < TOL and ev < TOL
    assert egx < TOL and egu < TOL


# ---- 3. a closed loop under a torch.nn policy ----------------------------------------------------------------------------------------
def closed_loop(step, pol, x0):
    xs, us = [x0], [pol(x0, t=0)]
    for t in range(1, T):
        xs.append(step(xs[-1], us[-1], t - 1))
        us.append(pol(xs[-1], t=t))
    return torch.stack(xs), torch.stack(us)


@pytest.mark.parametrize("name,sample,M", [("speed_se", False, 17), ("speed_poly2", True, 37), ("delta_angle", True, 5), ("wide", True, 17)])
def test_policy_gradients_of_a_closed_loop_against_autograd_on_the_oracle_step(name, sample, M):
    from mc_pilco_amd import ops

    c, pm = CASES[name], packed(name)
    x0, _, eps, w, wu = inputs(name, M)
    pol_o = TanhPolicy(c.S, c.U, seed=c.seed)
    pol_g = copy.deepcopy(pol_o).to(dev())
    torch.set_num_threads(1)
    ost, oin = closed_loop(lambda x, u, t: oracle_step(name, x, u, eps[t], sample)[0], pol_o, x0)
    ((w * ost).sum() + (wu * oin).sum()).backward()
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    eg = G(eps)
    step = lambda x, u, t: ops.model_step(pm, x, u, t, noise=ops.NoiseSpec(eps=eg[t]) if sample else None, particle_pred=sample, status=status)[0]  # noqa: E731
    st, inp = closed_loop(step, pol_g, G(x0))
    ((G(w) * st).sum() + (G(wu) * inp).sum()).backward()
    es = float((st.detach().cpu() - ost.detach()).abs().max())
    eg_ = [relmax(a.grad, b.grad) for a, b in zip(pol_g.parameters(), pol_o.parameters())]
    print("%s sample %d M %d: states %.3e, d cost / d (W1, b1, W2, b2) %s" % (name, sample, M, es, " ".join("%.3e" % e for e in eg_)))
    assert int(status.item()) == 0
    assert es < TOL
    assert max(eg_) < TOL


# ---- 4. status -------------------------------------------------------------------------------------------------------------------------
def test_the_status_word_is_the_rollouts():
    """A known non-positive variance, by the recipe of tests/test_gpu_dropin.py::test_zero_predictive_variance_raises_like_the_reference_normal:
    one training point exactly at the GP input of x = 0, u = 0, no noise, Kinv = I -> var = 1 - 1 = 0.  And a NaN state."""
    from mc_pilco_amd import hipabi, ops

    pm = zero_variance_model(6, 4, 4, 1, 0.05, [2], [0, 1, 3], [1, 3], [0, 2])  # z = [x0, x1, x3, sin x2, cos x2, u] at x = 0, u = 0
    nan = np.zeros((8, 4))
    nan[3, 1] = float("nan")
    for x, flag, other in ((np.zeros((8, 4)), hipabi.STATUS_NONPOS_VAR, hipabi.STATUS_NAN), (nan + 1.0, hipabi.STATUS_NAN, hipabi.STATUS_NONPOS_VAR)):
        nz = lambda: ops.NoiseSpec(seed=1, call=1)  # noqa: E731
        st, so = ops.rollout_open(pm, G(x), G(np.zeros((1, 8, 1))), noise=nz(), particle_pred=True)
        nx, ss = ops.model_step(pm, G(x), G(np.zeros((8, 1))), 0, noise=nz(), particle_pred=True)
        assert int(ss.item()) == int(so.item())
        assert int(ss.item()) & flag and not int(ss.item()) & other
        assert torch.equal(nx, st[1]) or flag == hipabi.STATUS_NAN
    # the mean step samples nothing: no flag, and the caller's word is ORed into, not overwritten
    word = torch.full((1,), 8, dtype=torch.int32, device=dev())
    _, ss = ops.model_step(pm, G(np.zeros((8, 4))), G(np.zeros((8, 1))), 0, particle_pred=False, status=word)
    assert ss is word and int(word.item()) == 8


# ---- 5. the class path -----------------------------------------------------------------------------------------------------------------
def _apply(obj, M, seed):
    from test_gpu_dropin import T as TD

    torch.manual_seed(seed)
    return obj.apply_policy(particles_initial_state_mean=TD(np.array([0.0, 0.0, 0.1, 0.0])), particles_initial_state_var=TD(1e-2 * np.ones(4)),
                            flg_particles_init_uniform=False, particles_init_up_bound=None, particles_init_low_bound=None,
                            flg_particles_init_multi_gauss=False, num_particles=M, T_control=T)


@pytest.mark.parametrize("pms", [False, True])
def test_fused_step_in_the_class_path(golden, pms):
    """MC_PILCO / MC_PILCO4PMS under the tanh policy, ``fused_step`` True against False (the step loop on get_next_state).  MC_PILCO: the
    mean step on both sides (``particle_pred=False`` bound to the model object's two step methods).  MC_PILCO4PMS's own loop samples with
    an eps it draws itself and has no mean mode; in "reference" noise mode both sides consume the torch generator in the reference's order
    (eps_t, position noise), so the comparison is seed for seed on the sampled step -- the mean and the variance both enter it."""
    from test_gpu_open_rollout import _cartpole_object, quiet

    obj, _ = _cartpole_object(golden, pms)
    assert obj.fused_step is False and obj.last_step_fused is False  # the default: nothing that exists changes
    obj.control_policy = TanhPolicy(4, 1, seed=5, u_max=10.0).to(dev())
    ml = obj.model_learning
    if pms:
        obj.noise_mode = "reference"
    else:
        ml.get_next_state = functools.partial(ml.get_next_state, particle_pred=False)
        ml.fused_next_state = functools.partial(ml.fused_next_state, particle_pred=False)
    M, out = 17, {}
    for fused in (False, True):
        obj.fused_step = fused
        with quiet():
            st, inp = _apply(obj, M, seed=3)
        assert obj.last_step_fused is fused and obj.last_feedback_fused is False
        if fused:
            assert obj.last_status is not None and int(obj.last_status.item()) == 0
            assert float(obj._step_flags(st.sum())[1:].abs().max()) == 0.0
        else:
            assert obj.last_status is None
        assert st.shape == (T, M, 4) and inp.shape == (T, M, 1) and st.requires_grad
        out[fused] = (st.detach(), inp.detach())
    es, ei = (float((out[True][k] - out[False][k]).abs().max()) for k in (0, 1))
    print("pms %d: fused_step on vs off: states %.3e inputs %.3e" % (pms, es, ei))
    assert torch.equal(out[True][0][0], out[False][0][0])  # the same x0
    assert es < TOL
    # a fused policy class resets the report
    obj.fused_step = True
    obj.last_step_fused = True
    obj.control_policy = _cartpole_object(golden, pms)[0].control_policy
    with quiet(), torch.no_grad():
        _apply(obj, M, seed=3)
    assert obj.last_step_fused is False


# ---- 6. the rungs of the ladder --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,deg", [(640, 0), (640, 2), (2600, 0), (2600, 2)])
def test_the_smaller_tiles(N, deg):
    """Sampled, M = 5, T = 3 on the cart-pole shape, as tests/test_gpu_open_rollout_grad.py::test_the_smaller_tiles_of_the_recording_form:
    the recording step runs 4 particles per workgroup at N = 640 and one at N = 2600 (the plain step 16 and 4).  Status 0; plain and
    recording chains carry the bits of the rollout; states and both gradients against the oracle."""
    from mc_pilco_amd import ops
    from open_grad_models import inputs_for, oracle_truth

    c, m, pm = open_pair("speed", N, deg)
    M, Tn = 5, 3
    x0, u, eps, w = inputs_for(c, M, Tn, seed=Tn * 100 + M)
    torch.set_num_threads(1)
    ost, ogx, ogu, vmin = oracle_truth("speed", m, x0, u, eps, w, True)
    assert vmin > 0.0
    sp, status_p = ops.rollout_open(pm, G(x0), G(u), noise=ops.NoiseSpec(eps=G(eps)), particle_pred=True)
    plain, _, _, status_c = chain(pm, G(x0), G(u), G(eps), "eps")
    assert int(status_p.item()) == 0 and status_c == 0 and torch.equal(plain, sp)
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    xg, ug, eg = G(x0).requires_grad_(True), G(u).requires_grad_(True), G(eps)
    xs = [xg]
    for t in range(Tn - 1):
        xs.append(ops.model_step(pm, xs[-1], ug[t], t, noise=ops.NoiseSpec(eps=eg[t]), particle_pred=True, status=status)[0])
    st = torch.stack(xs)
    (G(w) * st).sum().backward()
    es, ex, eu = float((st.detach().cpu() - ost).abs().max()), relmax(xg.grad, ogx), relmax(ug.grad, ogu)
    print("rung N %d deg %d: states %.3e g_x0 %.3e g_u %.3e (min var %.3e)" % (N, deg, es, ex, eu, vmin))
    assert int(status.item()) == 0
    assert torch.equal(st.detach(), sp)
    assert es < TOL and ex < TOL and eu < TOL
