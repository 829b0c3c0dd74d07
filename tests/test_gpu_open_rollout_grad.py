"""GPU: gradients through the fused open-loop rollout (mcp_rollout_open_rec + mcp_rollout_open_bwd, ops.rollout_open_diff,
Model_learning.open_loop_rollout(differentiable=True)) against torch autograd through the oracle's step loop on the same operands, and the
bitwise contracts of the recording form.

Bounds (the ones tests/test_gpu_parity.py holds the closed-loop adjoint to on the oracle's own Kinv / alpha): states 1e-9
absolute, gradients 1e-9 relative to the gradient's largest magnitude.

The tiles of the recording form: its two panels (k and v = Kinv k, [Npad][pitch] each) fit the LDS with 16 trajectories per workgroup up to
Npad ~ 540 and with 4 up to ~ 2450, beyond that one trajectory.  CASES stops at N = 300, so test_the_smaller_tiles_of_the_recording_form
launches the 4- and the 1-trajectory kernels (N = 640, Npad 640; N = 2600, Npad 2608) at degree classes 0 and 2."""
import numpy as np
import pytest
import torch

from closed_loop_family import open_pair as pair
from gpu_helpers import DT, G, dev, rbf_dict, relmax
from open_grad_models import CASES, inputs_for, oracle_truth

pytestmark = pytest.mark.gpu
STATE_TOL = 1e-9  # absolute, states
GRAD_TOL = 1e-9   # relative to max |gradient|


def gpu_grads(pm, x0, u, eps, w, sample, lengths=None, noise=None):
    from mc_pilco_amd import ops

    xg, ug = G(x0).requires_grad_(True), G(u).requires_grad_(True)
    nz = noise if noise is not None else (ops.NoiseSpec(eps=G(eps)) if sample else None)
    st, status = ops.rollout_open_diff(pm, xg, ug, lengths=lengths, noise=nz, particle_pred=sample)
    (G(w) * st).sum().backward()
    return st.detach(), xg.grad, ug.grad, int(status.item())


@pytest.mark.parametrize("mode,shape,deg,N,T,M,vs", CASES)
def test_gradients_against_the_oracle(mode, shape, deg, N, T, M, vs):
    sample = mode == "sampled"
    c, m, pm = pair(shape, N, deg, None if vs is None else tuple(vs))
    x0, u, eps, w = inputs_for(c, M, T, seed=T * 100 + M)
    torch.set_num_threads(1)
    ost, ogx, ogu, vmin = oracle_truth(shape, m, x0, u, eps, w, sample, var_scale=vs)
    if sample:
        assert vmin > 0.0  # the oracle alone keeps every step's variance positive on this seed
    st, gx, gu, status = gpu_grads(pm, x0, u, eps, w, sample)
    es, ex, eu = float((st.cpu() - ost).abs().max()), relmax(gx, ogx), relmax(gu, ogu)
    print("%s %s deg %d N %d T %d M %d: states %.3e g_x0 %.3e g_u %.3e (min var %.3e)" % (mode, shape, deg, N, T, M, es, ex, eu, vmin))
    assert status == 0
    assert es < 1e-9  # states, absolute
    assert ex < 1e-9 and eu < 1e-9  # gradients, relative to the gradient's largest magnitude


def _ragged():
    c, m, pm = pair("speed", 37, 1)
    M, T, lens = 5, 8, [1, 2, 8, 5, 8]
    x0, u, eps, w = inputs_for(c, M, T, seed=77)
    _, us, _, _ = inputs_for(c, M, T, seed=78, shared=True)
    return c, m, pm, M, T, lens, x0, u, us, eps, w


@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_states_carry_the_bits_of_the_plain_call(noise):
    """rollout_open_diff with inputs that require grad against rollout_open on the same arguments: torch.equal, with ragged lengths, for
    per-trajectory and shared input sequences."""
    from mc_pilco_amd import ops

    c, m, pm, M, T, lens, x0, u, us, eps, w = _ragged()
    sample = noise != "mean"
    for uu in (u, us, us[:, 0, :]):
        for ln in (None, lens):
            nz = (lambda: None if not sample else (ops.NoiseSpec(eps=G(eps)) if noise == "eps" else ops.NoiseSpec(seed=11, call=3)))
            xg, ug = G(x0).requires_grad_(True), G(uu).requires_grad_(True)
            sd, status_d = ops.rollout_open_diff(pm, xg, ug, lengths=ln, noise=nz(), particle_pred=sample)
            sp, status_p = ops.rollout_open(pm, G(x0), G(uu), lengths=ln, noise=nz(), particle_pred=sample)
            assert sd.requires_grad and int(status_d.item()) == 0 and int(status_p.item()) == 0
            assert torch.equal(sd.detach(), sp)
    # nothing requires grad: nothing is recorded, the call is rollout_open
    s0, _ = ops.rollout_open_diff(pm, G(x0), G(u), lengths=lens)
    assert not s0.requires_grad and torch.equal(s0, ops.rollout_open(pm, G(x0), G(u), lengths=lens)[0])


# The rungs below are held to the bounds of the N = 300 cases of CASES (STATE_TOL, GRAD_TOL): the library of the commit before the host path
# was unified measured below them on an MI355X at every rung (states / g_x0 / g_u; a case measuring above would have been given four times
# its measurement, the headroom the N = 1100 / 1500 bounds of tests/test_gpu_open_rollout.py carry):
#   N 640  degree 0  5.7e-12 / 1.3e-12 / 1.4e-11      N 640  degree 2  6.3e-12 / 1.6e-12 / 1.3e-11
#   N 2600 degree 0  5.8e-11 / 1.2e-11 / 4.6e-11      N 2600 degree 2  6.8e-11 / 1.7e-11 / 7.2e-11
@pytest.mark.parametrize("N,deg", [(640, 0), (640, 2), (2600, 0), (2600, 2)])
def test_the_smaller_tiles_of_the_recording_form(N, deg):
    """Sampled, M = 5, T = 3 on the base shape: the recording launch runs 4 trajectories per workgroup at N = 640 and one at N = 2600 (the
    plain launch 16 and 4).  Status 0; the states carry the bits of the plain call; states and both gradients against the oracle."""
    from mc_pilco_amd import ops

    c, m, pm = pair("speed", N, deg)
    M, T = 5, 3
    x0, u, eps, w = inputs_for(c, M, T, seed=T * 100 + M)
    torch.set_num_threads(1)
    ost, ogx, ogu, vmin = oracle_truth("speed", m, x0, u, eps, w, True)
    assert vmin > 0.0
    st, gx, gu, status = gpu_grads(pm, x0, u, eps, w, True)
    sp, status_p = ops.rollout_open(pm, G(x0), G(u), noise=ops.NoiseSpec(eps=G(eps)), particle_pred=True)
    es, ex, eu = float((st.cpu() - ost).abs().max()), relmax(gx, ogx), relmax(gu, ogu)
    print("rung N %d deg %d: states %.3e g_x0 %.3e g_u %.3e (min var %.3e)" % (N, deg, es, ex, eu, vmin))
    assert status == 0 and int(status_p.item()) == 0
    assert torch.equal(st, sp)
    assert es < STATE_TOL and ex < GRAD_TOL and eu < GRAD_TOL


def test_philox_mode_against_central_differences():
    """The draws cannot be handed to the oracle: central differences of the op itself, same seed / call.  Step 1e-6 and bound 1e-5 relative
    (floor 1e-3) as tests/test_gpu_parity.py::test_adjoint_matches_finite_difference_at_full_width."""
    from mc_pilco_amd import ops

    c, m, pm = pair("speed", 37, 2)
    M, T = 3, 6
    x0, u, _, w = inputs_for(c, M, T, seed=5)
    nz = lambda: ops.NoiseSpec(seed=77, call=5)
    _, gx, gu, status = gpu_grads(pm, x0, u, None, w, True, noise=nz())
    assert status == 0

    def loss(x0_, u_):
        st, s = ops.rollout_open(pm, G(x0_), G(u_), noise=nz(), particle_pred=True)
        assert int(s.item()) == 0
        return float((G(w) * st).sum())

    h = 1e-6
    for idx in ((0, 0, 0), (2, 1, 0), (4, 2, 0)):
        up, um = u.clone(), u.clone()
        up[idx] += h
        um[idx] -= h
        fd, g = (loss(x0, up) - loss(x0, um)) / (2 * h), float(gu[idx])
        print("u%s: fd %.9e adjoint %.9e" % (idx, fd, g))
        assert abs(fd - g) < 1e-5 * max(abs(g), 1e-3)
    for idx in ((0, 2), (2, 1)):
        xp, xm = x0.clone(), x0.clone()
        xp[idx] += h
        xm[idx] -= h
        fd, g = (loss(xp, u) - loss(xm, u)) / (2 * h), float(gx[idx])
        print("x0%s: fd %.9e adjoint %.9e" % (idx, fd, g))
        assert abs(fd - g) < 1e-5 * max(abs(g), 1e-3)


@pytest.mark.parametrize("sample", [False, True])
def test_ragged_lengths_and_shared_inputs(sample):
    c, m, pm, M, T, lens, x0, u, us, eps, w = _ragged()
    torch.set_num_threads(1)
    ost, ogx, ogu, vmin = oracle_truth("speed", m, x0, u, eps, w, sample, lengths=lens)  # each trajectory truncated at its length
    st, gx, gu, status = gpu_grads(pm, x0, u, eps, w, sample, lengths=lens)
    assert status == 0 and (not sample or vmin > 0.0)
    assert float((st.cpu() - ost).abs().max()) < 1e-9  # states, absolute
    assert relmax(gx, ogx) < 1e-9 and relmax(gu, ogu) < 1e-9  # gradients, relative to max |g|
    for p, ln in enumerate(lens):
        assert bool((gu[ln - 1:, p, :] == 0).all())  # rows from len - 1 on: exactly zero
    assert torch.equal(gx[0], G(w)[0, 0])  # len == 1: g_x0 = g_states[0]
    # one shared input sequence: its gradient is the sum over the trajectories of the per-trajectory run on expanded inputs
    ue = us.expand(-1, M, -1).contiguous()
    _, gxe, gue, _ = gpu_grads(pm, x0, ue, eps, w, sample, lengths=lens)
    for ush in (us, us[:, 0, :]):
        _, gxs, gus, status = gpu_grads(pm, x0, ush, eps, w, sample, lengths=lens)
        assert status == 0 and gus.shape == ush.shape
        assert relmax(gus.reshape(T - 1, 1, -1), gue.sum(1, keepdim=True)) < 1e-9 and relmax(gxs, gxe) < 1e-9  # the parity bound
        _, gxs2, gus2, _ = gpu_grads(pm, x0, ush, eps, w, sample, lengths=lens)
        assert torch.equal(gus, gus2) and torch.equal(gxs, gxs2)  # bitwise equal run to run


def test_shard_invariance():
    """Trajectories [a, b) launched with particle_offset = a: bitwise the rows [a, b) of one launch over all of them (Philox)."""
    from mc_pilco_amd import ops

    c, m, pm = pair("speed", 37, 0)
    M, T, cut = 20, 6, 7
    x0, u, _, w = inputs_for(c, M, T, seed=9)
    _, gx, gu, status = gpu_grads(pm, x0, u, None, w, True, noise=ops.NoiseSpec(seed=4, call=2))
    assert status == 0
    for a, b in ((0, cut), (cut, M)):
        _, gxa, gua, status = gpu_grads(pm, x0[a:b], u[:, a:b], None, w[:, a:b], True, noise=ops.NoiseSpec(seed=4, call=2, particle_offset=a))
        assert status == 0
        assert torch.equal(gxa, gx[a:b]) and torch.equal(gua, gu[:, a:b])


def test_saved_record_refuses_in_place_changes():
    from mc_pilco_amd import ops

    c, m, pm = pair("speed", 37, 0)
    x0, u, _, w = inputs_for(c, 2, 4, seed=3)
    st, _ = ops.rollout_open_diff(pm, G(x0).requires_grad_(True), G(u))
    with torch.no_grad():
        st.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        st.sum().backward()


@pytest.mark.parametrize("family", ["speed", "delta"])
def test_class_path(golden, family):
    """Model_learning.open_loop_rollout(differentiable=True) gives the op's gradients; the default call returns tensors without a graph; a
    model with an overridden step refuses."""
    import contextlib
    import io

    from mc_pilco_amd import ops
    from mc_pilco_amd.model_learning import Model_learning as ML
    from test_gpu_dropin import build_cartpole

    fx = golden("mean_rollout")
    with contextlib.redirect_stdout(io.StringIO()):
        if family == "speed":
            ml = build_cartpole(fx, 0, False)
        else:
            ml = ML.Model_learning_RBF_angle_state(num_gp=4, init_dict_list=[rbf_dict(6, np.ones(6) * 2.0, 0.05)] * 4, angle_indeces=[2],
                                                   not_angle_indeces=[0, 1, 3], dtype=DT, device=dev())
            ml.add_data(fx["states_tr"], fx["inputs_tr"])
            with torch.no_grad():
                for g in range(4):
                    ml.pretrain_gp(g)
            ml.set_eval_mode()
    pm = ml.packed()
    gen = torch.Generator().manual_seed(2)
    x0 = 0.4 * (torch.rand(3, 4, dtype=DT, generator=gen) - 0.5)
    u = torch.rand(5, 3, 1, dtype=DT, generator=gen) - 0.5
    w = torch.randn(6, 3, 4, dtype=DT, generator=gen)
    for sample in (False, True):
        nz = lambda: ops.NoiseSpec(seed=3, call=1) if sample else None
        xg, ug = G(x0).requires_grad_(True), G(u).requires_grad_(True)
        st, status = ml.open_loop_rollout(xg, ug, particle_pred=sample, noise=nz(), differentiable=True)
        (G(w) * st).sum().backward()
        _, gx, gu, _ = gpu_grads(pm, x0, u, None, w, sample, noise=nz())
        assert int(status.item()) == 0 and torch.equal(xg.grad, gx) and torch.equal(ug.grad, gu)
        assert float(gx.abs().max()) > 0 and float(gu.abs().max()) > 0
        st0, _ = ml.open_loop_rollout(G(x0), G(u), particle_pred=sample, noise=nz())  # the default: today's call, no graph
        assert not st0.requires_grad and torch.equal(st0, st.detach())

    class Mine(type(ml)):
        def get_next_state(self, current_state, current_input, particle_pred=True):
            nxt, a, b = super().get_next_state(current_state, current_input, particle_pred)
            return nxt + 1.0, a, b

    ml.__class__ = Mine
    with pytest.raises(NotImplementedError):
        ml.open_loop_rollout(G(x0).requires_grad_(True), G(u), differentiable=True)
