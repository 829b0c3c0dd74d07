"""GPU: the fused closed loop under the tanh-MLP policy (mcp_rollout_mlp + mcp_rollout_mlp_bwd, ops.rollout_mlp, MC_PILCO.apply_policy with
a Policy.MLP_policy) against torch autograd through the oracle's step with the network written out (tests/mlp_models.mlp_truth; conditioning
checked by tests/test_mlp_models_cpu.py), and the bitwise contracts with the open-loop kernels it shares its phases with.

Bounds (tests/test_gpu_pd_rollout.py, on the oracle's own Kinv / alpha): states 1e-9 absolute, inputs 2e-9 absolute,
every parameter gradient and g_x0 1e-9 relative to that tensor's largest magnitude."""
import contextlib
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
from closed_loop_family import MLP, policy
from gpu_helpers import G, dev, relmax
from mlp_models import CASES, SHAPES, case_id, case_truth, inputs_for, network

pytestmark = pytest.mark.gpu
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9
TOLS = (STATE_TOL, INPUT_TOL, GRAD_TOL)
pair = MLP.pair


def gpu_run(pm, pol, x0, eps, w, wu, sample, T, noise=None, x0_grad=True):
    """(states, inputs, [parameter gradients or None], g_x0, status) of the op with L = sum w states + sum wu inputs."""
    r = MLP.run(pm, pol, x0, T, noise if noise is not None else (clf.noise_buffer(eps) if sample else None), w, wu, sample, x0_grad=x0_grad)
    return r.states, r.inputs, r.grads, r.g_x0, r.status


# ---- 1. parity with the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_truth(case):
    mode, shape, deg, N, T, M, hidden, opt = case
    sample = mode == "sampled"
    vs = opt.get("var_scale")
    c, m, ins, truth = case_truth(case)
    truth = clf.mlp_truth_of(truth)
    _, _, pm = pair(shape, N, deg, None if vs is None else tuple(vs))
    if sample and T > 1:
        assert truth.vmin > 0.0
    pol = policy(c, ins["params"], hidden, ins["angle"], ins["non_angle"], u_max=ins["u_max"], squash=ins["squash"])
    only = opt.get("only_grad")
    if only is not None:  # requires_grad on one tensor alone: neither x0 nor the other parameters get a gradient
        for i, q in enumerate(pol.mlp_parameters()):
            q.requires_grad_(i == only)
    got = MLP.run(pm, pol, ins["x0"], T, clf.noise_buffer(ins["eps"]) if sample else None, ins["w"], ins["wu"], sample, x0_grad=only is None)
    clf.check_against(MLP, case_id(case), truth, got, TOLS, only)


# ---- 2. bit identities: against the open-loop launch on the launch's own inputs; the plain against the recording launch -----------------------
def _bit_identities(pm, c, hidden, M, T, noise, seed):
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=seed)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], seed), hidden)
    clf.three_way_bit_identity(MLP, pm, pol, x0, eps, T, noise, sweep=(w, wu))


@pytest.mark.parametrize("M", [17, 1041])  # 4 trajectories per workgroup up to MLP_SMALL_SWARM = 1024 of them, 16 beyond: the bits of either
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_states_carry_the_bits_of_the_open_loop_launch(noise, M):
    c, m, pm = pair("arm2", 37, 1)
    _bit_identities(pm, c, (7, 3), M, 6, noise, seed=21)


# ---- 3. the ladder's smaller tiles (no oracle at these sizes: the bit identities of 2) -----------------------------------------------------------
# (N, M, hidden) and what the two launches run by LDS fit (doubles of 20 480; layouts of csrc/rollout_mlp.hip worked out by hand):
#   640, 5     recording 4 per workgroup, plain 4 (a small swarm)            2600, 5   recording 1, plain 4
#   640, 1041  M > MLP_SMALL_SWARM: the ladder starts at 16; the recording launch falls through to 4 (two k panels of 16: 23 040), plain runs 16
#   2600, 1041 the recording launch falls through 16 -> 4 -> 1; the plain launch 16 -> 4
#   1900, 5 with (64, 64)   recording 4 per workgroup WITHOUT the weights' LDS copy (two panels 15 232 + the copy 4 868 do not fit: the forms
#              that read the weights from global memory through the address table in LDS); the plain launch has the copy -- and the same bits
@pytest.mark.parametrize("N,M,hidden", [(640, 5, (33, 64)), (2600, 5, (33, 64)), (640, 1041, (33, 64)), (2600, 1041, (33, 64)), (1900, 5, (64, 64))])
def test_the_smaller_tiles_of_the_recording_form(N, M, hidden):
    """Sampled, degree 0, T = 3 on arm2, built as tests/test_gpu_pd_rollout.py builds its rungs."""
    c, m, pm = pair("arm2", N, 0)
    _bit_identities(pm, c, hidden, M, 3, "eps", seed=305)


def test_the_wide_model_without_the_weights_copy():
    """UR5 shape, degree 1, N = 1700, (64, 64): the recording launch runs 4 per workgroup and reads the weights from global memory (15 658 doubles
    without the copy, 5 900 more with it); the plain launch has the copy."""
    c, m, pm = pair("ur5", 1700, 1)
    _bit_identities(pm, c, (64, 64), 5, 3, "eps", seed=305)


def test_the_four_trajectory_tile_without_a_record():
    """Sampled, degree 2, N = 1200: the k panel of 16 trajectories does not fit, the plain launch runs 4 per workgroup."""
    c, m, pm = pair("arm2", 1200, 2)
    M, T = 5, 3
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=305)
    pol = policy(c, network(c, (64,), c["angle"], c["not_angle"], 305), (64,), trainable=False)
    clf.four_trajectory_tile_without_a_record(MLP, None, pm, pol, x0, eps, T, None, TOLS)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------------
def test_determinism_and_shard_invariance():
    """Two runs: bit-equal slabs and gradients.  Rows [a, b) launched with particle_offset = a, a a multiple of 16: states, inputs, g_x0 and
    the workgroups' slabs are bitwise those of one launch over all rows (Philox)."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    M, T, cut, hidden = 37, 6, 16, (7, 3)
    x0, _, _, _, _, w, wu = inputs_for(c, M, T, seed=9)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 9), hidden)
    mlp = pol.packed()
    tensors = [q.detach() for q in pol.mlp_parameters()]

    def run(a, b):
        x = G(x0[a:b])
        st, inp, jac = ops._closed_launch(pm, mlp, tensors, ops.NoiseSpec(seed=4, call=2, particle_offset=a), x, T, True,
                                          torch.zeros(1, dtype=torch.int32, device=dev()), True)
        slabs, gx = ops._closed_sweep(pm, mlp, tensors, st, inp, jac, G(w[:, a:b]), G(wu[:, a:b]), True, True)
        torch.cuda.synchronize()
        return st, inp, slabs, gx

    st, inp, slabs, gx = run(0, M)
    assert tuple(slabs.shape) == (3, mlp.n_param) and all(float(slabs[i].abs().max()) > 0 for i in range(3))
    st2, inp2, slabs2, gx2 = run(0, M)
    assert torch.equal(st, st2) and torch.equal(inp, inp2) and torch.equal(slabs, slabs2) and torch.equal(gx, gx2)
    for a, b in ((0, cut), (cut, M)):
        sa, ia, la, xa = run(a, b)
        assert torch.equal(sa, st[:, a:b]) and torch.equal(ia, inp[:, a:b])
        assert torch.equal(la, slabs[a // 16:(b + 15) // 16]) and torch.equal(xa, gx[a:b])
    # the op: two backward passes leave the same bits in every .grad
    _, _, g1, x1, _ = gpu_run(pm, pol, x0, None, w, wu, True, T, noise=ops.NoiseSpec(seed=4, call=2))
    _, _, g2, x2, _ = gpu_run(pm, pol, x0, None, w, wu, True, T, noise=ops.NoiseSpec(seed=4, call=2))
    assert all(torch.equal(p, q) for p, q in zip(g1, g2)) and torch.equal(x1, x2)
    assert all(torch.equal(g.reshape(-1), f) for g, f in zip(g1, torch.split(slabs.sum(0), [q.numel() for q in tensors])))


# ---- 5. Philox mode: central differences of the op ------------------------------------------------------------------------------------------
def test_philox_mode_against_central_differences():
    """Step 1e-6, bound 1e-5 relative with floor 1e-3, as tests/test_gpu_open_rollout_grad.py::test_philox_mode_against_central_differences;
    two entries of every parameter tensor and of x0."""
    c, m, pm = pair("arm2", 37, 2)
    M, T, hidden = 3, 6, (7, 3)
    x0, _, _, _, _, w, wu = inputs_for(c, M, T, seed=5)
    params = network(c, hidden, c["angle"], c["not_angle"], 5)
    policy_of = lambda tensors, trainable: policy(c, tensors, hidden, trainable=trainable)
    clf.central_differences(MLP, pm, policy_of, params, x0, w, wu, T, clf.first_and_last_entries(params + [x0]), step=1e-6,
                            bound=(1e-5, 1e-3))


# ---- 6. status word --------------------------------------------------------------------------------------------------------------------------
def test_status_word():
    c, m, pm = pair("arm2", 37, 0)
    M, T, hidden = 5, 4, (5,)
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=31)
    params = network(c, hidden, c["angle"], c["not_angle"], 31)
    bad = [q.clone() for q in params]
    bad[2][1, 3] = float("nan")  # a NaN weight of the output layer: input 1 of every trajectory
    packed = lambda tensors: policy(c, tensors, hidden, trainable=False).packed()
    zero = packed([torch.zeros_like(q) for q in params])  # a network of zeros gives u = 0 exactly
    clf.status_word(MLP, pm, c, packed(params), (packed(bad), x0), zero, x0, eps, T)


# ---- 7. class path ---------------------------------------------------------------------------------------------------------------------------
def _arm_object(params, hidden, M):
    """MC_PILCO over a fused-layout arm2 speed model trained on a short recorded trajectory (the object of tests/test_gpu_pd_rollout.py's class
    path), with the MLP policy."""
    from mc_pilco_amd.policy_learning import Policy

    return clf.arm_object(Policy.MLP_policy, clf.arm_mlp_par(params, hidden))


def test_class_path():
    M, T, c = 16, 8, SHAPES["arm2"]
    sim = clf.sim_args(M, T)
    net = lambda hidden: network(c, hidden, c["angle"], c["not_angle"], 40)

    def rollout(fused, hidden=(7, 3), expect=None, edit=None):
        obj = _arm_object(net(hidden), hidden, M)
        obj.fused_feedback = fused
        if edit:
            edit(obj)
        torch.manual_seed(5)
        with clf.normal_draws_on_the_cpu():
            st, inp = obj.apply_policy(**sim)
        expect = fused if expect is None else expect
        assert obj.last_feedback_fused is expect and (obj.last_status is not None) is expect
        cost, _ = obj.cost_function(st, inp, 0)
        cost.backward()
        return st.detach(), inp.detach(), [q.grad.clone() for q in obj.control_policy.mlp_parameters()]

    fs, fi, fg = rollout(True)
    ss, si, sg = rollout(False)  # fused_feedback off: the same object runs the generic loop
    es, ei, eg = float((fs - ss).abs().max()), float((fi - si).abs().max()), [relmax(a, b) for a, b in zip(fg, sg)]
    print("class path, fused vs step: states %.3e inputs %.3e g_params %s" % (es, ei, " ".join("%.3e" % e for e in eg)))
    assert es < STATE_TOL and ei < INPUT_TOL and max(eg) < GRAD_TOL
    # what the kernels do not take falls through to the generic branch
    rollout(True, hidden=(65,), expect=False)  # a width beyond MCP_MAX_HIDDEN

    def no_layout(obj):
        obj.model_learning.has_fused_layout = lambda: False

    rollout(True, expect=False, edit=no_layout)  # a model without a fused layout

    obj = _arm_object(net((7, 3)), (7, 3), M)
    before = [q.detach().clone() for q in obj.control_policy.mlp_parameters()]
    torch.manual_seed(6)
    with clf.normal_draws_on_the_cpu(), contextlib.redirect_stdout(io.StringIO()):
        out = obj.reinforce_policy(**clf.reinforce_args(sim, T, 3))
    assert obj.last_feedback_fused is True
    costs = np.asarray(out[0], dtype=float).reshape(-1)
    assert costs.shape == (3,) and np.isfinite(costs).all()
    assert all(float((q.detach() - b).abs().max()) > 1e-4 for q, b in zip(obj.control_policy.mlp_parameters(), before))  # every tensor moved


# ---- 8. saved record -------------------------------------------------------------------------------------------------------------------------
def test_saved_record_refuses_in_place_changes():
    c, m, pm = pair("arm2", 37, 0)
    x0, _, _, _, _, w, wu = inputs_for(c, 2, 4, seed=3)
    clf.saved_record_refuses_in_place_changes(MLP, pm, policy(c, network(c, (5,), c["angle"], c["not_angle"], 3), (5,)), x0, 4)
