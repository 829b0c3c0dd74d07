"""GPU: target-trajectory features in the fused closed loop under the tanh-MLP policy (mcp_rollout_mlp_track + mcp_rollout_mlp_track_bwd,
ops.rollout_mlp with a tracking ops.PackedMLP, MC_PILCO / MC_PILCO4PMS.apply_policy with a Policy.MLP_policy(target_traj=...), and that
policy under particle sharding) against torch autograd through the oracle's step with the network and its error features written out
(tests/mlp_track_models.track_truth; conditioning and near misses checked by tests/test_mlp_track_cpu.py), and the bitwise contracts the
tracking forms keep.

Bounds (tests/test_gpu_mlp_rollout.py, on the oracle's own Kinv / alpha): states and measurements 1e-9 absolute, inputs
2e-9 absolute, every parameter gradient and g_x0 1e-9 relative to that tensor's largest magnitude."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
from closed_loop_family import MLP
from closed_loop_family import meas_spec as spec
from gpu_helpers import DT, G, dev, relmax
from mlp_meas_models import meas_model
from mlp_models import SHAPES, inputs_for
from mlp_models import network as plain_network
from mlp_track_models import CASES, case_id, case_truth, network, target_for
from pd_meas_models import pos_noise_for
from rank_harness import rank_group, run_ranks

pytestmark = pytest.mark.gpu
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9
TOLS = (STATE_TOL, INPUT_TOL, GRAD_TOL)


def pair(shape, N, deg):
    """(cfg, oracle model, PackedModel) of tests/test_gpu_mlp_meas.py: shared with that module, with the sampling time a measurement needs."""
    return MLP.pair(shape, N, deg, measured=True)


def policy(c, params, hidden, target, idx=None, angle=None, non_angle=None, squash=True, trainable=True, u_max=1.0, **kw):
    """clf.policy with a target trajectory (``idx`` None: errors on every component)."""
    from mc_pilco_amd.policy_learning import Policy

    angle = c["angle"] if angle is None else angle
    non_angle = c["not_angle"] if non_angle is None else non_angle
    pol = Policy.MLP_policy(state_dim=c["S"], input_dim=c["U"], hidden_sizes=list(hidden), angle_indices=angle or None, non_angle_indices=non_angle or None,
                            u_max=u_max, flg_squash=squash, weight_init=params, dtype=DT, device=dev(), target_traj=None if target is None else G(target),
                            error_indices=idx, **kw)
    for q in pol.parameters():
        q.requires_grad_(trainable)
    return pol


def arm_setup(M, T, hidden, seed, idx=None, N=37, deg=1):
    """arm2 at (N, deg): (cfg, PackedModel, x0, eps, w, wu, target [T + 2, S], network with the error columns)."""
    c, m, pm = pair("arm2", N, deg)
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=seed)
    n = c["S"] if idx is None else len(idx)
    return c, pm, x0, eps, w, wu, target_for(c, T, x0), network(c, hidden, c["angle"], c["not_angle"], n, seed)


def K(masks):
    return masks.to(torch.uint8).to(dev()).contiguous()


# ---- 1. parity with the truth -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_truth(case):
    from mc_pilco_amd import ops

    mode, shape, deg, N, T, M, hidden, opt = case
    c, m, ins, truth = case_truth(case)
    truth = clf.mlp_truth_of(truth)
    _, _, pm = pair(shape, N, deg)
    if ins["sample"] and T > 1:
        assert truth.vmin > 0.0
    pol = policy(c, ins["params"], hidden, ins["target"], ins["idx"], ins["angle"], ins["non_angle"], squash=ins["squash"], flg_drop=ins["p"] > 0.0)
    assert pol.packed().P == ins["params"][0].shape[1] and pol.packed().track_c().n == len(ins["idx"])
    only = opt.get("only_grad")
    if only is not None:  # requires_grad on one tensor alone: neither x0 nor the other parameters get a gradient
        for i, q in enumerate(pol.mlp_parameters()):
            q.requires_grad_(i == only)
    noise = ops.NoiseSpec(eps=G(ins["eps"]) if ins["sample"] else None, masks=None if ins["masks"] is None else K(ins["masks"]))
    got = MLP.run(pm, pol, ins["x0"], T, noise, ins["w"], ins["wu"], ins["sample"], meas=spec(ins["ms"], ins["pos_noise"]), p_drop=ins["p"] or None,
                  x0_grad=only is None)
    clf.check_against(MLP, case_id(case), truth, got, TOLS, only)


# ---- 2. no track through the new entries ----------------------------------------------------------------------------------------------------------
def raw(entries, head, pm, noise, p, x0, T, w, wu, meas, n_param):
    """A recording launch and its sweep through the C entries ``entries`` as they are, ``head``: the arguments between the policy and the
    measurement model: (states, inputs, measurements or None, slabs, g_x0)."""
    from mc_pilco_amd import hipabi as abi
    from mc_pilco_amd import ops

    M = int(x0.shape[0])
    states, inputs, jac = ops._record_buffers(dev(), T, M, pm.S, pm.U, pm.G, pm.D, T > 1)
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    buf = None
    if meas is not None:
        buf = meas.measured = torch.empty(T, M, pm.S, dtype=DT, device=dev())
    nz = noise.to_c()
    marg = ops._meas_arg(meas, T, M, buf)
    args = head + [marg[0] if marg else None, C.byref(nz), float(p), M, T]
    abi.check(getattr(abi.lib(), entries[0])(*args, 1, abi.ptr(x0), abi.ptr(states), abi.ptr(inputs), None, None, abi.ptr(jac), abi.ptr(status),
                                             abi.stream()), entries[0])
    slabs, gx = torch.empty((M + 15) // 16, n_param, dtype=DT, device=dev()), torch.empty(M, pm.S, dtype=DT, device=dev())
    abi.check(getattr(abi.lib(), entries[1])(*args, abi.ptr(states), abi.ptr(inputs), abi.ptr(jac), abi.ptr(w), abi.ptr(wu), abi.ptr(slabs), abi.ptr(gx),
                                             abi.stream()), entries[1])
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return states, inputs, buf, slabs, gx


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
def test_no_track_through_the_new_entries_is_the_dropout_entries(measured, p):
    """track NULL and track->n == 0: the bits of mcp_rollout_mlp_drop and its sweep -- states, inputs, measurements, slabs and g_x0 -- on
    M = 37 (three slabs)."""
    from mc_pilco_amd import hipabi as abi
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 1)
    M, T, hidden = 37, 6, (7, 3)
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=9)
    pol = clf.policy(c, plain_network(c, hidden, c["angle"], c["not_angle"], 9), hidden)
    mlp, tensors = pol.packed(), [q.detach() for q in pol.mlp_parameters()]
    pc = mlp.to_c(*tensors)
    ms = meas_model("arm2", "all", 0.1) if measured else None
    pn = pos_noise_for(T, M, 2, 9) if measured else None
    keep = torch.empty(T, M, 10, dtype=DT).bernoulli_(0.75, generator=torch.Generator().manual_seed(8))
    nz = lambda: ops.NoiseSpec(eps=G(eps), masks=K(keep))
    run = lambda entries, head: raw(entries, [C.byref(pm.c), C.byref(pc)] + head, pm, nz(), p, G(x0), T, G(w), G(wu), spec(ms, pn), mlp.n_param)
    old = run(("mcp_rollout_mlp_drop", "mcp_rollout_mlp_drop_bwd"), [])
    assert tuple(old[3].shape) == (3, mlp.n_param) and float(old[3].abs().max()) > 0 and (old[2] is not None) is measured
    empty = abi.MLPTrack()  # n == 0: nothing else of it is read
    for track in (None, C.byref(empty)):
        new = run(("mcp_rollout_mlp_track", "mcp_rollout_mlp_track_bwd"), [track])
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(old, new))


# ---- 3. zero error columns ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
def test_zero_error_columns_are_the_untracked_policy(measured):
    """W0' = [W0 | 0]: the states and inputs of the policy without a target, bit for bit (mlp_unit adds the products in feature order, and
    fma(0, e, acc) == acc); the common gradients and g_x0 to the gradient bound; the error columns still get a gradient."""
    c, pm, x0, eps, w, wu, target, _ = arm_setup(17, 6, (7, 3), 9)
    hidden, idx = (7, 3), [3, 0, 1]
    params = plain_network(c, hidden, c["angle"], c["not_angle"], 9)
    wide = [torch.cat([params[0], torch.zeros(hidden[0], len(idx), dtype=DT)], dim=1)] + params[1:]
    ms = meas_model("arm2", "all", 0.1) if measured else None
    pn = pos_noise_for(6, 17, 2, 9) if measured else None
    a = MLP.run(pm, clf.policy(c, params, hidden), x0, 6, clf.noise_buffer(eps), w, wu, True, meas=spec(ms, pn))
    b = MLP.run(pm, policy(c, wide, hidden, target[:6], idx), x0, 6, clf.noise_buffer(eps), w, wu, True, meas=spec(ms, pn))
    assert a.status == 0 and b.status == 0
    assert torch.equal(a.states, b.states) and torch.equal(a.inputs, b.inputs) and (not measured or torch.equal(a.meas, b.meas))
    eg = [relmax(b.grads[0][:, :-len(idx)], a.grads[0])] + [relmax(q, r) for q, r in zip(b.grads[1:], a.grads[1:])] + [relmax(b.g_x0, a.g_x0)]
    print("zero error columns: common gradients %s" % " ".join("%.3e" % e for e in eg))
    assert max(eg) < GRAD_TOL and float(b.grads[0][:, -len(idx):].abs().max()) > 0


# ---- 4. bit identities ----------------------------------------------------------------------------------------------------------------------------
def _bit_identities(N, deg, hidden, M, T, noise, seed, idx=None):
    c, pm, x0, eps, w, wu, target, params = arm_setup(M, T, hidden, seed, idx, N, deg)
    clf.three_way_bit_identity(MLP, pm, policy(c, params, hidden, target[:T], idx), x0, eps, T, noise, sweep=(w, wu))


@pytest.mark.parametrize("M", [17, 1041])  # 4 trajectories per workgroup, and 16
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_states_carry_the_bits_of_the_open_loop_launch(noise, M):
    _bit_identities(37, 1, (7, 3), M, 6, noise, seed=21)


@pytest.mark.parametrize("N,M", [(640, 5), (2600, 5), (640, 1041), (2600, 1041)])
def test_the_smaller_tiles_of_the_recording_form(N, M):
    """The rungs of tests/test_gpu_mlp_rollout.py::test_the_smaller_tiles_of_the_recording_form (sampled, degree 0, T = 3 on arm2, hidden
    (33, 64)) under a tracking policy: the recording launch runs a narrower tile than the plain one, and carries its bits."""
    _bit_identities(N, 0, (33, 64), M, 3, "eps", seed=305, idx=[2, 0, 3])


# ---- 5. determinism and shard invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
def test_determinism_and_shard_invariance_under_philox(measured):
    """Two runs: the same bits.  Rows [a, b) launched with particle_offset = a, a a multiple of 16: states, inputs, g_x0 and the workgroups'
    slabs are bitwise those of one launch over all rows."""
    from mc_pilco_amd import ops

    M, T, cut, hidden = 37, 6, 16, (7, 3)
    c, pm, x0, _, w, wu, target, params = arm_setup(M, T, hidden, 9, deg=0)
    pol = policy(c, params, hidden, target[:T])
    mlp, tensors = pol.packed(), [q.detach() for q in pol.mlp_parameters()]
    ms = meas_model("arm2", "all", 0.1) if measured else None

    def run(a, b):
        nz, sp = ops.NoiseSpec(seed=4, call=2, particle_offset=a), spec(ms)
        st, inp, jac = ops._closed_launch(pm, mlp, tensors, nz, G(x0[a:b]), T, True, torch.zeros(1, dtype=torch.int32, device=dev()), True, sp)
        slabs, gx = ops._closed_sweep(pm, mlp, tensors, st, inp, jac, G(w[:, a:b]), G(wu[:, a:b]), True, True, sp, None if sp is None else sp.measured)
        torch.cuda.synchronize()
        return st, inp, slabs, gx

    st, inp, slabs, gx = run(0, M)
    assert tuple(slabs.shape) == (3, mlp.n_param) and all(float(slabs[i].abs().max()) > 0 for i in range(3))
    assert all(torch.equal(p, q) for p, q in zip(run(0, M), (st, inp, slabs, gx)))
    for a, b in ((0, cut), (cut, M)):
        sa, ia, la, xa = run(a, b)
        assert torch.equal(sa, st[:, a:b]) and torch.equal(ia, inp[:, a:b])
        assert torch.equal(la, slabs[a // 16:(b + 15) // 16]) and torch.equal(xa, gx[a:b])


# ---- 6. Philox mode: central differences of the op ------------------------------------------------------------------------------------------------
def test_philox_mode_against_central_differences():
    """Step 1e-6, bound 1e-5 relative with floor 1e-3, as tests/test_gpu_mlp_rollout.py::test_philox_mode_against_central_differences; two
    entries of every parameter tensor and of x0 -- the last entry of W0 is in an error column, the last of x0 a component with an error --
    and one more of each."""
    M, T, hidden, idx = 3, 6, (7, 3), [3, 0]
    c, pm, x0, _, w, wu, target, params = arm_setup(M, T, hidden, 5, idx, deg=2)
    policy_of = lambda tensors, trainable: policy(c, tensors, hidden, target[:T], idx, trainable=trainable)
    P = params[0].shape[1]
    checks = clf.first_and_last_entries(params + [x0]) + [("W0 error column 0, unit 2", 0, 2 * P + P - 2), ("x0 of trajectory 1, component 0", len(params), c["S"])]
    clf.central_differences(MLP, pm, policy_of, params, x0, w, wu, T, checks, step=1e-6, bound=(1e-5, 1e-3))


# ---- 7. status word -------------------------------------------------------------------------------------------------------------------------------
def test_status_word():
    """A NaN in a row of the target reaches the inputs: MCP_STATUS_NAN.  (A NaN operand only.)"""
    M, T, hidden = 5, 4, (5,)
    c, pm, x0, eps, w, wu, target, params = arm_setup(M, T, hidden, 31, deg=0)
    bad = target[:T].clone()
    bad[2, 1] = float("nan")
    packed = lambda tensors, tgt: policy(c, tensors, hidden, tgt, trainable=False).packed()
    zero = packed([torch.zeros_like(q) for q in params], target[:T])  # a network of zeros gives u = 0 exactly
    clf.status_word(MLP, pm, c, packed(params, target[:T]), (packed(params, bad), x0), zero, x0, eps, T)


# ---- 8. class path, "reference" noise mode --------------------------------------------------------------------------------------------------------
ARM_IDX = [1, 3, 0]


def _object(cls_name, params, hidden, target):
    from mc_pilco_amd.policy_learning import Policy

    par = clf.arm_mlp_par(params, hidden, target_traj=G(target), error_indices=ARM_IDX)
    return clf.arm_object(Policy.MLP_policy, par, clf.ARM_PMS if cls_name == "MC_PILCO4PMS" else None)


def _arm_net(hidden, T):
    c = SHAPES["arm2"]
    return network(c, hidden, c["angle"], c["not_angle"], len(ARM_IDX), 40), target_for(c, T, torch.tensor([[0.1, -0.1, 0.0, 0.05]], dtype=DT))


@pytest.mark.parametrize("cls_name", ["MC_PILCO", "MC_PILCO4PMS"])
def test_class_path(cls_name):
    M, T, hidden = 16, 8, (7, 3)
    sim = clf.sim_args(M, T)
    net, target = _arm_net(hidden, T)

    def rollout(fused):
        obj = _object(cls_name, net, hidden, target[:T])
        obj.fused_feedback = fused
        torch.manual_seed(5)
        with clf.normal_draws_on_the_cpu():
            st, inp = obj.apply_policy(**sim)
        assert obj.last_feedback_fused is fused and (obj.last_status is not None) is fused
        if fused:
            assert int(obj.last_status.item()) == 0
        cost, _ = obj.cost_function(st, inp, 0)
        cost.backward()
        return st.detach(), inp.detach(), [q.grad.clone() for q in obj.control_policy.mlp_parameters()]

    fs, fi, fg = rollout(True)
    ss, si, sg = rollout(False)  # fused_feedback off: the same object runs the step loop, seed for seed
    es, ei, eg = float((fs - ss).abs().max()), float((fi - si).abs().max()), [relmax(a, b) for a, b in zip(fg, sg)]
    print("%s, fused vs step: states %.3e inputs %.3e g_params %s" % (cls_name, es, ei, " ".join("%.3e" % e for e in eg)))
    assert es < STATE_TOL and ei < INPUT_TOL and max(eg) < GRAD_TOL
    assert float(fg[0][:, -len(ARM_IDX):].abs().max()) > 0

    short = _object(cls_name, net, hidden, target[:T - 2])  # rows < T_control steps: not fused -- and the step loop runs out of rows
    torch.manual_seed(5)
    with clf.normal_draws_on_the_cpu(), pytest.raises(IndexError):
        short.apply_policy(**sim)
    assert short.last_feedback_fused is False

    obj = _object(cls_name, net, hidden, target[:T])
    before = [q.detach().clone() for q in obj.control_policy.mlp_parameters()]
    torch.manual_seed(6)
    with clf.normal_draws_on_the_cpu(), contextlib.redirect_stdout(io.StringIO()):
        out = obj.reinforce_policy(**clf.reinforce_args(sim, T, 3))
    assert obj.last_feedback_fused is True
    costs = np.asarray(out[0], dtype=float).reshape(-1)
    assert costs.shape == (3,) and np.isfinite(costs).all()
    after = list(obj.control_policy.mlp_parameters())
    assert all(float((q.detach() - b).abs().max()) > 1e-4 for q, b in zip(after, before))  # every tensor moved
    assert float((after[0].detach() - before[0])[:, -len(ARM_IDX):].abs().max()) > 1e-4  # the error columns of W0 too


# ---- 9. two ranks on one device, Philox mode ------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401

    torch.cuda.set_device(dev())
    with rank_group(rank, world, port):
        M, T, hidden = 17, 6, (7, 3)
        net, target = _arm_net(hidden, T)
        res = {}
        for cls_name in ("MC_PILCO", "MC_PILCO4PMS"):
            obj = _object(cls_name, net, hidden, target[:T])
            obj.noise_mode = "philox"
            res[cls_name] = clf.sharded_step(MLP, obj, world, clf.sim_args(M, T))
        out_q.put((rank, res))


def test_two_rank_particle_sharding_matches_single_process():
    """MC_PILCO and MC_PILCO4PMS with the tracking policy under shard_particles (M = 17, T = 6, Philox): each rank's states are the matching
    slice of the one-process run bit for bit; the pooled cost, its std and the six parameter gradients agree to the bounds (another order of
    the sums)."""
    one = run_ranks(_rank, 1)
    two = run_ranks(_rank, 2)
    clf.two_ranks_match_one_process(MLP, one, two, GRAD_TOL, n_grads=6)


def test_packed_follows_the_target():
    """packed() is kept while nothing changes and rebuilt when the target is replaced: the launch then reads the new rows."""
    from mc_pilco_amd import ops

    c, pm, x0, eps, w, wu, target, params = arm_setup(5, 4, (5,), 3, deg=0)
    pol = policy(c, params, (5,), target[:4], trainable=False)
    first = pol.packed()
    assert pol.packed() is first and first.target.data_ptr() == pol.target_traj.data_ptr() and first.P == 10
    run = lambda q: ops.rollout_mlp(pm, q.packed(), clf.noise_buffer(eps), G(x0), 4)[1]
    a = run(pol)
    pol.target_traj = G(target[1:5])
    assert pol.packed() is not first and pol.packed().target.data_ptr() == pol.target_traj.data_ptr()
    b = run(pol)
    assert torch.equal(b, run(policy(c, params, (5,), target[1:5], trainable=False))) and float((a - b).abs().max()) > 1e-3


# ---- 10. saved record -----------------------------------------------------------------------------------------------------------------------------
def test_saved_record_refuses_in_place_changes():
    c, pm, x0, _, w, wu, target, params = arm_setup(2, 4, (5,), 3, deg=0)
    clf.saved_record_refuses_in_place_changes(MLP, pm, policy(c, params, (5,), target[:4]), x0, 4)
