"""GPU: the fused closed loop under the tanh-MLP policy on a simulated measurement (mcp_rollout_mlp_meas + mcp_rollout_mlp_meas_bwd,
ops.rollout_mlp(meas=...), MC_PILCO4PMS.apply_policy with a Policy.MLP_policy, and the MLP policy under particle sharding) against torch
autograd through the oracle's step with the measurement and the network written out (tests/mlp_meas_models.mlp_meas_truth; conditioning and
sensitivity checked by tests/test_mlp_meas_cpu.py), and the bitwise contracts it shares with mcp_rollout_mlp and the open-loop kernels.

Bounds (tests/test_gpu_mlp_rollout.py, on the oracle's own Kinv / alpha): states and measurements 1e-9 absolute, inputs
2e-9 absolute, every parameter gradient and g_x0 1e-9 relative to that tensor's largest magnitude."""
import contextlib
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
from closed_loop_family import MLP, controller, policy
from closed_loop_family import meas_spec as spec
from closed_loop_family import noise_of as _noise
from gpu_helpers import G, dev, relmax
from mlp_meas_models import CASES, case_id, case_truth, meas_model, mlp_meas_truth
from mlp_models import SHAPES, inputs_for, network
from pd_meas_models import pos_noise_for
from rank_harness import rank_group, run_ranks

pytestmark = pytest.mark.gpu
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9
TOLS = (STATE_TOL, INPUT_TOL, GRAD_TOL)


def pair(shape, N, deg, vs=None):
    """MLP.pair with the sampling time a measurement model needs on the delta-state layout too."""
    return MLP.pair(shape, N, deg, vs, measured=True)


# ---- 1. parity with the truth ---------------------------------------------------------------------------------------------------------
# Measured on an MI355X (the largest figure over the table, per quantity): see DESIGN section 4.10.
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_truth(case):
    mode, shape, deg, N, T, M, hidden, variant, opt = case
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
    got = MLP.run(pm, pol, ins["x0"], T, clf.noise_buffer(ins["eps"]) if sample else None, ins["w"], ins["wu"], sample,
                  meas=spec(ins["ms"], ins["pos_noise"]), x0_grad=only is None)
    clf.check_against(MLP, case_id(case), truth, got, TOLS, only)


# ---- 2. bit identities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_plain_launch_recording_launch_and_open_loop_launch_carry_the_same_bits(noise):
    c, m, pm = pair("arm2", 37, 1)
    M, T, hidden = 17, 6, (7, 3)
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=21)
    ms = meas_model("arm2")
    pn = pos_noise_for(T, M, 2, seed=21)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 21), hidden)
    clf.three_way_bit_identity(MLP, pm, pol, x0, eps, T, noise, meas=lambda: spec(ms, None if noise == "philox" else pn), sweep=(w, wu))


@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_no_pairs_is_the_unmeasured_launch(noise):
    """A measurement model without pairs: the kernels of mcp_rollout_mlp / mcp_rollout_mlp_bwd, the same bits, gradients included."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 2)
    M, T, hidden = 17, 6, (7, 3)
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=9)
    sample = noise != "mean"
    none = dict(pos=[], vel=[], std=[], b=[0.42, 0.31], a=[1.25, -0.38])
    out = []
    for ms in (None, none):
        pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 9), hidden)
        xg = G(x0).requires_grad_(True)
        st, inp, status = ops.rollout_mlp(pm, pol.packed(), _noise(noise, eps), xg, T, particle_pred=sample, meas=None if ms is None else spec(ms))
        ((G(w) * st).sum() + (G(wu) * inp).sum()).backward()
        assert int(status.item()) == 0
        out.append([st.detach(), inp.detach(), xg.grad] + [q.grad for q in pol.mlp_parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*out))


@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_the_two_tile_widths_carry_the_same_bits(noise):
    """M = 17 runs 4 trajectories per workgroup, M = 1041 runs 16 (MLP_SMALL_SWARM): the particles they share carry the same states, inputs
    and measurements."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 1)
    T, hidden, big, small = 4, (7, 3), 1041, 17
    x0, _, _, _, eps, _, _ = inputs_for(c, big, T, seed=21)
    ms = meas_model("arm2")
    pn = pos_noise_for(T, big, 2, seed=21)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 21), hidden, trainable=False)
    sample = noise != "mean"
    out = []
    for M in (big, small):
        sp = spec(ms, None if noise == "philox" else pn[:, :M])
        st, inp, status = ops.rollout_mlp(pm, pol.packed(), _noise(noise, eps[:, :M]), G(x0[:M]), T, particle_pred=sample, meas=sp)
        assert int(status.item()) == 0
        out.append((st, inp, sp.measured))
    assert all(torch.equal(a[:, :small], b) for a, b in zip(*out))
    assert float((out[0][2][1:, :, :2] - out[0][0][1:, :, :2]).abs().min()) > 0


# ---- 3. the smaller rungs -------------------------------------------------------------------------------------------------------------------
# Held to the bounds of the N = 300 case of CASES.  A swarm of 5 enters the ladder at 4 trajectories per workgroup (MLP_SMALL_SWARM): the
# recording launch runs 4 at N = 640 and one at N = 2600, the launch without a record 4.
def _rung_case(N):
    c, m, pm = pair("arm2", N, 0)
    M, T, hidden = 5, 3, (16,)
    seed = T * 100 + M
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=seed)
    ms = meas_model("arm2")
    pn = pos_noise_for(T, M, 2, seed=seed)
    params = network(c, hidden, c["angle"], c["not_angle"], seed)
    torch.set_num_threads(1)
    truth = clf.mlp_truth_of(mlp_meas_truth("arm2", m, x0, params, eps, pn, w, wu, True, c["angle"], c["not_angle"], ms))
    assert truth.vmin > 0.0
    return pm, lambda **kw: policy(c, params, hidden, **kw), x0, eps, T, w, wu, truth, lambda: spec(ms, pn)


@pytest.mark.parametrize("N", [640, 2600])
def test_the_smaller_tiles_of_the_recording_form(N):
    """Sampled, degree 0, M = 5, T = 3 on arm2, every joint measured.  Status 0; states, inputs and measurements carry the bits of the launch
    without a record, whose states carry the bits of the open-loop launch on its inputs; everything against the truth."""
    pm, pol, x0, eps, T, w, wu, truth, meas = _rung_case(N)
    clf.rung_of_the_recording_form(MLP, "rung N %d" % N, pm, pol(), x0, eps, T, w, wu, truth, TOLS, meas)


def test_the_four_trajectory_tile_without_a_record():
    """Nothing requires grad: status 0, the states carry the bits of the open-loop launch on the inputs; states, inputs and measurements
    against the truth.  (No record, so no gradient to compare.)"""
    pm, pol, x0, eps, T, w, wu, truth, meas = _rung_case(640)
    clf.four_trajectory_tile_without_a_record(MLP, "rung N 640", pm, pol(trainable=False), x0, eps, T, truth, TOLS, meas)


# ---- 4. shard invariance of the op ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["buffers", "philox"])
def test_shard_invariance(noise):
    """M = 17 in one call against 16 + 1 with particle_offset (buffers: the matching slices): states, inputs, meas and g_x0 are bitwise those
    of the one call, and so are the workgroups' slabs -- the split is at a multiple of 16, a slab depends on its own trajectories alone.  Two
    runs of the one call give the same bits."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    M, T, cut, hidden = 17, 6, 16, (7, 3)
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=9)
    ms = meas_model("arm2")
    pn = pos_noise_for(T, M, 2, seed=9)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 9), hidden)
    mlp = pol.packed()
    tensors = [q.detach() for q in pol.mlp_parameters()]

    def run(a, b):
        if noise == "buffers":
            nz, sp = ops.NoiseSpec(eps=G(eps[:, a:b])), spec(ms, pn[:, a:b])
        else:
            nz, sp = ops.NoiseSpec(seed=4, call=2, particle_offset=a), spec(ms)
        status = torch.zeros(1, dtype=torch.int32, device=dev())
        st, inp, jac = ops._closed_launch(pm, mlp, tensors, nz, G(x0[a:b]), T, True, status, True, sp)
        slabs, gx = ops._closed_sweep(pm, mlp, tensors, st, inp, jac, G(w[:, a:b]), G(wu[:, a:b]), True, True, sp, sp.measured)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        return st, inp, sp.measured, slabs, gx

    whole = run(0, M)
    assert tuple(whole[3].shape) == (2, mlp.n_param) and all(float(whole[3][i].abs().max()) > 0 for i in range(2))
    assert all(torch.equal(p, q) for p, q in zip(whole, run(0, M)))
    for a, b in ((0, cut), (cut, M)):
        st, inp, ym, slabs, gx = run(a, b)
        assert torch.equal(st, whole[0][:, a:b]) and torch.equal(inp, whole[1][:, a:b]) and torch.equal(ym, whole[2][:, a:b])
        assert torch.equal(slabs, whole[3][a // 16:(b + 15) // 16]) and torch.equal(gx, whole[4][a:b])


# ---- 5. Philox position noise ---------------------------------------------------------------------------------------------------------------
def test_philox_position_noise_is_the_pd_forms():
    """The position noise recovered as (meas[t][p] - states[t][p]) / std equals the noise recovered the same way from mcp_rollout_pd_meas at
    the same seed, call and particles (an offset included).  Under policies that return u = 0 exactly (zero gains, zero weights) the two
    launches evolve the same states, so the recovery rounds alike: bound 4.4e-16.  Under the cases' own policies the states differ, and each
    recovery is within ulp(1) / 2 / std = 1.12e-15 of the draw while |y[p]| < 1 (one rounding of x + std n, the subtraction and the division
    adding less than a tenth of that): the two agree to 2.3e-15."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    M, T, off, hidden, std = 5, 6, 3, (7, 3), 0.1
    x0, kp, kd, target, _, _, _ = inputs_for(c, M, T, seed=13)
    ms = dict(meas_model("arm2"), std=[std, std])
    params = network(c, hidden, c["angle"], c["not_angle"], 13)
    nz = lambda: ops.NoiseSpec(seed=21, call=7, particle_offset=off)

    def recovered(zero):
        sm, sd = spec(ms), spec(ms)
        net = [torch.zeros_like(q) for q in params] if zero else params
        gains = (torch.zeros_like(kp), torch.zeros_like(kd)) if zero else (kp, kd)
        with torch.no_grad():
            st, inp, status = ops.rollout_mlp(pm, policy(c, net, hidden, trainable=False).packed(), nz(), G(x0), T, particle_pred=True, meas=sm)
            sp_, ip_, status_p = ops.rollout_pd(pm, controller(c, gains[0], gains[1], target, trainable=False).packed(), nz(), G(x0), T,
                                                particle_pred=True, meas=sd)
        assert int(status.item()) == 0 and int(status_p.item()) == 0
        assert float(sm.measured[:, :, :2].abs().max()) < 1.0 and float(sd.measured[:, :, :2].abs().max()) < 1.0
        if zero:
            assert float(inp.abs().max()) == 0.0 and float(ip_.abs().max()) == 0.0 and torch.equal(st, sp_)
        return (sm.measured[1:, :, :2] - st[1:, :, :2]) / std, (sd.measured[1:, :, :2] - sp_[1:, :, :2]) / std

    a, b = recovered(True)
    print("recovered position noise, MLP vs PD, u = 0: %.3e" % float((a - b).abs().max()))
    assert float(a.abs().max()) > 0.5 and float((a - b).abs().max()) <= 4.4e-16
    a2, b2 = recovered(False)
    print("recovered position noise, MLP vs PD, the policies of the cases: %.3e" % float((a2 - b2).abs().max()))
    assert float((a2 - b2).abs().max()) < 2.3e-15 and float((a2 - a).abs().max()) < 2.3e-15


# ---- 6. class path, one process -----------------------------------------------------------------------------------------------------------
def _object(cls_name, params, hidden):
    """MC_PILCO, or MC_PILCO4PMS (both joints measured, a first-order filter with memory, fc = 0.3, position noise on both), over the model
    and with the MLP policy of tests/test_gpu_mlp_rollout.py's class path."""
    from mc_pilco_amd.policy_learning import Policy

    return clf.arm_object(Policy.MLP_policy, clf.arm_mlp_par(params, hidden), clf.ARM_PMS if cls_name == "MC_PILCO4PMS" else None)


def _pms_object(params, hidden, M):
    return _object("MC_PILCO4PMS", params, hidden)


_sim = clf.sim_args


def test_class_path():
    M, T, c = 16, 8, SHAPES["arm2"]
    sim = _sim(M, T)
    net = lambda hidden: network(c, hidden, c["angle"], c["not_angle"], 40)

    def rollout(fused, hidden=(7, 3), expect=None, edit=None):
        obj = _pms_object(net(hidden), hidden, M)
        obj.fused_feedback = fused
        if edit:
            edit(obj)
        torch.manual_seed(5)
        with clf.normal_draws_on_the_cpu():
            st, inp = obj.apply_policy(**sim)
        expect = fused if expect is None else expect
        assert obj.last_feedback_fused is expect and (obj.last_status is not None) is expect
        if expect:
            assert int(obj.last_status.item()) == 0
        cost, _ = obj.cost_function(st, inp, 0)
        cost.backward()
        return st.detach(), inp.detach(), [q.grad.clone() for q in obj.control_policy.mlp_parameters()]

    fs, fi, fg = rollout(True)
    ss, si, sg = rollout(False)  # fused_feedback off: the same object runs the step loop, seed for seed
    es, ei, eg = float((fs - ss).abs().max()), float((fi - si).abs().max()), [relmax(a, b) for a, b in zip(fg, sg)]
    print("class path, fused vs step: states %.3e inputs %.3e g_params %s" % (es, ei, " ".join("%.3e" % e for e in eg)))
    assert es < STATE_TOL and ei < INPUT_TOL and max(eg) < GRAD_TOL
    # what the kernels do not take falls through to the step loop
    rollout(True, hidden=(65,), expect=False)  # a width beyond MCP_MAX_HIDDEN

    def no_layout(obj):
        obj.model_learning.has_fused_layout = lambda: False

    def unfused(obj):
        obj.fused = False

    rollout(True, expect=False, edit=no_layout)  # a model without a fused layout
    rollout(True, expect=False, edit=unfused)  # fused = False

    obj = _pms_object(net((7, 3)), (7, 3), M)
    before = [q.detach().clone() for q in obj.control_policy.mlp_parameters()]
    torch.manual_seed(6)
    with clf.normal_draws_on_the_cpu(), contextlib.redirect_stdout(io.StringIO()):
        out = obj.reinforce_policy(**clf.reinforce_args(sim, T, 3))
    assert obj.last_feedback_fused is True
    costs = np.asarray(out[0], dtype=float).reshape(-1)
    assert costs.shape == (3,) and np.isfinite(costs).all()
    assert all(float((q.detach() - b).abs().max()) > 1e-4 for q, b in zip(obj.control_policy.mlp_parameters(), before))  # every tensor moved


# ---- 7. class path, two ranks on one device -------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401

    torch.cuda.set_device(dev())
    with rank_group(rank, world, port):
        M, T, hidden, c = 17, 6, (7, 3), SHAPES["arm2"]
        res = {}
        for cls_name in ("MC_PILCO", "MC_PILCO4PMS"):
            obj = _object(cls_name, network(c, hidden, c["angle"], c["not_angle"], 40), hidden)
            obj.noise_mode = "philox"
            res[cls_name] = clf.sharded_step(MLP, obj, world, _sim(M, T))
        out_q.put((rank, res))


def test_two_rank_particle_sharding_matches_single_process():
    """MC_PILCO and MC_PILCO4PMS with the MLP policy under shard_particles (M = 17, T = 6, Philox): each rank's states are the matching slice
    of the one-process run bit for bit; the pooled cost, its std and the six parameter gradients agree to the bounds (another order of the
    sums)."""
    one = run_ranks(_rank, 1)
    two = run_ranks(_rank, 2)
    clf.two_ranks_match_one_process(MLP, one, two, GRAD_TOL, n_grads=6)


# ---- 8. saved record -------------------------------------------------------------------------------------------------------------------------
def test_saved_record_refuses_in_place_changes():
    c, m, pm = pair("arm2", 37, 0)
    x0, _, _, _, _, w, wu = inputs_for(c, 2, 4, seed=3)
    ms = meas_model("arm2")
    pn = pos_noise_for(4, 2, 2, seed=3)
    pol = policy(c, network(c, (5,), c["angle"], c["not_angle"], 3), (5,))
    clf.saved_record_refuses_in_place_changes(MLP, pm, pol, x0, 4, meas=lambda: spec(ms, pn), weights=(w, wu))
