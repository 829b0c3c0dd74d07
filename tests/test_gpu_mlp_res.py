"""GPU: the residual policy u = squash(PD(x, t) + net(x, t)) in the fused closed loop (mcp_rollout_mlp_res + mcp_rollout_mlp_res_bwd,
ops.rollout_mlp with an ops.PackedMLP that carries the PD term, MC_PILCO / MC_PILCO4PMS.apply_policy with a Policy.Residual_MLP_policy, and
that policy under particle sharding) against torch autograd through the oracle's step with the law written out
(tests/mlp_res_models.res_truth; conditioning and near misses checked by tests/test_mlp_res_cpu.py), and the bitwise contracts the residual
forms keep.

Bounds (those of tests/test_gpu_mlp_track.py): states and measurements 1e-9 absolute, inputs 2e-9 absolute, every parameter gradient -- both
gains included -- and g_x0 1e-9 relative to that tensor's largest magnitude."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
from closed_loop_family import MLP, PD
from closed_loop_family import meas_spec as spec
from gpu_helpers import DT, G, dev, relmax
from mlp_meas_models import meas_model
from mlp_models import SHAPES
from mlp_res_models import CASES, case_id, case_truth, gains_for, pd_target_for
from mlp_track_models import network, target_for
from pd_meas_models import pos_noise_for
from rank_harness import rank_group, run_ranks
from test_gpu_mlp_track import K, arm_setup, pair, raw
from test_gpu_mlp_track import policy as track_policy

pytestmark = pytest.mark.gpu
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9
TOLS = (STATE_TOL, INPUT_TOL, GRAD_TOL)


def _grad_text(e):
    """(one entry: requires_grad was on one tensor alone)"""
    if len(e) < 3:
        return "g " + " ".join("%.3e" % v for v in e)
    return "g_params " + " ".join("%.3e" % v for v in e[:-2]) + " g_sqrt_kp %.3e g_sqrt_kd %.3e" % tuple(e[-2:])


# the family of the residual policy: ops.rollout_mlp, the gradients of the network's tensors and of the two gains behind them
RES = clf.Family("rollout_mlp", lambda pol: list(pol.mlp_parameters()) + [pol.sqrt_Kp_gains, pol.sqrt_Kd_gains], _grad_text, MLP.models, MLP.pair_seed)


def policy(c, params, kp, kd, hidden, target, idx=None, angle=None, non_angle=None, squash=True, trainable=True, train_gains=True, u_max=1.0,
           pd_target=None, pos=None, vel=None, **kw):
    """A Residual_MLP_policy on the GPU (``idx`` None: errors on every component; ``pos`` None: the default layout)."""
    from mc_pilco_amd.policy_learning import Policy

    angle = c["angle"] if angle is None else angle
    non_angle = c["not_angle"] if non_angle is None else non_angle
    lists = {} if pos is None else dict(pd_pos_indices=pos, pd_vel_indices=vel)
    pol = Policy.Residual_MLP_policy(state_dim=c["S"], input_dim=c["U"], hidden_sizes=list(hidden), angle_indices=angle or None,
                                     non_angle_indices=non_angle or None, u_max=u_max, flg_squash=squash, weight_init=params, dtype=DT, device=dev(),
                                     target_traj=None if target is None else G(target), error_indices=idx, sqrt_Kp_gains=kp, sqrt_Kd_gains=kd,
                                     pd_target_traj=None if pd_target is None else G(pd_target), **lists, **kw)
    for q in pol.mlp_parameters():
        q.requires_grad_(trainable)
    for q in (pol.sqrt_Kp_gains, pol.sqrt_Kd_gains):
        q.requires_grad_(trainable and train_gains)
    return pol


def arm_res(M, T, hidden, seed, idx=None, N=37, deg=1):
    """test_gpu_mlp_track.arm_setup and the gains of the seed."""
    return arm_setup(M, T, hidden, seed, idx, N, deg) + gains_for(2, seed)


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
    other = ins["pd_target"] is not ins["target"]
    pol = policy(c, ins["params"], ins["kp"], ins["kd"], hidden, ins["target"], ins["idx"], ins["angle"], ins["non_angle"], squash=ins["squash"],
                 train_gains=not opt.get("fixed_gains"), pd_target=ins["pd_target"] if other else None, pos=opt.get("pos"), vel=opt.get("vel"),
                 flg_drop=ins["p"] > 0.0)
    pk = pol.packed()
    assert pk.P == ins["params"][0].shape[1] and pk.track_c().n == len(ins["idx"])
    assert pk.n_param == sum(q.numel() for q in ins["params"]) + 2 * c["U"] and (pk.res_target is pk.target) is (not other)
    assert (pk.res_pos, pk.res_vel) == (ins["pos"], ins["vel"])
    only = opt.get("only_grad")
    n_net = len(ins["params"])
    if only is not None:  # requires_grad on sqrt_kp alone: neither x0 nor any other tensor gets a gradient
        assert only == "kp"
        for q in RES.params(pol):
            q.requires_grad_(q is pol.sqrt_Kp_gains)
        only = n_net
    noise = ops.NoiseSpec(eps=G(ins["eps"]) if ins["sample"] else None, masks=None if ins["masks"] is None else K(ins["masks"]))
    got = RES.run(pm, pol, ins["x0"], T, noise, ins["w"], ins["wu"], ins["sample"], meas=spec(ins["ms"], ins["pos_noise"]), p_drop=ins["p"] or None,
                  x0_grad=only is None)
    if opt.get("fixed_gains"):  # the gains get nothing; everything else is compared
        assert got.grads[-2] is None and got.grads[-1] is None
        got = got._replace(grads=got.grads[:-2])
        truth = truth._replace(grads=truth.grads[:-2])
        clf.check_against(MLP, case_id(case), truth, got, TOLS)
        return
    clf.check_against(RES, case_id(case), truth, got, TOLS, only)


# ---- 2. no term through the new entries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
def test_no_term_through_the_new_entries_is_the_track_entries(measured, p):
    """res NULL and res->on == 0: the bits of mcp_rollout_mlp_track and its sweep -- states, inputs, measurements, slabs and g_x0 -- on
    M = 37 (three slabs)."""
    from mc_pilco_amd import hipabi as abi
    from mc_pilco_amd import ops

    M, T, hidden, idx = 37, 6, (7, 3), [3, 0, 1]
    c, pm, x0, eps, w, wu, target, params = arm_setup(M, T, hidden, 9, idx)
    pol = track_policy(c, params, hidden, target[:T], idx)
    mlp, tensors = pol.packed(), [q.detach() for q in pol.mlp_parameters()]
    pc, tc = mlp.to_c(*tensors), mlp.track_c()
    ms = meas_model("arm2", "all", 0.1) if measured else None
    pn = pos_noise_for(T, M, 2, 9) if measured else None
    keep = torch.empty(T, M, 10, dtype=DT).bernoulli_(0.75, generator=torch.Generator().manual_seed(8))
    nz = lambda: ops.NoiseSpec(eps=G(eps), masks=K(keep))
    run = lambda entries, head: raw(entries, [C.byref(pm.c), C.byref(pc), C.byref(tc)] + head, pm, nz(), p, G(x0), T, G(w), G(wu), spec(ms, pn), mlp.n_param)
    old = run(("mcp_rollout_mlp_track", "mcp_rollout_mlp_track_bwd"), [])
    assert tuple(old[3].shape) == (3, mlp.n_param) and float(old[3].abs().max()) > 0 and (old[2] is not None) is measured
    off = abi.MLPResidual()  # on == 0: nothing else of it is read
    for res in (None, C.byref(off)):
        new = run(("mcp_rollout_mlp_res", "mcp_rollout_mlp_res_bwd"), [res])
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(old, new))


# ---- 3. zero gains ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
def test_zero_gains_are_the_tracking_policy(measured):
    """sqrt_kp = sqrt_kd = 0 with the term on: the states and inputs of the tracking policy bit for bit (0 e vanishes under any contraction,
    and a + 0 == a); the network's gradients and g_x0 to the gradient bound; the gains' gradients are zero (2 * 0 * e * abar)."""
    M, T, hidden, idx = 17, 6, (7, 3), [3, 0, 1]
    c, pm, x0, eps, w, wu, target, params = arm_setup(M, T, hidden, 9, idx)
    zero = torch.zeros(2, dtype=DT)
    ms = meas_model("arm2", "all", 0.1) if measured else None
    pn = pos_noise_for(T, M, 2, 9) if measured else None
    a = MLP.run(pm, track_policy(c, params, hidden, target[:T], idx), x0, T, clf.noise_buffer(eps), w, wu, True, meas=spec(ms, pn))
    b = RES.run(pm, policy(c, params, zero, zero, hidden, target[:T], idx), x0, T, clf.noise_buffer(eps), w, wu, True, meas=spec(ms, pn))
    assert a.status == 0 and b.status == 0
    assert torch.equal(a.states, b.states) and torch.equal(a.inputs, b.inputs) and (not measured or torch.equal(a.meas, b.meas))
    eg = [relmax(q, r) for q, r in zip(b.grads[:-2], a.grads)] + [relmax(b.g_x0, a.g_x0)]
    print("zero gains: network gradients and g_x0 %s" % " ".join("%.3e" % e for e in eg))
    assert max(eg) < GRAD_TOL
    assert float(b.grads[-2].abs().max()) == 0 and float(b.grads[-1].abs().max()) == 0


# ---- 4. zero output layer -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
def test_zero_output_layer_is_the_pd_law(measured):
    """zero_output=True: the states and inputs of ops.rollout_pd with the same gains and target within the bounds, the gains' gradients
    within the gradient bound of the PD sweep's."""
    M, T, hidden = 17, 6, (7, 3)
    c, pm, x0, eps, w, wu, target, params, kp, kd = arm_res(M, T, hidden, 9)
    ms = meas_model("arm2", "all", 0.1) if measured else None
    pn = pos_noise_for(T, M, 2, 9) if measured else None
    pol = policy(c, params, kp, kd, hidden, target[:T], zero_output=True)
    assert float(pol.Wout.detach().abs().max()) == 0 and float(pol.bout.detach().abs().max()) == 0
    a = PD.run(pm, clf.controller(c, kp, kd, target[:T]), x0, T, clf.noise_buffer(eps), w, wu, True, meas=spec(ms, pn))
    b = RES.run(pm, pol, x0, T, clf.noise_buffer(eps), w, wu, True, meas=spec(ms, pn))
    assert a.status == 0 and b.status == 0
    es, ei = float((a.states - b.states).abs().max()), float((a.inputs - b.inputs).abs().max())
    eg = [relmax(b.grads[-2], a.grads[0]), relmax(b.grads[-1], a.grads[1]), relmax(b.g_x0, a.g_x0)]
    print("zero output layer vs rollout_pd: states %.3e inputs %.3e g_sqrt_kp %.3e g_sqrt_kd %.3e g_x0 %.3e (bit-equal states: %s)"
          % (es, ei, eg[0], eg[1], eg[2], torch.equal(a.states, b.states)))
    assert es < STATE_TOL and ei < INPUT_TOL and max(eg) < GRAD_TOL
    assert float(a.grads[0].abs().max()) > 0 and float(a.grads[1].abs().max()) > 0


# ---- 5. bit identities --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [17, 1041])  # 4 trajectories per workgroup, and 16
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_states_carry_the_bits_of_the_open_loop_launch(noise, M):
    T, hidden = 6, (7, 3)
    c, pm, x0, eps, w, wu, target, params, kp, kd = arm_res(M, T, hidden, 21)
    clf.three_way_bit_identity(RES, pm, policy(c, params, kp, kd, hidden, target[:T]), x0, eps, T, noise, sweep=(w, wu))


def test_states_carry_the_bits_of_the_open_loop_launch_measured():
    M, T, hidden = 17, 6, (7, 3)
    c, pm, x0, eps, w, wu, target, params, kp, kd = arm_res(M, T, hidden, 21)
    ms = meas_model("arm2", "all", 0.1)
    clf.three_way_bit_identity(RES, pm, policy(c, params, kp, kd, hidden, target[:T]), x0, eps, T, "eps", meas=lambda: spec(ms, pos_noise_for(T, M, 2, 21)),
                               sweep=(w, wu))


# ---- 6. Philox mode -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
def test_determinism_and_shard_invariance_under_philox(measured):
    """Two runs: the same bits.  Rows [a, b) launched with particle_offset = a, a a multiple of 16: states, inputs, g_x0 and the workgroups'
    slabs -- the gains' entries in their tails -- are bitwise those of one launch over all rows."""
    from mc_pilco_amd import ops

    M, T, cut, hidden = 37, 6, 16, (7, 3)
    c, pm, x0, _, w, wu, target, params, kp, kd = arm_res(M, T, hidden, 9, deg=0)
    pol = policy(c, params, kp, kd, hidden, target[:T])
    mlp = pol.packed()
    tensors = [q.detach().contiguous() for q in mlp.tensors()]
    ms = meas_model("arm2", "all", 0.1) if measured else None

    def run(a, b):
        nz, sp = ops.NoiseSpec(seed=4, call=2, particle_offset=a), spec(ms)
        st, inp, jac = ops._closed_launch(pm, mlp, tensors, nz, G(x0[a:b]), T, True, torch.zeros(1, dtype=torch.int32, device=dev()), True, sp)
        slabs, gx = ops._closed_sweep(pm, mlp, tensors, st, inp, jac, G(w[:, a:b]), G(wu[:, a:b]), True, True, sp, None if sp is None else sp.measured)
        torch.cuda.synchronize()
        return st, inp, slabs, gx

    st, inp, slabs, gx = run(0, M)
    assert tuple(slabs.shape) == (3, mlp.n_param) and all(float(slabs[i, -4:].abs().min()) > 0 for i in range(3))  # U = 2: kp | kd
    assert all(torch.equal(p, q) for p, q in zip(run(0, M), (st, inp, slabs, gx)))
    for a, b in ((0, cut), (cut, M)):
        sa, ia, la, xa = run(a, b)
        assert torch.equal(sa, st[:, a:b]) and torch.equal(ia, inp[:, a:b])
        assert torch.equal(la, slabs[a // 16:(b + 15) // 16]) and torch.equal(xa, gx[a:b])


def _split(tensors):
    """(network tensors, sqrt_kp, sqrt_kd) of central_differences' flat list."""
    return list(tensors[:-2]), tensors[-2], tensors[-1]


@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
def test_philox_mode_against_central_differences(measured):
    """Step 1e-6, bound 1e-5 relative with floor 1e-3, as tests/test_gpu_mlp_track.py: the first and the last entry of every tensor -- the
    two gains among them -- and of x0."""
    M, T, hidden, idx = 3, 6, (7, 3), [3, 0]
    c, pm, x0, _, w, wu, target, params, kp, kd = arm_res(M, T, hidden, 5, idx, deg=2)
    ms = meas_model("arm2", "all", 0.1) if measured else None

    def policy_of(tensors, trainable):
        net, p, d = _split(tensors)
        return policy(c, net, p, d, hidden, target[:T], idx, trainable=trainable)

    fam = RES if not measured else clf.Family("rollout_mlp", RES.params, RES.grad_text, MLP.models, MLP.pair_seed)
    if measured:  # (central_differences has no meas keyword: the family's op carries the measurement model, Philox position noise)
        fam.op = lambda *a, **kw: RES.op(*a, **dict(kw, meas=spec(ms)))
    tensors = params + [kp, kd]
    clf.central_differences(fam, pm, policy_of, tensors, x0, w, wu, T, clf.first_and_last_entries(tensors + [x0]), step=1e-6, bound=(1e-5, 1e-3))


# ---- 7. status word -----------------------------------------------------------------------------------------------------------------------------
def test_status_word():
    """A NaN gain, and a NaN in a row of the PD target, reach the inputs: MCP_STATUS_NAN.  A flag, not a fault (NaN operands only)."""
    from mc_pilco_amd import hipabi

    M, T, hidden = 5, 4, (5,)
    c, pm, x0, eps, w, wu, target, params, kp, kd = arm_res(M, T, hidden, 31, deg=0)
    bad = target[:T].clone()
    bad[2, 1] = float("nan")
    nan_gain = kp.clone()
    nan_gain[1] = float("nan")
    packed = lambda tensors, p, d, tgt, pd_tgt=None: policy(c, tensors, p, d, hidden, tgt, idx=[], trainable=False, pd_target=pd_tgt).packed()
    zero = packed([torch.zeros_like(q) for q in network(c, hidden, c["angle"], c["not_angle"], 0, 31)], torch.zeros(2, dtype=DT), torch.zeros(2, dtype=DT),
                  target[:T])  # zeros everywhere give u = 0 exactly
    net = network(c, hidden, c["angle"], c["not_angle"], 0, 31)
    good = packed(net, kp, kd, target[:T])
    clf.status_word(RES, pm, c, good, (packed(net, kp, kd, target[:T], bad), x0), zero, x0, eps, T)  # the network's target is clean: the PD row alone
    for sample in (False, True):
        nz = clf.noise_buffer(eps) if sample else None
        assert int(RES.op(pm, packed(net, nan_gain, kd, target[:T]), nz, G(x0), T, particle_pred=sample)[-1].item()) & hipabi.STATUS_NAN
        assert int(RES.op(pm, packed(net, kp, nan_gain, target[:T]), nz, G(x0), T, particle_pred=sample)[-1].item()) & hipabi.STATUS_NAN


# ---- 8. class path, "reference" noise mode --------------------------------------------------------------------------------------------------------
ARM_IDX = [1, 3, 0]
ARM_KP, ARM_KD = [1.4, 1.6], [0.6, 0.7]


def _object(cls_name, params, hidden, target, train_gains=True):
    from mc_pilco_amd.policy_learning import Policy

    par = clf.arm_mlp_par(params, hidden, target_traj=G(target), error_indices=ARM_IDX, sqrt_Kp_gains=np.asarray(ARM_KP), sqrt_Kd_gains=np.asarray(ARM_KD),
                          flg_train_gains=train_gains)
    return clf.arm_object(Policy.Residual_MLP_policy, par, clf.ARM_PMS if cls_name == "MC_PILCO4PMS" else None)


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
        return st.detach(), inp.detach(), [q.grad.clone() for q in RES.params(obj.control_policy)]

    fs, fi, fg = rollout(True)
    ss, si, sg = rollout(False)  # fused_feedback off: the same object runs the step loop, seed for seed
    es, ei, eg = float((fs - ss).abs().max()), float((fi - si).abs().max()), [relmax(a, b) for a, b in zip(fg, sg)]
    print("%s, fused vs step: states %.3e inputs %.3e %s" % (cls_name, es, ei, RES.grad_text(eg)))
    assert es < STATE_TOL and ei < INPUT_TOL and max(eg) < GRAD_TOL
    assert len(fg) == 8 and float(fg[-2].abs().max()) > 0 and float(fg[-1].abs().max()) > 0

    for train in (True, False):
        obj = _object(cls_name, net, hidden, target[:T], train_gains=train)
        pol = obj.control_policy
        before = [q.detach().clone() for q in RES.params(pol)]
        torch.manual_seed(6)
        with clf.normal_draws_on_the_cpu(), contextlib.redirect_stdout(io.StringIO()):
            out = obj.reinforce_policy(**clf.reinforce_args(sim, T, 3))
        assert obj.last_feedback_fused is True
        costs = np.asarray(out[0], dtype=float).reshape(-1)
        assert costs.shape == (3,) and np.isfinite(costs).all()
        after = RES.params(pol)
        assert all(float((q.detach() - b).abs().max()) > 1e-4 for q, b in zip(after[:-2], before[:-2]))  # the network moved
        if train:
            assert all(float((q.detach() - b).abs().max()) > 1e-4 for q, b in zip(after[-2:], before[-2:]))  # and so did the gains
        else:
            assert all(torch.equal(q.detach(), b) for q, b in zip(after[-2:], before[-2:]))  # fixed gains: bit-equal


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
            res[cls_name] = clf.sharded_step(RES, obj, world, clf.sim_args(M, T))
        out_q.put((rank, res))


def test_two_rank_particle_sharding_matches_single_process():
    """MC_PILCO and MC_PILCO4PMS with the residual policy under shard_particles (M = 17, T = 6, Philox): each rank's states are the matching
    slice of the one-process run bit for bit; the pooled cost, its std and the eight parameter gradients -- the two gains' among them --
    agree to the bounds (another order of the sums)."""
    one = run_ranks(_rank, 1)
    two = run_ranks(_rank, 2)
    clf.two_ranks_match_one_process(RES, one, two, GRAD_TOL, n_grads=8)


# ---- 10. packed() and the saved record --------------------------------------------------------------------------------------------------------
def test_packed_follows_the_gains_and_the_pd_target():
    """packed() is kept while nothing changes and rebuilt when a gain tensor or the PD target is replaced: the launch then reads the new one.
    An optimizer's in-place update of a gain needs no rebuild."""
    from mc_pilco_amd import ops

    c, pm, x0, eps, w, wu, target, params, kp, kd = arm_res(5, 4, (5,), 3, deg=0)
    pol = policy(c, params, kp, kd, (5,), target[:4], trainable=False, pd_target=pd_target_for(c, 4, x0)[:4])
    first = pol.packed()
    assert pol.packed() is first and first.res_target.data_ptr() == pol.pd_target_traj.data_ptr() and first.res_target is not first.target
    run = lambda q: ops.rollout_mlp(pm, q.packed(), clf.noise_buffer(eps), G(x0), 4)[1]
    a = run(pol)
    with torch.no_grad():
        pol.sqrt_Kp_gains.mul_(1.5)
    assert pol.packed() is first
    b = run(pol)
    assert float((a - b).abs().max()) > 1e-3
    pol.sqrt_Kd_gains = torch.nn.Parameter(G(2.0 * kd), requires_grad=False)
    second = pol.packed()
    assert second is not first
    d = run(pol)
    assert torch.equal(d, run(policy(c, params, 1.5 * kp, 2.0 * kd, (5,), target[:4], trainable=False, pd_target=pd_target_for(c, 4, x0)[:4])))
    assert float((d - b).abs().max()) > 1e-3
    pol.pd_target_traj = G(pd_target_for(c, 4, x0)[1:5])
    assert pol.packed() is not second and pol.packed().res_target.data_ptr() == pol.pd_target_traj.data_ptr()
    e = run(pol)
    assert torch.equal(e, run(policy(c, params, 1.5 * kp, 2.0 * kd, (5,), target[:4], trainable=False, pd_target=pd_target_for(c, 4, x0)[1:5])))
    assert float((e - d).abs().max()) > 1e-3


def test_saved_record_refuses_in_place_changes():
    c, pm, x0, _, w, wu, target, params, kp, kd = arm_res(2, 4, (5,), 3, deg=0)
    clf.saved_record_refuses_in_place_changes(RES, pm, policy(c, params, kp, kd, (5,), target[:4]), x0, 4)
