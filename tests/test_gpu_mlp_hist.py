"""GPU: the tanh-MLP policy WITH MEMORY in the fused closed loop (mcp_rollout_mlp_hist + mcp_rollout_mlp_hist_bwd, ops.rollout_mlp with an
ops.PackedMLP that carries ``history``, MC_PILCO.apply_policy with a Policy.MLP_policy(history=H), and that policy under particle
sharding; the forms on the true state -- a measured form is not built) against torch autograd through the oracle's step with the network and its window written out
(tests/mlp_hist_models.hist_truth; near misses checked by tests/test_mlp_hist_truth_cpu.py), and the bitwise contracts the history forms keep.

Bounds (the family's own, tests/test_gpu_mlp_rollout.py): states and measurements 1e-9 absolute, inputs 2e-9 absolute, every parameter
gradient and g_x0 1e-9 relative to that tensor's largest magnitude."""
import ctypes as C

import pytest
import torch

import closed_loop_family as clf
from closed_loop_family import MLP
from closed_loop_family import meas_spec as spec
from gpu_helpers import DT, G, dev, relmax
from mlp_hist_models import CASES, case_id, case_truth, gains_for, network, target_for
from mlp_meas_models import meas_model
from mlp_meas_models import pm as pd_meas
from mlp_models import SHAPES, inputs_for
from rank_harness import rank_group, run_ranks

pytestmark = pytest.mark.gpu
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9
TOLS = (STATE_TOL, INPUT_TOL, GRAD_TOL)


def _grad_text(e):
    return "g " + " ".join("%.3e" % v for v in e)


# the family of a policy with the PD term: the gradients of the network's tensors and of the two gains behind them
RES = clf.Family("rollout_mlp", lambda pol: list(pol.mlp_parameters()) + [pol.sqrt_Kp_gains, pol.sqrt_Kd_gains], _grad_text, MLP.models, MLP.pair_seed)
HIST = clf.Family("rollout_mlp", MLP.params, _grad_text, MLP.models, MLP.pair_seed)


def pair(shape, N, deg):
    """(cfg, oracle model, PackedModel), with the sampling time a measurement needs."""
    return MLP.pair(shape, N, deg, measured=True)


def K(masks):
    return masks.to(torch.uint8).to(dev()).contiguous()


def policy(c, params, hidden, H, angle=None, non_angle=None, target=None, idx=(), res=None, trainable=True, flg_drop=False):
    """An MLP_policy(history=H) on the GPU, or with ``res`` = dict(kp, kd, pos, vel, target) a Residual_MLP_policy with trainable gains."""
    from mc_pilco_amd.policy_learning import Policy

    angle = c["angle"] if angle is None else angle
    non_angle = c["not_angle"] if non_angle is None else non_angle
    kw = dict(state_dim=c["S"], input_dim=c["U"], hidden_sizes=list(hidden), angle_indices=angle or None, non_angle_indices=non_angle or None, u_max=1.0,
              flg_squash=True, weight_init=params, dtype=DT, device=dev(), flg_drop=flg_drop, history=H)
    if len(idx):
        kw.update(target_traj=G(target), error_indices=list(idx))
    if res is None:
        pol = Policy.MLP_policy(**kw)
    else:
        pol = Policy.Residual_MLP_policy(**kw, sqrt_Kp_gains=res["kp"], sqrt_Kd_gains=res["kd"], flg_train_gains=True, pd_target_traj=G(res["target"]),
                                         pd_pos_indices=res["pos"], pd_vel_indices=res["vel"])
    for q in pol.parameters():
        q.requires_grad_(trainable)
    return pol


def policy_of_case(c, ins, hidden, **kw):
    return policy(c, ins["params"], hidden, ins["H"], ins["angle"], ins["non_angle"], ins["target"], ins["idx"], ins["res"], flg_drop=ins["p"] > 0.0, **kw)


def arm_setup(M, T, hidden, H, seed, N=37, deg=1, idx=()):
    """arm2 at (N, deg): (cfg, PackedModel, x0, eps, w, wu, network [h0][6 H + len(idx)], target [T, S])."""
    c, m, pm = pair("arm2", N, deg)
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=seed)
    return c, pm, x0, eps, w, wu, network(c, hidden, 6 * H + len(idx), seed), target_for(c, T, x0)


# ---- 1. parity with the truth ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_truth(case):
    from mc_pilco_amd import ops

    mode, shape, deg, N, T, M, hidden, H, opt = case
    c, m, ins, truth = case_truth(case)
    truth = clf.mlp_truth_of(truth)
    _, _, pm = pair(shape, N, deg)
    if ins["sample"] and T > 1:
        assert truth.vmin > 0.0
    pol = policy_of_case(c, ins, hidden)
    pk = pol.packed()
    assert pk.history == H and pk.P == ins["params"][0].shape[1] == H * ins["P0"] + len(ins["idx"]) and pk.hist_c().h == H
    fam = RES if ins["res"] else HIST
    only = opt.get("only_grad")
    if only is not None:  # requires_grad on one tensor alone: neither x0 nor the other parameters get a gradient
        for i, q in enumerate(fam.params(pol)):
            q.requires_grad_(i == only)
    noise = ops.NoiseSpec(eps=G(ins["eps"]) if ins["sample"] else None, masks=None if ins["masks"] is None else K(ins["masks"]))
    got = fam.run(pm, pol, ins["x0"], T, noise, ins["w"], ins["wu"], ins["sample"], p_drop=ins["p"] or None, x0_grad=only is None)
    clf.check_against(fam, case_id(case), truth, got, TOLS, only)
    assert pol._window is None and pol._t_prev is None  # the launch never touches the object's window


# ---- 3. bit identities ---------------------------------------------------------------------------------------------------------------------------
def raw(entries, head, pm, noise, p, x0, T, w, wu, meas, n_param):
    """A recording launch and its sweep through the C entries ``entries`` as they are, ``head``: the arguments between the model and the
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
    args = [C.byref(pm.c)] + head + [marg[0] if marg else None, C.byref(nz), float(p), M, T]
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
def test_no_memory_through_the_new_entries_is_the_residual_entries(measured, p):
    """hist NULL and hist->h == 1: the bits of mcp_rollout_mlp_res and its sweep -- states, inputs, measurements, slabs (the gains' tails
    included) and g_x0 -- on M = 37 (three slabs), with the track and the PD term on."""
    from mc_pilco_amd import hipabi as abi
    from mc_pilco_amd import ops

    M, T, hidden, idx = 37, 6, (7, 3), [3, 0, 1]
    c, pm, x0, eps, w, wu, params, target = arm_setup(M, T, hidden, 1, 9, idx=idx)
    kp, kd = gains_for(2, 9)
    pol = policy(c, params, hidden, 1, target=target, idx=idx, res=dict(kp=kp, kd=kd, pos=[0, 1], vel=[2, 3], target=target), trainable=False)
    mlp = pol.packed()
    pc = mlp.to_c(*[q.detach().contiguous() for q in mlp.tensors()])
    tc, rc = mlp.track_c(), mlp.res_c()
    ms = meas_model("arm2", "all", 0.1) if measured else None
    pn = pd_meas.pos_noise_for(T, M, 2, 9) if measured else None
    keep = torch.empty(T, M, 10, dtype=DT).bernoulli_(0.75, generator=torch.Generator().manual_seed(8))
    nz = lambda: ops.NoiseSpec(eps=G(eps), masks=K(keep))
    run = lambda entries, head: raw(entries, [C.byref(pc)] + head + [C.byref(tc), C.byref(rc)], pm, nz(), p, G(x0), T, G(w), G(wu), spec(ms, pn), mlp.n_param)
    old = run(("mcp_rollout_mlp_res", "mcp_rollout_mlp_res_bwd"), [])
    assert tuple(old[3].shape) == (3, mlp.n_param) and float(old[3].abs().max()) > 0 and (old[2] is not None) is measured
    one = abi.MLPHist()
    one.h = 1
    for hist in (None, C.byref(one)):
        new = run(("mcp_rollout_mlp_hist", "mcp_rollout_mlp_hist_bwd"), [hist])
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(old, new))


@pytest.mark.parametrize("M", [17, 1041])  # 4 trajectories per workgroup, and 16
@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_states_carry_the_bits_of_the_open_loop_launch(noise, M):
    """Plain against recording launch; the states against mcp_rollout_open fed the launch's own inputs[:T - 1]."""
    T, hidden, H = 6, (7, 3), 3
    c, pm, x0, eps, w, wu, params, _ = arm_setup(M, T, hidden, H, 21)
    clf.three_way_bit_identity(HIST, pm, policy(c, params, hidden, H), x0, eps, T, noise, sweep=(w, wu))


@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_the_two_tile_widths_carry_the_same_bits(noise):
    """M = 17 runs 4 trajectories per workgroup, M = 1041 runs 16 (MLP_SMALL_SWARM): the particles they share carry the same states and
    inputs (the body of tests/test_gpu_mlp_meas.py's test of that name, on the true state)."""
    T, hidden, H, big, small = 4, (7, 3), 3, 1041, 17
    c, pm, x0, eps, _, _, params, _ = arm_setup(big, T, hidden, H, 21)
    pol = policy(c, params, hidden, H, trainable=False)
    sample = noise != "mean"
    out = []
    for M in (big, small):
        st, inp, status = HIST.op(pm, pol.packed(), clf.noise_of(noise, eps[:, :M]), G(x0[:M]), T, particle_pred=sample)
        assert int(status.item()) == 0
        out.append((st, inp))
    assert all(torch.equal(a[:, :small], b) for a, b in zip(*out))


def test_determinism_and_shard_invariance_under_philox():
    """Two runs: the same bits.  Rows [a, b) launched with particle_offset = a -- a 16 + 1 split -- carry the states, inputs, g_x0 and
    workgroup slabs of one launch over all 17 rows, bit for bit: a trajectory's window is its own."""
    from mc_pilco_amd import ops

    M, T, cut, hidden, H = 17, 6, 16, (7, 3), 4
    c, pm, x0, _, w, wu, params, _ = arm_setup(M, T, hidden, H, 9, deg=0)
    mlp = policy(c, params, hidden, H).packed()
    tensors = [q.detach().contiguous() for q in mlp.tensors()]

    def run(a, b):
        nz = ops.NoiseSpec(seed=4, call=2, particle_offset=a)
        st, inp, jac = ops._closed_launch(pm, mlp, tensors, nz, G(x0[a:b]), T, True, torch.zeros(1, dtype=torch.int32, device=dev()), True)
        slabs, gx = ops._closed_sweep(pm, mlp, tensors, st, inp, jac, G(w[:, a:b]), G(wu[:, a:b]), True, True)
        torch.cuda.synchronize()
        return st, inp, slabs, gx

    st, inp, slabs, gx = run(0, M)
    assert tuple(slabs.shape) == (2, mlp.n_param) and all(float(slabs[i].abs().max()) > 0 for i in range(2))
    assert all(torch.equal(p, q) for p, q in zip(run(0, M), (st, inp, slabs, gx)))
    for a, b in ((0, cut), (cut, M)):
        sa, ia, la, xa = run(a, b)
        assert torch.equal(sa, st[:, a:b]) and torch.equal(ia, inp[:, a:b])
        assert torch.equal(la, slabs[a // 16:(b + 15) // 16]) and torch.equal(xa, gx[a:b])


# ---- 4. central differences -------------------------------------------------------------------------------------------------------------------------
def test_philox_mode_against_central_differences():
    """Step 1e-6, bound 1e-5 relative with floor 1e-3 (the family's, tests/test_gpu_mlp_track.py): entries of W0's history columns -- one in
    every older block, plain, sine and cosine columns among them -- and the first and last entry of x0."""
    M, T, hidden, H = 3, 6, (7, 3), 4
    c, pm, x0, _, w, wu, params, _ = arm_setup(M, T, hidden, H, 5, deg=2)
    P = 6 * H
    checks = [("W0[%d][%d]" % (j, col), 0, j * P + col) for j, col in ((0, 6), (2, 9), (4, 12), (1, 16), (6, 18), (3, 23))]
    checks += [("x0 entry %d" % e, len(params), e) for e in (0, x0.numel() - 1)]
    clf.central_differences(HIST, pm, lambda ts, trainable: policy(c, ts, hidden, H, trainable=trainable), params, x0, w, wu, T, checks, step=1e-6,
                            bound=(1e-5, 1e-3))


# ---- 5. status word ---------------------------------------------------------------------------------------------------------------------------------
def test_status_word():
    """A NaN in a history column of W0 reaches the inputs: MCP_STATUS_NAN and nothing else.  A flag, not a fault (NaN operands only)."""
    from mc_pilco_amd import hipabi

    M, T, hidden, H = 5, 4, (5,), 2
    c, pm, x0, eps, w, wu, params, _ = arm_setup(M, T, hidden, H, 31, deg=0)
    bad = [q.clone() for q in params]
    bad[0][2, 6 + 3] = float("nan")  # (the older block's columns are 6 .. 11)
    for sample in (False, True):
        nz = clf.noise_buffer(eps) if sample else None
        assert int(HIST.op(pm, policy(c, params, hidden, H, trainable=False).packed(), nz, G(x0), T, particle_pred=sample)[-1].item()) == 0
        assert int(HIST.op(pm, policy(c, bad, hidden, H, trainable=False).packed(), nz, G(x0), T, particle_pred=sample)[-1].item()) == hipabi.STATUS_NAN


# ---- 6. class path, "reference" noise mode ------------------------------------------------------------------------------------------------------------
ARM_H = 3


def _object(cls_name, params, hidden):
    from mc_pilco_amd.policy_learning import Policy

    return clf.arm_object(Policy.MLP_policy, clf.arm_mlp_par(params, hidden, history=ARM_H), clf.ARM_PMS if cls_name == "MC_PILCO4PMS" else None)


def _arm_net(hidden):
    return network(SHAPES["arm2"], hidden, 6 * ARM_H, 40)


def test_class_path():
    """MC_PILCO.apply_policy fused against ``fused_feedback = False`` (the same object on the step loop, seed for seed) at the bounds of
    tests/test_gpu_mlp_rollout.py's class path; the fused call leaves the policy object's own window alone."""
    M, T, hidden, cls_name = 16, 8, (7, 3), "MC_PILCO"
    sim = clf.sim_args(M, T)
    net = _arm_net(hidden)

    def rollout(fused):
        obj = _object(cls_name, net, hidden)
        obj.fused_feedback = fused
        torch.manual_seed(5)
        with clf.normal_draws_on_the_cpu():
            st, inp = obj.apply_policy(**sim)
        assert obj.last_feedback_fused is fused and (obj.last_status is not None) is fused
        pol = obj.control_policy
        if fused:
            assert int(obj.last_status.item()) == 0
            assert pol._window is None and pol._t_prev is None  # untouched
        else:
            assert pol._t_prev == T - 1 and len(pol._window) == ARM_H - 1  # the step loop drove it from t = 0
        cost, _ = obj.cost_function(st, inp, 0)
        cost.backward()
        return st.detach(), inp.detach(), [q.grad.clone() for q in HIST.params(pol)]

    fs, fi, fg = rollout(True)
    ss, si, sg = rollout(False)
    es, ei, eg = float((fs - ss).abs().max()), float((fi - si).abs().max()), [relmax(a, b) for a, b in zip(fg, sg)]
    print("%s, fused vs step: states %.3e inputs %.3e %s" % (cls_name, es, ei, HIST.grad_text(eg)))
    assert es < STATE_TOL and ei < INPUT_TOL and max(eg) < GRAD_TOL
    assert len(fg) == 6 and all(float(g.abs().max()) > 0 for g in fg)
    assert float(fg[0][:, 6:].abs().max()) > 0  # the history columns of W0 get a gradient


@pytest.mark.parametrize("fused_step", [False, True])
def test_the_measured_class_runs_a_policy_with_memory_on_the_step_loop(fused_step):
    """MC_PILCO4PMS has no fused form for history > 1 (no measured form of the kernels is built): ``_fused_rollout`` returns None, and
    apply_policy runs the step loop -- which starts at t = 0 and drives the object's window to t = T - 1 -- with ``last_feedback_fused``
    False; under ``fused_step`` every model step is one launch (``last_step_fused``).  The gradient reaches W0's history columns through
    the held window.  With history = 1 the same object fuses as before.  ops.rollout_mlp refuses the pair before any launch."""
    from functools import partial

    from mc_pilco_amd import ops

    M, T, hidden = 16, 8, (7, 3)
    sim = clf.sim_args(M, T)
    obj = _object("MC_PILCO4PMS", _arm_net(hidden), hidden)
    obj.fused_step = fused_step
    pol = obj.control_policy
    x0 = G(torch.zeros(M, 4, dtype=DT))
    assert obj._fused_rollout(x0, T, 0.0, obj._measured_model, partial(obj._meas_spec, [0.4, 0.3], [1.2, -0.3]), 2) is None
    assert pol._window is None and pol._t_prev is None  # nothing ran
    torch.manual_seed(5)
    with clf.normal_draws_on_the_cpu():
        st, inp = obj.apply_policy(**sim)
    assert obj.last_feedback_fused is False and obj.last_step_fused is fused_step
    assert pol._t_prev == T - 1 and len(pol._window) == ARM_H - 1 and pol._window[0].shape[0] == M
    assert tuple(st.shape) == (T, M, 4) and bool(torch.isfinite(st).all()) and bool(torch.isfinite(inp).all())
    cost, _ = obj.cost_function(st, inp, 0)
    cost.backward()
    assert float(pol.W0.grad[:, 6:].abs().max()) > 0
    pol.reset_window()
    assert pol._window is None and pol._t_prev is None
    with pytest.raises(RuntimeError, match="history"):
        ops.rollout_mlp(obj._measured_model(), pol.packed(), None, x0, T, meas=obj._meas_spec([0.4, 0.3], [1.2, -0.3], None))
    from mc_pilco_amd.policy_learning import Policy

    plain = clf.arm_object(Policy.MLP_policy, clf.arm_mlp_par(network(SHAPES["arm2"], hidden, 6, 40), hidden), clf.ARM_PMS)
    with clf.normal_draws_on_the_cpu():
        plain.apply_policy(**sim)
    assert plain.last_feedback_fused is True  # history = 1: the measured fused form, as before


# ---- 7. two ranks on one device, Philox mode ------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401

    torch.cuda.set_device(dev())
    with rank_group(rank, world, port):
        M, T, hidden = 17, 6, (7, 3)
        net = _arm_net(hidden)
        obj = _object("MC_PILCO", net, hidden)  # (MC_PILCO4PMS runs a policy with memory on the step loop, which does not shard)
        obj.noise_mode = "philox"
        out_q.put((rank, {"MC_PILCO": clf.sharded_step(HIST, obj, world, clf.sim_args(M, T))}))


def test_two_rank_particle_sharding_matches_single_process():
    """MC_PILCO with the policy with memory under shard_particles (M = 17, T = 6, Philox): each rank's states are the matching slice of the
    one-process run bit for bit; the pooled cost, its std and the six parameter gradients agree to the bounds (the family's two-rank body,
    for the one class that fuses it)."""
    import numpy as np

    one = dict(run_ranks(_rank, 1))[0]["MC_PILCO"]
    two = dict(run_ranks(_rank, 2))
    c1, s1, f1, g1, st1, _ = one[:6]
    assert f1 == [0.0, 0.0, 0.0] and len(g1) == 6 and all(float(np.abs(g).max()) > 0 for g in g1)
    seen = 0
    for r in range(2):
        c2, s2, f2, g2, st2, (off, cnt) = two[r]["MC_PILCO"]
        assert np.array_equal(st2, st1[:, off:off + cnt])  # same noise per GLOBAL particle: a trajectory's window is its own
        seen += cnt
        eg = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g2, g1)]
        print("rank %d: cost %.3e std %.3e %s" % (r, abs(c2 - c1), abs(s2 - s1), HIST.grad_text(eg)))
        assert f2 == [0.0, 0.0, 0.0] and abs(c2 - c1) < GRAD_TOL * abs(c1) and abs(s2 - s1) < GRAD_TOL * abs(s1)
        assert len(g2) == 6 and max(eg) < GRAD_TOL
    assert seen == 17
