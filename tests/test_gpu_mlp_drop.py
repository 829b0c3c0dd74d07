"""GPU: dropout in the fused closed loop under the tanh-MLP policy (mcp_rollout_mlp_drop + mcp_rollout_mlp_drop_bwd, ops.rollout_mlp(p_drop=...),
MC_PILCO / MC_PILCO4PMS.apply_policy with a Policy.MLP_policy(flg_drop=True), and that policy under particle sharding) against torch autograd
through the oracle's step with the network and its keep-masks written out (tests/mlp_drop_models.drop_truth; conditioning checked by
tests/test_mlp_drop_cpu.py), the Philox masks against the buffer masks bit for bit, and the bitwise contracts that survive dropout.

Bounds (tests/test_gpu_mlp_rollout.py, on the oracle's own Kinv / alpha; 1 / (1 - p) <= 2 does not change the scale):
states and measurements 1e-9 absolute, inputs 2e-9 absolute, every parameter gradient and g_x0 1e-9 relative to that tensor's largest magnitude."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
from closed_loop_family import MLP, policy
from closed_loop_family import meas_spec as spec
from gpu_helpers import DT, G, dev, relmax
from mlp_drop_models import CASES, case_id, case_truth, truth_of
from mlp_meas_models import meas_model
from mlp_models import SHAPES, inputs_for, network
from pd_meas_models import pos_noise_for
from rank_harness import rank_group, run_ranks

pytestmark = pytest.mark.gpu
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9
TOLS = (STATE_TOL, INPUT_TOL, GRAD_TOL)


def K(masks):
    return masks.to(torch.uint8).to(dev()).contiguous()


def pair(shape, N, deg):
    """(cfg, oracle model, PackedModel) of tests/test_gpu_mlp_meas.py: shared with that module, with the sampling time a measurement needs."""
    return MLP.pair(shape, N, deg, measured=True)


def gpu_run(pm, pol, ins, T, noise, p, x0_grad=True, **edit):
    """The Run of the op with L = sum w states + sum wu inputs on a case's inputs."""
    q = dict(ins, **edit)
    return MLP.run(pm, pol, q["x0"], T, noise, q["w"], q["wu"], q["sample"], meas=spec(q["ms"], q["pos_noise"]), p_drop=p, x0_grad=x0_grad)


def buffers(ins, masks=None):
    from mc_pilco_amd import ops

    return ops.NoiseSpec(eps=G(ins["eps"]) if ins["sample"] else None, masks=K(ins["masks"] if masks is None else masks))


def check_against(truth, got, only=None, what=""):
    """The states, inputs and gradients of a Run against drop_truth's tuple.  (The measurements are not part of that truth.)"""
    clf.check_against(MLP, what, clf.mlp_truth_of(truth), got, TOLS, only)


# ---- 1. parity with the truth, buffer mode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_truth(case):
    mode, shape, deg, N, T, M, hidden, p, opt = case
    c, m, ins, truth = case_truth(case)
    _, _, pm = pair(shape, N, deg)
    if ins["sample"] and T > 1:
        assert truth[-1] > 0.0
    pol = policy(c, ins["params"], hidden, ins["angle"], ins["non_angle"], u_max=ins["u_max"], squash=ins["squash"])
    only = opt.get("only_grad")
    if only is not None:  # requires_grad on one tensor alone: neither x0 nor the other parameters get a gradient
        for i, q in enumerate(pol.mlp_parameters()):
            q.requires_grad_(i == only)
    check_against(truth, gpu_run(pm, pol, ins, T, buffers(ins), p, x0_grad=only is None), only, case_id(case))


# ---- 2. p_drop = 0 through the new entries; an all-ones mask buffer --------------------------------------------------------------------------------
def raw_drop(pm, mlp, tensors, noise, p, x0, T, sample, w, wu, meas=None):
    """mcp_rollout_mlp_drop (recording) and mcp_rollout_mlp_drop_bwd called as they are, whatever p is: (states, inputs, slabs, g_x0)."""
    from mc_pilco_amd import hipabi as abi
    from mc_pilco_amd import ops

    M = int(x0.shape[0])
    states, inputs, jac = ops._record_buffers(dev(), T, M, pm.S, pm.U, pm.G, pm.D, T > 1)
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    buf = None
    if meas is not None:
        buf = meas.measured = torch.empty(T, M, pm.S, dtype=DT, device=dev())
    pc, nz = mlp.to_c(*tensors), noise.to_c()
    marg = ops._meas_arg(meas, T, M, buf)
    head = [C.byref(pm.c), C.byref(pc), marg[0] if marg else None, C.byref(nz), float(p), M, T]
    abi.check(abi.lib().mcp_rollout_mlp_drop(*head, int(sample), abi.ptr(x0), abi.ptr(states), abi.ptr(inputs), None, None, abi.ptr(jac),
                                             abi.ptr(status), abi.stream()), "mcp_rollout_mlp_drop")
    slabs, gx = torch.empty((M + 15) // 16, mlp.n_param, dtype=DT, device=dev()), torch.empty(M, pm.S, dtype=DT, device=dev())
    abi.check(abi.lib().mcp_rollout_mlp_drop_bwd(*head, abi.ptr(states), abi.ptr(inputs), abi.ptr(jac), abi.ptr(w), abi.ptr(wu), abi.ptr(slabs),
                                                 abi.ptr(gx), abi.stream()), "mcp_rollout_mlp_drop_bwd")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return states, inputs, slabs, gx


@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
def test_no_dropout_through_the_new_entries_is_the_old_entries(measured):
    """p_drop = 0: the bits of mcp_rollout_mlp(_meas) and its sweep -- states, inputs, measurements, slabs and g_x0 -- on M = 37 (three slabs)."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 1)
    M, T, hidden = 37, 6, (7, 3)
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=9)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 9), hidden)
    mlp, tensors = pol.packed(), [q.detach() for q in pol.mlp_parameters()]
    ms = meas_model("arm2", "all", 0.1) if measured else None
    pn = pos_noise_for(T, M, 2, 9) if measured else None
    nz = lambda: ops.NoiseSpec(eps=G(eps))
    sp_old, sp_new = spec(ms, pn), spec(ms, pn)
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    st, inp, jac = ops._closed_launch(pm, mlp, tensors, nz(), G(x0), T, True, status, True, sp_old)
    slabs, gx = ops._closed_sweep(pm, mlp, tensors, st, inp, jac, G(w), G(wu), True, True, sp_old, None if sp_old is None else sp_old.measured)
    st2, inp2, slabs2, gx2 = raw_drop(pm, mlp, tensors, nz(), 0.0, G(x0), T, True, G(w), G(wu), sp_new)
    assert int(status.item()) == 0 and tuple(slabs.shape) == (3, mlp.n_param) and float(slabs.abs().max()) > 0
    assert torch.equal(st, st2) and torch.equal(inp, inp2) and torch.equal(slabs, slabs2) and torch.equal(gx, gx2)
    if measured:
        assert torch.equal(sp_old.measured, sp_new.measured)
    # and through the op: the keyword at 0 is the call without it
    a = ops.rollout_mlp(pm, mlp, nz(), G(x0), T, meas=spec(ms, pn))
    b = ops.rollout_mlp(pm, mlp, nz(), G(x0), T, meas=spec(ms, pn), p_drop=0.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0].detach(), st)


def test_all_ones_masks_scale_the_activations():
    """Nothing dropped at p > 0: every hidden unit is 1 / (1 - p) times its tanh -- against the truth with an all-ones buffer."""
    case = CASES[2]
    mode, shape, deg, N, T, M, hidden, p, opt = case
    assert hidden == (7, 3)
    c, m, ins = case_truth(case)[:3]
    ones = torch.ones_like(ins["masks"])
    truth = truth_of(m, ins, masks=ones)
    s0 = truth_of(m, ins, masks=None)[0]
    assert float((truth[0] - s0).abs().max()) > 1e-3  # (the scale is seen)
    _, _, pm = pair(shape, N, deg)
    pol = policy(c, ins["params"], hidden, ins["angle"], ins["non_angle"])
    check_against(truth, gpu_run(pm, pol, ins, T, buffers(ins, ones), p), None, "all-ones masks")


# ---- 3. Philox against buffer -------------------------------------------------------------------------------------------------------------------
def decode_keep_bits(pm, c, hidden, noise, p, M, T):
    """The keep decisions [T, M, 16] of the LAST hidden layer's 16 units in a Philox launch, read off its inputs: that layer has W = 0,
    b = 0.5, so a unit is c0 = tanh(0.5) / (1 - p) or 0 whatever feeds it; no squashing, bout = 0 and Wout[k, j] = 2^(j // U) for j % U == k,
    so input k is c0 times the 8-bit integer of the bits of the units k, k + U, ..."""
    from mc_pilco_amd import ops

    U = c["U"]
    assert hidden[-1] == 16 and 16 % U == 0 and 16 // U <= 8
    params = network(c, hidden, c["angle"], c["not_angle"], 1)
    params[-4], params[-3] = torch.zeros_like(params[-4]), torch.full_like(params[-3], 0.5)
    wout = torch.zeros(U, 16, dtype=DT)
    for j in range(16):
        wout[j % U, j] = 2.0 ** (j // U)
    params[-2], params[-1] = wout, torch.zeros(U, dtype=DT)
    pol = policy(c, params, hidden, squash=False, trainable=False)
    x0 = inputs_for(c, M, T, seed=3)[0]
    with torch.no_grad():
        _, inp, _ = ops.rollout_mlp(pm, pol.packed(), noise, G(x0), T, particle_pred=False, p_drop=p)
    v = inp.cpu().numpy() / (np.tanh(0.5) / (1.0 - p))
    n = np.rint(v)
    assert np.abs(v - n).max() < 1e-9 and n.min() >= 0 and n.max() <= 2 ** (16 // U) - 1
    bits = np.zeros((T, M, 16), dtype=np.uint8)
    for j in range(16):
        bits[:, :, j] = (n[:, :, j % U].astype(np.int64) >> (j // U)) & 1
    return bits


@pytest.mark.parametrize("p", [0.25, 0.5])
def test_philox_masks_against_the_buffer(p):
    """The bits a Philox launch draws, decoded from two decoding networks (units 0..15 as layer 0 of a one-layer net; units 7..22 as layer 1
    behind a layer 0 of 7: off_1 = h[0]) and fed back as a buffer to a general (7, 3) network with the same seed, call and offset, reproduce the
    Philox launch's states, inputs, slabs and g_x0 bit for bit.  Keep rate, and other bits under another call."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 1)
    M, T, hidden, off = 1041, 12, (7, 3), 32
    nz = lambda call=5, **kw: ops.NoiseSpec(seed=91, call=call, particle_offset=off, **kw)
    k0 = decode_keep_bits(pm, c, (16,), nz(), p, M, T)      # units 0 .. 15
    k1 = decode_keep_bits(pm, c, (7, 16), nz(), p, M, T)    # units 7 .. 22
    assert np.array_equal(k0[:, :, 7:], k1[:, :, :9])       # the unit's index is its place in the row, whichever layer it is in
    n, q = k0.size, 1.0 - p
    assert abs(k0.mean() - q) < 4.0 * np.sqrt(p * q) / np.sqrt(n)  # (the bound of test_gpu_realsize.py::test_philox_dropout_keep_rate_and_independence)
    other = decode_keep_bits(pm, c, (16,), nz(call=6), p, M, T)
    assert not np.array_equal(other, k0) and abs(float(np.corrcoef(other.reshape(-1), k0.reshape(-1))[0, 1])) < 4.5 / np.sqrt(n)
    masks = torch.as_tensor(np.concatenate([k0[:, :, :7], k1[:, :, :3]], axis=2))
    x0, _, _, _, _, w, wu = inputs_for(c, M, T, seed=21)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 21), hidden)
    mlp, tensors = pol.packed(), [t.detach() for t in pol.mlp_parameters()]

    def run(noise):
        status = torch.zeros(1, dtype=torch.int32, device=dev())
        st, inp, jac = ops._closed_launch(pm, mlp, tensors, noise, G(x0), T, True, status, True, None, p)
        slabs, gx = ops._closed_sweep(pm, mlp, tensors, st, inp, jac, G(w), G(wu), True, True, None, None, noise, p)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        return st, inp, slabs, gx

    ph, bf = run(nz()), run(nz(masks=K(masks)))  # (eps: Philox in both)
    assert all(torch.equal(a, b) for a, b in zip(ph, bf))
    assert float(ph[2].abs().max()) > 0 and float(ph[3].abs().max()) > 0
    nodrop = ops.rollout_mlp(pm, mlp, nz(), G(x0), T)[0]
    assert float((nodrop.detach() - ph[0]).abs().max()) > 1e-3


# ---- 4. bit contracts that survive dropout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [17, 1041])  # 4 trajectories per workgroup, and 16
@pytest.mark.parametrize("kind", ["buffer", "philox"])
def test_states_carry_the_bits_of_the_open_loop_launch(kind, M):
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 1)
    T, hidden, p = 6, (7, 3), 0.25
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=21)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 21), hidden)
    keep = torch.empty(T, M, 10, dtype=DT).bernoulli_(1 - p, generator=torch.Generator().manual_seed(8))
    nz = lambda: ops.NoiseSpec(eps=G(eps), masks=K(keep)) if kind == "buffer" else ops.NoiseSpec(seed=11, call=3)
    plain = lambda: ops.NoiseSpec(eps=G(eps)) if kind == "buffer" else ops.NoiseSpec(seed=11, call=3)  # (the same eps, no masks)
    with torch.no_grad():
        st, inp, status = ops.rollout_mlp(pm, pol.packed(), nz(), G(x0), T, p_drop=p)
    assert int(status.item()) == 0 and not st.requires_grad
    so, status_o = ops.rollout_open(pm, G(x0), inp[:T - 1].contiguous(), noise=plain(), particle_pred=True)
    assert int(status_o.item()) == 0 and torch.equal(st, so)  # the same phases on the same operands
    sr, ir, status_r = ops.rollout_mlp(pm, pol.packed(), nz(), G(x0), T, p_drop=p)  # the parameters require grad: the recording launch
    assert sr.requires_grad and int(status_r.item()) == 0
    assert torch.equal(sr.detach(), st) and torch.equal(ir.detach(), inp)
    with torch.no_grad():
        s0 = ops.rollout_mlp(pm, pol.packed(), plain(), G(x0), T)[0]
    assert float((s0 - st).abs().max()) > 1e-3  # (dropout was applied)
    ((G(w) * sr).sum() + (G(wu) * ir).sum()).backward()
    g1 = [q.grad.clone() for q in pol.mlp_parameters()]
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in g1)
    for q in pol.mlp_parameters():  # two runs: the same bits
        q.grad = None
    sr2, ir2, _ = ops.rollout_mlp(pm, pol.packed(), nz(), G(x0), T, p_drop=p)
    ((G(w) * sr2).sum() + (G(wu) * ir2).sum()).backward()
    assert torch.equal(sr2.detach(), st) and all(torch.equal(q.grad, g) for q, g in zip(pol.mlp_parameters(), g1))


@pytest.mark.parametrize("measured", [False, True], ids=["plain", "meas"])
def test_shard_invariance_under_philox(measured):
    """Rows [a, b) launched with particle_offset = a, a a multiple of 16: states, inputs, g_x0 and the workgroups' slabs are bitwise those of
    one launch over all rows."""
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    M, T, cut, hidden, p = 37, 6, 16, (7, 3), 0.5
    x0, _, _, _, _, w, wu = inputs_for(c, M, T, seed=9)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 9), hidden)
    mlp, tensors = pol.packed(), [q.detach() for q in pol.mlp_parameters()]
    ms = meas_model("arm2", "all", 0.1) if measured else None

    def run(a, b):
        nz, sp = ops.NoiseSpec(seed=4, call=2, particle_offset=a), spec(ms)
        st, inp, jac = ops._closed_launch(pm, mlp, tensors, nz, G(x0[a:b]), T, True, torch.zeros(1, dtype=torch.int32, device=dev()), True, sp, p)
        slabs, gx = ops._closed_sweep(pm, mlp, tensors, st, inp, jac, G(w[:, a:b]), G(wu[:, a:b]), True, True, sp, None if sp is None else sp.measured,
                                      nz, p)
        torch.cuda.synchronize()
        return st, inp, slabs, gx

    st, inp, slabs, gx = run(0, M)
    assert tuple(slabs.shape) == (3, mlp.n_param) and all(float(slabs[i].abs().max()) > 0 for i in range(3))
    for a, b in ((0, cut), (cut, M)):
        sa, ia, la, xa = run(a, b)
        assert torch.equal(sa, st[:, a:b]) and torch.equal(ia, inp[:, a:b])
        assert torch.equal(la, slabs[a // 16:(b + 15) // 16]) and torch.equal(xa, gx[a:b])


def test_mask_buffers_are_checked():
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    M, T, hidden = 5, 3, (7, 3)
    x0 = G(inputs_for(c, M, T, seed=9)[0])
    mlp = policy(c, network(c, hidden, c["angle"], c["not_angle"], 9), hidden, trainable=False).packed()
    good = torch.ones(T, M, 10, dtype=torch.uint8, device=dev())
    for sample in (True, False):
        assert int(ops.rollout_mlp(pm, mlp, ops.NoiseSpec(masks=good, seed=1), x0, T, particle_pred=sample, p_drop=0.25)[2].item()) == 0
        for bad in (good[:, :, :9].contiguous(), good[:2], good.to(torch.float64), good.cpu(), good.transpose(0, 1)):
            with pytest.raises(RuntimeError, match="masks must be"):
                ops.rollout_mlp(pm, mlp, ops.NoiseSpec(masks=bad, seed=1), x0, T, particle_pred=sample, p_drop=0.25)
    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(RuntimeError, match="p_drop"):
            ops.rollout_mlp(pm, mlp, ops.NoiseSpec(seed=1), x0, T, p_drop=p)


# ---- 5. Philox mode: central differences of the op ---------------------------------------------------------------------------------------------
def test_philox_mode_against_central_differences():
    """Step 1e-6, bound 1e-5 relative with floor 1e-3, as tests/test_gpu_mlp_rollout.py::test_philox_mode_against_central_differences; two
    entries of every parameter tensor and of x0.  (The keep decisions do not depend on the operands: the loss is smooth in them.)"""
    c, m, pm = pair("arm2", 37, 2)
    M, T, hidden, p = 3, 6, (7, 3), 0.25
    x0, _, _, _, _, w, wu = inputs_for(c, M, T, seed=5)
    params = network(c, hidden, c["angle"], c["not_angle"], 5)
    policy_of = lambda tensors, trainable: policy(c, tensors, hidden, trainable=trainable)
    clf.central_differences(MLP, pm, policy_of, params, x0, w, wu, T, clf.first_and_last_entries(params + [x0]), step=1e-6,
                            bound=(1e-5, 1e-3), p_drop=p)


# ---- 6. class path, "reference" noise mode ------------------------------------------------------------------------------------------------------
def _object(cls_name, params, hidden, M, flg_drop=True):
    """The MC_PILCO / MC_PILCO4PMS objects of tests/test_gpu_mlp_rollout.py and tests/test_gpu_mlp_meas.py with a policy built with ``flg_drop``;
    its masks are drawn where "reference" mode draws everything: on the CPU."""
    from mc_pilco_amd.policy_learning import Policy

    obj = clf.arm_object(Policy.MLP_policy, clf.arm_mlp_par(params, hidden), clf.ARM_PMS if cls_name == "MC_PILCO4PMS" else None)
    obj.control_policy = Policy.MLP_policy(**clf.arm_mlp_par(params, hidden, **(dict(flg_drop=True) if flg_drop else {})))
    obj.control_policy.draw_device = torch.device("cpu")
    return obj


_sim = clf.sim_args


@pytest.mark.parametrize("cls_name", ["MC_PILCO", "MC_PILCO4PMS"])
def test_class_path(cls_name):
    M, T, c, hidden = 16, 8, SHAPES["arm2"], (7, 3)
    sim = _sim(M, T)
    net = network(c, hidden, c["angle"], c["not_angle"], 40)

    def rollout(fused, p, flg_drop=True):
        obj = _object(cls_name, net, hidden, M, flg_drop)
        obj.fused_feedback = fused
        torch.manual_seed(5)
        with clf.normal_draws_on_the_cpu():
            st, inp = obj.apply_policy(p_dropout=p, **sim)
        assert obj.last_feedback_fused is fused and (obj.last_status is not None) is fused
        if fused:
            assert int(obj.last_status.item()) == 0
        cost, _ = obj.cost_function(st, inp, 0)
        cost.backward()
        return st.detach(), inp.detach(), [q.grad.clone() for q in obj.control_policy.mlp_parameters()]

    fs, fi, fg = rollout(True, 0.25)
    ss, si, sg = rollout(False, 0.25)  # fused_feedback off: the same object runs the step loop, seed for seed -- masks included
    es, ei, eg = float((fs - ss).abs().max()), float((fi - si).abs().max()), [relmax(a, b) for a, b in zip(fg, sg)]
    print("%s, fused vs step at p = 0.25: states %.3e inputs %.3e g_params %s" % (cls_name, es, ei, " ".join("%.3e" % e for e in eg)))
    assert es < STATE_TOL and ei < INPUT_TOL and max(eg) < GRAD_TOL
    ns, ni, ng = rollout(True, 0.0)
    assert float((fs - ns).abs().max()) > 1e-3  # the probability reached the kernels
    # a policy built without flg_drop: today's bits whatever p_dropout is
    os_, oi, og = rollout(True, 0.25, flg_drop=False)
    assert torch.equal(os_, ns) and torch.equal(oi, ni) and all(torch.equal(a, b) for a, b in zip(og, ng))

    obj = _object(cls_name, net, hidden, M)
    before = [q.detach().clone() for q in obj.control_policy.mlp_parameters()]
    torch.manual_seed(6)
    with clf.normal_draws_on_the_cpu(), contextlib.redirect_stdout(io.StringIO()):
        out = obj.reinforce_policy(**clf.reinforce_args(sim, T, 3, p_dropout_list=[0.25]))
    assert obj.last_feedback_fused is True
    costs = np.asarray(out[0], dtype=float).reshape(-1)
    assert costs.shape == (3,) and np.isfinite(costs).all()
    assert all(float((q.detach() - b).abs().max()) > 1e-4 for q, b in zip(obj.control_policy.mlp_parameters(), before))  # every tensor moved


# ---- 7. two ranks on one device, Philox mode ----------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401

    torch.cuda.set_device(dev())
    with rank_group(rank, world, port):
        M, T, hidden, c = 17, 6, (7, 3), SHAPES["arm2"]
        res = {}
        for cls_name in ("MC_PILCO", "MC_PILCO4PMS"):
            obj = _object(cls_name, network(c, hidden, c["angle"], c["not_angle"], 40), hidden, M)
            obj.noise_mode = "philox"
            res[cls_name] = clf.sharded_step(MLP, obj, world, _sim(M, T), p_dropout=0.25)
            if world == 1:  # (once: the run without dropout differs)
                torch.manual_seed(23)
                obj._rollout_calls = 0
                res[cls_name] += (obj.apply_policy(p_dropout=0.0, **_sim(M, T))[0].detach().cpu().numpy(),)
        out_q.put((rank, res))


def test_two_rank_particle_sharding_matches_single_process():
    """MC_PILCO and MC_PILCO4PMS with the dropout policy under shard_particles (M = 17, T = 6, Philox, p = 0.25): each rank's states are the
    matching slice of the one-process run bit for bit (the same noise, the same masks per global particle); the pooled cost, its std and the
    six parameter gradients agree to the bounds (another order of the sums)."""
    one = run_ranks(_rank, 1)
    two = run_ranks(_rank, 2)
    one = clf.two_ranks_match_one_process(MLP, one, two, GRAD_TOL, n_grads=6)
    for cls_name in ("MC_PILCO", "MC_PILCO4PMS"):
        assert np.abs(one[cls_name][6] - one[cls_name][4]).max() > 1e-3  # (dropout was applied)
