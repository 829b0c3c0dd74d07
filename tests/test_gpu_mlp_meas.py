"""GPU: the fused closed loop under the tanh-MLP policy on a simulated measurement (mcp_rollout_mlp_meas + mcp_rollout_mlp_meas_bwd,
ops.rollout_mlp(meas=...), MC_PILCO4PMS.apply_policy with a Policy.MLP_policy, and the MLP policy under particle sharding) against torch
autograd through the oracle's step with the measurement and the network written out (tests/mlp_meas_models.mlp_meas_truth; conditioning and
sensitivity checked by tests/test_mlp_meas_cpu.py), and the bitwise contracts it shares with mcp_rollout_mlp and the open-loop kernels.

Bounds (tests/test_gpu_mlp_rollout.py:19, on the oracle's own Kinv / alpha): states and measurements 1e-9 absolute, inputs
2e-9 absolute, every parameter gradient and g_x0 1e-9 relative to that tensor's largest magnitude."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import conftest  # noqa: F401  (registers the package, also in spawned workers)
from mlp_meas_models import CASES, case_id, case_truth, meas_model, mlp_meas_truth
from mlp_models import PAIR_SEED, SHAPES, build_pair, family, inputs_for, network
from pd_meas_models import pos_noise_for

pytestmark = pytest.mark.gpu
DT = torch.float64
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9


def dev():
    return torch.device("cuda", 0)


def G(a):
    return torch.as_tensor(np.asarray(a), dtype=DT).to(dev()).contiguous()


def relmax(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


@functools.lru_cache(maxsize=None)
def pair(shape, N, deg, vs=None):
    """(cfg, oracle model, PackedModel on the oracle's own Kinv / alpha), with the sampling time a measurement model needs on the delta-state
    layout too; built once per process and shared, never modified."""
    from mc_pilco_amd import ops
    from test_gpu_mlp_rollout import packed_model

    c, m, specs = build_pair(shape, N, deg, seed=PAIR_SEED)
    pm = packed_model(c, m, specs, shape, vs)
    if family(shape) == "delta":
        pm = ops.PackedModel.delta(pm.gps, c["S"], c["U"], c["angle"], c["not_angle"], Ts=c["Ts"], var_scale=None if vs is None else list(vs))
    return c, m, pm


def policy(*a, **kw):
    from test_gpu_mlp_rollout import policy as base

    return base(*a, **kw)


def spec(ms, pos_noise=None):
    from mc_pilco_amd import ops

    return ops.MeasSpec(pos=ms["pos"], vel=ms["vel"], std_pos=ms["std"], b=ms["b"], a=ms["a"], pos_noise=None if pos_noise is None else G(pos_noise))


def gpu_run(pm, pol, x0, eps, pn, w, wu, sample, T, ms, noise=None, x0_grad=True):
    """(states, inputs, meas, [parameter gradients or None], g_x0, status) of the op with L = sum w states + sum wu inputs."""
    from mc_pilco_amd import ops

    for q in pol.parameters():
        q.grad = None
    xg = G(x0).requires_grad_(x0_grad)
    nz = noise if noise is not None else (ops.NoiseSpec(eps=G(eps)) if sample else None)
    sp = spec(ms, pn)
    st, inp, status = ops.rollout_mlp(pm, pol.packed(), nz, xg, T, particle_pred=sample, meas=sp)
    ym = sp.measured
    assert not ym.requires_grad and tuple(ym.shape) == tuple(st.shape)
    L = (G(w) * st).sum() + (0.0 if wu is None else (G(wu) * inp).sum())
    L.backward()
    return st.detach(), inp.detach(), ym, [None if q.grad is None else q.grad.clone() for q in pol.mlp_parameters()], xg.grad, int(status.item())


# ---- 1. parity with the truth ---------------------------------------------------------------------------------------------------------
# Measured on an MI355X (the largest figure over the table, per quantity): see DESIGN section 4.10.
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_truth(case):
    mode, shape, deg, N, T, M, hidden, variant, opt = case
    sample = mode == "sampled"
    vs = opt.get("var_scale")
    c, m, ins, (ost, oin, oym, ograds, ogx, vmin) = case_truth(case)
    _, _, pm = pair(shape, N, deg, None if vs is None else tuple(vs))
    if sample and T > 1:
        assert vmin > 0.0
    pol = policy(c, ins["params"], hidden, ins["angle"], ins["non_angle"], u_max=ins["u_max"], squash=ins["squash"])
    only = opt.get("only_grad")
    if only is not None:  # requires_grad on one tensor alone: neither x0 nor the other parameters get a gradient
        for i, q in enumerate(pol.mlp_parameters()):
            q.requires_grad_(i == only)
    st, inp, ym, grads, gx, status = gpu_run(pm, pol, ins["x0"], ins["eps"], ins["pos_noise"], ins["w"], ins["wu"], sample, T, ins["ms"],
                                             x0_grad=only is None)
    es, ei, em = float((st.cpu() - ost).abs().max()), float((inp.cpu() - oin).abs().max()), float((ym.cpu() - oym).abs().max())
    if only is None:
        eg, ex = [relmax(g, o) for g, o in zip(grads, ograds)], relmax(gx, ogx)
    else:
        assert gx is None and all((g is None) == (i != only) for i, g in enumerate(grads))
        eg, ex = [relmax(grads[only], ograds[only])], 0.0
    print("%s: states %.3e inputs %.3e meas %.3e g_params %s g_x0 %.3e (min var %.3e)" % (case_id(case), es, ei, em, " ".join("%.3e" % e for e in eg),
                                                                                          ex, vmin))
    assert status == 0
    assert es < STATE_TOL and ei < INPUT_TOL and em < STATE_TOL
    assert max(eg) < GRAD_TOL and ex < GRAD_TOL


# ---- 2. bit identities ------------------------------------------------------------------------------------------------------------------
def _noise(kind, eps, **kw):
    from mc_pilco_amd import ops

    return None if kind == "mean" else (ops.NoiseSpec(eps=G(eps)) if kind == "eps" else ops.NoiseSpec(seed=11, call=3, **kw))


@pytest.mark.parametrize("noise", ["mean", "eps", "philox"])
def test_plain_launch_recording_launch_and_open_loop_launch_carry_the_same_bits(noise):
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 1)
    M, T, hidden = 17, 6, (7, 3)
    x0, _, _, _, eps, w, wu = inputs_for(c, M, T, seed=21)
    ms = meas_model("arm2")
    pn = pos_noise_for(T, M, 2, seed=21)
    pol = policy(c, network(c, hidden, c["angle"], c["not_angle"], 21), hidden)
    sample = noise != "mean"
    sp = lambda: spec(ms, None if noise == "philox" else pn)
    s1, s2 = sp(), sp()
    with torch.no_grad():
        st, inp, status = ops.rollout_mlp(pm, pol.packed(), _noise(noise, eps), G(x0), T, particle_pred=sample, meas=s1)
    ym = s1.measured
    assert int(status.item()) == 0 and not st.requires_grad
    so, status_o = ops.rollout_open(pm, G(x0), inp[:T - 1].contiguous(), noise=_noise(noise, eps), particle_pred=sample)
    assert int(status_o.item()) == 0
    assert torch.equal(st, so)  # the same phases on the same operands
    sr, ir, status_r = ops.rollout_mlp(pm, pol.packed(), _noise(noise, eps), G(x0), T, particle_pred=sample, meas=s2)  # the parameters require grad: recording
    yr = s2.measured
    assert sr.requires_grad and int(status_r.item()) == 0
    assert torch.equal(sr.detach(), st) and torch.equal(ir.detach(), inp) and torch.equal(yr, ym)
    assert float((ym[1:, :, :2] - st[1:, :, :2]).abs().min()) > 0 and torch.equal(ym[0], st[0])  # a measurement was simulated; row 0 is true
    ((G(w) * sr).sum() + (G(wu) * ir).sum()).backward()  # the sweep over that record runs and leaves finite gradients
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0 for q in pol.mlp_parameters())


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
    truth = mlp_meas_truth("arm2", m, x0, params, eps, pn, w, wu, True, c["angle"], c["not_angle"], ms)
    assert truth[-1] > 0.0
    return c, pm, M, T, hidden, x0, params, eps, w, wu, ms, pn, truth


@pytest.mark.parametrize("N", [640, 2600])
def test_the_smaller_tiles_of_the_recording_form(N):
    """Sampled, degree 0, M = 5, T = 3 on arm2, every joint measured.  Status 0; states, inputs and measurements carry the bits of the launch
    without a record, whose states carry the bits of the open-loop launch on its inputs; everything against the truth."""
    from mc_pilco_amd import ops

    c, pm, M, T, hidden, x0, params, eps, w, wu, ms, pn, (ost, oin, oym, ograds, ogx, vmin) = _rung_case(N)
    pol = policy(c, params, hidden)
    st, inp, ym, grads, gx, status = gpu_run(pm, pol, x0, eps, pn, w, wu, True, T, ms)
    s0 = spec(ms, pn)
    with torch.no_grad():
        st0, i0, status0 = ops.rollout_mlp(pm, pol.packed(), ops.NoiseSpec(eps=G(eps)), G(x0), T, particle_pred=True, meas=s0)
    so, status_o = ops.rollout_open(pm, G(x0), i0[:T - 1].contiguous(), noise=ops.NoiseSpec(eps=G(eps)), particle_pred=True)
    es, ei, em = float((st.cpu() - ost).abs().max()), float((inp.cpu() - oin).abs().max()), float((ym.cpu() - oym).abs().max())
    eg, ex = [relmax(g, o) for g, o in zip(grads, ograds)], relmax(gx, ogx)
    print("rung N %d: states %.3e inputs %.3e meas %.3e g_params %s g_x0 %.3e (min var %.3e)" % (N, es, ei, em, " ".join("%.3e" % e for e in eg), ex, vmin))
    assert status == 0 and int(status0.item()) == 0 and int(status_o.item()) == 0
    assert torch.equal(st, st0) and torch.equal(inp, i0) and torch.equal(ym, s0.measured) and torch.equal(st0, so)
    assert es < STATE_TOL and ei < INPUT_TOL and em < STATE_TOL
    assert max(eg) < GRAD_TOL and ex < GRAD_TOL


def test_the_four_trajectory_tile_without_a_record():
    """Nothing requires grad: status 0, the states carry the bits of the open-loop launch on the inputs; states, inputs and measurements
    against the truth.  (No record, so no gradient to compare.)"""
    from mc_pilco_amd import ops

    c, pm, M, T, hidden, x0, params, eps, w, wu, ms, pn, (ost, oin, oym, _, _, vmin) = _rung_case(640)
    sp = spec(ms, pn)
    st, inp, status = ops.rollout_mlp(pm, policy(c, params, hidden, trainable=False).packed(), ops.NoiseSpec(eps=G(eps)), G(x0), T, particle_pred=True,
                                      meas=sp)
    so, status_o = ops.rollout_open(pm, G(x0), inp[:T - 1].contiguous(), noise=ops.NoiseSpec(eps=G(eps)), particle_pred=True)
    es, ei, em = float((st.cpu() - ost).abs().max()), float((inp.cpu() - oin).abs().max()), float((sp.measured.cpu() - oym).abs().max())
    print("rung N 640, no record: states %.3e inputs %.3e meas %.3e (min var %.3e)" % (es, ei, em, vmin))
    assert int(status.item()) == 0 and int(status_o.item()) == 0 and not st.requires_grad
    assert torch.equal(st, so)
    assert es < STATE_TOL and ei < INPUT_TOL and em < STATE_TOL


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
    from test_gpu_pd_rollout import controller

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
def _pms_object(params, hidden, M):
    """MC_PILCO4PMS over the model and with the MLP policy of tests/test_gpu_mlp_rollout._arm_object: both joints measured, a first-order
    filter with memory (fc = 0.3), position noise on both."""
    from mc_pilco_amd.policy_learning import MC_PILCO
    from test_gpu_mlp_rollout import _arm_object

    base = _arm_object(params, hidden, M)
    ml, pol, cf = base.model_learning, base.control_policy, base.cost_function
    c = SHAPES["arm2"]
    from mc_pilco_amd.policy_learning import Policy

    with contextlib.redirect_stdout(io.StringIO()):
        obj = MC_PILCO.MC_PILCO4PMS(T_sampling=c["Ts"], state_dim=4, input_dim=2, f_sim=lambda y, t, u: None, f_model_learning=lambda **kw: ml,
                                    model_learning_par={}, f_rand_exploration_policy=Policy.Random_exploration,
                                    rand_exploration_policy_par=dict(state_dim=4, input_dim=2, u_max=1.0, dtype=DT),
                                    f_control_policy=lambda **kw: pol, control_policy_par={}, f_cost_function=lambda **kw: cf, cost_function_par={},
                                    pos_indeces=[0, 1], vel_indeces=[2, 3], std_meas_noise=np.array([0.02, 0.03, 0.0, 0.0]),
                                    filtering_dict={"fc": 0.3}, log_path=None, dtype=DT, device=dev())
    obj.noise_mode = "reference"
    return obj


def _sim(M, T):
    return dict(particles_initial_state_mean=G([0.1, -0.1, 0.0, 0.05]), particles_initial_state_var=G([1e-2, 1e-2, 2e-2, 2e-2]),
                flg_particles_init_uniform=False, particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
                num_particles=M, T_control=T)


def test_class_path():
    from test_gpu_pd_rollout import _normal_draws_on_the_cpu

    M, T, c = 16, 8, SHAPES["arm2"]
    sim = _sim(M, T)
    net = lambda hidden: network(c, hidden, c["angle"], c["not_angle"], 40)

    def rollout(fused, hidden=(7, 3), expect=None, edit=None):
        obj = _pms_object(net(hidden), hidden, M)
        obj.fused_feedback = fused
        if edit:
            edit(obj)
        torch.manual_seed(5)
        with _normal_draws_on_the_cpu():
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
    with _normal_draws_on_the_cpu(), contextlib.redirect_stdout(io.StringIO()):
        out = obj.reinforce_policy(T_control=0.05 * T, num_particles=M, trial_index=0, particles_initial_state_mean=sim["particles_initial_state_mean"],
                                   particles_initial_state_var=sim["particles_initial_state_var"], flg_particles_init_uniform=False,
                                   particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
                                   opt_steps_list=[3], lr_list=[0.01], f_optimizer="lambda p, lr : torch.optim.Adam(p, lr)", num_step_print=10,
                                   policy_reinit_dict=None)
    assert obj.last_feedback_fused is True
    costs = np.asarray(out[0], dtype=float).reshape(-1)
    assert costs.shape == (3,) and np.isfinite(costs).all()
    assert all(float((q.detach() - b).abs().max()) > 1e-4 for q, b in zip(obj.control_policy.mlp_parameters(), before))  # every tensor moved


# ---- 7. class path, two ranks on one device -------------------------------------------------------------------------------------------------
def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, out_q):
    import torch.distributed as dist

    import mcp_boot  # noqa: F401
    from test_gpu_mlp_rollout import _arm_object

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(dev())
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    M, T, hidden, c = 17, 6, (7, 3), SHAPES["arm2"]
    res = {}
    for cls_name, make in (("MC_PILCO", _arm_object), ("MC_PILCO4PMS", _pms_object)):
        obj = make(network(c, hidden, c["angle"], c["not_angle"], 40), hidden, M)
        obj.noise_mode = "philox"
        obj.seed = 17
        if world > 1:
            obj.shard_particles()
        torch.manual_seed(23)  # (every rank alike: x0 is drawn for the whole swarm and sliced)
        st, inp = obj.apply_policy(**_sim(M, T))
        assert obj.last_feedback_fused is True
        cost, std, flags = obj._cost_backward(st, inp, 0)
        torch.cuda.synchronize()
        res[cls_name] = (float(cost.detach()), float(std.detach()), [float(v) for v in flags.tolist()],
                         [q.grad.cpu().numpy().copy() for q in obj.control_policy.mlp_parameters()], st.detach().cpu().numpy(), obj._shard)
    out_q.put((rank, res))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_rank_particle_sharding_matches_single_process():
    """MC_PILCO and MC_PILCO4PMS with the MLP policy under shard_particles (M = 17, T = 6, Philox): each rank's states are the matching slice
    of the one-process run bit for bit; the pooled cost, its std and the six parameter gradients agree to the bounds (another order of the
    sums)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p1 = ctx.Process(target=_rank, args=(0, 1, 0, q))
    p1.start()
    _, one = q.get(timeout=300)
    p1.join(timeout=60)
    assert p1.exitcode == 0
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    two = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for cls_name in ("MC_PILCO", "MC_PILCO4PMS"):
        c1, s1, f1, g1, st1, _ = one[cls_name]
        assert f1 == [0.0, 0.0, 0.0] and len(g1) == 6 and all(float(np.abs(g).max()) > 0 for g in g1)
        seen = 0
        for r in range(2):
            c2, s2, f2, g2, st2, (off, cnt) = two[r][cls_name]
            assert np.array_equal(st2, st1[:, off:off + cnt])  # same noise per GLOBAL particle
            seen += cnt
            eg = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g2, g1)]
            print("%s rank %d: cost %.3e std %.3e g_params %s" % (cls_name, r, abs(c2 - c1), abs(s2 - s1), " ".join("%.3e" % e for e in eg)))
            assert f2 == [0.0, 0.0, 0.0]
            assert abs(c2 - c1) < GRAD_TOL * abs(c1) and abs(s2 - s1) < GRAD_TOL * abs(s1)
            assert len(g2) == 6 and max(eg) < GRAD_TOL
        assert seen == 17


# ---- 8. saved record -------------------------------------------------------------------------------------------------------------------------
def test_saved_record_refuses_in_place_changes():
    from mc_pilco_amd import ops

    c, m, pm = pair("arm2", 37, 0)
    x0, _, _, _, _, w, wu = inputs_for(c, 2, 4, seed=3)
    ms = meas_model("arm2")
    pn = pos_noise_for(4, 2, 2, seed=3)
    pol = policy(c, network(c, (5,), c["angle"], c["not_angle"], 3), (5,))
    for which in (0, 1, 2):
        sp = spec(ms, pn)
        out = ops.rollout_mlp(pm, pol.packed(), None, G(x0), 4, particle_pred=False, meas=sp)
        with torch.no_grad():
            (sp.measured if which == 2 else out[which]).mul_(2.0)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            ((G(w) * out[0]).sum() + (G(wu) * out[1]).sum()).backward()
