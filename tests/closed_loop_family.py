"""What the GPU tests of the fused closed-loop rollouts share: the cached model pairs, the class-path objects, a ``Family`` record per
policy (PD law, tanh MLP) that states as data what differs between them -- as ops.PackedPD / ops.PackedMLP do for the product -- and the
test bodies every form repeats, written once over a family.  The test modules keep their docstrings, tables, tolerance constants and test
functions; a function there is a call of a body here with the module's family, shapes, seeds and sizes.

A new closed-loop form adds: a Family record (or a keyword of ``Family.run``), its table of cases and its truth function."""
import collections
import contextlib
import functools
import io

import numpy as np
import torch

import conftest  # noqa: F401  (registers the package, also in spawned workers)
import mlp_models
import open_grad_models
import pd_models
from gpu_helpers import G, dev, rbf_dict, relmax, spec_from

DT = torch.float64
# the results of one differentiated call / of a truth function, in one layout for every family (meas None: nothing was measured)
Run = collections.namedtuple("Run", "states inputs meas grads g_x0 status")
Truth = collections.namedtuple("Truth", "states inputs meas grads g_x0 vmin")


# ---- model pairs ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_pair(build_pair, shape, N, deg, seed):
    return build_pair(shape, N, deg, seed=seed)


@functools.lru_cache(maxsize=None)
def pair(build_pair, shape, N, deg, seed, vs=None, delta=False, delta_ts=False):
    """(cfg, oracle model, PackedModel on the oracle's own Kinv / alpha); built once per process and shared, never modified.  ``build_pair``
    and ``seed`` name the oracle pair (one pretrain per key, whoever asks), ``vs`` the var_scale, ``delta`` the delta-state layout and
    ``delta_ts`` whether that layout gets the sampling time a measurement model needs."""
    from mc_pilco_amd import ops

    c, m, specs = _oracle_pair(build_pair, shape, N, deg, seed)
    gps = [ops.PackedGP(spec_from(*specs[g]), G(m.cache[g].X), G(m.cache[g].alpha), G(m.cache[g].Kinv)) for g in range(c["G"])]
    scale = None if vs is None else list(vs)
    if delta:
        ts = dict(Ts=c["Ts"]) if delta_ts else {}
        return c, m, ops.PackedModel.delta(gps, c["S"], c["U"], c["angle"], c["not_angle"], var_scale=scale, **ts)
    return c, m, ops.PackedModel(gps, c["S"], c["U"], c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"], var_scale=scale)


def open_pair(shape, N, deg, vs=None):
    """The pairs of tests/open_grad_models.py (seed N + deg)."""
    return pair(open_grad_models.build_pair, shape, N, deg, N + deg, vs, shape == "delta")


def zero_variance_model(D, at_one, S, U, Ts, angle, not_angle, vel, not_vel):
    """Two GPs with a known non-positive variance, by the recipe of tests/test_gpu_dropin.py::
    test_zero_predictive_variance_raises_like_the_reference_normal: one training point exactly at the GP input of x = 0, u = 0 (its cosine
    features ``at_one``), no noise, Kinv = I -> var = 1 - 1 = 0; the other rows far away (k = 0 there)."""
    from mc_pilco_amd import ops

    X = np.zeros((16, D))
    X[:, at_one] = 1.0
    X[1:, 0] = 50.0 + np.arange(15)
    gp = ops.PackedGP(spec_from(np.ones(D), 0.0), G(X), G(np.zeros(16)), G(np.eye(16)))
    return ops.PackedModel([gp, gp], S, U, Ts, angle, not_angle, vel, not_vel)


def zero_variance_arm(c):
    """On the arm2 shape: z = [x2, x3, sin x0, sin x1, cos x0, cos x1, u0, u1]."""
    return zero_variance_model(8, slice(4, 6), c["S"], c["U"], c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])


# ---- noise, measurement, class-path arguments ---------------------------------------------------------------------------------------------------
def noise_of(kind, eps, **kw):
    """``kind`` in ("mean", "eps", "philox"): None, the buffer, or Philox at seed 11 / call 3."""
    from mc_pilco_amd import ops

    return None if kind == "mean" else (ops.NoiseSpec(eps=G(eps)) if kind == "eps" else ops.NoiseSpec(seed=11, call=3, **kw))


def noise_buffer(eps):
    from mc_pilco_amd import ops

    return ops.NoiseSpec(eps=G(eps))


def meas_spec(ms, pos_noise=None):
    from mc_pilco_amd import ops

    if ms is None:
        return None
    return ops.MeasSpec(pos=ms["pos"], vel=ms["vel"], std_pos=ms["std"], b=ms["b"], a=ms["a"], pos_noise=None if pos_noise is None else G(pos_noise))


def sim_args(M, T, mean=(0.1, -0.1, 0.0, 0.05), var=(1e-2, 1e-2, 2e-2, 2e-2)):
    return dict(particles_initial_state_mean=G(mean), particles_initial_state_var=G(var), flg_particles_init_uniform=False,
                particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False, num_particles=M, T_control=T)


def reinforce_args(sim, T, steps, **kw):
    """reinforce_policy's arguments for ``steps`` Adam steps at lr 0.01 on the particles of ``sim``."""
    out = {k: v for k, v in sim.items() if k != "T_control"}
    return dict(out, T_control=0.05 * T, trial_index=0, opt_steps_list=[steps], lr_list=[0.01], f_optimizer="lambda p, lr : torch.optim.Adam(p, lr)",
                num_step_print=10, policy_reinit_dict=None, **kw)


@contextlib.contextmanager
def normal_draws_on_the_cpu():
    """The step path samples with Normal(mu, sigma).rsample() on the model's device; the reference runs on the CPU, and "reference" noise mode
    replays ITS draws.  For the comparison the step path's standard normals are taken from the CPU generator, as the reference takes them."""
    import torch.distributions.normal as tdn

    orig = tdn._standard_normal
    tdn._standard_normal = lambda shape, dtype, device: torch.empty(tuple(shape), dtype=dtype).normal_().to(device)
    try:
        yield
    finally:
        tdn._standard_normal = orig


# ---- class-path objects ---------------------------------------------------------------------------------------------------------------------
def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def policy_learning_object(ml, Ts, f_policy, policy_par, pms=None):
    """MC_PILCO around the trained model ``ml`` and the policy ``f_policy(**policy_par)``, or MC_PILCO4PMS with the keywords ``pms``."""
    from mc_pilco_amd.policy_learning import MC_PILCO, Cost_function, Policy

    common = dict(T_sampling=Ts, state_dim=4, input_dim=2, f_sim=lambda y, t, u: None, f_model_learning=lambda **kw: ml, model_learning_par={},
                  f_rand_exploration_policy=Policy.Random_exploration, rand_exploration_policy_par=dict(state_dim=4, input_dim=2, u_max=1.0, dtype=DT),
                  f_control_policy=f_policy, control_policy_par=policy_par, f_cost_function=Cost_function.Expected_saturated_distance,
                  cost_function_par=dict(target_state=G([0.2, -0.1]), lengthscales=G([0.5, 0.5]), active_dims=np.array([0, 1])), log_path=None,
                  dtype=DT, device=dev())
    with quiet():
        return MC_PILCO.MC_PILCO(**common) if pms is None else MC_PILCO.MC_PILCO4PMS(**common, **pms)


def trained(ml, x, u):
    with quiet():
        ml.add_data(x, u)
        with torch.no_grad():
            for g in range(ml.num_gp):
                ml.pretrain_gp(g)
        ml.set_eval_mode()
    return ml


ARM_PMS = dict(pos_indeces=[0, 1], vel_indeces=[2, 3], std_meas_noise=np.array([0.02, 0.03, 0.0, 0.0]), filtering_dict={"fc": 0.3})


def arm_object(f_policy, policy_par, pms=None):
    """MC_PILCO (``pms``: MC_PILCO4PMS with those keywords, e.g. ARM_PMS: both joints measured, a first-order filter with memory, position
    noise on both) over a fused-layout arm2 speed model trained on a short recorded trajectory, in "reference" noise mode."""
    from mc_pilco_amd.model_learning import Model_learning as ML

    c = pd_models.SHAPES["arm2"]
    rs = np.random.RandomState(3)
    n, Ts = 60, c["Ts"]
    tt = Ts * np.arange(n + 1).reshape(-1, 1)
    u = 0.8 * np.sin(2 * np.pi * (0.3 + 0.9 * rs.rand(1, 2)) * tt + 6.28 * rs.rand(1, 2))
    x = np.zeros((n + 1, 4))
    x[0] = [0.3, -0.2, 0.0, 0.0]
    for i in range(n):
        q, qd = x[i, :2], x[i, 2:]
        qdd = -4.0 * np.sin(q) - 0.4 * qd + 3.0 * u[i]
        x[i + 1, 2:] = qd + Ts * qdd
        x[i + 1, :2] = q + Ts * qd + 0.5 * Ts * Ts * qdd
    with quiet():
        ml = ML.Speed_Model_learning_RBF_angle_state(num_gp=2, init_dict_list=[rbf_dict(8, np.ones(8) * 2.0, 0.05)] * 2, T_sampling=Ts,
                                                     angle_indeces=c["angle"], not_angle_indeces=c["not_angle"], vel_indeces=c["vel"],
                                                     not_vel_indeces=c["not_vel"], dtype=DT, device=dev())
    obj = policy_learning_object(trained(ml, x, u), Ts, f_policy, policy_par, pms)
    obj.noise_mode = "reference"
    return obj


# ---- policies -------------------------------------------------------------------------------------------------------------------------------
def controller(c, kp, kd, target, u_max=1.0, squash=True, trainable=True):
    from mc_pilco_amd.policy_learning import Policy

    return Policy.PD_controller(state_dim=c["S"], input_dim=c["U"], sqrt_Kp_gains=kp.numpy(), sqrt_Kd_gains=kd.numpy(), target_traj=G(target),
                                flg_squash=squash, u_max=u_max, flg_trainable=trainable, dtype=DT, device=dev())


def policy(c, params, hidden, angle=None, non_angle=None, u_max=1.0, squash=True, trainable=True):
    from mc_pilco_amd.policy_learning import Policy

    angle = c["angle"] if angle is None else angle
    non_angle = c["not_angle"] if non_angle is None else non_angle
    pol = Policy.MLP_policy(state_dim=c["S"], input_dim=c["U"], hidden_sizes=list(hidden), angle_indices=angle or None, non_angle_indices=non_angle or None,
                            u_max=u_max, flg_squash=squash, weight_init=params, dtype=DT, device=dev())
    for q in pol.parameters():
        q.requires_grad_(trainable)
    return pol


def arm_pd_par(kp, kd, target):
    return dict(state_dim=4, input_dim=2, sqrt_Kp_gains=np.asarray(kp), sqrt_Kd_gains=np.asarray(kd), target_traj=G(target), flg_squash=True, u_max=1.5,
                flg_trainable=True, dtype=DT, device=dev())


def arm_mlp_par(params, hidden, **kw):
    c = pd_models.SHAPES["arm2"]
    return dict(state_dim=4, input_dim=2, hidden_sizes=list(hidden), angle_indices=c["angle"], non_angle_indices=c["not_angle"], u_max=1.5,
                flg_squash=True, weight_init=params, dtype=DT, device=dev(), **kw)


# ---- the families ---------------------------------------------------------------------------------------------------------------------------
class Family:
    """One policy of the fused closed loop: ``op`` (the name of the ops function: ``meas=`` and ``p_drop=`` where they apply), ``params``
    (policy object -> the tensors whose .grad is compared), ``grad_text`` (their errors as the printed lines name them), ``models`` (whose
    build_pair makes the pairs) and ``pair_seed`` ((N, deg) -> the seed of a pair)."""

    def __init__(self, op, params, grad_text, models, pair_seed):
        self.op_name, self.params, self.grad_text, self.models, self.pair_seed = op, params, grad_text, models, pair_seed

    def op(self, *a, **kw):
        from mc_pilco_amd import ops

        return getattr(ops, self.op_name)(*a, **{k: v for k, v in kw.items() if not (k == "p_drop" and v is None)})

    def pair(self, shape, N, deg, vs=None, measured=False):
        """``measured``: with the sampling time a measurement model needs on the delta-state layout too."""
        return pair(self.models.build_pair, shape, N, deg, self.pair_seed(N, deg), vs, pd_models.family(shape) == "delta", measured)

    def run(self, pm, pol, x0, T, noise, w, wu, sample, meas=None, p_drop=None, x0_grad=True):
        """One differentiated call of the op with L = sum w states + sum wu inputs (wu None: states only): a Run, its gradients in the order
        of ``params`` (None where a tensor does not require grad)."""
        for q in pol.parameters():
            q.grad = None
        xg = G(x0).requires_grad_(x0_grad)
        st, inp, status = self.op(pm, pol.packed(), noise, xg, T, particle_pred=sample, meas=meas, p_drop=p_drop)
        ym = None
        if meas is not None:
            ym = meas.measured
            assert not ym.requires_grad and tuple(ym.shape) == tuple(st.shape)
        L = (G(w) * st).sum() + (0.0 if wu is None else (G(wu) * inp).sum())
        L.backward()
        return Run(st.detach(), inp.detach(), ym, [None if q.grad is None else q.grad.clone() for q in self.params(pol)], xg.grad, int(status.item()))


PD = Family("rollout_pd", lambda pol: [pol.sqrt_Kp_gains, pol.sqrt_Kd_gains], lambda e: "g_sqrt_kp %.3e g_sqrt_kd %.3e" % tuple(e), pd_models,
            lambda N, deg: N + deg)
MLP = Family("rollout_mlp", lambda pol: list(pol.mlp_parameters()), lambda e: "g_params " + " ".join("%.3e" % v for v in e), mlp_models,
             lambda N, deg: mlp_models.PAIR_SEED)


def pd_truth_of(t):
    """The tuples of pd_models.pd_truth / pd_meas_models.pd_meas_truth as a Truth."""
    return Truth(t[0], t[1], t[2] if len(t) == 7 else None, list(t[-4:-2]), t[-2], t[-1])


def mlp_truth_of(t):
    """The tuples of mlp_models.mlp_truth / mlp_meas_models.mlp_meas_truth / mlp_drop_models.drop_truth as a Truth."""
    return Truth(t[0], t[1], t[2] if len(t) == 6 else None, t[-3], t[-2], t[-1])


# ---- the repeated bodies ----------------------------------------------------------------------------------------------------------------------
def errors(truth, got, only=None):
    """(max |states|, max |inputs|, max |meas| or None, [relmax per parameter gradient], relmax g_x0) of a Run against a Truth.  ``only``:
    requires_grad was on that tensor alone -- neither x0 nor the other parameters got a gradient."""
    es, ei = float((got.states.cpu() - truth.states).abs().max()), float((got.inputs.cpu() - truth.inputs).abs().max())
    em = None if truth.meas is None else float((got.meas.cpu() - truth.meas).abs().max())
    if only is None:
        return es, ei, em, [relmax(g, o) for g, o in zip(got.grads, truth.grads)], relmax(got.g_x0, truth.g_x0)
    assert got.g_x0 is None and all((g is None) == (i != only) for i, g in enumerate(got.grads))
    return es, ei, em, [relmax(got.grads[only], truth.grads[only])], 0.0


def check_against(fam, what, truth, got, tols, only=None):
    """The printed line of a comparison and its assertions: status 0, states (and measurements) / inputs / every gradient within
    ``tols`` = (STATE_TOL, INPUT_TOL, GRAD_TOL) of the calling module."""
    es, ei, em, eg, ex = errors(truth, got, only)
    meas = "" if em is None else "meas %.3e " % em
    print("%s: states %.3e inputs %.3e %s%s g_x0 %.3e (min var %.3e)" % (what, es, ei, meas, fam.grad_text(eg), ex, truth.vmin))
    assert got.status == 0
    assert es < tols[0] and ei < tols[1] and (em is None or em < tols[0])
    assert max(eg) < tols[2] and ex < tols[2]


def three_way_bit_identity(fam, pm, pol, x0, eps, T, kind, meas=None, sweep=None):
    """The plain launch (nothing requires grad), the open-loop launch on that launch's own inputs and the recording launch carry the same
    bits.  ``meas``: () -> a MeasSpec; the measurements agree too, a measurement was simulated and row 0 is the true state.  ``sweep`` =
    (w, wu): the sweep over that record runs and leaves finite, non-zero gradients."""
    from mc_pilco_amd import ops

    sample = kind != "mean"
    s1, s2 = (meas(), meas()) if meas else (None, None)
    with torch.no_grad():
        st, inp, status = fam.op(pm, pol.packed(), noise_of(kind, eps), G(x0), T, particle_pred=sample, meas=s1)
    assert int(status.item()) == 0 and not st.requires_grad
    so, status_o = ops.rollout_open(pm, G(x0), inp[:T - 1].contiguous(), noise=noise_of(kind, eps), particle_pred=sample)
    assert int(status_o.item()) == 0
    assert torch.equal(st, so)  # the same phases on the same operands
    sr, ir, status_r = fam.op(pm, pol.packed(), noise_of(kind, eps), G(x0), T, particle_pred=sample, meas=s2)  # the parameters require grad: recording
    assert sr.requires_grad and int(status_r.item()) == 0
    assert torch.equal(sr.detach(), st) and torch.equal(ir.detach(), inp)
    if meas:
        ym = s1.measured
        assert torch.equal(s2.measured, ym)
        assert float((ym[1:, :, :2] - st[1:, :, :2]).abs().min()) > 0 and torch.equal(ym[0], st[0])  # a measurement was simulated; row 0 is true
    if sweep:
        ((G(sweep[0]) * sr).sum() + (G(sweep[1]) * ir).sum()).backward()
        assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0 for q in fam.params(pol))


def rung_of_the_recording_form(fam, what, pm, pol, x0, eps, T, w, wu, truth, tols, meas=None):
    """Sampled: status 0; states, inputs (and measurements) of the recording launch carry the bits of the launch without a record, whose
    states carry the bits of the open-loop launch on its inputs; everything against the truth."""
    from mc_pilco_amd import ops

    got = fam.run(pm, pol, x0, T, noise_buffer(eps), w, wu, True, meas=meas() if meas else None)
    s0 = meas() if meas else None
    with torch.no_grad():
        st0, i0, status0 = fam.op(pm, pol.packed(), noise_buffer(eps), G(x0), T, particle_pred=True, meas=s0)
    so, status_o = ops.rollout_open(pm, G(x0), i0[:T - 1].contiguous(), noise=noise_buffer(eps), particle_pred=True)
    assert int(status0.item()) == 0 and int(status_o.item()) == 0
    assert torch.equal(got.states, st0) and torch.equal(got.inputs, i0) and torch.equal(st0, so)
    assert meas is None or torch.equal(got.meas, s0.measured)
    check_against(fam, what, truth, got, tols)


def four_trajectory_tile_without_a_record(fam, what, pm, pol, x0, eps, T, truth, tols, meas=None):
    """Sampled, nothing requires grad: status 0, the states carry the bits of the open-loop launch on the inputs; states, inputs (and
    measurements) against the truth -- without a truth, finite inputs.  (No record, so no gradient to compare.)"""
    from mc_pilco_amd import ops

    sp = meas() if meas else None
    st, inp, status = fam.op(pm, pol.packed(), noise_buffer(eps), G(x0), T, particle_pred=True, meas=sp)
    so, status_o = ops.rollout_open(pm, G(x0), inp[:T - 1].contiguous(), noise=noise_buffer(eps), particle_pred=True)
    assert int(status.item()) == 0 and int(status_o.item()) == 0 and not st.requires_grad
    assert torch.equal(st, so)
    if truth is None:
        assert bool(torch.isfinite(inp).all())
        return
    es, ei = float((st.cpu() - truth.states).abs().max()), float((inp.cpu() - truth.inputs).abs().max())
    em = None if sp is None else float((sp.measured.cpu() - truth.meas).abs().max())
    print("%s, no record: states %.3e inputs %.3e %s(min var %.3e)" % (what, es, ei, "" if em is None else "meas %.3e " % em, truth.vmin))
    assert es < tols[0] and ei < tols[1] and (em is None or em < tols[0])


def central_differences(fam, pm, policy_of, tensors, x0, w, wu, T, checks, step, bound, p_drop=None):
    """Philox mode (seed 77, call 5): central differences of the op with ``step`` against the adjoint's gradient, to ``bound`` = (relative,
    floor).  ``policy_of(tensors, trainable)`` makes the policy; ``checks`` lists (printed name, place in tensors + [x0], flat entry)."""
    from mc_pilco_amd import ops

    nz = lambda: ops.NoiseSpec(seed=77, call=5)
    got = fam.run(pm, policy_of(tensors, True), x0, T, nz(), w, wu, True, p_drop=p_drop)
    assert got.status == 0

    def loss(ts):
        st, inp, s = fam.op(pm, policy_of(ts[:-1], False).packed(), nz(), G(ts[-1]), T, particle_pred=True, p_drop=p_drop)
        assert int(s.item()) == 0
        return float((G(w) * st).sum() + (G(wu) * inp).sum())

    for name, i, e in checks:
        g = float((got.grads + [got.g_x0])[i].cpu().reshape(-1)[e])
        plus, minus = [t.clone() for t in list(tensors) + [x0]], [t.clone() for t in list(tensors) + [x0]]
        plus[i].reshape(-1)[e] += step
        minus[i].reshape(-1)[e] -= step
        fd = (loss(plus) - loss(minus)) / (2 * step)
        print("%s: fd %.9e adjoint %.9e" % (name, fd, g))
        assert abs(fd - g) < bound[0] * max(abs(g), bound[1])


def first_and_last_entries(tensors):
    """The ``checks`` of central_differences that name the first and the last entry of every tensor."""
    return [("tensor %d entry %d" % (i, e), i, e) for i, q in enumerate(tensors) for e in (0, q.numel() - 1)]


def saved_record_refuses_in_place_changes(fam, pm, pol, x0, T, meas=None, weights=None):
    """Each saved output of the mean launch (states, inputs, and the measurements of a measured one), changed in place, makes backward raise."""
    import pytest

    for which in range(3 if meas else 2):
        sp = meas() if meas else None
        out = fam.op(pm, pol.packed(), None, G(x0), T, particle_pred=False, meas=sp)
        with torch.no_grad():
            (sp.measured if which == 2 else out[which]).mul_(2.0)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            (out[0].sum() + out[1].sum() if weights is None else (G(weights[0]) * out[0]).sum() + (G(weights[1]) * out[1]).sum()).backward()


def status_word(fam, pm, c, good, nan, zero, x0, eps, T):
    """Status 0 on a clean launch, STATUS_NAN on ``nan`` = (policy, x0) in both modes; STATUS_NONPOS_VAR alone, and finite states, under the
    zero-variance model with ``zero``, a policy that returns u = 0 exactly.  (Policies untrainable and packed.)"""
    from mc_pilco_amd import hipabi, ops

    for sample in (False, True):
        nz = noise_buffer(eps) if sample else None
        assert int(fam.op(pm, good, nz, G(x0), T, particle_pred=sample)[-1].item()) == 0
        assert int(fam.op(pm, nan[0], nz, G(nan[1]), T, particle_pred=sample)[-1].item()) & hipabi.STATUS_NAN
    st, _, status = fam.op(zero_variance_arm(c), zero, ops.NoiseSpec(seed=1, call=1), G(np.zeros((8, 4))), 2, particle_pred=True)
    assert int(status.item()) & hipabi.STATUS_NONPOS_VAR and not (int(status.item()) & hipabi.STATUS_NAN)
    assert bool(torch.isfinite(st).all())


# ---- two ranks --------------------------------------------------------------------------------------------------------------------------------
def sharded_step(fam, obj, world, sim, **apply_kw):
    """A rank's step of the two-rank tests (seed 17, Philox; every rank seeds torch alike: x0 is drawn for the whole swarm and sliced):
    (cost, std, flags, [parameter gradients], states, (offset, count))."""
    obj.seed = 17
    if world > 1:
        obj.shard_particles()
    torch.manual_seed(23)
    st, inp = obj.apply_policy(**sim, **apply_kw)
    assert obj.last_feedback_fused is True
    cost, std, flags = obj._cost_backward(st, inp, 0)
    torch.cuda.synchronize()
    grads = [q.grad.cpu().numpy().copy() for q in fam.params(obj.control_policy)]
    return float(cost.detach()), float(std.detach()), [float(v) for v in flags.tolist()], grads, st.detach().cpu().numpy(), obj._shard


def two_ranks_match_one_process(fam, one, two, tol, n_grads, M=17):
    """Per class: each rank's states are the matching slice of the one-process run bit for bit; the pooled cost, its std and the parameter
    gradients agree to ``tol`` (another order of the sums)."""
    one, two = dict(one)[0], dict(two)
    for cls_name in ("MC_PILCO", "MC_PILCO4PMS"):
        c1, s1, f1, g1, st1, _ = one[cls_name][:6]
        assert f1 == [0.0, 0.0, 0.0] and len(g1) == n_grads and all(float(np.abs(g).max()) > 0 for g in g1)
        seen = 0
        for r in range(2):
            c2, s2, f2, g2, st2, (off, cnt) = two[r][cls_name]
            assert np.array_equal(st2, st1[:, off:off + cnt])  # same noise (and masks) per GLOBAL particle
            seen += cnt
            eg = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g2, g1)]
            print("%s rank %d: cost %.3e std %.3e %s" % (cls_name, r, abs(c2 - c1), abs(s2 - s1), fam.grad_text(eg)))
            assert f2 == [0.0, 0.0, 0.0]
            assert abs(c2 - c1) < tol * abs(c1) and abs(s2 - s1) < tol * abs(s1)
            assert len(g2) == n_grads and max(eg) < tol
        assert seen == M
    return one
