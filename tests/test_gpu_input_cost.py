"""GPU: the control-effort and input-rate terms on the HIP cost kernels (mcp_cost_u_fwd / mcp_cost_u_bwd, ops.PackedCostInputs,
Cost_function.Input_penalty) against tests/input_cost_models.truth (the torch formula under autograd on CPU fp64) at the smallest shapes where
the indexing can go wrong; the dispatch without input terms, the status word, reproducibility, the sharded (summable) form, the class path of
every closed-loop policy against the torch path of the same cost, the recorded optimizer loop and two ranks on one device."""
import contextlib
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
import input_cost_models as icm
from closed_loop_family import MLP
from mlp_models import SHAPES as MLP_SHAPES
from mlp_models import network
from rank_harness import rank_group, run_ranks

pytestmark = pytest.mark.gpu
DT = torch.float64
CASES = icm.gpu_cases()
THIRD = icm.SHAPES[2]


def dev():
    return torch.device("cuda", 0)


def G(a):
    return torch.tensor(np.asarray(a), dtype=DT, device=dev())


def relerr(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def rel(a, b):
    a, b = (float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in (a, b))
    return abs(a - b) / abs(b)


def packed(c):
    """(PackedCost, PackedCostInputs) of a case of input_cost_models."""
    from mc_pilco_amd import ops

    S, U = c["x"].shape[2], c["u"].shape[2]
    if c["kind"] == "cartpole":
        pc = ops.PackedCost("cartpole", S, dev(), target_state=c["tg"], lengthscales=c["ls"], angle_index=c["used_x"][0], pos_index=c["used_x"][1])
    elif c["kind"] == "traj":
        pc = ops.PackedCost("traj", S, dev(), target_traj=c["tg"], lengthscales=c["ls"], used=c["used_x"])
    else:
        pc = ops.PackedCost("target", S, dev(), target_state=c["tg"], lengthscales=c["ls"], active_dims=c["used_x"], saturate=c["kind"] == "sat")
    return pc, ops.PackedCostInputs(U, dev(), c["used_u"], c["l"], c["r"], c["ustar"], c["joint"])


def run(pc, cin, x, u):
    """cost, std and both gradients through ops.expected_cost."""
    from mc_pilco_amd import ops

    st, inp = G(x).requires_grad_(True), G(u).requires_grad_(True)
    c, s = ops.expected_cost(pc, st, None, None, inp, cin)
    c.backward()
    return c.detach(), s.detach(), st.grad, inp.grad


@pytest.fixture(scope="module")
def truths():
    """Per case: the truth (CPU fp64 autograd), computed once."""
    return {name: icm.truth(c) for name, c in CASES}


# ---- 1: parity with the truth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_cost_and_gradients_match_the_truth(truths, name, c):
    """1e-12 relative on the max norm for cost, std, per-particle costs, g_states and g_inputs: the project's per-op bound, the one
    test_gpu_target_cost.py holds the state costs to.  Columns the cost does not read get exactly 0.0 in both gradients."""
    from mc_pilco_amd import ops

    tr = truths[name]
    pc, cin = packed(c)
    cost, std, gx, gu = run(pc, cin, c["x"], c["u"])
    _, costs, _ = ops.cost_moments(pc, G(c["x"]), None, G(c["u"]), cin)
    T, M, S = c["x"].shape
    U = c["u"].shape[2]
    assert costs.shape == (T, M) and gx.shape == (T, M, S) and gu.shape == (T, M, U)
    ec, es, ep, ex, eu = rel(cost, tr["cost"]), rel(std, tr["std"]), relerr(costs, tr["costs"]), relerr(gx, tr["g_states"]), relerr(gu, tr["g_inputs"])
    print("%s: cost %.2e std %.2e per-particle %.2e g_states %.2e g_inputs %.2e" % (name, ec, es, ep, ex, eu))
    assert ec < 1e-12 and es < 1e-12 and ep < 1e-12 and ex < 1e-12 and eu < 1e-12
    for g, used, n in ((gx, c["used_x"], S), (gu, c["used_u"], U)):
        unused = [i for i in range(n) if i not in used]
        if unused:
            assert float(g[:, :, unused].abs().sum()) == 0.0  # exactly zero, not small
    assert bool((gx[:, :, c["used_x"]] != 0).any())
    if float(tr["g_inputs"].abs().max()) > 0:  # (the rate-only case with one time step has no input gradient at all)
        assert bool((gu[:, :, c["used_u"]] != 0).any())


# ---- 2: without input terms the entries are mcp_cost_fwd / mcp_cost_bwd -----------------------------------------------------------------------
def test_descriptors_without_input_terms_give_the_bits_of_the_state_cost():
    from mc_pilco_amd import ops

    c = dict(CASES)["%s-sat-add-both" % icm.shape_id(THIRD)]
    pc, _ = packed(c)
    st = G(c["x"]).requires_grad_(True)
    c0, s0 = ops.expected_cost(pc, st)
    c0.backward()
    no_index, no_scales = packed(c)[1], packed(c)[1]
    no_index.c.n_used = 0
    no_scales.c.scales, no_scales.c.rate_scales = None, None
    for cin in (no_index, no_scales):
        cost, std, gx, gu = run(pc, cin, c["x"], c["u"])
        assert torch.equal(cost, c0.detach()) and torch.equal(std, s0.detach()) and torch.equal(gx, st.grad)
        assert gu.shape == c["u"].shape and float(gu.abs().sum()) == 0.0


# ---- 3: the status word -------------------------------------------------------------------------------------------------------------------------
def test_nan_in_a_used_input_column_raises_the_status_flag():
    """T = 3, M = 257, U = 3 with columns [1, 0] read: a NaN at [1, 256] in a used column raises MCP_STATUS_NAN and makes exactly that row's
    moment NaN (the rate term of row 2 reads it too, for that particle: its cost is NaN, so is row 2's moment when the rate term is on);
    a NaN in the column the cost does not read does neither."""
    from mc_pilco_amd import hipabi, ops

    T, M, S, _, used_x, used_u = THIRD
    d = icm.draw(T, M, S, 3, used_x, used_u)
    for kind in ("sat", "quad"):
        for terms in ("effort", "both"):
            c = icm.make_case(d, kind, False, terms)
            pc, cin = packed(c)
            for col, flagged in ((1, True), (2, False)):
                u = G(c["u"])
                u[1, 256, col] = float("nan")
                status = torch.zeros(1, dtype=torch.int32, device=dev())
                mom, costs, status = ops.cost_moments(pc, G(c["x"]), status, u, cin)
                assert bool(int(status.item()) & hipabi.STATUS_NAN) == flagged
                assert bool(torch.isnan(costs[1, 256])) == flagged and bool(torch.isnan(mom[1, 0])) == flagged
                after = flagged and terms == "both"  # (row 2 of that particle steps away from the NaN)
                assert bool(torch.isnan(mom[2, 0])) == after and bool(torch.isfinite(mom[0]).all())
                assert int(torch.isnan(costs).sum()) == (2 if after else (1 if flagged else 0))


# ---- 4: reproducible; a shard's rows are the whole swarm's ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,joint", [("sat", False), ("sat", True), ("quad", False), ("cartpole", True), ("traj", True)])
def test_two_runs_give_the_same_bits_and_columns_give_rows_of_the_whole(kind, joint):
    from mc_pilco_amd import ops

    c = icm.make_case(icm.draw(*THIRD), kind, joint, "both")
    pc, cin = packed(c)
    first, again = run(pc, cin, c["x"], c["u"]), run(pc, cin, c["x"], c["u"])
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    M = c["x"].shape[1]
    for a, b in ((0, 1), (3, 200), (200, 257)):  # columns [a, b) of the swarm with the whole swarm's gscale = 1 / M
        st, inp = G(c["x"][:, a:b]).requires_grad_(True), G(c["u"][:, a:b]).requires_grad_(True)
        share, _ = ops.local_cost(pc, st, M, None, None, inp, cin)
        share.backward()
        assert torch.equal(st.grad, first[2][:, a:b]) and torch.equal(inp.grad, first[3][:, a:b])


# ---- 5: the summable form of a sharded step, in one process ------------------------------------------------------------------------------------------
def penalty(state_cost, U, joint=False):
    """Input_penalty with both terms and a non-zero u* on every one of U inputs."""
    from mc_pilco_amd.policy_learning import Cost_function as CF

    return CF.Input_penalty(state_cost, lengthscales=[2.0, 1.5, 1.0][:U], rate_lengthscales=[1.0, 0.8, 1.2][:U], target_input=[0.3, -0.2, 0.1][:U],
                            joint=joint)


@pytest.mark.parametrize("with_shift", [False, True])
def test_sharded_sums_pool_to_the_whole_swarm(with_shift):
    """M = 24 as shards of 16 and 8, the body of test_gpu_target_cost.py's test of this name with inputs: local_moments into two sums buffers,
    added, then from_sums, against forward on the whole swarm.  Pooled cost 1e-13, std 1e-10 relative (tests/test_gpu_sharding.py:95-96); both
    gradients of the shards are rows of the whole swarm's, bit for bit."""
    from mc_pilco_amd.policy_learning import Cost_function as CF

    T, M, S, U, used = 6, 24, 4, 3, [2, 0]
    d = icm.draw(T, M, S, U, used, [0, 1, 2], seed=11)
    for cls in (CF.Expected_saturated_distance, CF.Expected_distance):
        for joint in (False, True):
            cf = penalty(cls(target_state=G(d["tg"].reshape(1, -1)), lengthscales=G(d["ls"]), active_dims=used), U, joint)
            whole, win = G(d["x"]).requires_grad_(True), G(d["u"]).requires_grad_(True)
            c, s = cf(whole, win, 0)
            c.backward()
            shift = torch.full((T,), float(c) / T, dtype=DT, device=dev()) if with_shift else None
            sums, gx, gu = [], [], []
            for a, b in ((0, 16), (16, 24)):
                part, pin = G(d["x"][:, a:b]).requires_grad_(True), G(d["u"][:, a:b]).requires_grad_(True)
                buf = torch.zeros(2 * T, dtype=DT, device=dev())
                share, sm = cf.local_moments(part, pin, 0, M, shift, sums_out=buf)
                assert sm.data_ptr() == buf.data_ptr()
                share.backward()
                sums.append(sm)
                gx.append(part.grad)
                gu.append(pin.grad)
            cp, sp = cf.from_sums(sums[0] + sums[1], M, shift)
            ec, es = rel(cp, c), rel(sp, s)
            print("%s joint=%s shift=%s: pooled cost %.2e std %.2e" % (cls.__name__, joint, with_shift, ec, es))
            assert cf._packed is not None and cf._in_packs
            assert ec < 1e-13 and es < 1e-10
            assert torch.equal(torch.cat(gx, 1), whole.grad) and torch.equal(torch.cat(gu, 1), win.grad)
            assert bool((win.grad != 0).all())


# ---- 6: the class path -- kernels against the torch path of the same cost ----------------------------------------------------------------------------
def _cartpole_object():
    from test_gpu_target_cost import tiny_mcpilco

    from mc_pilco_amd import synthetic as sy
    from mc_pilco_amd.policy_learning import Cost_function as CF

    c = sy.CARTPOLE
    obj = tiny_mcpilco()
    obj.noise_mode = "reference"
    sim = dict(particles_initial_state_mean=G(c["x0_mean"]), particles_initial_state_var=G(c["x0_var"]), flg_particles_init_uniform=False,
               particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False, num_particles=16, T_control=6)
    return obj, sim, CF.Cart_pole_cost(target_state=[np.pi, 0.0], lengthscales=[3.0, 1.0], angle_index=2, pos_index=0), 1


def _arm_object(policy, pms=False):
    from mc_pilco_amd.policy_learning import Cost_function as CF
    from mc_pilco_amd.policy_learning import Policy

    c = MLP_SHAPES["arm2"]
    if policy == "pd":
        target = 0.3 * np.sin(0.3 * np.arange(8).reshape(-1, 1) + np.array([0.0, 1.0, 2.0, 3.0]).reshape(1, -1))
        obj = clf.arm_object(Policy.PD_controller, clf.arm_pd_par([1.0, 1.2], [0.5, 0.4], target))
    else:
        obj = clf.arm_object(Policy.MLP_policy, clf.arm_mlp_par(network(c, (7, 3), c["angle"], c["not_angle"], 40), (7, 3)),
                             clf.ARM_PMS if pms else None)
    state_cost = CF.Expected_saturated_distance(target_state=G([0.2, -0.1]), lengthscales=G([0.5, 0.5]), active_dims=np.array([0, 1]))
    return obj, clf.sim_args(16, 6), state_cost, 2


@pytest.mark.parametrize("which", ["rbf", "pd", "mlp", "mlp-pms"])
def test_class_path_on_the_kernels_matches_the_torch_path(which):
    """One apply_policy + _cost_backward in "reference" noise mode with Input_penalty(state cost, both terms) on the kernels, with the same
    formula on the torch path (Expected_cost(cf.cost_function)), and with the state cost alone: the cost does not touch the forward (states
    and inputs equal bit for bit); cost and std agree to 1e-12; every parameter gradient to 1e-10 of its largest entry (the bound
    tests/test_gpu_policy_limits.py holds input functionals through rollout_backward_raw to); and the penalty reached the sweep (each
    parameter gradient differs from the one without it by more than 1e-6 of its largest entry)."""
    from mc_pilco_amd.policy_learning import Cost_function as CF

    obj, sim, state_cost, U = _cartpole_object() if which == "rbf" else _arm_object("pd" if which == "pd" else "mlp", which == "mlp-pms")
    cf = penalty(state_cost, U)
    params = [q for q in obj.control_policy.parameters() if q.requires_grad]
    assert params

    def step(cost_function):
        obj.cost_function = cost_function
        for q in params:
            q.grad = None
        torch.manual_seed(5)
        with clf.normal_draws_on_the_cpu(), clf.quiet():
            st, inp = obj.apply_policy(**sim)
            cost, std, _ = obj._cost_backward(st, inp, 0)
        return st.detach(), inp.detach(), cost.detach(), std.detach(), [q.grad.clone() for q in params]

    ks, ki, kc, kd, kg = step(cf)
    assert cf._packed is not None and cf._in_packs, "the kernels did not run"
    ts, ti, tc, td, tg = step(CF.Expected_cost(cf.cost_function))
    ps, pi, pc, _, pg = step(state_cost)
    assert torch.equal(ks, ts) and torch.equal(ki, ti) and torch.equal(ks, ps) and torch.equal(ki, pi)
    eg = [relerr(a, b) for a, b in zip(kg, tg)]
    moved = [relerr(a, b) for a, b in zip(pg, kg)]
    print("%s: cost %.2e std %.2e gradients %s; against the state cost alone: cost %.2e gradients %s"
          % (which, rel(kc, tc), rel(kd, td), " ".join("%.2e" % e for e in eg), rel(pc, kc), " ".join("%.2e" % e for e in moved)))
    assert rel(kc, tc) < 1e-12 and rel(kd, td) < 1e-12 and max(eg) < 1e-10
    assert min(moved) > 1e-6


# ---- 7: the optimizer loop records its attempts with the penalty ----------------------------------------------------------------------------------
def test_loop_with_an_input_penalty_replays_graphs_and_takes_the_eager_steps():
    """test_gpu_target_cost.py's loop test (4 steps, N = 48, M = 16, T = 6) with Input_penalty(Expected_saturated_distance, both terms):
    attempts replayed from HIP graphs against eager launches give the same cost list and policy parameters, bit for bit; the recording run
    did replay; and the cost list is not the one of the run without the penalty."""
    from test_gpu_target_cost import tiny_mcpilco

    from mc_pilco_amd import synthetic as sy
    from mc_pilco_amd.policy_learning import Cost_function as CF

    c = sy.CARTPOLE
    out = []
    for capture, with_penalty in ((True, True), (False, True), (False, False)):
        obj = tiny_mcpilco()
        obj.noise_mode = "philox"
        obj.capture_attempts = capture
        if with_penalty:
            obj.cost_function = CF.Input_penalty(obj.cost_function, lengthscales=[4.0], rate_lengthscales=[2.0])
        torch.manual_seed(1234)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = obj.reinforce_policy(T_control=0.31, num_particles=16, trial_index=0, particles_initial_state_mean=G(c["x0_mean"]),
                                       particles_initial_state_var=G(c["x0_var"]), flg_particles_init_uniform=False, particles_init_up_bound=None,
                                       particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
                                       f_optimizer="lambda p, lr : torch.optim.Adam(p, lr)", opt_steps_list=[4], lr_list=[0.01],
                                       p_dropout_list=[0.25], num_step_print=100)
        cf = obj.cost_function
        assert cf._packed is not None and cf._packed.kind == "target", "the loop's cost did not run on the kernels"
        assert bool(getattr(cf, "_in_packs", None)) == with_penalty
        if capture:
            assert "recording an attempt into a graph failed" not in buf.getvalue(), buf.getvalue()[-2000:]
            assert obj.attempts_replayed > 0, buf.getvalue()[-2000:]
        else:
            assert obj.attempts_replayed == 0
        pol = obj.control_policy
        out.append((np.asarray(res[0]), [q.detach().cpu().numpy().copy() for q in (pol.log_lengthscales, pol.centers, pol.f_linear.weight)]))
    (c1, p1), (c0, p0), (cn, _) = out
    assert c0.shape == (4,) and np.isfinite(c0).all()
    assert np.array_equal(c1, c0)
    for a, b in zip(p1, p0):
        assert np.array_equal(a, b)
    assert cn.shape == (4,) and not np.array_equal(cn, c0) and bool(np.all(np.abs(cn - c0) > 1e-6 * np.abs(c0)))


# ---- 8: two ranks on one device ---------------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401

    torch.cuda.set_device(dev())
    with rank_group(rank, world, port):
        obj, _, state_cost, U = _arm_object("mlp")
        obj.noise_mode = "philox"
        obj.cost_function = penalty(state_cost, U)
        res = clf.sharded_step(MLP, obj, world, clf.sim_args(17, 6))
        assert obj.cost_function._packed is not None and obj.cost_function._in_packs
        out_q.put((rank, res))


def test_two_rank_particle_sharding_matches_single_process():
    """MLP_policy under shard_particles with the penalty (M = 17, T = 6, Philox; three GPU processes in all): each rank's states are the
    matching slice of the one-process run bit for bit; the pooled cost agrees to 1e-13, its std to 1e-10 (tests/test_gpu_sharding.py:95-96);
    the six parameter gradients to 1e-9, the bound tests/test_gpu_mlp_meas.py's two-rank test asserts (another order of the sums)."""
    c1, s1, f1, g1, st1, _ = dict(run_ranks(_rank, 1))[0]
    two = dict(run_ranks(_rank, 2))
    assert f1 == [0.0, 0.0, 0.0] and len(g1) == 6 and all(float(np.abs(g).max()) > 0 for g in g1)
    seen = 0
    for r in range(2):
        c2, s2, f2, g2, st2, (off, cnt) = two[r]
        assert np.array_equal(st2, st1[:, off:off + cnt])
        seen += cnt
        eg = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g2, g1)]
        print("rank %d: cost %.3e std %.3e gradients %s" % (r, abs(c2 - c1) / abs(c1), abs(s2 - s1) / abs(s1), " ".join("%.3e" % e for e in eg)))
        assert f2 == [0.0, 0.0, 0.0]
        assert abs(c2 - c1) < 1e-13 * abs(c1) and abs(s2 - s1) < 1e-10 * abs(s1)
        assert len(g2) == 6 and max(eg) < 1e-9
    assert seen == 17
