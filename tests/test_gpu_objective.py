"""GPU: the time-weighted, risk-sensitive objective on the HIP cost kernels (mcp_cost_rows / mcp_cost_rows_sums / mcp_cost_bwd_shaped,
ops.PackedObjective, Cost_function.Cost_shaping) against tests/objective_truth.truth (torch autograd of sum_t w_t (mean + kappa std) on CPU
fp64) at the smallest shapes where the indexing can go wrong; the stride of the rows kernels, the identity with today's entries, reproducibility
and shard-exactness, the zero-spread convention, the status word, the class path of every closed-loop policy, the recorded optimizer loop and
two ranks on one device."""
import contextlib
import io

import numpy as np
import pytest
import torch

import closed_loop_family as clf
import input_cost_models as icm
import objective_truth as ot
from closed_loop_family import MLP
from rank_harness import rank_group, run_ranks
from test_gpu_input_cost import G, _arm_object, _cartpole_object, dev, packed, penalty, rel, relerr
from test_objective_cpu import cost_object, zero_spread_case

pytestmark = pytest.mark.gpu
DT = torch.float64
CASES = ot.gpu_cases()
THIRD = icm.SHAPES[2]


def objective(ws, kappa, T):
    from mc_pilco_amd import ops

    w = ot.weights(ws, T)
    return w, ops.PackedObjective(T, dev(), time_weights=(w if ws == "explicit" else None), discount=(0.9 if ws == "discount" else None), risk=kappa)


def packed_cost(c):
    """The PackedCost of a case (test_gpu_input_cost.packed without the inputs descriptor: a state-only case has none)."""
    from mc_pilco_amd import ops

    S = c["x"].shape[2]
    if c["kind"] == "cartpole":
        return ops.PackedCost("cartpole", S, dev(), target_state=c["tg"], lengthscales=c["ls"], angle_index=c["used_x"][0], pos_index=c["used_x"][1])
    if c["kind"] == "traj":
        return ops.PackedCost("traj", S, dev(), target_traj=c["tg"], lengthscales=c["ls"], used=c["used_x"])
    return ops.PackedCost("target", S, dev(), target_state=c["tg"], lengthscales=c["ls"], active_dims=c["used_x"], saturate=c["kind"] == "sat")


def run(pc, cin, obj, x, u):
    """J, S, rows and both gradients through ops.expected_cost (cin None: the state cost alone, no inputs gradient)."""
    from mc_pilco_amd import ops

    st, inp = G(x).requires_grad_(True), G(u).requires_grad_(True)
    J, S = ops.expected_cost(pc, st, None, None, None if cin is None else inp, cin, obj)
    J.backward()
    mom, _, _ = ops.cost_moments(pc, G(x), None, None if cin is None else G(u), cin)
    rows, out = ops.cost_rows(mom.unsqueeze(0), [x.shape[1]], obj)
    assert torch.equal(out[0], J.detach()) and torch.equal(out[1], S.detach())
    return J.detach(), S.detach(), rows, st.grad, (torch.zeros_like(inp) if inp.grad is None else inp.grad)


@pytest.fixture(scope="module")
def truths():
    """Per (case, objective): the truth (CPU fp64 autograd), computed once."""
    return {(name, ws, k): ot.truth(c, ot.weights(ws, c["x"].shape[0]), k) for name, c, _ in CASES for ws, k in ot.OBJECTIVES}


# ---- 1: parity with the truth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,c,has_inputs", CASES, ids=[n for n, _, _ in CASES])
def test_objective_and_gradients_match_the_truth(truths, name, c, has_inputs):
    """1e-12 of each tensor's largest entry on J, S, rows, g_states and g_inputs, with (discount, kappa = 0), (no weights, kappa = 0.7) and
    (explicit weights holding a zero, kappa = -0.5): the bound tests/test_gpu_input_cost.py holds these kernels to, kept because every case has
    sigma_t >= 0.05 max|c| (tests/test_objective_cpu.py).  Columns the cost does not read stay exactly 0."""
    T, M, S = c["x"].shape
    pc, cin = packed(c) if has_inputs else (packed_cost(c), None)
    for ws, kappa in ot.OBJECTIVES:
        tr = truths[(name, ws, kappa)]
        _, obj = objective(ws, kappa, T)
        J, Sd, rows, gx, gu = run(pc, cin, obj, c["x"], c["u"])
        errs = (rel(J, tr["J"]), rel(Sd, tr["S"]), relerr(rows, tr["rows"]), relerr(gx, tr["g_states"]),
                relerr(gu, tr["g_inputs"]) if has_inputs else float(gu.abs().max()))
        print("%s %s kappa %+.1f: J %.2e S %.2e rows %.2e g_states %.2e g_inputs %.2e" % ((name, ws, kappa) + errs))
        assert max(errs) < 1e-12
        assert gx.shape == (T, M, S) and bool((gx[:, :, c["used_x"]] != 0).any())
        unused = [i for i in range(S) if i not in c["used_x"]]
        if unused:
            assert float(gx[:, :, unused].abs().sum()) == 0.0
        if ws == "explicit" and T >= 3:  # (the zero weight: that row's gradients are exactly zero, apart from the rate term reaching in from row 2)
            assert float(gx[1].abs().sum()) == 0.0


# ---- 2: the stride of the rows kernels --------------------------------------------------------------------------------------------------------
def test_rows_kernels_take_more_than_256_time_steps():
    """T = 257, M = 3, S = 1: thread 0 takes rows 0 and 256, through mcp_cost_rows and mcp_cost_rows_sums (shift: the true means, so that the
    summable form has nothing to cancel), with explicit weights and kappa = -0.5."""
    from mc_pilco_amd import ops

    T, M = 257, 3
    c = ot.no_inputs(icm.make_case(icm.draw(T, M, 1, 1, [0], [0]), "sat", False, "both"))
    w, obj = objective("explicit", -0.5, T)
    tr = ot.truth(c, w, -0.5)
    pc = packed_cost(c)
    mom, _, _ = ops.cost_moments(pc, G(c["x"]))
    rows, out = ops.cost_rows(mom.unsqueeze(0), [M], obj)
    shift = tr["rows"][:, 0].to(dev()).contiguous()
    sums = torch.empty(2 * T, dtype=DT, device=dev())
    ops.abi.check(ops.abi.lib().mcp_cost_sums(T, M, ops.abi.ptr(mom), ops.abi.ptr(shift), ops.abi.ptr(sums), ops.abi.stream()), "mcp_cost_sums")
    mean_out = torch.empty(T, dtype=DT, device=dev())
    rows_s, out_s = ops.cost_rows_sums(sums, M, shift, mean_out, obj)
    for r, o in ((rows, out), (rows_s, out_s)):
        e = (relerr(r[:, 0], tr["rows"][:, 0]), relerr(r[:, 1], tr["rows"][:, 1]), rel(o[0], tr["J"]), rel(o[1], tr["S"]))
        print("T = 257: mean rows %.2e std rows %.2e J %.2e S %.2e" % e)
        assert max(e) < 1e-12
        assert float((r[256] - tr["rows"][256].to(dev())).abs().max()) < 1e-12
    assert torch.equal(mean_out, rows_s[:, 0])


# ---- 3: without an objective the entries give today's bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("joint", [False, True])
def test_no_objective_gives_the_bits_of_the_plain_entries(joint):
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import Cost_function as CF

    c = dict((n, c) for n, c, _ in CASES)["%s-sat-%s-both" % (icm.shape_id(THIRD), "joint" if joint else "add")]
    T, M, _ = c["x"].shape
    pc, cin = packed(c)
    trivial = ops.PackedObjective(T, dev())
    assert trivial.w is None and trivial.c.w is None and trivial.c.kappa == 0.0
    one = torch.ones(1, dtype=DT, device=dev())
    for ci in (None, cin):
        st, inp = G(c["x"]).requires_grad_(True), G(c["u"]).requires_grad_(True)
        J0, S0 = ops.expected_cost(pc, st, None, None, None if ci is None else inp, ci)
        J0.backward()
        mom, costs, _ = ops.cost_moments(pc, G(c["x"]), None, None if ci is None else G(c["u"]), ci)
        fin = ops.cost_finalize(mom.unsqueeze(0), [M])
        assert torch.equal(fin[0], J0.detach()) and torch.equal(fin[1], S0.detach())
        for obj in (None, trivial):
            rows, out = ops.cost_rows(mom.unsqueeze(0), [M], obj)
            assert torch.equal(out, fin)
            gx, gu = ops._cost_bwd_shaped(pc, ci, obj, G(c["x"]), None if ci is None else G(c["u"]), costs, rows, one, M, True)
            assert torch.equal(gx, st.grad)
            assert (ci is None and gu is None) or torch.equal(gu, inp.grad)
    # the class with no option: the wrapped cost's outputs and gradients
    inner = cost_object(c, dev())
    res = []
    for cf in (CF.Cost_shaping(inner), inner):
        st, inp = G(c["x"]).requires_grad_(True), G(c["u"]).requires_grad_(True)
        J, S = cf(st, inp, 0)
        J.backward()
        res.append((J.detach(), S.detach(), st.grad, inp.grad))
    assert inner._packed is not None and all(torch.equal(a, b) for a, b in zip(*res))


# ---- 4: reproducible; a shard's rows are the whole swarm's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,joint", [("sat", True), ("quad", False), ("cartpole", False), ("traj", True)])
def test_two_runs_give_the_same_bits_and_shards_give_columns_of_the_whole(kind, joint):
    """M = 257 as 100 + 157 with explicit weights and kappa = -0.5: mcp_cost_rows on the two shards' moments pools to the one-swarm rows at
    1e-12; mcp_cost_bwd_shaped on each shard, fed the SAME rows and n_total = 257, gives the matching columns of the whole-swarm launch bit
    for bit; the summable form (mcp_cost_sums -> add -> mcp_cost_rows_sums, with and without a shift) pools J to 1e-13 and S to 1e-10, the bounds
    of test_gpu_input_cost.py::test_sharded_sums_pool_to_the_whole_swarm."""
    from mc_pilco_amd import ops

    c = icm.make_case(icm.draw(*THIRD), kind, joint, "both")
    T, M, _ = c["x"].shape
    pc, cin = packed(c)
    _, obj = objective("explicit", -0.5, T)
    first, again = run(pc, cin, obj, c["x"], c["u"]), run(pc, cin, obj, c["x"], c["u"])
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    J, S, rows, gx, gu = first
    one = torch.ones(1, dtype=DT, device=dev())
    parts = []
    for a, b in ((0, 100), (100, 257)):
        x, u = G(c["x"][:, a:b]), G(c["u"][:, a:b])
        mom, costs, _ = ops.cost_moments(pc, x, None, u, cin)
        px, pu = ops._cost_bwd_shaped(pc, cin, obj, x, u, costs, rows, one, M, True)
        assert torch.equal(px, gx[:, a:b]) and torch.equal(pu, gu[:, a:b])
        parts.append((mom, b - a))
    prow, pout = ops.cost_rows(torch.stack([p[0] for p in parts]), [p[1] for p in parts], obj)
    e = (relerr(prow, rows), rel(pout[0], J), rel(pout[1], S))
    print("%s joint=%s: pooled rows %.2e J %.2e S %.2e" % ((kind, joint) + e))
    assert max(e) < 1e-12
    for ws, kappa in (("explicit", -0.5), ("discount", 0.0)):
        _, ob = objective(ws, kappa, T)
        _, whole = ops.cost_rows(torch.stack([ops.cost_moments(pc, G(c["x"]), None, G(c["u"]), cin)[0]]), [M], ob)
        for shift in (None, torch.full((T,), float(rows[:, 0].mean()), dtype=DT, device=dev())):
            total = torch.zeros(2 * T, dtype=DT, device=dev())
            for mom, n in parts:
                sums = torch.empty(2 * T, dtype=DT, device=dev())
                ops.abi.check(ops.abi.lib().mcp_cost_sums(T, n, ops.abi.ptr(mom), ops.abi.ptr(shift), ops.abi.ptr(sums), ops.abi.stream()), "mcp_cost_sums")
                total += sums
            out = ops.cost_from_sums(total, M, shift, None, ob)
            print("%s joint=%s %s kappa %+.1f shift=%s: pooled J %.2e S %.2e" % (kind, joint, ws, kappa, shift is not None, rel(out[0], whole[0]), rel(out[1], whole[1])))
            assert rel(out[0], whole[0]) < 1e-13 and rel(out[1], whole[1]) < 1e-10


# ---- 5: a row without spread ---------------------------------------------------------------------------------------------------------------------
def test_a_row_of_identical_costs_keeps_the_mean_only_factor():
    """T = 2, M = 4, row 0 the same for every particle: finite gradients equal to the convention's truth at 1e-12 (row 0: w_0 / n times the
    gradient of the plain sum), and no status flag."""
    from mc_pilco_amd import ops

    c = zero_spread_case()
    w = np.array([0.6, 1.7])
    tr = ot.truth(c, w, 0.7)
    pc, cin = packed(c)
    obj = ops.PackedObjective(2, dev(), time_weights=w, risk=0.7)
    J, S, rows, gx, gu = run(pc, cin, obj, c["x"], c["u"])
    assert float(rows[0, 1]) == 0.0 and float(rows[1, 1]) > 0.0
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gu).all())
    e = (rel(J, tr["J"]), rel(S, tr["S"]), relerr(gx, tr["g_states"]), relerr(gu, tr["g_inputs"]))
    print("zero-spread row: J %.2e S %.2e g_states %.2e g_inputs %.2e" % e)
    assert max(e) < 1e-12
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    ops.cost_moments(pc, G(c["x"]), status, G(c["u"]), cin)
    assert int(status.item()) == 0


# ---- 6: the status word ----------------------------------------------------------------------------------------------------------------------------
def test_a_nan_particle_raises_the_status_flag_and_makes_J_nan():
    from mc_pilco_amd import hipabi, ops

    c = icm.make_case(icm.draw(*THIRD), "sat", False, "both")
    pc, cin = packed(c)
    _, obj = objective("discount", 0.7, 3)
    x = G(c["x"])
    x[1, 256, c["used_x"][0]] = float("nan")
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    mom, _, status = ops.cost_moments(pc, x, status, G(c["u"]), cin)
    assert int(status.item()) & hipabi.STATUS_NAN
    J, _ = ops.expected_cost(pc, x, None, None, G(c["u"]), cin, obj)
    assert bool(torch.isnan(J))


# ---- 7: the class path -- kernels against the same objective written as torch ops -----------------------------------------------------------------
class TorchObjective(torch.nn.Module):
    """sum_t 0.9^t (mean_m c + 0.5 std_m c) and its monitor as plain torch ops on the torch formula of ``cf`` (an Input_penalty)."""

    def __init__(self, cf, discount, risk):
        super().__init__()
        self.cf, self.discount, self.risk = cf, discount, risk

    def forward(self, states, inputs, trial_index):
        costs = self.cf.cost_function(states, inputs, trial_index)
        w = self.discount ** torch.arange(costs.shape[0], dtype=costs.dtype, device=costs.device)
        return torch.sum(w * (costs.mean(1) + self.risk * costs.std(1))), torch.sum(w * costs.detach().std(1))


@pytest.mark.parametrize("which", ["rbf", "pd", "mlp", "mlp-pms"])
def test_class_path_on_the_kernels_matches_the_torch_objective(which):
    """One apply_policy + _cost_backward in "reference" noise mode (M = 16, T = 6) with Cost_shaping(Input_penalty(state cost, both terms),
    discount = 0.9, risk = 0.5) on the kernels, with the same objective as torch ops backpropagated through the same rollout, and with the
    penalty unshaped: states and inputs equal bit for bit; J and S to 1e-12; every parameter gradient to 1e-10 of its largest entry; each
    gradient differs from the unshaped run's by more than 1e-6."""
    from mc_pilco_amd.policy_learning import Cost_function as CF

    obj, sim, state_cost, U = _cartpole_object() if which == "rbf" else _arm_object("pd" if which == "pd" else "mlp", which == "mlp-pms")
    pen = penalty(state_cost, U)
    cf = CF.Cost_shaping(pen, discount=0.9, risk=0.5)
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
    assert cf._packed is not None and pen._in_packs and cf._objectives, "the kernels did not run"
    ts, ti, tc, td, tg = step(TorchObjective(pen, 0.9, 0.5))
    ps, pi, pc, _, pg = step(pen)
    assert torch.equal(ks, ts) and torch.equal(ki, ti) and torch.equal(ks, ps) and torch.equal(ki, pi)
    eg = [relerr(a, b) for a, b in zip(kg, tg)]
    moved = [relerr(a, b) for a, b in zip(pg, kg)]
    print("%s: J %.2e S %.2e gradients %s; against the unshaped cost: J %.2e gradients %s"
          % (which, rel(kc, tc), rel(kd, td), " ".join("%.2e" % e for e in eg), rel(pc, kc), " ".join("%.2e" % e for e in moved)))
    assert rel(kc, tc) < 1e-12 and rel(kd, td) < 1e-12 and max(eg) < 1e-10
    assert min(moved) > 1e-6


# ---- 8: the optimizer loop records its attempts under the objective -----------------------------------------------------------------------------
def test_loop_with_a_shaped_cost_replays_graphs_and_takes_the_eager_steps():
    """test_gpu_input_cost.py's loop test (4 steps, N = 48, M = 16, T = 6) with Cost_shaping(Input_penalty(...), discount, risk): attempts
    replayed from HIP graphs against eager launches give the same cost list and policy parameters, bit for bit; the recording run did replay;
    and the cost list is not the unshaped one."""
    from test_gpu_target_cost import tiny_mcpilco

    from mc_pilco_amd import synthetic as sy
    from mc_pilco_amd.policy_learning import Cost_function as CF

    c = sy.CARTPOLE
    out = []
    for capture, shaped in ((True, True), (False, True), (False, False)):
        obj = tiny_mcpilco()
        obj.noise_mode = "philox"
        obj.capture_attempts = capture
        obj.cost_function = CF.Input_penalty(obj.cost_function, lengthscales=[4.0], rate_lengthscales=[2.0])
        if shaped:
            obj.cost_function = CF.Cost_shaping(obj.cost_function, discount=0.9, risk=0.5)
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
        assert bool(getattr(cf, "_objectives", None)) == shaped
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


# ---- 9: two ranks on one device ---------------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401
    from mc_pilco_amd.policy_learning import Cost_function as CF

    torch.cuda.set_device(dev())
    with rank_group(rank, world, port):
        obj, _, state_cost, U = _arm_object("mlp")
        obj.noise_mode = "philox"
        obj.cost_function = CF.Cost_shaping(penalty(state_cost, U), discount=0.9, risk=0.5)
        res = clf.sharded_step(MLP, obj, world, clf.sim_args(17, 6))
        assert obj.cost_function._packed is not None and obj.cost_function._objectives
        out_q.put((rank, res))


def test_two_rank_particle_sharding_matches_single_process():
    """MLP_policy under shard_particles with Cost_shaping(penalty, discount = 0.9, risk = 0.5) (M = 17, T = 6, Philox; three GPU processes in
    all): each rank's states are the matching slice of the one-process run bit for bit; J and S agree to 1e-10 (with kappa != 0 J holds the
    pooled std, which agrees at the std's bound, not at the 1e-13 of a pure mean); the six parameter gradients to 1e-9; every rank reports the
    same bits of J."""
    c1, s1, f1, g1, st1, _ = dict(run_ranks(_rank, 1))[0]
    two = dict(run_ranks(_rank, 2))
    assert f1 == [0.0, 0.0, 0.0] and len(g1) == 6 and all(float(np.abs(g).max()) > 0 for g in g1)
    seen = 0
    for r in range(2):
        c2, s2, f2, g2, st2, (off, cnt) = two[r]
        assert np.array_equal(st2, st1[:, off:off + cnt])
        seen += cnt
        eg = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g2, g1)]
        print("rank %d: J %.3e S %.3e gradients %s" % (r, abs(c2 - c1) / abs(c1), abs(s2 - s1) / abs(s1), " ".join("%.3e" % e for e in eg)))
        assert f2 == [0.0, 0.0, 0.0]
        assert abs(c2 - c1) <= 1e-10 * abs(c1) and abs(s2 - s1) <= 1e-10 * abs(s1)
        assert len(g2) == 6 and max(eg) < 1e-9
    assert seen == 17 and two[0][0] == two[1][0]


# ---- 10: ops.expected_cost(group=...) under an objective ------------------------------------------------------------------------------------------
def _group_rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401
    from mc_pilco_amd import ops

    torch.cuda.set_device(dev())
    c = icm.make_case(icm.draw(*THIRD), "sat", True, "both")
    a, b = ((0, 100), (100, 257))[rank]
    with rank_group(rank, world, port) as group:
        pc, cin = packed(c)
        _, obj = objective("explicit", -0.5, 3)
        st, inp = G(c["x"][:, a:b]).requires_grad_(True), G(c["u"][:, a:b]).requires_grad_(True)
        J, S = ops.expected_cost(pc, st, group, [100, 157], inp, cin, obj)
        J.backward()
        torch.cuda.synchronize()
        out_q.put((rank, (float(J.detach()), float(S.detach()), st.grad.cpu().numpy(), inp.grad.cpu().numpy())))


def test_expected_cost_with_a_group_pools_the_rows_of_all_ranks():
    """M = 257 as 100 + 157 on two ranks of one device (gloo): the rows come from the gathered moments, the backward takes n_total = 257 -- J, S
    and the gradients (each rank's columns) agree with the truth of the whole swarm to 1e-12, and both ranks report the same bits of J."""
    c = icm.make_case(icm.draw(*THIRD), "sat", True, "both")
    tr = ot.truth(c, ot.weights("explicit", 3), -0.5)
    two = dict(run_ranks(_group_rank, 2))
    assert two[0][0] == two[1][0] and two[0][1] == two[1][1]
    gx, gu = np.concatenate([two[r][2] for r in range(2)], 1), np.concatenate([two[r][3] for r in range(2)], 1)
    e = (rel(two[0][0], tr["J"]), rel(two[0][1], tr["S"]), relerr(gx, tr["g_states"]), relerr(gu, tr["g_inputs"]))
    print("group of two: J %.2e S %.2e g_states %.2e g_inputs %.2e" % e)
    assert max(e) < 1e-12

