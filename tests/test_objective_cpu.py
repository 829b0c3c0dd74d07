"""CPU-only checks of the time-weighted, risk-sensitive objective (mcp_objective, mcp_cost_rows / mcp_cost_rows_sums / mcp_cost_bwd_shaped,
ops.PackedObjective, Cost_function.Cost_shaping): the hand gradient form the kernels implement is autograd's, the GPU cases are conditioned
well enough for the cost kernels' 1e-12, the truth feels every mistake a kernel could make, the class evaluates the same objective as torch ops
wherever the kernels do not apply (two gloo ranks included), and bad objectives and bad calls are refused on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import input_cost_models as icm
import objective_truth as ot
from rank_harness import rank_group, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64
CASES = ot.gpu_cases()
THIRD = icm.SHAPES[2]


def relerr(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    top = np.max(np.abs(b))
    return float(np.max(np.abs(a - b))) if top == 0.0 else float(np.max(np.abs(a - b)) / top)


def cost_object(c, device="cpu", has_inputs=True):
    """The package's cost object of a case of input_cost_models: the state cost, inside an Input_penalty where the case has input terms."""
    from mc_pilco_amd.policy_learning import Cost_function as CF

    def t(a):
        return torch.as_tensor(np.asarray(a), dtype=D, device=device)

    if c["kind"] == "cartpole":
        sc = CF.Cart_pole_cost(target_state=c["tg"], lengthscales=c["ls"], angle_index=c["used_x"][0], pos_index=c["used_x"][1])
    elif c["kind"] == "traj":
        sc = CF.Expected_saturated_distance_from_trajectory(t(c["tg"]), t(c["ls"]), used_indeces=c["used_x"])
    else:
        cls = CF.Expected_saturated_distance if c["kind"] == "sat" else CF.Expected_distance
        sc = cls(target_state=t(c["tg"]).reshape(1, -1), lengthscales=t(c["ls"]), active_dims=np.array(c["used_x"]))
    if not has_inputs:
        return sc
    return CF.Input_penalty(sc, lengthscales=c["l"], rate_lengthscales=c["r"], target_input=c["ustar"], input_indices=c["used_u"], joint=c["joint"])


def objectives(T):
    """Every (weight set, kappa) the tests use: the three of the GPU parity test and the other combinations."""
    out = list(ot.OBJECTIVES) + [(ws, k) for ws in ot.WEIGHT_SETS for k in ot.KAPPAS if (ws, k) not in ot.OBJECTIVES]
    return [(ws, ot.weights(ws, T), k) for ws, k in out]


# ---- the truth -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,c,has_inputs", CASES, ids=[n for n, _, _ in CASES])
def test_hand_form_is_autograds(name, c, has_inputs):
    """dJ/dc_tm = w_t [1/n + kappa (c_tm - mu_t) / ((n - 1) sigma_t)] carried through the cost's own hand gradient, with the rate term's
    neighbour factor built from row t + 1: within 1e-12 of each tensor's largest entry of what autograd gives for sum_t w_t (mean + kappa std)."""
    T = c["x"].shape[0]
    for _, w, kappa in objectives(T):
        tr = ot.truth(c, w, kappa)
        gx, gu = ot.hand(c, w, kappa)
        assert relerr(gx, tr["g_states"]) <= 1e-12 and relerr(gu, tr["g_inputs"]) <= 1e-12


def test_every_gpu_case_keeps_its_spread():
    """min_t sigma_t / max_m |c_tm| >= 0.05 on every case the GPU parity test runs: the sigma term amplifies the error of the mean by at most
    max|c| / sigma <= 20, which is what lets the GPU bound stay at the cost kernels' 1e-12."""
    worst = min((ot.conditioning(c), name) for name, c, _ in CASES)
    print("smallest sigma / max|c|: %.4f at %s" % worst)
    assert worst[0] >= 0.05
    assert len(CASES) == 5 * 4 + 4 + 4 and len({n for n, _, _ in CASES}) == len(CASES)


def _shard(c, a, b):
    return dict(c, x=c["x"][:, a:b], u=c["u"][:, a:b])


def test_the_truth_feels_every_variant():
    """kappa dropped, w dropped, w shifted by one row, the biased std, the local instead of the pooled mean, the rate term's neighbour built with
    G_t: each moves some gradient by more than 1e-6 of its largest entry on at least one case where it applies."""
    felt = {v: 0.0 for v in ot.VARIANTS}
    runs = []
    for name, c, _ in CASES:
        for _, w, kappa in objectives(c["x"].shape[0]):
            runs.append((c, w, kappa, None, None))
    whole = dict((n, c) for n, c, _ in CASES)["%s-sat-joint-both" % icm.shape_id(THIRD)]
    for _, w, kappa in objectives(3):
        rows = ot.truth(whole, w, kappa)["rows"].numpy()
        runs.append((_shard(whole, 0, 100), w, kappa, 257, rows))
    for c, w, kappa, n, rows in runs:
        tr = ot.truth(c, w, kappa, n, rows)
        for v in ot.VARIANTS:
            if ot.applies(v, c, w, kappa, rows is not None):
                gx, gu = ot.hand(c, w, kappa, n, rows, variant=v)
                felt[v] = max(felt[v], relerr(gx, tr["g_states"]), relerr(gu, tr["g_inputs"]))
    print(" ".join("%s: %.2e" % kv for kv in felt.items()))
    assert all(m > 1e-6 for m in felt.values()), felt


def test_a_shards_gradients_are_columns_of_the_whole_swarms():
    """The truth of a shard (pooled rows, n_total) is the matching columns of the whole swarm's truth, and so is the hand form."""
    whole = dict((n, c) for n, c, _ in CASES)["%s-sat-joint-both" % icm.shape_id(THIRD)]
    for _, w, kappa in objectives(3):
        tr = ot.truth(whole, w, kappa)
        for a, b in ((0, 100), (100, 257)):
            part = ot.truth(_shard(whole, a, b), w, kappa, 257, tr["rows"].numpy())
            assert relerr(part["g_states"], tr["g_states"][:, a:b]) <= 1e-12 and relerr(part["g_inputs"], tr["g_inputs"][:, a:b]) <= 1e-12
            assert abs(float(part["J"]) - float(tr["J"])) <= 1e-14 * abs(float(tr["J"]))
            gx, gu = ot.hand(_shard(whole, a, b), w, kappa, 257, tr["rows"].numpy())
            assert relerr(gx, tr["g_states"][:, a:b]) <= 1e-12 and relerr(gu, tr["g_inputs"][:, a:b]) <= 1e-12


# ---- Cost_function.Cost_shaping on CPU tensors: its torch path ----------------------------------------------------------------------------------
def _shaping_kw(ws, w, kappa):
    return dict(time_weights=(None if ws != "explicit" else w), discount=(0.9 if ws == "discount" else None), risk=kappa)


@pytest.mark.parametrize("name,c,has_inputs", CASES, ids=[n for n, _, _ in CASES])
def test_cost_shaping_on_cpu_tensors_is_the_truth(name, c, has_inputs):
    from mc_pilco_amd.policy_learning import Cost_function as CF

    T = c["x"].shape[0]
    inner = cost_object(c, "cpu", has_inputs)
    for ws, w, kappa in objectives(T):
        cf = CF.Cost_shaping(inner, **_shaping_kw(ws, w, kappa))
        assert isinstance(cf, CF._HipExpectedCost) and cf.runs_on_kernels() == inner.runs_on_kernels()
        x, u = icm._t(c["x"]).requires_grad_(True), icm._t(c["u"]).requires_grad_(True)
        assert not cf.runs_on_kernels(x)
        J, S = cf(x, u, 0)
        J.backward()
        tr = ot.truth(c, w, kappa)
        assert abs(float(J.detach()) - float(tr["J"])) <= 1e-12 * abs(float(tr["J"])) and abs(float(S) - float(tr["S"])) <= 1e-12 * abs(float(tr["S"]))
        assert relerr(x.grad, tr["g_states"]) <= 1e-12
        if has_inputs:
            assert relerr(u.grad, tr["g_inputs"]) <= 1e-12
        else:
            assert u.grad is None
        assert not S.requires_grad and cf._packed is None


def test_cost_shaping_with_no_option_is_the_wrapped_cost_bit_for_bit():
    from mc_pilco_amd.policy_learning import Cost_function as CF

    for name, c, has_inputs in CASES:
        if not name.startswith("T3M257"):
            continue
        inner = cost_object(c, "cpu", has_inputs)
        if inner.cost_function is None:  # (the two launch-script costs keep no torch formula of their own: nothing to compare on CPU tensors)
            continue
        x, u = icm._t(c["x"]).requires_grad_(True), icm._t(c["u"]).requires_grad_(True)
        J, S = CF.Cost_shaping(inner)(x, u, 0)
        J.backward()
        y, v = icm._t(c["x"]).requires_grad_(True), icm._t(c["u"]).requires_grad_(True)
        J0, S0 = inner(y, v, 0)
        J0.backward()
        assert torch.equal(J, J0) and torch.equal(S, S0) and torch.equal(x.grad, y.grad)
        assert (u.grad is None and v.grad is None) or torch.equal(u.grad, v.grad)
        sh, sm = CF.Cost_shaping(inner).local_moments(y.detach(), v.detach(), 0, 300)
        sh0, sm0 = inner.local_moments(y.detach(), v.detach(), 0, 300)
        assert torch.equal(sh, sh0) and torch.equal(sm, sm0)
        for a, b in zip(CF.Cost_shaping(inner).from_sums(sm, 257), inner.from_sums(sm0, 257)):
            assert torch.equal(a, b)


def test_a_trainable_weight_vector_keeps_the_torch_path_and_gets_its_gradient():
    """dJ/dw_t = mu_t + kappa sigma_t."""
    from mc_pilco_amd.policy_learning import Cost_function as CF

    c = dict((n, c) for n, c, _ in CASES)["T4M5S4U3-sat-add-both"]
    w = torch.tensor([1.0, 0.5, 2.0, 0.25], dtype=D, requires_grad=True)
    cf = CF.Cost_shaping(cost_object(c), time_weights=w, risk=0.7)
    assert not cf.runs_on_kernels()
    J, _ = cf(icm._t(c["x"]), icm._t(c["u"]), 0)
    J.backward()
    rows = ot.truth(c, w.detach().numpy(), 0.7)["rows"]
    assert relerr(w.grad, rows[:, 0] + 0.7 * rows[:, 1]) <= 1e-12


def test_a_row_of_identical_costs_keeps_the_mean_only_factor():
    """Row 0 holds the same state and input for every particle (T = 2, M = 4): the gradients are finite, and row 0's are w_0 / n times the
    gradient of the plain sum of costs -- the sigma term of that row is dropped."""
    from mc_pilco_amd.policy_learning import Cost_function as CF

    c = zero_spread_case()
    w = np.array([0.6, 1.7])
    tr = ot.truth(c, w, 0.7)
    assert float(tr["rows"][0, 1]) == 0.0 and float(tr["rows"][1, 1]) > 0.0
    plain = icm.truth(c, gscale=1.0)
    M = c["x"].shape[1]
    assert relerr(tr["g_states"][0], w[0] / M * plain["g_states"][0]) <= 1e-14
    for g in ot.hand(c, w, 0.7):
        assert np.isfinite(g).all()
    assert relerr(ot.hand(c, w, 0.7)[0], tr["g_states"]) <= 1e-12 and relerr(ot.hand(c, w, 0.7)[1], tr["g_inputs"]) <= 1e-12
    x, u = icm._t(c["x"]).requires_grad_(True), icm._t(c["u"]).requires_grad_(True)
    J, S = CF.Cost_shaping(cost_object(c), time_weights=w, risk=0.7)(x, u, 0)
    J.backward()
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(u.grad).all())
    assert relerr(x.grad, tr["g_states"]) <= 1e-12 and relerr(u.grad, tr["g_inputs"]) <= 1e-12
    assert abs(float(J.detach()) - float(tr["J"])) <= 1e-12 * abs(float(tr["J"])) and abs(float(S) - float(tr["S"])) <= 1e-12 * abs(float(tr["S"]))


def zero_spread_case(M=4):
    """T = 2, S = 4, U = 2, saturated target cost in ADD mode with both terms; every particle of row 0 is particle 0.  M is a power of two: the
    mean of M identical values is then that value in any order of the additions, so the row's centred sum of squares is exactly 0."""
    d = icm.draw(2, M, 4, 2, [2, 0], [1, 0], seed=3)
    c = icm.make_case(d, "sat", False, "both")
    c["x"], c["u"] = c["x"].copy(), c["u"].copy()
    c["x"][0], c["u"][0] = c["x"][0, :1], c["u"][0, :1]
    return c


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_bad_objectives_are_refused_on_the_host():
    """ValueError from the host values alone, from ops.PackedObjective (no device is touched before the checks) and from the class."""
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import Cost_function as CF

    sc = CF.Cart_pole_cost([3.0, 0.1], [3.0, 1.0], 2, 0)
    bad = (dict(time_weights=[1.0, -0.1, 1.0]), dict(time_weights=[1.0, float("nan"), 1.0]), dict(time_weights=[1.0, float("inf"), 1.0]),
           dict(time_weights=[0.0, 0.0, 0.0]), dict(time_weights=[1.0, 1.0]), dict(discount=0.0), dict(discount=-0.5), dict(discount=1.5),
           dict(discount=float("nan")), dict(risk=float("nan")), dict(risk=float("inf")), dict(time_weights=torch.tensor([1.0, -1.0, 1.0], dtype=D)))
    st, u = torch.zeros(3, 5, 4, dtype=D), torch.zeros(3, 5, 1, dtype=D)
    for kw in bad:
        with pytest.raises(ValueError):
            ops.PackedObjective(3, "cuda:0", **kw)
        with pytest.raises(ValueError):
            CF.Cost_shaping(sc, **kw)(st, u, 0)
    with pytest.raises(ValueError):
        ops.PackedObjective(0, "cuda:0")
    # weights that are fine for a short horizon and all zero (or too few) over the one that is run
    with pytest.raises(ValueError):
        ops.PackedObjective(2, "cuda:0", time_weights=[0.0, 0.0, 1.0])
    with pytest.raises(ValueError):
        CF.Cost_shaping(sc, time_weights=[0.0, 0.0, 0.0, 1.0])(st, u, 0)
    with pytest.raises(ValueError):
        CF.Cost_shaping(sc, time_weights=[1.0, 1.0])(st, u, 0)
    # the std term with one particle
    with pytest.raises(ValueError):
        CF.Cost_shaping(sc, risk=0.5)(st[:, :1], u[:, :1], 0)
    with pytest.raises(ValueError):
        CF.Cost_shaping(sc, risk=0.5).local_moments(st[:, :1], u[:, :1], 0, 1)
    CF.Cost_shaping(sc, discount=0.9)(st[:, :1], u[:, :1], 0)  # (kappa = 0 with one particle is today's cost: J finite, S NaN)
    # what it wraps
    for other in (CF.Expected_cost(lambda x, u, k: x.sum(2)), None, CF.Cost_shaping(sc, discount=0.9)):
        with pytest.raises(TypeError):
            CF.Cost_shaping(other, discount=0.9)
    ok = CF.Cost_shaping(CF.Input_penalty(sc, lengthscales=[2.0]), time_weights=[1.0, 0.0, 2.0, 5.0], discount=1.0, risk=-0.5)
    assert ok.runs_on_kernels() and ok.needs_pooled_rows and not CF.Cost_shaping(sc, discount=0.5).needs_pooled_rows
    assert CF.Cost_shaping(sc).objective_for(st) is None


def test_objective_layout_matches_the_header_and_the_abi_did_not_move(tmp_path):
    from mc_pilco_amd import hipabi

    names = [f[0] for f in hipabi.Objective._fields_]
    assert names == ["w", "kappa"]
    src = tmp_path / "ob.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(){printf("%zu %zu %zu %d", sizeof(mcp_objective),'
                   " sizeof(mcp_cost), sizeof(mcp_cost_inputs), MCP_ABI_VERSION);"
                   + "".join('printf(" %%zu", offsetof(mcp_objective, %s));' % n for n in names) + "return 0;}\n")
    exe = tmp_path / "ob"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(hipabi.Objective), C.sizeof(hipabi.Cost), C.sizeof(hipabi.CostInputs), hipabi.ABI_VERSION] \
        + [getattr(hipabi.Objective, n).offset for n in names]
    assert C.sizeof(hipabi.Objective) == 16 and C.sizeof(hipabi.Cost) == 136


P = C.c_void_p(8)  # (a non-null stand-in for buffers; the checks fail first, nothing dereferences it)


def test_bad_calls_of_the_new_entries_are_refused_before_any_launch():
    """-1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT, each from the host-side checks: a call that got past them would try to launch and, without a device,
    answer -4 MCP_ERR_LAUNCH.  So a refusal here enqueued nothing."""
    from test_input_cost_cpu import _cin, _cost

    from mc_pilco_amd import hipabi

    lib = hipabi.lib()
    assert lib.mcp_abi_version() == hipabi.ABI_VERSION == 7
    raw = C.CDLL(hipabi.LIB_PATH)
    for n in ("mcp_cost_rows", "mcp_cost_rows_sums", "mcp_cost_bwd_shaped"):
        assert hasattr(raw, n) and n in hipabi.EXPORTED

    def obj(kappa=0.0, w=None):
        o = hipabi.Objective()
        o.w, o.kappa = w, kappa
        return o

    cnt = (C.c_int64 * 2)(3, 4)
    one = (C.c_int64 * 1)(1)

    def rows(T=3, R=2, moments=P, counts=cnt, o=None, rows=P, out=P):
        return lib.mcp_cost_rows(T, R, moments, counts, None if o is None else C.byref(o), rows, out, None)

    for kw in (dict(T=0), dict(R=0), dict(moments=None), dict(counts=None), dict(rows=None), dict(out=None), dict(o=obj(float("nan"))),
               dict(o=obj(float("inf"))), dict(R=1, counts=one, o=obj(0.5))):
        assert rows(**kw) == -1, kw
    assert rows(R=65) == -2

    def rsums(T=3, n=7, sums=P, o=None, rows=P, out=P):
        return lib.mcp_cost_rows_sums(T, n, sums, None, None if o is None else C.byref(o), rows, out, None, None)

    for kw in (dict(T=0), dict(n=0), dict(sums=None), dict(rows=None), dict(out=None), dict(o=obj(float("nan"))), dict(n=1, o=obj(-0.5))):
        assert rsums(**kw) == -1, kw

    def bwd(c=_cost(), ci=_cin(), o=None, T=3, M=4, n=4, states=P, inputs=P, costs=P, rows=P, g_states=P, g_inputs=P):
        return lib.mcp_cost_bwd_shaped(None if c is None else C.byref(c), None if ci is None else C.byref(ci), None if o is None else C.byref(o), T, M,
                                       n, states, inputs, costs, rows, None, g_states, g_inputs, None)

    for kw in (dict(c=None), dict(c=_cost(kind=7)), dict(ci=_cin(used=(1, 1))), dict(ci=_cin(mode=2)), dict(T=0), dict(M=0), dict(n=3),
               dict(states=None), dict(inputs=None), dict(costs=None), dict(rows=None), dict(g_states=None), dict(o=obj(float("nan"))),
               dict(o=obj(float("-inf"))), dict(M=1, n=1, o=obj(0.5)), dict(ci=None, inputs=None), dict(ci=_cin(U=0))):
        assert bwd(**kw) == -1, kw
    assert bwd(ci=_cin(U=hipabi.MAX_INPUT + 1)) == -2
    if not torch.cuda.is_available():  # (past every check the launch itself is what fails here)
        assert bwd(o=obj(0.5)) == -4 and bwd(ci=None, inputs=None, g_inputs=None) == -4 and rows(o=obj(0.5)) == -4 and rsums(o=obj(0.5)) == -4


# ---- two gloo ranks on the torch path ---------------------------------------------------------------------------------------------------------
class CountingReducer:
    """A sharding.StepReducer whose all-reduces are counted."""

    def __init__(self, group):
        from mc_pilco_amd import sharding

        self.inner = sharding.StepReducer(group)
        self.calls = 0

    def allreduce_(self, flat):
        self.calls += 1
        return self.inner.allreduce_(flat)

    def reduce(self, params, sums, flags):
        from mc_pilco_amd import sharding

        return sharding.StepReducer.reduce(self, params, sums, flags)


def _gloo_rank(rank, world, port, out_q):
    import mcp_boot  # noqa: F401
    from mc_pilco_amd import sharding
    from mc_pilco_amd.policy_learning import Cost_function as CF

    torch.set_num_threads(1)
    c = icm.make_case(icm.draw(4, 17, 4, 3, [0, 3], [2, 0], seed=9), "sat", True, "both")
    a, b = (0, 17) if world == 1 else ((0, 7), (7, 17))[rank]
    with rank_group(rank, world, port) as group:
        res = {}
        for ws, kappa in (("discount", 0.0), ("explicit", -0.5), ("none", 0.7)):
            w = ot.weights(ws, 4)
            cf = CF.Cost_shaping(cost_object(c), **_shaping_kw(ws, w, kappa))
            x, u = icm._t(c["x"][:, a:b]).requires_grad_(True), icm._t(c["u"][:, a:b]).requires_grad_(True)
            if world == 1:
                J, S = cf(x, u, 0)
                J.backward()
                calls = 0
            else:
                red = CountingReducer(group)
                shift = torch.full((4,), 0.3, dtype=D)
                share, sums = cf.local_moments(x, u, 0, 17, shift, reducer=red) if cf.needs_pooled_rows else cf.local_moments(x, u, 0, 17, shift)
                share.backward()
                J, S, flags, nxt = sharding.finish_step(cf, red, [], sums, torch.zeros(3, dtype=D), 17, shift)
                assert float(flags.sum()) == 0.0 and bool(torch.isfinite(nxt).all())
                calls = red.calls
            res[(ws, kappa)] = (float(J.detach()), float(S.detach()), x.grad.numpy().copy(), u.grad.numpy().copy(), calls)
        out_q.put((rank, (a, b), res))


def test_two_gloo_ranks_with_uneven_shards_match_one_process():
    """17 particles as 7 + 10 on the torch path: pooled J, S and both gradients agree with one process to 1e-12; the step makes ONE all-reduce
    with kappa = 0 and exactly one more with kappa != 0."""
    one = run_ranks(_gloo_rank, 1)[0][2]
    two = sorted(run_ranks(_gloo_rank, 2))
    for key, (J1, S1, gx1, gu1, _) in one.items():
        gx = np.concatenate([r[2][key][2] for r in two], 1)
        gu = np.concatenate([r[2][key][3] for r in two], 1)
        for _, _, res in two:
            J2, S2, _, _, calls = res[key]
            assert abs(J2 - J1) <= 1e-12 * abs(J1) and abs(S2 - S1) <= 1e-12 * abs(S1)
            assert calls == (1 if key[1] == 0.0 else 2)
        assert two[0][2][key][0] == two[1][2][key][0]  # every rank reports the same J
        assert relerr(gx, gx1) <= 1e-12 and relerr(gu, gu1) <= 1e-12
    # and one process is the truth
    c = icm.make_case(icm.draw(4, 17, 4, 3, [0, 3], [2, 0], seed=9), "sat", True, "both")
    for (ws, kappa), (J1, _, gx1, _, _) in one.items():
        tr = ot.truth(c, ot.weights(ws, 4), kappa)
        assert abs(J1 - float(tr["J"])) <= 1e-12 * abs(J1) and relerr(gx1, tr["g_states"]) <= 1e-12
