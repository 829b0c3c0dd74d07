"""GPU: the optimizer loop's two operators, `mcp_adam_step_guarded` and `mcp_policy_step_commit` (csrc/policy_opt.hip), through the C ABI
against the truth of tests/opt_truth.py (pinned to the reference by tests/test_opt_truth_cpu.py), and the class loop on the same scripts.

STATE MACHINE.  A driver holds the device buffers the loop uses (mcp_opt_state as 7 words, the four arrays, the record, the cost / std /
flags / status scalars, parameters / gradients / moments); per scripted attempt it writes the scalars and gradients, calls the two entry
points, reads everything back, steps the truth and compares; where the truth says the host acts it repeats what
MC_PILCO.reinforce_policy does there.  Compared BITWISE (NaN-aware) after every attempt: the integer state, es2, cost_prev, cost_list,
std_list, es1, ratio and all twelve record entries -- the monitor arithmetic is a dozen correctly rounded + - x / sqrt in the reference's
order and the library is built without floating-point contraction.  One operation is NOT the same on both sides: torch's CPU square root
is off by one ulp for just under 1 % of its arguments (tests/test_opt_truth_cpu.py measures it), the device's is correctly rounded.  The
kernels are therefore compared with LoopTruth(sqrt="ieee") -- the same restatement with `math.sqrt` for `ES2_diff_cost.sqrt()` -- which the
CPU test ties to the reference: same decisions, |ratio| within the one-ulp error of the root (profiles/NOTES.md, part J).

ADAM.  The kernel forms beta^t with the device pow, torch with Python's: equality is likely, not derivable.  Bound: the kernel's distance
to AdamTruth (max |difference| per tensor over the finite entries / the truth's largest magnitude in the tensor) <= 8 x the distance of
AdamTruth from the longdouble update over the SAME gradient sequence (measured at test time on the CPU; the float64 rounding level of the
operation), floored at 2^-50; the Inf / NaN patterns equal.  In failed and void attempts parameters and moments bitwise unchanged.
"""
import contextlib
import ctypes as C
import io
import re

import numpy as np
import pytest
import torch

import opt_truth as ot

pytestmark = pytest.mark.gpu
f64, i64 = torch.float64, torch.int64
ERR_ARG, ERR_LIMIT = -1, -2
SCRIPTS = ["a_thresholds", "b_retries", "c_reinit", "d_n0", "d_n_gt_k", "d_n_gt_steps", "d_min_step_neg", "e_zero_diff"]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("opt_loop_script")


def dev():
    return torch.device("cuda", 0)


def G(a, dtype=f64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev()).contiguous()


def same_bits(a, b):
    """Bitwise equality of two float64 arrays, any two NaNs counting as equal."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def adam_call(ps, gs, ms, vs, lr, state=None, step=0, n_steps=0, cost=None, flags=None, status=None, numel=None):
    from mc_pilco_amd import hipabi as abi

    n = len(ps)
    arr = lambda ts: (abi.dptr * n)(*[None if (t is None or t.numel() == 0) else t.data_ptr() for t in ts])
    numel = [t.numel() for t in ps] if numel is None else numel
    return abi.lib().mcp_adam_step_guarded(n, arr(ps), arr(gs), arr(ms), arr(vs), (C.c_int64 * n)(*numel), float(lr), 0.9, 0.999, 1e-8, abi.ptr(state),
                                           int(step), int(n_steps), abi.ptr(cost), abi.ptr(flags), abi.ptr(status), abi.stream())


class Driver:
    """The device side of one reinforce_policy call, as MC_PILCO.reinforce_policy lays it out."""

    def __init__(self, n_steps, warm, params, with_flags=True, with_status=True, with_std=True):
        d = dev()
        self.n_steps = n_steps
        self.st = torch.zeros(7, dtype=i64, device=d)  # step, attempt, pending, adam_t, total_attempts | es2, cost_prev
        self.st[5:].view(f64)[1:2].copy_(G([warm]))
        self.cost_list, self.std_list = torch.zeros(n_steps, dtype=f64, device=d), torch.zeros(n_steps, dtype=f64, device=d)
        self.es1, self.ratio = torch.zeros(n_steps + 1, dtype=f64, device=d), torch.zeros(n_steps + 1, dtype=f64, device=d)
        self.rec = torch.full((12,), -7.0, dtype=f64, device=d)
        self.cost, self.std = torch.zeros(1, dtype=f64, device=d), torch.zeros(1, dtype=f64, device=d)
        self.flags = torch.zeros(3, dtype=f64, device=d) if with_flags else None
        self.status = torch.zeros(1, dtype=torch.int32, device=d) if with_status else None
        self.with_std = with_std
        self.p = [G(q) for q in params]
        self.g = [torch.zeros_like(q) for q in self.p]
        self.fresh_moments()

    def fresh_moments(self):
        self.m, self.v = [torch.zeros_like(q) for q in self.p], [torch.zeros_like(q) for q in self.p]

    def commit_call(self, alpha, min_step, min_diff, n_win, n_steps=None, **null):
        from mc_pilco_amd import hipabi as abi

        a = dict(state=self.st, cost=self.cost, std=self.std if self.with_std else None, cost_list=self.cost_list, std_list=self.std_list,
                 es1=self.es1, ratio=self.ratio)
        a.update(null)
        return abi.lib().mcp_policy_step_commit(abi.ptr(a["state"]), self.n_steps if n_steps is None else n_steps, abi.ptr(a["cost"]), abi.ptr(a["std"]),
                                                abi.ptr(self.flags), abi.ptr(self.status), abi.ptr(a["cost_list"]), abi.ptr(a["std_list"]),
                                                abi.ptr(a["es1"]), abi.ptr(a["ratio"]), float(alpha), float(min(min_step, 1e300)), float(min_diff),
                                                int(n_win), abi.ptr(self.rec), abi.stream())

    def attempt(self, cost, std, w, lt, flags=(0.0, 0.0, 0.0), status=0):
        """Writes the attempt's scalars and gradients, then the two launches of MC_PILCO.reinforce_policy's ``commit``."""
        self.cost.copy_(G([cost]))
        self.std.copy_(G([std]))
        if self.flags is not None:
            self.flags.copy_(G(flags))
        if self.status is not None:
            self.status.fill_(int(status))
        o = 0
        for g in self.g:
            g.copy_(G(w[o:o + g.numel()]).reshape(g.shape))
            o += g.numel()
        rc = adam_call(self.p, self.g, self.m, self.v, lt.lr, state=self.st, n_steps=self.n_steps, cost=self.cost, flags=self.flags, status=self.status)
        assert rc == 0, rc
        rc = self.commit_call(lt.alpha, lt.min_step, lt.min_diff, lt.n_win)
        assert rc == 0, rc
        torch.cuda.synchronize()

    def snapshot(self):
        s = self.st.cpu()
        fl = s[5:].view(f64)
        out = dict(ints=s[:5].numpy().copy(), es2=fl[0:1].numpy().copy(), cost_prev=fl[1:2].numpy().copy(), rec=self.rec.cpu().numpy().copy())
        for k in ("cost_list", "std_list", "es1", "ratio"):
            out[k] = getattr(self, k).cpu().numpy().copy()
        for k in ("p", "m", "v"):
            out[k] = [t.cpu().numpy().copy() for t in getattr(self, k)]
        return out

    # the host's actions (MC_PILCO.reinforce_policy at its `pending` and ten-failure branches)
    def host_new_optimizer(self):
        self.fresh_moments()
        self.st[3:4].zero_()

    def host_clear_pending(self):
        self.st[2:3].zero_()

    def host_reinit(self, values):
        for q, v in zip(self.p, values):
            q.copy_(G(v).reshape(q.shape))
        self.st[0:5].zero_()
        for a in (self.cost_list, self.std_list, self.es1, self.ratio):
            a.zero_()
        self.host_new_optimizer()


def check_state(lt, snap, where):
    s = lt.state()
    assert list(snap["ints"]) == [s["step"], s["attempt"], s["pending"], s["adam_t"], s["total_attempts"]], (where, snap["ints"], s)
    assert same_bits(snap["es2"], [s["es2"]]), (where, "es2", snap["es2"], s["es2"])
    assert same_bits(snap["cost_prev"], [s["cost_prev"]]), (where, "cost_prev", snap["cost_prev"], s["cost_prev"])
    for k in ("cost_list", "std_list", "es1", "ratio"):
        assert same_bits(snap[k], getattr(lt, k).numpy()), (where, k, snap[k], getattr(lt, k).numpy())
    for j, name in enumerate(ot.RECORD):  # all twelve record entries
        assert same_bits([snap["rec"][j]], [lt.record[j]]), (where, "record." + name, snap["rec"][j], lt.record[j])


def unchanged(a, b, keys=("p", "m", "v")):
    return all(same_bits(x, y) for k in keys for x, y in zip(a[k], b[k]))


class AdamTally:
    """Worst distance of the kernel's p / m / v from AdamTruth over a run, and the fraction of bit-equal entries."""

    def __init__(self):
        self.worst, self.eq, self.n = dict(p=0.0, m=0.0, v=0.0), 0, 0

    def add(self, snap, at):
        for key, want in (("p", at.p()), ("m", at.m()), ("v", at.v())):
            for got, w in zip(snap[key], want):
                w = w.numpy()
                assert np.array_equal(np.isnan(got), np.isnan(w)) and np.array_equal(np.isinf(got), np.isinf(w)), key  # the Inf / NaN patterns
                self.worst[key] = max(self.worst[key], ot.tensor_distance(got, w))
                self.eq += int(np.sum((got.reshape(-1).view(np.int64) == w.reshape(-1).view(np.int64))))
                self.n += got.size

    def check(self, measured, what):
        print("%s: kernel vs AdamTruth p %.3g m %.3g v %.3g | AdamTruth vs longdouble p %.3g m %.3g v %.3g | bit-equal %d of %d entries"
              % (what, self.worst["p"], self.worst["m"], self.worst["v"], measured["p"], measured["m"], measured["v"], self.eq, self.n))
        for key in ("p", "m", "v"):
            # Bound: 8 x the float64 rounding level of the operation on this gradient sequence (AdamTruth vs adam_longdouble, measured on the
            # CPU: 9e-17 .. 3.7e-15 over the cases of this file), floored at 2^-50 = 8.9e-16.  One MI355X: the kernel's distance is
            # 0 .. 1.8e-15 (worst: exp_avg of the 32-tensor case, bound 1.4e-14), 69 - 98 % of the entries bit-equal to torch's; the table
            # per case is in profiles/NOTES.md, part J.
            assert self.worst[key] <= ot.adam_bound(measured[key]), (what, key, self.worst[key], measured[key])


def split(w, params):
    out, o = [], 0
    for q in params:
        out.append(torch.as_tensor(w[o:o + q.numel()]).reshape(q.shape))
        o += q.numel()
    return out


def run_script(script, kw, cause_of=None, probe_voids=True, **forms):
    """One script through the device and the truth, compared after every attempt.  ``cause_of(i)`` -> (failed_because, flags, status) of
    evaluation i (default: nothing but the cost).  Returns the tally of Adam's distances and the truth."""
    n_steps = kw["opt_steps_list"][0]
    lt = ot.LoopTruth(n_steps, script["warm"], kw["alpha_diff_cost"], kw["min_step"], kw["min_diff_cost"], kw["num_min_diff_cost"], kw["lr_list"][0],
                      lr_min=kw["lr_min"], lr_reduction_ratio=kw["lr_reduction_ratio"], sqrt="ieee")
    at = ot.AdamTruth(ot.params0(), lt.lr)
    dv = Driver(n_steps, script["warm"], ot.params0(), **forms)
    tally, kinds = AdamTally(), []

    def void_probe(where):
        # an attempt enqueued while the host has to act: total_attempts advances, everything else stays bit-identical
        before = dv.snapshot()
        dv.attempt(123.0, 9.0, np.ones(ot.N_THETA), lt)
        assert lt.attempt(123.0, 9.0 if dv.with_std else 0.0) == "void"
        snap = dv.snapshot()
        check_state(lt, snap, where + " void")
        assert unchanged(before, snap) and all(same_bits(before[k], snap[k]) for k in ("es2", "cost_prev", "cost_list", "std_list", "es1", "ratio"))
        assert list(snap["ints"][:4]) == list(before["ints"][:4]) and snap["ints"][4] == before["ints"][4] + 1

    i = 0
    while True:
        cause, flags, status = (None, (0.0, 0.0, 0.0), 0) if cause_of is None else cause_of(i)
        if dv.flags is None:
            flags = (0.0, 0.0, 0.0)
        before = dv.snapshot()
        c, sd, w = script["s"][i], script["std"][i], script["w"][i]
        dv.attempt(c, sd, w, lt, flags=flags, status=status)
        kind = lt.attempt(c, sd if dv.with_std else 0.0, cause)
        kinds.append(kind)
        snap = dv.snapshot()
        where = "evaluation %d (%s)" % (i, kind)
        check_state(lt, snap, where)
        if kind == "counted":
            at.step(split(w, at.params))
            tally.add(snap, at)
        else:
            assert unchanged(before, snap), where  # failed, tenth failure: no update
        i += 1
        if kind == "counted":
            if lt.pending:
                if probe_voids:
                    void_probe(where)
                what = lt.host_after_pending()
                if what == "lr":
                    at.new_optimizer(lt.lr)
                    dv.host_new_optimizer()
                dv.host_clear_pending()
                if what == "exit":
                    break
            if lt.step >= n_steps:
                if probe_voids:
                    void_probe(where)
                break
        elif kind == "tenth":
            if probe_voids:
                void_probe(where)
            lt.host_after_ten_failures()
            at.set_params(ot.reinit_values())
            at.new_optimizer(lt.lr)
            dv.host_reinit(ot.reinit_values())
            check_state(lt, dv.snapshot(), where + " re-initialised")
    return tally, lt, kinds


# ======================================================================================================================================
# the state machine
# ======================================================================================================================================
@pytest.mark.parametrize("name", SCRIPTS)
def test_fixture_scripts_state_machine_and_guarded_adam(fx, name):
    """Scripts (a) to (e) of the fixture: every attempt's state, arrays and record bitwise; parameters and moments follow AdamTruth in
    counted attempts (after a `pending` the bias correction restarts at t = 1 while `step` runs on) and are bitwise unchanged in failed
    and void ones; the decisions are the reference's."""
    script, kw = ot.load_case(fx, name)
    tally, lt, kinds = run_script(script, kw)
    g = lambda k: fx[name + "_" + k]
    done = len(g("cost_list"))
    assert same_bits(lt.cost_list.numpy()[:done], g("cost_list")) and same_bits(lt.std_list.numpy()[:done], g("std_list"))
    assert kinds.count("failed") + kinds.count("tenth") == int(g("n_retry")) and kinds.count("tenth") == int(g("n_reinit"))
    start, seq, restarts = ot.script_grad_seq(script, kw)
    tally.check(ot.adam_distance(start, seq, kw["lr_list"][0], restart_at=restarts), name)


CAUSES = {
    "flags0": ("nan", (1.0, 0.0, 0.0), 0), "flags1": ("sync", (0.0, 2.5, 0.0), 0), "flags2": ("nonpos", (0.0, 0.0, 1e-300), 0),
    "status_sync": ("sync", (0.0, 0.0, 0.0), 8), "status_nonpos": ("nonpos", (0.0, 0.0, 0.0), 2),
    "status_other_bits": (None, (0.0, -1.0, 0.0), 1 | 4 | 16),  # MCP_STATUS_NAN / NOT_SPD and an unknown bit, a negative flag: no failure
}


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_each_failure_cause_on_its_own(fx, cause):
    """A finite cost whose attempt fails by one flag or one status bit (evaluations 1, 2 and 3 of a plain script); a status word with only
    other bits set does not fail."""
    script, kw = ot.load_case(fx, "d_n_gt_steps")
    script = dict(script, s=np.where(np.isnan(script["s"]), 1.0, script["s"]))
    hit = (1, 2, 3)
    tally, lt, kinds = run_script(script, kw, cause_of=lambda i: CAUSES[cause] if i in hit else (None, (0.0, 0.0, 0.0), 0))
    expect = "counted" if cause == "status_other_bits" else "failed"
    assert [kinds[i] for i in hit] == [expect] * 3 and lt.step == 4


@pytest.mark.parametrize("form", ["no_flags", "no_status", "neither", "no_std"])
def test_null_forms(fx, form):
    """flags NULL, status NULL, both NULL (a NaN cost still fails), std_cost NULL (std_list 0): the retry script in each form."""
    script, kw = ot.load_case(fx, "b_retries")
    forms = dict(with_flags=form not in ("no_flags", "neither"), with_status=form not in ("no_status", "neither"), with_std=form != "no_std")
    tally, lt, kinds = run_script(script, kw, **forms)
    assert kinds.count("failed") == 17 and lt.step == 8
    if form == "no_std":
        assert not lt.std_list.any()


def test_tenth_failure_by_flag_updates_only_es2_and_cost_prev(fx):
    """Nine failures then a success reset `attempt`; ten failures (by flags[2], finite costs) freeze the loop, and the tenth updates only
    es2 and cost_prev -- with the failed attempt's finite cost -- before the host re-initialises."""
    script, kw = ot.load_case(fx, "d_n_gt_steps")
    script = dict(script, s=np.concatenate([script["s"][:1], 2.0 + 0.1 * np.arange(9), script["s"][1:2], 3.0 + 0.1 * np.arange(10), script["s"][2:8]]),
                  std=np.resize(script["std"], 27), w=np.resize(script["w"], (27, ot.N_THETA)))
    failing = set(range(1, 10)) | set(range(11, 21))
    tally, lt, kinds = run_script(script, kw, cause_of=lambda i: ("nonpos", (0.0, 0.0, 1.0), 0) if i in failing else (None, (0.0, 0.0, 0.0), 0))
    assert kinds[:21] == ["counted"] + ["failed"] * 9 + ["counted"] + ["failed"] * 9 + ["tenth"] and kinds[21:] == ["counted"] * 4
    assert np.isfinite(lt.state()["es2"]) and lt.reinits == 1


def test_commit_refuses_bad_arguments_and_touches_nothing(fx):
    script, kw = ot.load_case(fx, "d_n_gt_steps")
    lt = ot.LoopTruth(4, script["warm"], 0.9, -1, 1e9, 1, 0.01, sqrt="ieee")
    dv = Driver(4, script["warm"], ot.params0())
    dv.attempt(script["s"][0], script["std"][0], script["w"][0], lt)
    before = dv.snapshot()
    for null in ("state", "cost", "cost_list", "std_list", "es1", "ratio"):
        assert dv.commit_call(0.9, -1, 1e9, 1, **{null: None}) == ERR_ARG, null
    assert dv.commit_call(0.9, -1, 1e9, 1, n_steps=0) == ERR_ARG and dv.commit_call(0.9, -1, 1e9, 1, n_steps=-3) == ERR_ARG
    assert dv.commit_call(0.9, -1, 1e9, -1) == ERR_ARG
    torch.cuda.synchronize()
    after = dv.snapshot()
    assert unchanged(before, after) and all(same_bits(before[k], after[k]) for k in ("es2", "cost_prev", "cost_list", "std_list", "es1", "ratio", "rec"))
    assert list(before["ints"]) == list(after["ints"])


# ======================================================================================================================================
# Adam: layout
# ======================================================================================================================================
GUARD, SENTINEL = 64, -1234.5678


class Arena:
    """Tensors of the given sizes as views of ONE buffer, in shuffled order, not adjacent, a 64-element guard band on each side of each."""

    def __init__(self, sizes, order, fill):
        off, o = {}, 0
        for i in order:
            o += GUARD
            off[i] = o
            o += sizes[i] + GUARD + 3 * (i % 2)  # (odd gaps: no tensor but the first starts on a 256-element boundary)
        self.buf = torch.full((o,), SENTINEL, dtype=f64, device=dev())
        self.views = [self.buf[off[i]:off[i] + sizes[i]] for i in range(len(sizes))]
        self.inside = np.zeros(o, dtype=bool)
        for i, n in enumerate(sizes):
            self.inside[off[i]:off[i] + n] = True
            if fill is not None:
                self.views[i].copy_(G(fill[i]))

    def guards_intact(self):
        return bool(np.all(self.buf.cpu().numpy().copy()[~self.inside] == SENTINEL))


def run_layout(sizes, null_grad, seed, what):
    p0, seq = ot.adam_layout_case(sizes=sizes, null_grad=null_grad, seed=seed)
    n = len(sizes)
    order = list(np.random.RandomState(seed).permutation(n))
    zeros = [np.zeros(k) for k in sizes]
    P, Gr, M, V = Arena(sizes, order, p0), Arena(sizes, order[::-1], zeros), Arena(sizes, order[1:] + order[:1], zeros), Arena(sizes, order, zeros)
    at = ot.AdamTruth(p0, 0.01)
    tally = AdamTally()
    skipped = [i for i in range(n) if i in null_grad or sizes[i] == 0]
    for s, row in enumerate(seq):
        for i, g in enumerate(row):
            if g is not None and sizes[i]:
                Gr.views[i].copy_(G(g))
        gs = [None if row[i] is None else Gr.views[i] for i in range(n)]
        assert adam_call(P.views, gs, M.views, V.views, 0.01, step=s + 1) == 0
        at.step(row)
        torch.cuda.synchronize()
        tally.add(dict(p=[t.cpu().numpy().copy() for t in P.views], m=[t.cpu().numpy().copy() for t in M.views], v=[t.cpu().numpy().copy() for t in V.views]), at)
    for a in (P, Gr, M, V):
        assert a.guards_intact()
    for i in skipped:  # a NULL gradient, numel 0: bitwise untouched
        assert same_bits(P.views[i].cpu().numpy().copy(), p0[i]) and not M.views[i].cpu().numpy().copy().any() and not V.views[i].cpu().numpy().copy().any()
    tally.check(ot.adam_distance(p0, seq, 0.01), what)
    return P, Gr, M, V


def test_adam_layout_sizes_that_straddle_the_blocks():
    """One launch over tensors of 1, 255, 256, 257, 3 and 1025 elements, allocated out of order with guard bands, a NULL gradient in the
    middle of the list and a tensor without elements; 50 steps; gradients with exact zeros, negatives, 1e150, -1e160 (exp_avg_sq
    overflows) and +-1e-170 (g^2 underflows: denom = eps)."""
    run_layout(ot.LAYOUT_SIZES, (ot.LAYOUT_NULL_GRAD,), 5, "layout")


def test_adam_32_tensors_in_one_call_and_33_refused():
    sizes = [1 + (7 * i) % 13 for i in range(32)]
    P, Gr, M, V = run_layout(sizes, (), 6, "32 tensors")
    extra = torch.zeros(4, dtype=f64, device=dev())
    before = [a.buf.clone() for a in (P, M, V)]
    rc = adam_call(P.views + [extra], Gr.views + [extra.clone()], M.views + [extra.clone()], V.views + [extra.clone()], 0.01, step=51)
    torch.cuda.synchronize()
    assert rc == ERR_LIMIT
    assert all(torch.equal(a.buf, b) for a, b in zip((P, M, V), before)) and not extra.any()


def test_adam_gp_training_form():
    """state == NULL: `step` = 1 .. 50 follows the truth; step < 1 and a state without a cost are refused; a status word with
    MCP_STATUS_NOT_SPD skips that call and every later one (the bit is sticky), bitwise; other bits do not."""
    sizes = [5, 300]
    p0, seq = ot.adam_layout_case(sizes=sizes, null_grad=(), seed=8)
    p, g, m, v = [G(q) for q in p0], [G(np.zeros(k)) for k in sizes], [G(np.zeros(k)) for k in sizes], [G(np.zeros(k)) for k in sizes]
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    at, tally = ot.AdamTruth(p0, 0.01), AdamTally()
    snap = lambda: dict(p=[t.cpu().numpy().copy() for t in p], m=[t.cpu().numpy().copy() for t in m], v=[t.cpu().numpy().copy() for t in v])
    for bad in (0, -1):
        assert adam_call(p, g, m, v, 0.01, step=bad) == ERR_ARG
    state = torch.zeros(7, dtype=i64, device=dev())
    assert adam_call(p, g, m, v, 0.01, state=state, n_steps=5, cost=None) == ERR_ARG
    torch.cuda.synchronize()
    assert unchanged(snap(), dict(p=p0, m=[np.zeros(k) for k in sizes], v=[np.zeros(k) for k in sizes]))
    for s, row in enumerate(seq):
        for t, r in zip(g, row):
            t.copy_(G(r))
        status.fill_(0 if s % 3 else (1 | 2 | 8))  # bits that mean nothing here
        assert adam_call(p, g, m, v, 0.01, step=s + 1, status=status if s % 2 else None) == 0
        at.step(row)
        torch.cuda.synchronize()
        tally.add(snap(), at)
    tally.check(ot.adam_distance(p0, seq, 0.01), "GP-training form")
    before = snap()
    status.fill_(4 | 1)
    for s in (51, 52, 53):
        assert adam_call(p, g, m, v, 0.01, step=s, status=status) == 0
    torch.cuda.synchronize()
    assert unchanged(before, snap())


# ======================================================================================================================================
# the class loop on the same scripts
# ======================================================================================================================================
def parse_decisions(txt):
    steps, ratios, lr_steps, exit_steps = [], [], [], []
    for line in txt.splitlines():
        m = re.match(r"Optimization step:\s+(\d+)$", line)
        if m:
            steps.append(int(m.group(1)))
        if line.startswith("diff_cost_ratio:"):
            ratios.append(float(line.split(":", 1)[1]))
        if line.startswith("REDUCING THE LEARNING RATE"):
            lr_steps.append(steps[-1])
        if line.startswith("EXIT FROM OPTIMIZATION"):
            exit_steps.append(steps[-1])
    assert [int(s) for s in re.findall(r"^Optimization_step: (\d+)$", txt, flags=re.M)] == lr_steps
    return steps, ratios, lr_steps, exit_steps


def class_run(script, kw, depth):
    from mc_pilco_amd.policy_learning import MC_PILCO, Policy

    d = dev()
    with contextlib.redirect_stdout(io.StringIO()):
        obj = MC_PILCO.MC_PILCO(T_sampling=0.05, state_dim=2, input_dim=1, f_sim=lambda y, t, u: None, f_model_learning=lambda **k: None,
                                model_learning_par={}, f_rand_exploration_policy=Policy.Random_exploration,
                                rand_exploration_policy_par=dict(state_dim=2, input_dim=1, u_max=1.0, dtype=f64),
                                f_control_policy=Policy.Sum_of_gaussians, control_policy_par=dict(dtype=f64, device=d, **ot.POLICY, **ot.policy_init()),
                                f_cost_function=torch.nn.Identity, cost_function_par={}, log_path=None, dtype=f64, device=d)
    obj.pipeline_depth = depth
    params = list(obj.control_policy.parameters())
    assert [tuple(q.shape) for q in params] == [(1, 2), (3, 2), (1, 3)]
    xs, us = torch.zeros(1, 1, 2, dtype=f64, device=d), torch.zeros(1, 1, 1, dtype=f64, device=d)

    def apply_policy(**k):  # advances the rollout counter as the real one does: the host's rewind after discarded attempts keeps the script aligned
        obj._rollout_calls += 1
        obj.last_status = None
        return xs, us

    obj.apply_policy = apply_policy
    obj.cost_function = ot.ScriptedCost(params, script["warm"], script["s"], script["std"], script["w"], index=lambda: obj._rollout_calls - 1, device=d)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        costs, stds, _, _ = obj.reinforce_policy(
            T_control=0.5, num_particles=4, trial_index=0, particles_initial_state_mean=None, particles_initial_state_var=None,
            flg_particles_init_uniform=False, particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
            f_optimizer="lambda p, lr : torch.optim.Adam(p, lr)", num_step_print=1, policy_reinit_dict=ot.REINIT, p_dropout_list=None, **kw)
    txt = re.sub(r"time elapsed:  [0-9.e+-]+", "time elapsed", buf.getvalue())
    return dict(costs=costs, stds=stds, txt=txt, final=np.concatenate([q.detach().cpu().numpy().copy().reshape(-1) for q in params]), calls=obj._rollout_calls)


@pytest.mark.parametrize("name", ["a_thresholds", "b_retries", "c_reinit"])
def test_class_loop_takes_the_references_decisions_on_the_script(fx, name):
    """The drop-in MC_PILCO.reinforce_policy with apply_policy / cost_function scripted, at pipeline_depth 0 and 1: the host's reading of
    the record against a script with real thresholds.  Cost lists, decisions and their steps are the reference's, exactly; the printed
    |ratio| values are those of LoopTruth(sqrt="ieee"), bit for bit (the reference's own differ from them by its square root's last bit);
    the final parameters to Adam's bound; the two depths bit-equal."""
    script, kw = ot.load_case(fx, name)
    g = lambda k: fx[name + "_" + k]
    runs = {depth: class_run(script, kw, depth) for depth in (0, 1)}
    start, seq, restarts = ot.script_grad_seq(script, kw)
    measured = ot.adam_distance(start, seq, kw["lr_list"][0], restart_at=restarts)
    truth = ot.drive_script(script, kw, ot.params0(), sqrt="ieee")
    assert truth["lr_steps"] == list(g("lr_steps")) and truth["exit_steps"] == list(g("exit_steps"))
    for depth, r in runs.items():
        steps, ratios, lr_steps, exit_steps = parse_decisions(r["txt"])
        assert same_bits(r["costs"], g("cost_list")) and same_bits(r["stds"], g("std_list")), depth
        assert lr_steps == list(g("lr_steps")) and exit_steps == list(g("exit_steps")), (depth, lr_steps, exit_steps)
        assert steps == list(g("printed_steps")) and same_bits(ratios, [p[1] for p in truth["printed"]]), depth
        assert r["txt"].count("Cost is NaN: try sampling again") == int(g("n_retry")) and r["txt"].count("re-initialize control policy") == int(g("n_reinit"))
        assert r["calls"] == 1 + int(g("consumed")), (depth, r["calls"])
        dist = ot.tensor_distance(r["final"], g("final"))
        print("%s depth %d: final parameters vs the reference's %.3g (bound %.3g)" % (name, depth, dist, ot.adam_bound(measured["p"])))
        assert dist <= ot.adam_bound(measured["p"])
    a, b = runs[0], runs[1]
    assert same_bits(a["final"], b["final"]) and same_bits(a["costs"], b["costs"]) and same_bits(a["stds"], b["stds"]) and a["txt"] == b["txt"]
