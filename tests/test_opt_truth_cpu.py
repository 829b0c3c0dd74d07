"""CPU: the truth of the optimizer loop (tests/opt_truth.py) is pinned to the reference.

tests/golden/opt_loop_script.npz holds what the reference's own ``MC_PILCO.reinforce_policy`` did on scripted costs (made by
tests/golden/make_golden_opt_loop.py).  ``LoopTruth`` + ``AdamTruth`` driven by the same scripts must take the same decisions at the same
steps, print the same |ratio| values, keep the same cost / std lists and -- both sides being torch.optim.Adam on the CPU -- hold the same
parameters at every evaluation, exactly.  Neither a GPU nor the reference is needed here.

``adam_longdouble`` against ``AdamTruth``: the distance measured here is the float64 rounding level of the update, which bounds the
kernel's distance to AdamTruth in tests/test_gpu_opt_loop.py (8 x, floored at 2^-50).  Measured (x86-64, 80-bit long double):
    script a_thresholds (11 parameters, 24 steps)         p 9.5e-16   m 4.9e-16   v 4.8e-16
    script b_retries (8 steps)                            p 4.7e-16   m 6.4e-16   v 2.9e-16
    layout case (8 tensors, 50 steps, 1e150 / 1e-170)     p 8.8e-16   m 3.9e-16   v 6.1e-16
    32 tensors, 50 steps                                  p 1.1e-15   m 1.8e-15   v 9.3e-16
"""
import math

import numpy as np
import pytest
import torch

import opt_truth as ot

MARGIN = 1e-6


@pytest.fixture(scope="module")
def fx(golden):
    return golden("opt_loop_script")


def names(fx=None):
    return ["a_thresholds", "b_retries", "c_reinit", "d_n0", "d_n_gt_k", "d_n_gt_steps", "d_min_step_neg", "e_zero_diff"]


def test_fixture_holds_every_script(fx):
    assert sorted(str(n) for n in fx["names"]) == sorted(names())
    assert len(fx["a_thresholds_lr_steps"]) == 2 and len(fx["a_thresholds_exit_steps"]) == 1
    assert int(fx["b_retries_n_retry"]) == 1 + 9 + 2 + 5 and int(fx["c_reinit_n_reinit"]) == 1 and int(fx["c_reinit_n_retry"]) == 10
    assert np.all(np.isnan(fx["e_zero_diff_printed_ratio"]))


@pytest.mark.parametrize("name", names())
def test_truth_takes_the_references_decisions(fx, name):
    script, kw = ot.load_case(fx, name)
    g = lambda k: fx[name + "_" + k]
    tested = []

    def on_attempt(i, kind, lt, at):
        k, n = int(lt.record[2]), lt.n_win
        if kind == "counted" and k > lt.min_step and n > 0 and k + 1 - n >= 0:
            tested.append((np.abs(lt.ratio.numpy()[k + 1 - n:k + 1]).copy(), lt.min_diff))

    r = ot.drive_script(script, kw, ot.params0(), on_attempt=on_attempt)
    # the same decisions at the same steps
    assert r["lr_steps"] == list(g("lr_steps")) and r["exit_steps"] == list(g("exit_steps"))
    assert r["consumed"] == int(g("consumed"))
    assert r["kinds"].count("failed") + r["kinds"].count("tenth") == int(g("n_retry")) and r["kinds"].count("tenth") == int(g("n_reinit"))
    # |ratio| as printed (numpy prints a float64 so that it round-trips: equal means bit-equal), step by step
    assert [p[0] for p in r["printed"]] == list(g("printed_steps"))
    assert np.array_equal(np.array([p[1] for p in r["printed"]]), g("printed_ratio"), equal_nan=True)
    # the lists
    assert r["cost_list"].shape == g("cost_list").shape and np.array_equal(r["cost_list"], g("cost_list"), equal_nan=True)
    assert np.array_equal(r["std_list"], g("std_list"), equal_nan=True)
    # the parameters every evaluation saw (after every counted step, unchanged through retries, re-initialised), and the final ones:
    # torch.optim.Adam on the CPU on both sides, equal
    assert np.array_equal(np.array(r["thetas"]), g("thetas"))
    assert np.array_equal(r["final"], g("final"))
    # no decision hinges on a last bit: every |ratio| of every tested window is at least 1e-6 (relative) away from its bound
    for win, md in tested:
        win = win[np.isfinite(win)]
        assert win.size == 0 or float(np.min(np.abs(win - md) / md)) >= MARGIN
    if name == "a_thresholds":
        hits = [int(np.sum(w < md)) for w, md in tested]
        assert hits.count(2) >= 2 and hits.count(3) == 3 and min(hits) == 0  # windows that miss by exactly one entry, that hold, that are empty


@pytest.mark.parametrize("name", names())
def test_ieee_square_root_form_stays_with_the_reference(fx, name):
    """LoopTruth(sqrt="ieee"), the form the kernels are compared with bit for bit: everything but |ratio| is still the reference's
    exactly, the decisions are the same, and |ratio| differs by no more than the root's last bit allows.  ratio[k + 1] = a ratio[k] +
    (1 - a) q_k with q_k = es1 / sqrt(es2): a root off by one ulp moves q_k by at most 2^-52 |q_k| (plus the quotient's rounding), so the
    two recursions -- a convex combination -- stay within 2^-52 max|q| plus their own roundings of each other: bound 2^-50 max(|q|, |ratio|)."""
    script, kw = ot.load_case(fx, name)
    g = lambda k: fx[name + "_" + k]
    qmax = [0.0]

    def on_attempt(i, kind, lt, at):
        if kind == "counted":
            q = float(lt.es1[lt.step] / math.sqrt(float(lt.es2))) if float(lt.es2) > 0 else float("nan")
            if np.isfinite(q):
                qmax[0] = max(qmax[0], abs(q))

    r = ot.drive_script(script, kw, ot.params0(), sqrt="ieee", on_attempt=on_attempt)
    assert r["lr_steps"] == list(g("lr_steps")) and r["exit_steps"] == list(g("exit_steps")) and r["consumed"] == int(g("consumed"))
    assert np.array_equal(r["cost_list"], g("cost_list"), equal_nan=True) and np.array_equal(np.array(r["thetas"]), g("thetas"))
    got, want = np.array([p[1] for p in r["printed"]]), g("printed_ratio")
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = np.isfinite(want)
    if ok.any():
        scale = max(qmax[0], float(np.max(np.abs(want[ok]))))
        assert float(np.max(np.abs(got[ok] - want[ok]))) <= 2.0 ** -50 * scale
        print("%s: %d of %d printed |ratio| differ in the last bits, worst %.3g relative"
              % (name, int(np.sum(got[ok] != want[ok])), int(ok.sum()), float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok])))))


def test_torch_cpu_square_root_is_not_correctly_rounded_everywhere():
    """Why the kernels are compared with the "ieee" form: the share of float64 arguments whose torch CPU square root is not the IEEE one.
    (Where a torch build rounds correctly the two forms of LoopTruth coincide and nothing is lost.)"""
    v = np.abs(np.random.RandomState(1).standard_normal(20000)) + 1e-3
    off = torch.as_tensor(v).sqrt().numpy() != np.sqrt(v)
    print("torch CPU sqrt differs from the correctly rounded root for %.2f %% of %d arguments" % (100.0 * off.mean(), v.size))
    assert np.max(np.abs(torch.as_tensor(v).sqrt().numpy() - np.sqrt(v)) / np.sqrt(v)) <= 2.0 ** -52


def test_truth_state_and_record_of_each_attempt_class():
    """The device-side view: counters, the void classes, the record's layout."""
    lt = ot.LoopTruth(3, 2.0, 0.9, -1, 1e9, 1, 0.01, lr_min=0.004)
    assert lt.attempt(float("nan"), 0.5) == "failed" and lt.record == [0, 0, 0, 1, 0, lt.record[5], 0.5, 0, 1, 0, 0, 1] and np.isnan(lt.record[5])
    assert lt.attempt(1.5, 0.25, "sync") == "failed" and lt.record[8:11] == [0, 1, 0] and lt.state()["attempt"] == 2
    assert lt.attempt(1.5, 0.25, "nonpos") == "failed" and lt.record[8:11] == [0, 0, 1]
    assert lt.attempt(1.5, 0.25) == "counted"  # min_step -1, n 1: ratio[0] = 0 is below the bound -> pending
    s = lt.state()
    assert (s["step"], s["attempt"], s["pending"], s["adam_t"], s["total_attempts"]) == (1, 0, 1, 1, 4) and s["cost_prev"] == 1.5
    assert lt.record[:5] == [1, 0, 0, 0, 1] and lt.record[7] == abs(float(lt.ratio[1])) and lt.record[11] == 4
    before = (lt.state(), lt.ratio.clone(), lt.es1.clone())
    assert lt.attempt(7.0, 0.1) == "void" and lt.record[:5] == [0, 1, 1, 0, 1] and lt.record[5] == 7.0 and lt.record[11] == 5
    s2 = lt.state()
    assert {k: v for k, v in s2.items() if k != "total_attempts"} == {k: v for k, v in before[0].items() if k != "total_attempts"}
    assert torch.equal(lt.ratio, before[1]) and torch.equal(lt.es1, before[2])
    assert lt.host_after_pending() == "lr" and lt.lr == 0.005 and lt.min_diff == 5e8 and lt.min_step == 1 and lt.state()["adam_t"] == 0
    for _ in range(9):
        assert lt.attempt(float("nan"), 0.0) == "failed"
    es2 = lt.state()["es2"]
    assert lt.attempt(float("nan"), 0.0) == "tenth" and lt.state()["attempt"] == 10 and np.isnan(lt.state()["es2"]) and not np.isnan(es2)
    assert lt.attempt(1.0, 0.0) == "void"
    lt.host_after_ten_failures()
    s = lt.state()
    assert (s["step"], s["attempt"], s["pending"], s["adam_t"], s["total_attempts"]) == (0, 0, 0, 0, 0)
    assert np.isnan(s["es2"]) and np.isnan(s["cost_prev"]) and lt.lr == 0.01 and lt.min_diff == 1e9  # (:580-603 reset neither ES2 nor cost_tm1)
    assert lt.attempt(1.0, 0.0) == "counted" and lt.state()["pending"] == 1  # the window is ratio[0] = 0 of the re-made array
    assert lt.host_after_pending() == "lr" and lt.min_step == 1
    for c in (0.9, 0.8):
        assert lt.attempt(c, 0.0) == "counted" and lt.state()["pending"] == 0 and np.isnan(lt.record[7])  # NaN monitors: a window of them never fires
    assert lt.attempt(0.7, 0.0) == "void"  # step == n_steps


def test_adam_longdouble_measures_the_rounding_level_of_float64_adam(fx):
    """AdamTruth against the longdouble restatement over the GPU tests' own gradient sequences: the distances are at the float64 rounding
    level (a few 2^-53 per step taken), the Inf patterns agree, and the bound derived from them stays far below the suite's 1e-8."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("numpy.longdouble carries no more than float64 on this platform: nothing to measure against")
    worst = {}
    for name in ("a_thresholds", "b_retries"):
        start, seq, restarts = ot.script_grad_seq(*ot.load_case(fx, name))
        worst[name] = ot.adam_distance(start, seq, 0.01, restart_at=restarts)
    p0, seq = ot.adam_layout_case()
    worst["layout"] = ot.adam_distance(p0, seq, 0.01)
    p0, seq = ot.adam_layout_case(sizes=[1 + (7 * i) % 13 for i in range(32)], null_grad=(), seed=6)
    worst["32 tensors"] = ot.adam_distance(p0, seq, 0.01)
    for k, w in worst.items():
        print("%-12s p %.3g  m %.3g  v %.3g  -> bound p %.3g" % (k, w["p"], w["m"], w["v"], ot.adam_bound(w["p"])))
        assert 0 < max(w.values()) < 64 * 2.0 ** -53 * 50, (k, w)  # not bit-equal by construction, and a rounding level: < 64 ulp per step
        assert ot.adam_bound(max(w.values())) < 1e-12


def test_adam_truth_inf_patterns_match_longdouble():
    p0, seq = ot.adam_layout_case()
    at = ot.AdamTruth(p0, 0.01)
    L = np.longdouble
    i = 4  # the 257-element tensor: 1e150 once at step 7, -1e160 from step 20 on, 1e-170 always
    P, M, V = p0[i].astype(L), np.zeros(257, dtype=L), np.zeros(257, dtype=L)
    for s, row in enumerate(seq):
        at.step(row)
        P, M, V = ot.adam_longdouble(P, M, V, row[i], s + 1, 0.01)
        v = at.v()[i].numpy()
        assert np.array_equal(np.isinf(v), np.isinf(V.astype(np.float64))) and not np.isnan(v).any() and not np.isnan(at.p()[i].numpy()).any()
        assert np.isfinite(v[0]) and (v[0] > 1e290) == (s >= 7) and np.isinf(v[128]) == (s >= 20) and v[256] == 0.0
