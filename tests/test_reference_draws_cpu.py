"""CPU: the host-side pieces of the optimizer loop that need no device.

``MC_PILCO.reference_draws`` against the draw loops it replaced, written out here as they stood in ``_rollout_noise``, the former
``_feedback_noise`` and the two fused branches of ``MC_PILCO4PMS.apply_policy`` (the order of these draws is what seed-for-seed parity with the reference rests on);
``opt_loop.AttemptRecord`` against the record's order in tests/opt_truth.py; ``opt_loop.HostSchedule.lr_or_exit`` against the lines of the
loop it came from."""
import contextlib
import io
import types

import pytest
import torch

import opt_truth as ot
from mc_pilco_amd import hipabi
from mc_pilco_amd.policy_learning import opt_loop
from mc_pilco_amd.policy_learning.MC_PILCO import MC_PILCO, reference_draws

f64 = torch.float64
Mt, G, B, NPOS = 5, 2, 3, 2


def spelled_out(T, p, n_pos):
    """The loops as they were written at each of the four sites (masks only where p > 0, position noise only in the PMS branches)."""
    masks = [torch.empty(Mt, 1, B, dtype=f64).bernoulli_(1 - p).reshape(Mt, B)] if p > 0 else None
    eps, pn = [], []
    for _ in range(1, T):
        eps.append(torch.empty(Mt, G, dtype=f64).normal_())
        if n_pos:
            pn.append(torch.randn(Mt, n_pos, dtype=f64))
        if p > 0:
            masks.append(torch.empty(Mt, 1, B, dtype=f64).bernoulli_(1 - p).reshape(Mt, B))
    stack = lambda l, w: torch.stack(l) if l else torch.zeros(0, Mt, w, dtype=f64)
    return stack(eps, G), None if masks is None else torch.stack(masks).to(torch.uint8), stack(pn, n_pos) if n_pos else None


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("p,n_pos", [(0.0, 0), (0.25, 0), (0.0, NPOS), (0.25, NPOS)])
def test_reference_draws_are_the_spelled_out_sequences(T, p, n_pos):
    torch.manual_seed(1234)
    want = spelled_out(T, p, n_pos)
    want_rng = torch.get_rng_state()
    torch.manual_seed(1234)
    got = reference_draws(Mt, T, G, f64, B=B, p_drop=p, n_pos=n_pos)
    assert torch.equal(torch.get_rng_state(), want_rng)
    shapes = ((T - 1, Mt, G), (T, Mt, B), (T - 1, Mt, n_pos))
    for g, w, shape, present in zip(got, want, shapes, (True, p > 0, n_pos > 0)):
        assert (g is not None) == present and (w is not None) == present
        if present:
            assert tuple(g.shape) == shape and g.dtype == w.dtype and torch.equal(g, w)
            # a rank's shard, cut by the driver's own slicing, is the same rows of the spelled-out draw
            assert torch.equal(MC_PILCO._shard_slice(types.SimpleNamespace(_shard=(1, 2)), g, 1), w[:, 1:3])
    assert got[0].dtype == f64 and (got[1] is None or got[1].dtype == torch.uint8)


def test_attempt_record_names_the_commit_record_in_order():
    assert opt_loop.AttemptRecord._fields == ot.RECORD
    assert len(opt_loop.AttemptRecord._fields) == hipabi.OPT_RECORD_DOUBLES
    r = opt_loop.AttemptRecord(*[float(i) for i in range(hipabi.OPT_RECORD_DOUBLES)])
    assert [getattr(r, n) for n in ot.RECORD] == [float(i) for i in range(hipabi.OPT_RECORD_DOUBLES)]


def loop_lines(hs, k, lr_min, lr_reduction_ratio, p_drop_reduction, num_min_diff_cost):
    """``lr_or_exit`` as the loop had it, on the dict the loop kept."""
    if hs["lr"] > lr_min:
        print("Optimization_step:", k)
        print("\nREDUCING THE LEARNING RATE:")
        hs["lr"] = max(hs["lr"] * lr_reduction_ratio, lr_min)
        print("lr: ", hs["lr"])
        hs["min_diff"] = max(hs["min_diff"] / 2, 0.01)
        hs["min_step"] = k + num_min_diff_cost
        print("\nREDUCING THE DROPOUT:")
        hs["p_drop"] = max(hs["p_drop"] - p_drop_reduction, 0.0)
        print("p_dropout_applied: ", hs["p_drop"])
        return False
    print("\nEXIT FROM OPTIMIZATION: diff_cost_ratio < min_diff_cost for num_min_diff_cost steps")
    return True


@pytest.mark.parametrize("lr", [0.01, 0.004, 0.006], ids=["above lr_min", "at lr_min", "the ratio would go below lr_min"])
def test_host_schedule_lr_or_exit(lr):
    lr_min, ratio, p_red, n_win, k = 0.004, 0.5, 0.125, 7, 31
    hs = dict(lr=lr, p_drop=0.25, min_diff=0.03, min_step=12.0)
    sched = opt_loop.HostSchedule(lr, 0.25, 0.03, 12.0, lr_min, ratio, p_red, n_win)
    want_txt, got_txt = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(want_txt):
        want = loop_lines(hs, k, lr_min, ratio, p_red, n_win)
    with contextlib.redirect_stdout(got_txt):
        got = sched.lr_or_exit(k)
    assert got is want and got == (lr <= lr_min)
    assert (sched.lr, sched.p_drop, sched.min_diff, sched.min_step) == (hs["lr"], hs["p_drop"], hs["min_diff"], hs["min_step"])
    assert got_txt.getvalue() == want_txt.getvalue() and got_txt.getvalue() != ""
    if lr == 0.006:
        assert sched.lr == lr_min  # (0.003 clamped)
