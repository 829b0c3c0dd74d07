"""tests/rank_harness.run_ranks on workers that only put, leave or sleep (tests/rank_workers.py): results and exit codes on the passing path;
a rank that dies before it reports, and a deadline, end the call at once and leave no child behind.  No GPU, no torch.distributed.

The 30 s of the failure cases is a condition, not a measurement: far below the sleepers' 120 s, well above the start-up of a spawned child."""
import multiprocessing
import time

import pytest

import rank_workers as rw
from rank_harness import run_ranks

SOON = 30.0


def test_two_ranks_return_their_results():
    res = sorted(run_ranks(rw.report, 2, args=(10,)))
    assert [r[:2] for r in res] == [(0, 10), (1, 11)]
    assert res[0][2] == res[1][2] and res[0][2] > 0  # one free port, the same for both
    assert multiprocessing.active_children() == []
    assert run_ranks(rw.report, 1, args=(5,)) == [(0, 5, 0)]  # a single process: no port, the same supervision


@pytest.mark.parametrize("worker,code", [(rw.rank_1_leaves_with_3, 3), (rw.rank_1_raises, 1)], ids=["os._exit(3)", "exception"])
def test_a_rank_that_dies_before_it_reports_ends_the_call(worker, code):
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match=r"rank 1 of 2 ended with exit code %d\b" % code):
        run_ranks(worker, 2)
    assert time.monotonic() - t0 < SOON
    assert multiprocessing.active_children() == []  # the sleeper was terminated


def test_the_deadline_ends_the_call():
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match="deadline of 2 s passed with 0 of 2 results in"):
        run_ranks(rw.sleeper, 2, timeout=2)
    assert 2.0 <= time.monotonic() - t0 < SOON
    assert multiprocessing.active_children() == []


def test_results_from_rank_0_only():
    assert run_ranks(rw.report_from_rank_0, 2, expect=1) == [("rank 0 of", 2)]  # (both exit codes were checked before the return)
    assert multiprocessing.active_children() == []
    with pytest.raises(AssertionError, match="every rank ended with exit code 0, 1 of 2 results missing"):
        run_ranks(rw.report_from_rank_0, 2)
