"""The workers of tests/test_rank_harness_cpu.py: ordinary exits and sleeps, no torch, no process group."""
import os
import time


def report(rank, world, port, out_q, value):
    out_q.put((rank, value + rank, port))


def report_from_rank_0(rank, world, port, out_q):
    if rank == 0:
        out_q.put(("rank 0 of", world))


def rank_1_leaves_with_3(rank, world, port, out_q):
    if rank == 1:
        os._exit(3)
    time.sleep(120)
    out_q.put(rank)


def rank_1_raises(rank, world, port, out_q):
    if rank == 1:
        raise ValueError("an ordinary error in rank 1")
    time.sleep(120)
    out_q.put(rank)


def sleeper(rank, world, port, out_q):
    time.sleep(120)
    out_q.put(rank)
