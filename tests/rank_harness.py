"""One way to run rank processes from a test: ``run_ranks`` starts them, watches them while it waits for their results, and leaves none
behind; ``rank_group`` is the worker's side of the rendezvous.  A plain module: neither torch nor the package is imported at module level, so
a spawned child starts quickly."""
import contextlib
import multiprocessing
import os
import queue
import signal
import socket
import time

POLL = 0.25  # seconds between two looks at the children while the queue is empty
JOIN = 60.0  # seconds a child gets to leave after the results are in


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _exit_name(code):
    if code is not None and code < 0:
        try:
            return "signal %s" % signal.Signals(-code).name
        except ValueError:
            return "signal %d" % -code
    return "exit code %s" % code


def run_ranks(target, world, args=(), expect=None, timeout=300.0):
    """``target(rank, world, port, out_q, *args)`` in ``world`` fresh processes (the spawn context); ``port`` is a free port for world > 1,
    else 0.  Returns the ``expect`` (default: ``world``) results the workers put on ``out_q``, in the order they arrived, after every child
    has ended with exit code 0.  A child that ends with another code, children that all end with results missing, or the deadline raise
    AssertionError at once; whatever happens, no child of the call is alive afterwards."""
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    port = free_port() if world > 1 else 0
    expect = world if expect is None else expect
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    deadline = time.monotonic() + timeout
    results = []
    try:
        for p in procs:
            p.start()
        # the results first, the joins after: a child that has put a large array does not end before it is read
        while len(results) < expect:
            try:
                results.append(q.get(timeout=POLL))
                continue
            except queue.Empty:
                pass
            codes = [p.exitcode for p in procs]
            for r, code in enumerate(codes):
                assert code in (None, 0), "rank %d of %d ended with %s before the results were in" % (r, world, _exit_name(code))
            if all(code == 0 for code in codes):
                try:  # (what a child put just before it ended)
                    results.append(q.get(timeout=POLL))
                    continue
                except queue.Empty:
                    raise AssertionError("every rank ended with exit code 0, %d of %d results missing" % (expect - len(results), expect)) from None
            assert time.monotonic() < deadline, "deadline of %g s passed with %d of %d results in" % (timeout, len(results), expect)
        for r, p in enumerate(procs):
            p.join(JOIN)
            assert p.exitcode is not None, "rank %d of %d did not end within %g s of the results" % (r, world, JOIN)
            assert p.exitcode == 0, "rank %d of %d ended with %s" % (r, world, _exit_name(p.exitcode))
        return results
    finally:
        live = [p for p in procs if p.pid is not None and p.is_alive()]
        for p in live:
            p.terminate()
        for p in live:
            p.join(5.0)
        for p in live:
            if p.is_alive():
                p.kill()
        for p in procs:
            if p.pid is not None:
                p.join(5.0)
        q.close()
        q.cancel_join_thread()


@contextlib.contextmanager
def rank_group(rank, world, port, backend="gloo"):
    """The worker's process group: the rendezvous address, ``init_process_group`` for world > 1 (yields the group, else None), and on the way
    out the barrier and ``destroy_process_group``."""
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if world == 1:
        yield None
        return
    dist.init_process_group(backend, rank=rank, world_size=world)
    yield dist.group.WORLD
    dist.barrier()
    dist.destroy_process_group()
