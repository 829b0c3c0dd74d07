"""The parts of ``MC_PILCO.reinforce_policy``: the attempt record by name, the device-side loop state, the guarded Adam's operands, the host's
schedule of lr / dropout / exit window, the two HIP graphs of recorded attempts, and what one call of the method holds of them."""
import ctypes as C
import time
from collections import namedtuple

import torch

from mc_pilco_amd import hipabi as abi

# what mcp_policy_step_commit leaves per attempt, in its order (include/mcpilco_hip.h)
AttemptRecord = namedtuple("AttemptRecord", "counted void step attempt pending cost std abs_ratio nan sync nonpos total_attempts")
Attempt = namedtuple("Attempt", "states inputs cost rec ev snap")  # in flight: outputs, pinned record row, the copy's event, counters before


def read(attempt):
    attempt.ev.synchronize()
    return AttemptRecord(*attempt.rec.tolist())


class LoopState:
    """``st`` is mcp_opt_state: int64 words step, attempt, pending, adam_t, total_attempts, then the doubles es2, cost_prev.  An attempt writes
    its record into a device row (``rec_dev``; a replayed one into its graph's own) and the host reads it from the pinned row of the same slot
    (``ring``); with ``depth + 2`` slots none is written again before the host has read it."""

    def __init__(self, n_steps, depth, warm_cost, dtype, device):
        if dtype != torch.float64:
            # the loop state, the cost lists and the Adam kernel are double precision on the device (mcp_opt_state, mcp_adam_step_guarded):
            # another dtype would be read through double* -- refuse it here rather than take garbage decisions
            raise RuntimeError("reinforce_policy on the HIP path works in torch.float64 (the kernels are fp64); got dtype %s" % dtype)
        zeros = lambda *shape: torch.zeros(*shape, dtype=dtype, device=device)
        self.n_steps, self.slots, self.seq = n_steps, depth + 2, 0
        self.st = torch.zeros(7, dtype=torch.int64, device=device)
        self.cost_list, self.std_list, self.es1, self.ratio = zeros(n_steps), zeros(n_steps), zeros(n_steps + 1), zeros(n_steps + 1)
        self.ring = [torch.empty(abi.OPT_RECORD_DOUBLES, dtype=dtype).pin_memory() for _ in range(self.slots)]
        self.rec_dev = zeros(self.slots, abi.OPT_RECORD_DOUBLES)
        self.st[5:].view(torch.float64)[1:2].copy_(warm_cost.detach().reshape(1))   # cost_tm1 = the warm-up cost (MC_PILCO.py:462)

    def clear_pending(self):
        self.st[2:3].zero_()

    def zero_adam_t(self):
        self.st[3:4].zero_()

    def reset_after_reinit(self):
        self.st[0:5].zero_()  # (ES2 and cost_tm1 are NOT reset by the reference: they keep the failed step's values)
        for a in (self.cost_list, self.std_list, self.es1, self.ratio):
            a.zero_()


class GuardedAdam:
    """Parameters, fresh moments and their pointer arrays for ``opt``, a plain Adam; ``hyper`` = MC_PILCO._plain_adam(opt)."""

    def __init__(self, opt, hyper):
        _, self.beta1, self.beta2, self.eps = hyper  # (the rate comes with every step: the schedule's)
        self.ps = [q for q in opt.param_groups[0]["params"] if q.requires_grad]
        self.m, self.v = [torch.zeros_like(q) for q in self.ps], [torch.zeros_like(q) for q in self.ps]
        self.numel = (C.c_int64 * len(self.ps))(*[q.numel() for q in self.ps])
        self.c_ps, self.c_m, self.c_v = (self.pointers(t.data_ptr() for t in ts) for ts in (self.ps, self.m, self.v))

    def pointers(self, addresses):
        return (abi.dptr * len(self.ps))(*addresses)  # (one device address, or None, per parameter)

    def step(self, grads, lr, state, cost_ptr, flags, status):
        """The update, applied on the device only if this attempt counts.  ``grads``: ``pointers``; ``lr``: the schedule's rate."""
        abi.check(abi.lib().mcp_adam_step_guarded(len(self.ps), self.c_ps, grads, self.c_m, self.c_v, self.numel, float(lr), self.beta1, self.beta2,
                                                  self.eps, abi.ptr(state.st), 0, state.n_steps, cost_ptr, abi.ptr(flags), abi.ptr(status),
                                                  abi.stream()), "mcp_adam_step_guarded")


class HostSchedule:
    """What the host holds between the attempts: the learning rate, the dropout probability, the two thresholds of the exit window."""

    def __init__(self, lr, p_drop, min_diff_cost, min_step, lr_min, lr_reduction_ratio, p_drop_reduction, num_min_diff_cost):
        self.start = (lr, p_drop, min_diff_cost, min_step)
        self.lr_min, self.lr_reduction_ratio, self.p_drop_reduction, self.n_win = lr_min, lr_reduction_ratio, p_drop_reduction, num_min_diff_cost
        self.reset()

    def reset(self):
        self.lr, self.p_drop, self.min_diff, self.min_step = self.start
        self.prev_cost = 0.0

    def step_print(self, k, cost, ratio):
        print("\nOptimization step: ", k)
        print("cost: ", cost)
        print("cost improvement: ", self.prev_cost - cost)
        print("p_dropout_applied: ", self.p_drop)
        print("current_min_diff_cost; ", self.min_diff)
        print("current_min_step: ", self.min_step)
        print("diff_cost_ratio: ", ratio)
        print("time elapsed: ", time.time() - self.t_mark)
        self.prev_cost = cost
        self.t_mark = time.time()

    def lr_or_exit(self, k):
        """The condition of MC_PILCO.py:540-547 held at step k.  True: leave the loop."""
        if self.lr > self.lr_min:
            print("Optimization_step:", k)
            print("\nREDUCING THE LEARNING RATE:")
            self.lr = max(self.lr * self.lr_reduction_ratio, self.lr_min)
            print("lr: ", self.lr)
            self.min_diff = max(self.min_diff / 2, 0.01)
            self.min_step = k + self.n_win
            print("\nREDUCING THE DROPOUT:")
            self.p_drop = max(self.p_drop - self.p_drop_reduction, 0.0)
            print("p_dropout_applied: ", self.p_drop)
            return False
        print("\nEXIT FROM OPTIMIZATION: diff_cost_ratio < min_diff_cost for num_min_diff_cost steps")
        return True


class AttemptGraphs:
    """One attempt = rollout -> cost -> adjoint -> guarded Adam -> commit: ~15 launches and as many host calls.  In the pipelined loop it is
    recorded ONCE into a HIP graph and replayed (round 6): everything an attempt reads that changes from one attempt to the next lives in device
    memory -- the parameters, the loop state, torch's generator offset (graph-safe) and the rollout counter of the in-kernel noise
    (mcp_noise.call_dev, ``owner._call_dev``, advanced by the graph itself) -- so a replay takes the same step the eager calls would, bit for
    bit.  Two graphs alternate (each with its own trajectories and record row: an attempt voided while the host decides must not overwrite the
    outputs of the one before it).  The first two attempts after every (re)start run eagerly (they warm the launch paths); a host decision that
    changes a recorded value -- lr, dropout, new Adam moments, re-initialised parameters -- drops the graphs."""

    def __init__(self, owner, dtype, device):
        self.owner, self.on, self.device = owner, False, device
        self.rec = torch.zeros(2, abi.OPT_RECORD_DOUBLES, dtype=dtype, device=device)
        self.one = torch.ones(1, dtype=dtype, device=device)  # (the upstream gradient of the recorded cost)
        self.last_flat = None  # the gradients of the last attempt by id(parameter) when it was a replay, else None
        self.drop()

    def drop(self):
        self.graphs, self.outs, self.eager = [None, None], [None, None], 0
        self.owner._call_dev = None

    def run(self, gi, body, snap):
        """The next attempt as a replay of graph ``gi``, recorded first (``body(record row)``) where there is none: (what ``body`` returned, the
        record row).  None: the caller launches it eagerly -- no graphs, the first two attempts after a (re)start, recording raised."""
        mc, dev = self.owner, self.device
        if not self.on or self.eager < 2:
            return None
        if self.graphs[gi] is None:
            # record: the kernels are not run here; the replay below is this attempt
            if mc._call_dev is None:
                mc._call_dev = torch.zeros(1, dtype=torch.int64, device=dev)
            mc._call_dev.fill_(mc._rollout_calls)
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g):
                    self.outs[gi] = body(self.rec[gi])
                self.graphs[gi] = g
            except Exception as e:  # noqa: BLE001  (a runtime that cannot record this sequence: the eager loop is the same loop)
                print("\nreinforce_policy: recording an attempt into a graph failed (%r) -- continuing with eager launches" % (e,))
                self.on = False
                mc._rollout_calls = snap[0]
                if snap[1] is not None:
                    torch.cuda.set_rng_state(snap[1], dev)
                self.drop()
                return None
        else:
            mc._rollout_calls += 1  # (the host's mirror of the counter the replay advances)
        self.graphs[gi].replay()
        mc.attempts_replayed += 1
        return self.outs[gi], self.rec[gi]


class PolicyLoop:
    """What one call of ``reinforce_policy`` holds: the parts above, the optimizer f_optimizer built last, the arguments of the rollouts."""

    def __init__(self, owner, make_opt, sched, n_steps, warm_cost, sim, trial_index, alpha_diff_cost):
        self.owner, self.make_opt, self.sched, self.sim, self.trial_index, self.alpha = owner, make_opt, sched, sim, trial_index, float(alpha_diff_cost)
        self.depth = int(getattr(owner, "pipeline_depth", 1))
        self.state = LoopState(n_steps, self.depth, warm_cost, owner.dtype, owner.device)
        self.graphs = AttemptGraphs(owner, owner.dtype, owner.device)
        self.new_optimizer(same_kind=False)
        if self.adam is None or owner.noise_mode == "reference" or owner.dist_group is not None:
            self.depth = 0
        self.graphs.on = self.depth > 0 and owner._recordable()

    def new_optimizer(self, same_kind=True):
        """f_optimizer at the schedule's lr: new moments, adam_t = 0; what the graphs recorded is gone."""
        self.opt = self.make_opt(p=self.owner.control_policy.parameters(), lr=self.sched.lr)
        hyper = self.owner._plain_adam(self.opt)
        if same_kind and (hyper is None) != (self.adam is None):
            raise RuntimeError("f_optimizer must build the same kind of optimizer on every call")
        self.adam = None if hyper is None else GuardedAdam(self.opt, hyper)
        self.params = list(self.owner.control_policy.parameters())
        self.state.zero_adam_t()
        self.graphs.drop()

    def commit(self, cost, std, flags, status, grads, rec_row):
        """The attempt's guarded update and the device's decision about it (the record goes to ``rec_row``)."""
        st, sched, cost_ptr = self.state, self.sched, abi.ptr(cost.detach().reshape(1))
        if self.adam is not None:
            self.adam.step(grads, sched.lr, st, cost_ptr, flags, status)
        abi.check(abi.lib().mcp_policy_step_commit(abi.ptr(st.st), st.n_steps, cost_ptr, abi.ptr(std.detach().reshape(1)), abi.ptr(flags),
                                                   abi.ptr(status), abi.ptr(st.cost_list), abi.ptr(st.std_list), abi.ptr(st.es1), abi.ptr(st.ratio),
                                                   self.alpha, float(min(sched.min_step, 1e300)), float(sched.min_diff), int(sched.n_win),
                                                   abi.ptr(rec_row), abi.stream()), "mcp_policy_step_commit")
