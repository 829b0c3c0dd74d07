"""Truth of the optimizer loop's two operators (helper of tests/test_opt_truth_cpu.py and tests/test_gpu_opt_loop.py; no tests here).

Torch CPU float64 and numpy only -- no project code.

``LoopTruth``   the per-attempt state machine of the reference's ``reinforce_policy`` (policy_learning/MC_PILCO.py:475-607), restated line
                for line with the reference's own torch expressions on 0-dim float64 tensors, driven one ATTEMPT at a time by
                ``(cost, std, failed_because)``.  After every attempt it exposes what ``mcp_opt_state`` must hold, the four arrays and the
                12-double record of ``mcp_policy_step_commit`` (include/mcpilco_hip.h).  The host's half of the loop (:551-566, :573-607) are
                the methods ``host_after_pending`` and ``host_after_ten_failures``.  Two forms: ``sqrt="torch"`` (the reference's
                expression; torch's CPU square root is off by one ulp for some arguments) and ``sqrt="ieee"`` (correctly rounded, as on the
                device) -- see the class.
``AdamTruth``   ``torch.optim.Adam`` itself (the reference's optimizer, :468) on CPU float64 copies of the tensors; a new instance wherever
                the host builds a new optimizer (:558, :605).
``adam_longdouble``  the same update in ``numpy.longdouble``: only to MEASURE how far float64 Adam sits from the exact update
                (``adam_distance``), which is what the kernel's distance to ``AdamTruth`` is bounded by (ADAM_BOUND_FACTOR x, floored at
                ADAM_BOUND_FLOOR).

``ScriptedCost`` / ``script_cases`` / ``drive_script``: the scripted cost that makes ``reinforce_policy`` a pure function of a script
(tests/golden/make_golden_opt_loop.py puts it on the reference's MC_PILCO object, tests/test_gpu_opt_loop.py on the drop-in's), the scripts,
and the loop that drives LoopTruth + AdamTruth through one of them the way the reference's while-loops do.
"""
import math

import numpy as np
import torch

MAX_ATTEMPTS = 10  # MC_PILCO.py:482 (MCP_OPT_MAX_ATTEMPTS)
RECORD = ("counted", "void", "step", "attempt", "pending", "cost", "std", "abs_ratio", "nan", "sync", "nonpos", "total_attempts")
ADAM_BOUND_FACTOR, ADAM_BOUND_FLOOR = 8.0, 2.0 ** -50

f64 = lambda v: torch.tensor(float(v), dtype=torch.float64)


class LoopTruth:
    """One object = one call of ``reinforce_policy``.  ``attempt()`` returns the attempt's class: "counted", "failed", "tenth" (the
    tenth failure in a row: the reference takes the step on the failed cost and re-initialises) or "void" (the device ignores attempts
    enqueued while the host has to act: ``pending``, ten failures, ``step >= n_steps``).

    ``sqrt``: "torch" -- ``ES2_diff_cost.sqrt()`` as the reference writes it (:518); on the CPU that is torch's vectorised square root,
    which is NOT correctly rounded (it differs from the IEEE result by one ulp for just under 1 % of the arguments).  "ieee" -- the
    correctly rounded square root (``math.sqrt``), which is what the device has: the form the kernels are compared with bit for bit.
    Everything else in the monitors (+ - x /) is correctly rounded on both sides."""

    def __init__(self, n_steps, warm_cost, alpha_diff_cost, min_step, min_diff_cost, num_min_diff_cost, lr, lr_min=0.001,
                 lr_reduction_ratio=0.5, sqrt="torch"):
        assert sqrt in ("torch", "ieee")
        self.sqrt = sqrt
        self.n_steps, self.alpha, self.n_win = int(n_steps), float(alpha_diff_cost), int(num_min_diff_cost)
        self.min_step0, self.min_diff0, self.lr0 = min_step, float(min_diff_cost), float(lr)
        self.lr_min, self.lr_ratio = float(lr_min), float(lr_reduction_ratio)
        # :413-417
        self.cost_list = torch.zeros(self.n_steps, dtype=torch.float64)
        self.std_list = torch.zeros(self.n_steps, dtype=torch.float64)
        self.min_step = min_step
        self.reinits = 0
        # :459-466
        self.es1 = torch.zeros(self.n_steps + 1, dtype=torch.float64)
        self.es2 = 0.0
        self.ratio = torch.zeros(self.n_steps + 1, dtype=torch.float64)
        self.cost_tm1 = f64(warm_cost)
        self.min_diff = float(min_diff_cost)
        self.lr = float(lr)
        # :471 and the counters the device keeps beside it
        self.step = 0
        self.attempts = 0        # :479 num_attempts
        self.pending = 0         # the condition of :543-550 held at the last counted attempt
        self.adam_t = 0          # steps of the current optimizer
        self.total_attempts = 0
        self.record = [0.0] * len(RECORD)
        self.fired_at = None     # the step whose window test fired last

    # ---- what the device must hold -----------------------------------------------------------------------------------------------
    def state(self):
        return dict(step=self.step, attempt=self.attempts, pending=self.pending, adam_t=self.adam_t, total_attempts=self.total_attempts,
                    es2=float(self.es2), cost_prev=float(self.cost_tm1))

    def frozen(self):
        return self.pending != 0 or self.attempts >= MAX_ATTEMPTS or self.step >= self.n_steps

    # ---- one attempt -------------------------------------------------------------------------------------------------------------
    def attempt(self, cost, std, failed_because=None):
        """``failed_because``: None, "nan", "sync" or "nonpos" (what flags / status say); a NaN cost always fails (:497)."""
        a = self.alpha
        cost, std = f64(cost), f64(std)
        nan = bool(torch.isnan(cost)) or failed_because == "nan"
        sync, nonpos = failed_because == "sync", failed_because == "nonpos"
        fail = nan or sync or nonpos
        k = self.step
        counted = void = 0.0
        rabs = 0.0
        self.total_attempts += 1
        if self.frozen():
            void, kind = 1.0, "void"
        elif fail:
            self.attempts += 1                                                                     # :498
            kind = "failed"
            if self.attempts >= MAX_ATTEMPTS:
                # :482 leaves the retry loop with flg_nan still set; :503-519 run on the failed cost.  Of what they write only
                # ES2_diff_cost and cost_tm1 survive :573-607 (the arrays are re-made at :584-600, those two are not)
                with torch.no_grad():
                    self.es2 = a * (self.es2 + (1 - a) * ((cost - self.cost_tm1 - self.es1[k]) ** 2))   # :513-515
                    self.cost_tm1 = cost.clone()                                                   # :504, :516
                kind = "tenth"
        else:
            self.cost_list[k] = cost.data.clone().detach()                                         # :504
            self.std_list[k] = std.data.clone().detach()                                           # :505
            with torch.no_grad():
                self.es1[k + 1] = a * self.es1[k] + (1 - a) * (cost - self.cost_tm1)               # :510-512
                self.es2 = a * (self.es2 + (1 - a) * ((cost - self.cost_tm1 - self.es1[k]) ** 2))  # :513-515
                self.cost_tm1 = self.cost_list[k].clone()                                          # :516
                root = self.es2.sqrt() if self.sqrt == "torch" else f64(math.sqrt(float(self.es2)))
                self.ratio[k + 1] = a * self.ratio[k] + (1 - a) * (self.es1[k + 1] / (root))           # :517-519
            rabs = float(torch.abs(self.ratio[k + 1]))                                             # :538
            if k > self.min_step:                                                                  # :543
                n = self.n_win
                if torch.sum(torch.abs(self.ratio[k + 1 - n: k + 1]) < self.min_diff) >= n:        # :544-550, the literal slice
                    self.pending = 1
                    self.fired_at = k
            self.step = k + 1                                                                      # :569
            self.attempts = 0                                                                      # :479 of the next step
            self.adam_t += 1                                                                       # :525
            counted, kind = 1.0, "counted"
        self.record = [counted, void, float(k), float(self.attempts), float(self.pending), float(cost), float(std), rabs,
                       1.0 if nan else 0.0, 1.0 if sync else 0.0, 1.0 if nonpos else 0.0, float(self.total_attempts)]
        return kind

    # ---- the host's half ---------------------------------------------------------------------------------------------------------
    def host_after_pending(self):
        """:551-566 at the step whose window test fired.  "lr": a new optimizer with the reduced rate (adam_t restarts, ``step`` runs
        on); "exit": the optimisation ends.  ES2_diff_cost and cost_tm1 are untouched."""
        assert self.pending == 1
        k = self.fired_at
        self.pending = 0
        if self.lr > self.lr_min:                                                                  # :551
            self.lr = max(self.lr * self.lr_ratio, self.lr_min)                                    # :554
            self.min_diff = max(self.min_diff / 2, 0.01)                                           # :556
            self.min_step = k + self.n_win                                                         # :557
            self.adam_t = 0                                                                        # :558 a new optimizer
            return "lr"
        return "exit"                                                                              # :565-566

    def tenth_failure_messages(self):
        """What :543-566 print on the step taken with the failed cost (everything they set is reset right after): None, "lr" or
        "exit".  The window is the one BEFORE this step's ratio would be written... the reference has written ratio[k + 1] (NaN for
        a NaN cost), which the slice ends before."""
        k, n = self.step, self.n_win
        if k > self.min_step and torch.sum(torch.abs(self.ratio[k + 1 - n: k + 1]) < self.min_diff) >= n:
            return "lr" if self.lr > self.lr_min else "exit"
        return None

    def host_after_ten_failures(self):
        """:573-607: counters, lists, ES1 / ratio arrays, lr, min_diff, min_step and the optimizer start again; ES2_diff_cost and
        cost_tm1 are NOT reset there."""
        assert self.attempts >= MAX_ATTEMPTS
        self.reinits += 1                                                                          # :574
        self.step = 0                                                                              # :579
        self.attempts = 0
        self.pending = 0
        self.min_step = self.min_step0                                                             # :581
        self.cost_list = torch.zeros(self.n_steps, dtype=torch.float64)                            # :584
        self.std_list = torch.zeros(self.n_steps, dtype=torch.float64)                             # :585
        self.es1 = torch.zeros(self.n_steps + 1, dtype=torch.float64)                              # :599
        self.ratio = torch.zeros(self.n_steps + 1, dtype=torch.float64)                            # :600
        self.min_diff = self.min_diff0                                                             # :601
        self.lr = self.lr0                                                                         # :603
        self.adam_t = 0                                                                            # :605
        # (the device's word is zeroed with the others: st[0:5] -- total_attempts counts from the re-initialisation on)
        self.total_attempts = 0


# ======================================================================================================================================
# Adam
# ======================================================================================================================================
class AdamTruth:
    """torch.optim.Adam(params, lr) -- the optimizer every launch script of the reference builds -- on CPU float64 tensors.
    ``params``: list of tensors (cloned); ``step(grads)``: one optimizer step, a None gradient skips its tensor as torch does."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8):
        self.params = [torch.as_tensor(p, dtype=torch.float64).detach().cpu().clone().requires_grad_(True) for p in params]
        self.lr, self.betas, self.eps = float(lr), betas, eps
        self.new_optimizer(lr)

    def new_optimizer(self, lr):
        """Where the host builds a new optimizer (MC_PILCO.py:558, :605): fresh moments and step count, same parameter tensors."""
        self.lr = float(lr)
        self.opt = torch.optim.Adam(self.params, lr=self.lr, betas=self.betas, eps=self.eps)

    def set_params(self, values):
        with torch.no_grad():
            for p, v in zip(self.params, values):
                p.copy_(torch.as_tensor(v, dtype=torch.float64).reshape(p.shape))

    def step(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else torch.as_tensor(g, dtype=torch.float64).detach().cpu().reshape(p.shape).clone()
        self.opt.step()

    def p(self):
        return [q.detach().clone() for q in self.params]

    def _moment(self, key):
        return [self.opt.state[q][key].detach().clone() if key in self.opt.state.get(q, {}) else torch.zeros_like(q) for q in self.params]

    def m(self):
        return self._moment("exp_avg")

    def v(self):
        return self._moment("exp_avg_sq")


def _f64_range(x):
    """A longdouble value with float64's RANGE (not its precision): beyond DBL_MAX -> inf, below half the smallest subnormal -> 0, so the
    extended evaluation overflows and underflows where the float64 one does."""
    x = np.asarray(x, dtype=np.longdouble).copy()
    ax = np.abs(x)
    big = ax > np.longdouble(np.finfo(np.float64).max)
    x[big] = np.sign(x[big]) * np.longdouble(np.inf)
    x[ax < np.longdouble(2.0) ** -1075] = 0
    return x


def adam_longdouble(p, m, v, g, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """One Adam step (torch.optim.Adam's formula, weight_decay 0, no amsgrad) of longdouble arrays p, m, v with the float64 gradient g
    as step number t.  Returns the new (p, m, v).  The constants are the float64 ones the float64 update uses."""
    L = np.longdouble
    g = np.asarray(g, dtype=np.float64).astype(L)
    b1, b2, e, lr = L(beta1), L(beta2), L(eps), L(lr)
    m = m + (L(1) - b1) * (g - m)
    v = _f64_range(v * b2 + _f64_range((L(1) - b2) * g * g))
    bc1, bc2 = L(1) - b1 ** L(t), L(1) - b2 ** L(t)
    with np.errstate(invalid="ignore", over="ignore"):
        denom = np.sqrt(v) / np.sqrt(bc2) + e
        p = p + (-(lr / bc1)) * (m / denom)
    return p, m, v


def tensor_distance(got, want):
    """max |got - want| over the entries finite on both sides, divided by the largest finite |want| of the tensor."""
    got, want = np.asarray(got, dtype=np.longdouble).reshape(-1), np.asarray(want, dtype=np.longdouble).reshape(-1)
    if want.size == 0:
        return 0.0
    ok = np.isfinite(got) & np.isfinite(want)
    if not ok.any():
        return 0.0
    scale = np.max(np.abs(want[np.isfinite(want)]))
    return float(np.max(np.abs(got[ok] - want[ok])) / scale) if scale > 0 else float(np.max(np.abs(got[ok] - want[ok])))


def adam_distance(params0, grad_seq, lr, restart_at=()):
    """The float64 rounding level of the update over a gradient sequence: worst ``tensor_distance`` of AdamTruth's p / m / v from the
    longdouble trajectory, over all tensors and steps.  ``grad_seq[s][i]``: gradient of tensor i at step s (None skips);
    ``restart_at``: steps before which a new optimizer is built (moments and t restart)."""
    L = np.longdouble
    at = AdamTruth(params0, lr)
    P = [np.asarray(q, dtype=np.float64).astype(L) for q in params0]
    M, V = [np.zeros_like(q) for q in P], [np.zeros_like(q) for q in P]
    t = [0] * len(P)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for s, grads in enumerate(grad_seq):
        if s in restart_at:
            at.new_optimizer(lr)
            M, V, t = [np.zeros_like(q) for q in P], [np.zeros_like(q) for q in P], [0] * len(P)
        at.step(grads)
        for i, g in enumerate(grads):
            if g is None or P[i].size == 0:
                continue
            t[i] += 1
            P[i], M[i], V[i] = adam_longdouble(P[i], M[i], V[i], np.asarray(g, dtype=np.float64).reshape(P[i].shape), t[i], lr)
        for key, ext, got in (("p", P, at.p()), ("m", M, at.m()), ("v", V, at.v())):
            for i in range(len(P)):
                worst[key] = max(worst[key], tensor_distance(got[i].numpy(), ext[i]))
    return worst


def adam_bound(measured):
    return max(ADAM_BOUND_FACTOR * measured, ADAM_BOUND_FLOOR)


# ======================================================================================================================================
# the scripted cost and the scripts
# ======================================================================================================================================
class ScriptedCost(torch.nn.Module):
    """cost_function(states, inputs, trial_index) -> (cost, std) read from a script: call 0 is the warm-up rollout's (:448), call 1 + i
    evaluation i of the loop:  cost = s_i + (<w_i, theta> - <w_i, theta>.detach()),  i.e. the value is exactly s_i (NaN where the
    script says so) and the gradient in the policy parameters theta exactly w_i.  ``index``: callable -> number of the current call
    (None: count the calls); ``on_eval(i)``: hook."""

    def __init__(self, params, warm, s, std, w, index=None, device="cpu"):
        super().__init__()
        self._params = list(params)
        dev = torch.device(device)
        self.warm = torch.as_tensor(np.asarray(warm, dtype=np.float64)).reshape(()).to(dev)
        self.s = torch.as_tensor(np.asarray(s, dtype=np.float64)).to(dev)
        self.sd = torch.as_tensor(np.asarray(std, dtype=np.float64)).to(dev)
        self.w = torch.as_tensor(np.asarray(w, dtype=np.float64)).to(dev)
        self.zero = torch.zeros((), dtype=torch.float64, device=dev)
        self.index, self.calls = index, 0
        self.evals = []

    def forward(self, states_sequence=None, inputs_sequence=None, trial_index=None):
        c = self.calls if self.index is None else int(self.index())
        self.calls += 1
        if c == 0:
            return self.warm.clone(), self.zero.clone()
        i = c - 1
        self.evals.append(i)
        theta = torch.cat([q.reshape(-1) for q in self._params])
        d = torch.dot(self.w[i], theta)
        return self.s[i] + (d - d.detach()), self.sd[i].clone()


POLICY = dict(state_dim=2, input_dim=1, num_basis=3)  # Sum_of_gaussians: log_lengthscales [1, 2], centers [3, 2], weight [1, 3] -> 11 values
N_THETA = 11
REINIT = dict(lenghtscales_par=np.array([1.5, 0.75]), centers_par=np.zeros(2), weight_par=0.0)  # no random number survives: centres, weights -> 0


def policy_init():
    rs = np.random.RandomState(77)
    return dict(lengthscales_init=np.array([0.8, 1.3]), centers_init=rs.uniform(-1, 1, (3, 2)), weight_init=rs.uniform(-1, 1, (1, 3)))


def reinit_values():
    return [np.log(REINIT["lenghtscales_par"]).reshape(1, 2), np.zeros((3, 2)), np.zeros((1, 3))]


def _script(seed, n, nan_at=(), flat=False, warm=None):
    """Costs that fall towards a plateau (the monitors' ratio grows away from 0), or ``flat``: noise about a constant (the ratio stays
    small and changes sign: the shape that brings |ratio| under halving thresholds).  Gradients: standard normal with exact zeros."""
    rs = np.random.RandomState(seed)
    if flat:
        s = 3.0 + 0.3 * np.random.RandomState(seed).standard_normal(n)
    else:
        s = 5.0 * 0.93 ** np.arange(n) + 0.4 * rs.standard_normal(n)
    s = np.array(s, dtype=np.float64)
    s[list(nan_at)] = np.nan
    w = rs.standard_normal((n, N_THETA))
    w[rs.uniform(size=w.shape) < 0.1] = 0.0  # exact zeros among the gradients
    return dict(warm=np.float64(5.3 if warm is None else warm), s=s, std=np.abs(rs.standard_normal(n)) + 0.1, w=w)


def script_cases():
    """name -> (script, keyword arguments of reinforce_policy).  Every script is longer than the reference's run consumes: a pipelined
    loop evaluates a few attempts past a host decision before it rewinds."""
    base = dict(lr_list=[0.01], lr_reduction_ratio=0.5, lr_min=0.004, alpha_diff_cost=0.9)
    cases = {}
    # (a) thresholded windows.  min_diff_cost 0.03 -> 0.015 -> 0.01 lies between the |ratio| values of this script: the windows tested
    #     hold 0, 1, 2 (a miss by exactly one entry, six times) or 3 entries; lr halves at steps 4 and 16, the exit comes at step 23; no
    #     |ratio| of a tested window is closer than 5 % to its threshold (the maker and the CPU test assert >= 1e-6)
    cases["a_thresholds"] = (_script(100, 40, flat=True, warm=3.1), dict(base, opt_steps_list=[30], num_min_diff_cost=3, min_step=2, min_diff_cost=0.03))
    # (b) one to nine NaN retries, in different steps
    nan_b, i = [], 0
    for step, fails in enumerate([0, 1, 0, 9, 2, 0, 5, 0]):
        nan_b += list(range(i, i + fails))
        i += fails + 1
    cases["b_retries"] = (_script(12, i + 6, nan_b), dict(base, opt_steps_list=[8], num_min_diff_cost=3, min_step=2, min_diff_cost=0.02))
    # (c) ten NaNs in a row at step 2, then a full run with NaN monitors
    cases["c_reinit"] = (_script(13, 2 + 10 + 6 + 6, range(2, 12)), dict(base, opt_steps_list=[6], num_min_diff_cost=2, min_step=0, min_diff_cost=1e9))
    # (d) window edges
    cases["d_n0"] = (_script(14, 12), dict(base, opt_steps_list=[6], num_min_diff_cost=0, min_step=1, min_diff_cost=0.05))
    cases["d_n_gt_k"] = (_script(15, 12), dict(base, opt_steps_list=[6], num_min_diff_cost=4, min_step=0, min_diff_cost=1e9))
    cases["d_n_gt_steps"] = (_script(16, 12), dict(base, opt_steps_list=[4], num_min_diff_cost=7, min_step=-1, min_diff_cost=1e9))
    cases["d_min_step_neg"] = (_script(17, 12), dict(base, opt_steps_list=[6], num_min_diff_cost=1, min_step=-1, min_diff_cost=0.05))
    # (e) s_0 equal to the warm-up cost: 0 / sqrt(0), a NaN ratio from step 0 on
    e = _script(18, 12)
    e["s"][0] = e["warm"]
    cases["e_zero_diff"] = (e, dict(base, opt_steps_list=[6], num_min_diff_cost=2, min_step=0, min_diff_cost=1e9))
    return cases


def load_case(fx, name):
    """(script, reinforce_policy's keyword arguments) of a script stored in tests/golden/opt_loop_script.npz."""
    g = lambda k: fx[name + "_" + k]
    script = dict(warm=np.float64(g("warm")), s=g("s"), std=g("std"), w=g("w"))
    kw = dict(opt_steps_list=[int(g("n_steps"))], lr_list=[float(g("lr"))], lr_min=float(g("lr_min")), lr_reduction_ratio=float(g("lr_reduction_ratio")),
              alpha_diff_cost=float(g("alpha_diff_cost")), num_min_diff_cost=int(g("num_min_diff_cost")), min_step=float(g("min_step")),
              min_diff_cost=float(g("min_diff_cost")))
    return script, kw


def params0():
    pi = policy_init()
    return [np.log(pi["lengthscales_init"]).reshape(1, 2), pi["centers_init"], pi["weight_init"]]


def drive_script(script, kw, params0, on_attempt=None, on_host=None, sqrt="torch"):
    """LoopTruth + AdamTruth through a script, as the reference's loops consume it (MC_PILCO.py:475-607).  Returns a dict of what the
    reference's run shows: cost / std lists, |ratio| printed per counted step, the steps of the lr reductions and of the exit, the
    parameters after every counted step, the final parameters, the number of evaluations consumed.
    ``on_attempt(i, kind, lt, at)`` after every attempt, ``on_host(what, lt, at)`` after every host action."""
    n_steps = kw["opt_steps_list"][0]
    lt = LoopTruth(n_steps, script["warm"], kw["alpha_diff_cost"], kw["min_step"], kw["min_diff_cost"], kw["num_min_diff_cost"], kw["lr_list"][0],
                   lr_min=kw["lr_min"], lr_reduction_ratio=kw["lr_reduction_ratio"], sqrt=sqrt)
    at = AdamTruth(params0, lt.lr)
    out = dict(printed=[], lr_steps=[], exit_steps=[], params_steps=[], reinit_at=[], thetas=[], kinds=[])
    i, done = 0, 0
    while True:
        out["thetas"].append(np.concatenate([q.numpy().reshape(-1) for q in at.p()]))  # the parameters evaluation i sees
        kind = lt.attempt(script["s"][i], script["std"][i], None)
        w = torch.as_tensor(script["w"][i])
        if kind in ("counted", "tenth"):
            grads, o = [], 0
            for q in at.params:
                grads.append(w[o:o + q.numel()].reshape(q.shape))
                o += q.numel()
            at.step(grads)  # (:522-525; the tenth failure's step is undone by the re-initialisation below)
        out["kinds"].append(kind)
        if on_attempt is not None:
            on_attempt(i, kind, lt, at)
        i += 1
        if kind == "counted":
            k = int(lt.record[2])
            done = k + 1
            out["printed"].append((k, lt.record[7]))
            out["params_steps"].append(np.concatenate([q.numpy().reshape(-1) for q in at.p()]))
            if lt.pending:
                what = lt.host_after_pending()
                (out["lr_steps"] if what == "lr" else out["exit_steps"]).append(k)
                if what == "lr":
                    at.new_optimizer(lt.lr)
                if on_host is not None:
                    on_host(what, lt, at)
                if what == "exit":
                    break
            if done >= n_steps:
                break
        elif kind == "tenth":
            out["printed"].append((lt.step, float("nan")))  # (:528-540 print the failed step too)
            what = lt.tenth_failure_messages()
            if what is not None:
                (out["lr_steps"] if what == "lr" else out["exit_steps"]).append(lt.step)
            out["reinit_at"].append(i)
            lt.host_after_ten_failures()
            at.set_params(reinit_values())
            at.new_optimizer(lt.lr)
            done = 0
            if on_host is not None:
                on_host("reinit", lt, at)
    out.update(cost_list=lt.cost_list[:done].numpy().copy(), std_list=lt.std_list[:done].numpy().copy(), consumed=i,
               final=np.concatenate([q.numpy().reshape(-1) for q in at.p()]), lt=lt, at=at)
    return out


def script_grad_seq(script, kw):
    """(start parameters, grad_seq, restart_at) of the counted steps of a script, for ``adam_distance``: the steps since the last
    re-initialisation (from the start when there is none), and the steps before which the host built a new optimizer."""
    st = dict(start=params0(), seq=[], restarts=[])

    def on_attempt(i, kind, lt, at):
        if kind == "counted":
            w, o, row = script["w"][i], 0, []
            for q in at.params:
                row.append(w[o:o + q.numel()].reshape(q.shape))
                o += q.numel()
            st["seq"].append(row)

    def on_host(what, lt, at):
        if what == "lr":
            st["restarts"].append(len(st["seq"]))
        if what == "reinit":
            st.update(start=reinit_values(), seq=[], restarts=[])

    drive_script(script, kw, params0(), on_attempt=on_attempt, on_host=on_host)
    return st["start"], st["seq"], st["restarts"]


# ======================================================================================================================================
# Adam's layout cases (shared by the CPU measurement and the GPU test)
# ======================================================================================================================================
LAYOUT_SIZES = [1, 255, 256, 17, 257, 0, 3, 1025]  # sizes that straddle the 256-thread blocks; [3] gets a NULL gradient, [5] has no element
LAYOUT_NULL_GRAD = 3
BIG, HUGE, TINY = 1e150, 1e160, 1e-170             # g^2 overflows but (1 - beta2) g g in torch's order does not; that overflows too; g^2 underflows (denom = eps)


def adam_layout_case(sizes=None, null_grad=(LAYOUT_NULL_GRAD,), steps=50, seed=5):
    """(initial parameters, grad_seq): grad_seq[s][i] = gradient of tensor i at step s (None: NULL pointer).  Standard normal entries on
    a scale that drifts over the steps, one in ten exactly zero, negatives, 1e150 (once), -1e160 (from a step on) and +-1e-170 (always)."""
    sizes = LAYOUT_SIZES if sizes is None else sizes
    rs = np.random.RandomState(seed)
    p0 = [rs.standard_normal(n) for n in sizes]
    seq = []
    for s in range(steps):
        row = []
        for i, n in enumerate(sizes):
            if i in null_grad:
                row.append(None)
                continue
            g = rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 1)
            g[rs.uniform(size=n) < 0.1] = 0.0
            if n >= 257:
                g[n - 1] = TINY if n == 257 else -TINY
                if s == 7:
                    g[0] = BIG                      # once: exp_avg_sq ~ 1e297, finite only in torch's order ((1 - beta2) g) g
                if s >= 20:
                    g[n // 2] = -HUGE               # exp_avg_sq is inf from then on, the parameter stops
            if n == 3:
                g[1] = 0.0                          # never a gradient: m = v = 0, denom = eps
            row.append(g)
        seq.append(row)
    return p0, seq
