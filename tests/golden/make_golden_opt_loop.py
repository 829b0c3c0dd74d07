"""Golden vectors of the optimizer loop on a SCRIPTED cost, generated like make_golden_r2.py by IMPORTING THE REFERENCE (a checkout of
the original MC-PILCO code, named by the first argument) and running its own MC_PILCO.reinforce_policy (policy_learning/MC_PILCO.py:375-613).
Only arrays are stored.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_opt_loop.py <directory of the reference>

On the reference's MC_PILCO object (a 3-basis Sum_of_gaussians policy, 11 parameters) ``apply_policy`` and ``cost_function`` are replaced
by stubs (tests/opt_truth.py: ScriptedCost): evaluation i of the cost has the value s_i exactly (NaN where the script says so), the
gradient w_i exactly and the std scripted, so reinforce_policy is a pure function of the script.  It runs with num_step_print = 1 on
the scripts of opt_truth.script_cases():

  a_thresholds     min_diff_cost between the |ratio| values: windows that hold and windows that miss by exactly one entry, two lr
                   halvings, then the exit at lr_min
  b_retries        1, 9, 2 and 5 NaN retries in different steps
  c_reinit         ten NaNs in a row (re-initialisation), NaN monitors afterwards
  d_*              the window's edges: n = 0, n > k + 1, n > n_steps + 1, min_step = -1 with n = 1
  e_zero_diff      s_0 equal to the warm-up cost: 0 / sqrt(0), a NaN ratio from step 0 on

opt_loop_script.npz, per script <name>_...: the script (warm, s, std, w) and the loop's arguments; cost_list / std_list; the steps at
which "REDUCING THE LEARNING RATE" and "EXIT" were printed; the printed step numbers and diff_cost_ratio values (numpy prints a float64 so
that it round-trips); the parameters at every evaluation of the cost (so: after every counted step, and after the re-initialisation) and the
final ones; how many evaluations the run consumed, its retry and re-initialisation messages.
"""
import contextlib
import io
import os
import re
import sys

import numpy as np
import torch

if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "policy_learning")):
    sys.exit("usage: make_golden_opt_loop.py <directory of the reference (the one that holds policy_learning/)>")
REF = os.path.abspath(sys.argv[1])
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(1, os.path.dirname(HERE))  # tests/: opt_truth
os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True

with contextlib.redirect_stdout(io.StringIO()):
    import policy_learning.MC_PILCO as RMC
    import policy_learning.Policy as RP

import opt_truth as ot  # noqa: E402

dtype = torch.float64
dev = torch.device("cpu")
torch.set_num_threads(1)
MARGIN = 1e-6


def run(script, kw):
    holder = {}
    with contextlib.redirect_stdout(io.StringIO()):
        obj = RMC.MC_PILCO(T_sampling=0.05, state_dim=2, input_dim=1, f_sim=lambda y, t, u: None, f_model_learning=lambda **k: None,
                           model_learning_par={}, f_rand_exploration_policy=RP.Random_exploration,
                           rand_exploration_policy_par=dict(state_dim=2, input_dim=1, u_max=1.0, dtype=dtype, device=dev),
                           f_control_policy=RP.Sum_of_gaussians, control_policy_par=dict(dtype=dtype, device=dev, **ot.POLICY, **ot.policy_init()),
                           f_cost_function=lambda: holder.setdefault("cost", torch.nn.Identity()), cost_function_par={}, log_path=None,
                           dtype=dtype, device=dev)
    pol = obj.control_policy
    params = list(pol.parameters())
    assert [tuple(q.shape) for q in params] == [(1, 2), (3, 2), (1, 3)]
    cost = ot.ScriptedCost(params, script["warm"], script["s"], script["std"], script["w"])
    thetas = []
    inner = cost.forward

    def spying(*a, **k):  # the parameters every evaluation sees
        if cost.calls > 0:
            thetas.append(np.concatenate([q.detach().numpy().reshape(-1) for q in params]))
        return inner(*a, **k)

    cost.forward = spying
    obj.cost_function = cost
    obj.apply_policy = lambda **k: (torch.zeros(1, 1, 2, dtype=dtype), torch.zeros(1, 1, 1, dtype=dtype))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cost_list, std_list, _, _ = obj.reinforce_policy(
            T_control=0.5, num_particles=4, trial_index=0, particles_initial_state_mean=None, particles_initial_state_var=None,
            flg_particles_init_uniform=False, particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
            f_optimizer="lambda p, lr : torch.optim.Adam(p, lr)", num_step_print=1, policy_reinit_dict=ot.REINIT, p_dropout_list=None, **kw)
    return cost_list, std_list, buf.getvalue(), np.array(thetas), np.concatenate([q.detach().numpy().reshape(-1) for q in params]), cost.calls - 1


def parse(txt):
    """(printed steps, printed |ratio|, min_diff and min_step printed with them, steps of the lr reductions, steps of the exit)."""
    steps, ratios, mdiff, mstep, lr_steps, exit_steps = [], [], [], [], [], []
    for line in txt.splitlines():
        m = re.match(r"Optimization step:\s+(\d+)$", line)
        if m:
            steps.append(int(m.group(1)))
        if line.startswith("diff_cost_ratio:"):
            ratios.append(float(line.split(":", 1)[1]))
        if line.startswith("current_min_diff_cost;"):
            mdiff.append(float(line.split(";", 1)[1]))
        if line.startswith("current_min_step:"):
            mstep.append(float(line.split(":", 1)[1]))
        if line.startswith("REDUCING THE LEARNING RATE"):
            lr_steps.append(steps[-1])
        if line.startswith("EXIT FROM OPTIMIZATION"):
            exit_steps.append(steps[-1])
    assert len(steps) == len(ratios) == len(mdiff) == len(mstep)
    assert [int(s) for s in re.findall(r"^Optimization_step: (\d+)$", txt, flags=re.M)] == lr_steps
    return steps, ratios, mdiff, mstep, lr_steps, exit_steps


def window_margin(steps, ratios, mdiff, mstep, n):
    """Smallest relative distance of a |ratio| in a tested window (:543-547) from the bound it is compared with, and the number of
    entries below the bound per tested window."""
    worst, hits = np.inf, []
    hist = [0.0]  # diff_cost_ratio[0]
    for k, r, md, ms in zip(steps, ratios, mdiff, mstep):
        if k == 0:
            hist = [0.0]
        hist.append(r)
        if k > ms and n > 0 and k + 1 - n >= 0:
            win = np.array(hist[k + 1 - n:k + 1])
            win = win[np.isfinite(win)]
            if win.size:
                worst = min(worst, float(np.min(np.abs(win - md) / md)))
            hits.append(int(np.sum(win < md)))
    return worst, hits


out, hits_all = {}, {}
for name, (script, kw) in ot.script_cases().items():
    cost_list, std_list, txt, thetas, final, consumed = run(script, kw)
    steps, ratios, mdiff, mstep, lr_steps, exit_steps = parse(txt)
    n = kw["num_min_diff_cost"]
    margin, hits = window_margin(steps, ratios, mdiff, mstep, n)
    assert margin >= MARGIN, (name, margin)  # no decision hinges on a last bit
    hits_all[name] = hits
    assert consumed + 4 <= len(script["s"]), name
    pre = name + "_"
    out.update({pre + k: script[k] for k in ("warm", "s", "std", "w")})
    out.update({pre + "n_steps": kw["opt_steps_list"][0], pre + "lr": kw["lr_list"][0], pre + "lr_min": kw["lr_min"],
                pre + "lr_reduction_ratio": kw["lr_reduction_ratio"], pre + "alpha_diff_cost": kw["alpha_diff_cost"],
                pre + "num_min_diff_cost": n, pre + "min_step": kw["min_step"], pre + "min_diff_cost": kw["min_diff_cost"],
                pre + "cost_list": cost_list, pre + "std_list": std_list, pre + "printed_steps": np.array(steps, dtype=np.int64),
                pre + "printed_ratio": np.array(ratios), pre + "lr_steps": np.array(lr_steps, dtype=np.int64),
                pre + "exit_steps": np.array(exit_steps, dtype=np.int64), pre + "thetas": thetas, pre + "final": final,
                pre + "consumed": consumed, pre + "n_retry": txt.count("Cost is NaN: try sampling again"),
                pre + "n_reinit": txt.count("re-initialize control policy")})
    print("%-16s steps done %2d  evaluations %2d  lr at %s  exit at %s  retries %2d  reinit %d  window hits %s  margin %.3g"
          % (name, len(cost_list), consumed, lr_steps, exit_steps, out[pre + "n_retry"], out[pre + "n_reinit"], hits, margin))

a = "a_thresholds_"
assert hits_all["a_thresholds"].count(2) >= 2 and hits_all["a_thresholds"].count(3) == 3 and min(hits_all["a_thresholds"]) == 0
assert len(out[a + "lr_steps"]) == 2 and len(out[a + "exit_steps"]) == 1
assert out["b_retries_n_retry"] == 17 and out["c_reinit_n_retry"] == 10 and out["c_reinit_n_reinit"] == 1
assert np.all(np.isnan(out["e_zero_diff_printed_ratio"])) and np.isnan(out["c_reinit_printed_ratio"][-1])
out["names"] = np.array(sorted(ot.script_cases()))
np.savez_compressed(os.path.join(HERE, "opt_loop_script.npz"), **{k: np.asarray(v) for k, v in out.items()})
print("wrote opt_loop_script.npz", os.path.getsize(os.path.join(HERE, "opt_loop_script.npz")), "bytes")
