#!/usr/bin/env python3
"""ms per optimizer step (rollout + expected cost + adjoint) of a cart-pole full-state (delta-state) model, the fused HIP rollout against the
step-wise path (per step G single-step posterior launches + torch glue, backward through the autograd engine).  4 GPs, N = 300, SE and
SE + MPK(2), M = 400, T = 150, the project's own MC_PILCO with in-kernel noise.

    python tools/time_delta_rollout.py [--out DIR] [--reps 10] [--stepwise-reps 3]

Prints one line per (kernel, path) and writes DIR/time_delta_rollout.json."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcp_boot  # noqa: E402,F401

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mc_pilco_amd import synthetic as sy  # noqa: E402
from mc_pilco_amd.model_learning import Model_learning as ML  # noqa: E402
from mc_pilco_amd.policy_learning import MC_PILCO, Cost_function, Policy  # noqa: E402

DT = torch.float64


def build(kind, dev, N=300, B=200):
    c = sy.CARTPOLE
    cp = sy.cartpole_rollouts()
    x = np.concatenate([r[0] for r in cp], 0)[: N + 1]
    u = np.concatenate([r[1] for r in cp], 0)[: N + 1]
    rbf = dict(active_dims=np.arange(6), lengthscales_init=c["lengthscales"], flg_train_lengthscales=True, lambda_init=np.ones(1),
               flg_train_lambda=False, sigma_n_init=c["sigma_n"] * np.ones(1), sigma_n_num=None, flg_train_sigma_n=True, dtype=DT, device=dev)
    rs = np.random.RandomState(23)
    with contextlib.redirect_stdout(io.StringIO()):
        if kind == "se":
            ml = ML.Model_learning_RBF_angle_state(num_gp=4, init_dict_list=[rbf] * 4, angle_indeces=c["angle"], not_angle_indeces=c["not_angle"],
                                                   dtype=DT, device=dev)
        else:
            mpk = [dict(active_dims=np.arange(6), poly_deg=2, Sigma_pos_par_init_list=[0.02 * (0.5 + rs.rand(7)), 0.02 * (0.5 + rs.rand(12))],
                        flg_train_Sigma_pos_par_list=[True, True], dtype=DT, device=dev) for _ in range(4)]
            ml = ML.Model_learning_RBF_MPK_angle_state(num_gp=4, init_dict_list=[[rbf, mpk[g]] for g in range(4)], angle_indeces=c["angle"],
                                                       not_angle_indeces=c["not_angle"], dtype=DT, device=dev)
        ml.add_data(x, u)
        with torch.no_grad():
            for g in range(4):
                ml.pretrain_gp(g)
        ml.set_eval_mode()
        pi = sy.cartpole_policy_init(B=B, seed=4)
        ppar = dict(state_dim=4, input_dim=1, num_basis=B, angle_indices=np.array([2]), non_angle_indices=np.array([0, 1, 3]),
                    lengthscales_init=pi["lengthscales"], centers_init=pi["centers"], weight_init=pi["weight"], flg_squash=True, u_max=c["u_max"],
                    flg_drop=True, dtype=DT, device=dev)
        obj = MC_PILCO.MC_PILCO(T_sampling=c["Ts"], state_dim=4, input_dim=1, f_sim=lambda y, t, u: None, f_model_learning=lambda **k: ml,
                                model_learning_par={}, f_rand_exploration_policy=Policy.Random_exploration,
                                rand_exploration_policy_par=dict(state_dim=4, input_dim=1, u_max=1.0, dtype=DT),
                                f_control_policy=Policy.Sum_of_gaussians_with_angles, control_policy_par=ppar,
                                f_cost_function=Cost_function.Cart_pole_cost,
                                cost_function_par=dict(target_state=torch.tensor(c["cost_target"], dtype=DT, device=dev),
                                                       lengthscales=torch.tensor(c["cost_ls"], dtype=DT, device=dev), angle_index=2, pos_index=0),
                                log_path=None, dtype=DT, device=dev)
    return obj


def step(obj, M, T, dev):
    for q in obj.control_policy.parameters():
        q.grad = None
    st, inp = obj.apply_policy(particles_initial_state_mean=torch.zeros(4, dtype=DT, device=dev),
                               particles_initial_state_var=torch.full((4,), 1e-4, dtype=DT, device=dev), flg_particles_init_uniform=False,
                               particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False, num_particles=M,
                               T_control=T, p_dropout=0.25)
    cost, _ = obj.cost_function(st, inp, 0)
    cost.backward()
    return obj.last_status is not None


def timed(obj, M, T, dev, reps, warmup=2):
    for _ in range(warmup):
        fused = step(obj, M, T, dev)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        step(obj, M, T, dev)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return fused, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="time_delta_out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stepwise-reps", type=int, default=3)
    ap.add_argument("--M", type=int, default=400)
    ap.add_argument("--T", type=int, default=150)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = []
    for kind in ("se", "se_mpk2"):
        obj = build(kind, dev)
        ml = obj.model_learning
        for path in ("fused", "stepwise"):
            if path == "stepwise":
                ml.has_fused_layout = lambda: False  # (the instance attribute shadows the method: MC_PILCO takes the step-wise path)
            fused, ts = timed(obj, a.M, a.T, dev, a.reps if path == "fused" else a.stepwise_reps)
            assert fused == (path == "fused")
            row = dict(kernel=kind, path=path, G=4, N=300, M=a.M, T=a.T, ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), reps=len(ts))
            rows.append(row)
            print("%-8s %-9s ms/step median %8.3f  min %8.3f  (%d reps)" % (kind, path, row["ms_median"], row["ms_min"], row["reps"]))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_delta_rollout.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
