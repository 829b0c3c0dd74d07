"""Golden vectors of the closed loop under the reference's TRAINABLE PD controller (policy_learning/Policy.py:406-449) ON A SIMULATED
MEASUREMENT, by IMPORTING THE REFERENCE (a read-only checkout of merlresearch/MC-PILCO, named by the environment variable
MCPILCO_REFERENCE) and running its own MC_PILCO4PMS.apply_policy (policy_learning/MC_PILCO.py:808-906) -- the recipe of make_golden_pd.py
with the measurement model and its noise added, replayed as make_golden.py's rollout_pms fixture replays it.

    MCPILCO_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_pd_pms.py

Writes rollout_pd_pms.npz with two fixtures at the two-joint arm layout of rollout_pd.npz (S = 4, U = 2, D = 8, N = 40 training points):
  speed_*  Speed_Model_learning_RBF_angle_state (2 GPs, Ts = 0.05)
  delta_*  Model_learning_RBF_angle_state (4 GPs; the measured velocities use the class's T_sampling = 0.05)
each with the states and inputs of MC_PILCO4PMS.apply_policy under PD_controller(flg_trainable=True), pos_indeces = [0, 1], vel_indeces =
[2, 3], M = 6, T = 6, and the gradients of L = sum(w * states) + sum(w_u * inputs) in the two gain parameters and in the mean and the variance
of the initial distribution (x0 = mean + sqrt(var) eps0: sum_m dL/dx0[m] and sum_m dL/dx0[m] eps0[m] / (2 sqrt(var))) after L.backward().
Only arrays are stored.  The noise the reference drew is recovered by re-seeding torch and replaying its draw order -- x0, then per step
eps_t and the position noise; the script asserts that the replay reproduces the reference's x0 bit-exactly, and tests/test_pd_meas_cpu.py
reproduces the whole run from the replayed draws.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MCPILCO_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "model_learning")):
    sys.exit("set MCPILCO_REFERENCE to a checkout of the reference (merlresearch/MC-PILCO)")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True

with contextlib.redirect_stdout(io.StringIO()):
    import gpr_lib.Likelihood.Gaussian_likelihood  # noqa: F401
    import gpr_lib.Utils.Parameters_covariance_functions  # noqa: F401
    import model_learning.Model_learning as RML
    import policy_learning.Cost_function as RC
    import policy_learning.MC_PILCO as RMC
    import policy_learning.Policy as RP
from scipy import signal

dtype = torch.float64
dev = torch.device("cpu")
torch.set_num_threads(1)
quiet = contextlib.redirect_stdout(io.StringIO())
S, U, D, NTR = 4, 2, 8, 40
ANGLE, NOT_ANGLE, VEL, NOT_VEL, TS = [0, 1], [2, 3], [2, 3], [0, 1], 0.05
LS = np.array([2.0, 2.5, 1.5, 1.8, 1.6, 1.9, 3.0, 3.5])
SIGMA_N = 0.1
POS, VELM, FC = [0, 1], [2, 3], 0.3
STD_MEAS = np.array([0.004, 0.006, 0.01, 0.01])


def T(a):
    return torch.tensor(np.asarray(a), dtype=dtype)


def N(t):
    return t.detach().cpu().numpy().copy()


def rbf_dict():
    return dict(active_dims=np.arange(D), lengthscales_init=LS, flg_train_lengthscales=True, lambda_init=np.ones(1), flg_train_lambda=False,
                sigma_n_init=SIGMA_N * np.ones(1), sigma_n_num=None, flg_train_sigma_n=True, dtype=dtype, device=dev)


def build_model(kind):
    # the recorded trajectory of make_golden_pd.py (two damped pendulum joints, weakly coupled, driven by sums of sinusoids)
    rs = np.random.RandomState(11)
    tt = TS * np.arange(NTR + 1).reshape(-1, 1)
    u = (0.8 * np.sin(2.0 * np.pi * (0.3 + 0.9 * rs.rand(1, U)) * tt + 6.28 * rs.rand(1, U))
         + 0.5 * np.sin(2.0 * np.pi * (1.5 + rs.rand(1, U)) * tt + 6.28 * rs.rand(1, U)))
    x = np.zeros((NTR + 1, S))
    x[0] = [0.3, -0.2, 0.0, 0.0]
    for i in range(NTR):
        q, qd = x[i, :2], x[i, 2:]
        qdd = -4.0 * np.sin(q) - 0.4 * qd + 3.0 * u[i] + 0.5 * (q[::-1] - q)
        x[i + 1, 2:] = qd + TS * qdd
        x[i + 1, :2] = q + TS * qd + 0.5 * TS * TS * qdd
    x = x + 1e-3 * rs.randn(NTR + 1, S)
    with quiet:
        if kind == "speed":
            ml = RML.Speed_Model_learning_RBF_angle_state(num_gp=2, init_dict_list=[rbf_dict()] * 2, T_sampling=TS, angle_indeces=ANGLE,
                                                          not_angle_indeces=NOT_ANGLE, vel_indeces=VEL, not_vel_indeces=NOT_VEL, dtype=dtype, device=dev)
        else:
            ml = RML.Model_learning_RBF_angle_state(num_gp=4, init_dict_list=[rbf_dict()] * 4, angle_indeces=ANGLE, not_angle_indeces=NOT_ANGLE,
                                                    dtype=dtype, device=dev)
        ml.add_data(x, u)
        with torch.no_grad():
            for g in range(ml.num_gp):
                ml.pretrain_gp(g)
        ml.set_eval_mode()
    return ml, x, u


def replay_noise(seed, M, G, Tn):
    torch.manual_seed(seed)
    eps0 = torch.empty(M, S, dtype=dtype).normal_()
    eps, pn = [], []
    for _ in range(1, Tn):
        eps.append(torch.empty(M, G, dtype=dtype).normal_())
        pn.append(torch.randn(M, len(POS), dtype=dtype))
    return eps0, torch.stack(eps), torch.stack(pn)


def rollout_fixture(kind, M, Tn, seed):
    ml, xtr, utr = build_model(kind)
    G = ml.num_gp
    rs = np.random.RandomState(seed)
    kp, kd = 0.5 + rs.rand(U), 0.2 + 0.6 * rs.rand(U)
    tt = np.arange(Tn + 2).reshape(-1, 1)
    target = 0.3 * np.sin(0.35 * tt + np.array([0.0, 1.0, 2.0, 3.0]).reshape(1, -1))
    u_max = 1.5
    ppar = dict(state_dim=S, input_dim=U, sqrt_Kp_gains=kp, sqrt_Kd_gains=kd, target_traj=T(target), flg_squash=True, u_max=u_max,
                flg_trainable=True, dtype=dtype, device=dev)
    with quiet:
        obj = RMC.MC_PILCO4PMS(T_sampling=TS, state_dim=S, input_dim=U, f_sim=lambda y, t, u: None, f_model_learning=lambda **kw: ml,
                               model_learning_par={}, f_rand_exploration_policy=RP.Random_exploration,
                               rand_exploration_policy_par=dict(state_dim=S, input_dim=U, u_max=1.0, dtype=dtype, device=dev),
                               f_control_policy=RP.PD_controller, control_policy_par=ppar, f_cost_function=RC.Expected_distance,
                               cost_function_par=dict(target_state=T(np.zeros(S)), lengthscales=T(np.ones(S)), active_dims=np.arange(S)),
                               pos_indeces=POS, vel_indeces=VELM, std_meas_noise=STD_MEAS, log_path=None, filtering_dict={"fc": FC},
                               dtype=dtype, device=dev)
    pol = obj.control_policy
    x0m, x0v = T([0.1, -0.1, 0.0, 0.05]).requires_grad_(True), T([1e-2, 1e-2, 2e-2, 2e-2]).requires_grad_(True)
    torch.manual_seed(seed)
    st, inp = obj.apply_policy(particles_initial_state_mean=x0m, particles_initial_state_var=x0v, flg_particles_init_uniform=False,
                               particles_init_up_bound=None, particles_init_low_bound=None, flg_particles_init_multi_gauss=False,
                               num_particles=M, T_control=Tn, p_dropout=0.0)
    w, wu = T(rs.randn(Tn, M, S)), T(rs.randn(Tn, M, U))
    ((w * st).sum() + (wu * inp).sum()).backward()
    eps0, eps, pn = replay_noise(seed, M, G, Tn)
    x0 = x0m.detach().reshape(1, -1) + torch.sqrt(x0v.detach()).reshape(1, -1) * eps0
    assert torch.equal(x0, st[0].detach()), "noise replay does not reproduce the reference's x0"
    b, a = signal.butter(1, FC)
    out = dict(states_tr=xtr, inputs_tr=utr, sigma_n=SIGMA_N, lengthscales=LS, angle=np.array(ANGLE), not_angle=np.array(NOT_ANGLE),
               vel=np.array(VEL if kind == "speed" else range(S)), not_vel=np.array(NOT_VEL if kind == "speed" else [-1] * S), Ts=TS,
               pos_indeces=np.array(POS), vel_indeces=np.array(VELM), std_meas_noise=STD_MEAS, fc=FC, butter_b=np.asarray(b), butter_a=np.asarray(a),
               sqrt_kp=kp, sqrt_kd=kd, target=target, u_max=u_max, x0_mean=N(x0m), x0_var=N(x0v), eps0=N(eps0), eps=N(eps), pos_noise=N(pn),
               w=N(w), wu=N(wu), states=N(st), inputs=N(inp), g_sqrt_kp=N(pol.sqrt_Kp_gains.grad), g_sqrt_kd=N(pol.sqrt_Kd_gains.grad),
               g_x0_mean=N(x0m.grad), g_x0_var=N(x0v.grad))
    for g in range(G):
        out["Xtr%d" % g] = N(ml.gp_inputs_tr_list[g])
        out["alpha%d" % g] = N(ml.alpha_list[g])
        out["Kinv%d" % g] = N(ml.K_X_inv_list[g])
    return {kind + "_" + k: np.asarray(v) for k, v in out.items()}


fx = {}
fx.update(rollout_fixture("speed", M=6, Tn=6, seed=311))
fx.update(rollout_fixture("delta", M=6, Tn=6, seed=312))
path = os.path.join(HERE, "rollout_pd_pms.npz")
np.savez_compressed(path, **fx)
print("wrote rollout_pd_pms %.0f KB" % (os.path.getsize(path) / 1024.0))
assert os.path.getsize(path) < 400 * 1024
