/*
 * mcpilco_hip.h -- C ABI of libmcpilco_hip.so (gfx950 / MI355X).
 *
 * The reference (merlresearch/MC-PILCO) is pure Python on PyTorch and has no FFI of its own;
 * its extension mechanism is constructor injection of Python classes.  This header is the
 * boundary a maintainer would bind with ctypes underneath those classes:
 * every entry point names the reference function(s) it replaces as file:line relative to
 * the reference root.
 *
 * Conventions
 *   - all matrices float64, row-major, contiguous; every pointer is a DEVICE pointer unless
 *     the parameter is a `const mcp_*` descriptor struct (host memory, copied at launch);
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it; nothing here
 *     allocates, frees or synchronises (graph-capture safe) -- scratch comes from the caller
 *     through `workspace` (size from the matching *_workspace_bytes query);
 *   - return value: MCP_OK (0) or a negative MCP_ERR_* for arguments the kernels cannot take;
 *     never throws.  Numerical trouble is data, not an error: kernels OR bit flags into the
 *     device word `status` (MCP_STATUS_*), which the host may read after synchronising
 *     (reference behaviour: NaN cost -> retry, policy_learning/MC_PILCO.py:479-501,573-607);
 *   - re-entrant per stream; the caller owns every buffer.
 */
#ifndef MCPILCO_HIP_H
#define MCPILCO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCP_ABI_VERSION 7 /* 5: mcp_kernel.scal, MCP_FWD_NO_GP_SHARDING, MCP_STATUS_NONPOS_VAR now means a FINITE variance <= 0, mcp_nll_epoch, \
                             mcp_adam_step_guarded, mcp_policy_step_commit (round 4).                                                            \
                             6 (round 6; the round-5 contract changes, which had kept the number 5, are part of it): mcp_sod_select needs       \
                             mcp_sod_workspace_bytes(N) = 8 (N^2 + 2 N) + the exchange area (was 8 N^2) and may report *n_out = -1;             \
                             MCP_MAX_TRAIN 1024 -> 4096; the process-wide mcp_debug_* setters are gone (mcpilco_hip_debug.h: per-call           \
                             mcp_dispatch); mcp_adam_step_guarded skips a not-SPD epoch; new: mcp_sym_sandwich, mcp_noise.call_dev, MCP_FWD_KT_PACKED / MCP_FWD_XJ_PACKED. \
                             7: mcp_dispatch loses the Cholesky form request, mcp_chol_factor_ex / mcp_chol_inverse_ex are gone (debug header) */

#define MCP_OK 0
#define MCP_ERR_ARG (-1)       /* null pointer / non-positive size                       */
#define MCP_ERR_LIMIT (-2)     /* a dimension exceeds a compiled limit (MCP_MAX_*)        */
#define MCP_ERR_WORKSPACE (-3) /* workspace too small                                     */
#define MCP_ERR_LAUNCH (-4)    /* hipLaunchKernel reported an error                       */
#define MCP_ERR_COMM (-5)      /* RCCL is not loadable / no communicator / a collective failed */

#define MCP_STATUS_NAN 1u         /* a NaN was produced in a state / input / cost          */
#define MCP_STATUS_NONPOS_VAR 2u  /* a FINITE GP posterior variance <= 0 (torch Normal raises ValueError); a NaN variance sets MCP_STATUS_NAN only */
#define MCP_STATUS_NOT_SPD 4u     /* Cholesky met a non-positive pivot                     */
#define MCP_STATUS_SYNC 8u        /* GP-sharded rollout: a partner workgroup never arrived   */

#define MCP_MAX_GP 8
#define MCP_MAX_STATE 16
#define MCP_MAX_INPUT 8
#define MCP_MAX_GPDIM 32   /* D  : GP input dimension                                   */
#define MCP_MAX_PFEAT 32   /* P  : policy feature dimension                             */
#define MCP_MAX_BASIS 1024 /* B  : policy basis functions                               */
#define MCP_MAX_BASIS_WIDE 512 /* B of a WIDE policy (P > 16 or U > 4): the adjoint sweep of those widths has one thread per basis function in
                                * workgroups of at most 512, so mcp_rollout_fwd and mcp_rollout_bwd both refuse more (MCP_ERR_LIMIT) */
#define MCP_MAX_TRAIN 4096 /* N  : training points kept per GP (fused rollout kernels; round 5: was 1024) */

/* Kernel hyper-parameters of one GP: squared-exponential (+ Volterra polynomial of degree
 * 0, 1 or 2) -- gpr_lib/GP_prior/Stationary_GP.py:112-181 (RBF), gpr_lib/GP_prior/Sparse_GP.py:
 * 559-737 (MPK_GP, get_Volterra_MPK_GP), gpr_lib/GP_prior/GP_prior.py:299-347 (Sum_Independent_GP).
 * k(a,b) = lambda * exp(-sum_d ((a_d-b_d)/l_d)^2)                     (no factor 1/2)
 *        + [deg>=1] sum_d w1_d a_d b_d + w1_D                         (MPK_1, offset feature)
 *        + [deg==2] (sum_d w20_d a_d b_d) * (sum_d w21_d a_d b_d)     (MPK_2)
 * where w = s^2 and s_d=(k-d)*exp(par) as the reference's get_Sigma builds it (host side). */
typedef struct mcp_kernel {
  int32_t D;
  int32_t poly_deg;       /* 0, 1, 2                                                   */
  double lambda;          /* exp(log_lambda_par)                                       */
  double sigma_n2;        /* exp(sigma_n_log)^2 + sigma_n_num^2 (GP_prior.py:87-89)    */
  double mean;            /* constant prior mean (RBF.mean_par)                        */
  const double* inv_ls;   /* [D]      1/lengthscale                                    */
  const double* w1;       /* [D+1]    MPK_1 weights s^2 (NULL when poly_deg==0)        */
  const double* w20;      /* [D]      MPK_2 first-factor weights  (NULL unless deg==2) */
  const double* w21;      /* [D]      MPK_2 second-factor weights                      */
  const double* scal;     /* optional, device: [lambda, sigma_n2, mean] -- when non-NULL these override the three by-value
                             fields above (GP training keeps its hyper-parameters on the device: GP_prior.fit_model's epoch
                             then needs no device->host round trip to fill this descriptor)                              */
} mcp_kernel;

/* One pretrained GP = what Model_learning.pretrain_gp caches (model_learning/Model_learning.py:
 * 163-208: gp_inputs_tr_list, alpha_list, K_X_inv_list) in the kernels' layout.            */
typedef struct mcp_gp {
  mcp_kernel kern;
  int32_t N;              /* training points kept (all, or the SOD subset)             */
  int32_t Npad;           /* row pitch of X^T / Kinv, multiple of 16, >= N             */
  const double* Xt;       /* [D][Npad]    training inputs, transposed, zero padded     */
  const double* X;        /* [Npad][D]    same, row-major, zero padded                 */
  const double* alpha;    /* [Npad]       K^-1 (Y - m), zero padded                    */
  const double* Kinv;     /* [Npad][Npad] (K + sigma_n^2 I)^-1, symmetric, zero padded */
  const double* aX;       /* [D]          sum_j alpha_j X_jd (used when poly_deg>=1)   */
} mcp_gp;

/* Dynamics model.  Speed integration -- Speed_Model_learning_RBF(_MPK)_angle_state,
 * model_learning/Model_learning.py:619-760: GP g predicts the change of state vel[g];
 * not_vel[g] is the matching position (v' = v + d, q' = q + Ts v + Ts/2 d).
 * not_vel[g] == -1: GP g has no integrated position, x'[vel[g]] = x[vel[g]] + d_g -- the delta-state
 * models Model_learning_RBF(_angle_state), Model_learning_RBF_MPK_angle_state (Model_learning.py:471-493,
 * 495-618) are G = S, vel = 0..S-1, every not_vel = -1 (Ts then only serves a measurement model).
 * A library older than this rule refuses such a descriptor (MCP_ERR_ARG).
 * GP input z=[x[not_angle], sin x[angle], cos x[angle], u].
 * The index lists: no index twice within angle, none twice within not_angle (an index may be in angle AND in
 * not_angle: both features are formed); no index twice in vel, no non-negative index twice in not_vel, and no
 * component that is vel[g] and not_vel[g'] -- every component is written by at most one GP.  A descriptor that
 * breaks one of these is refused by every entry point (MCP_ERR_ARG) before any HIP call.  A component that is
 * neither a vel nor a not_vel is 0 from row 1 on. */
typedef struct mcp_model {
  int32_t S, U, G, D;
  int32_t n_angle, n_not_angle;
  int32_t angle[MCP_MAX_STATE];
  int32_t not_angle[MCP_MAX_STATE];
  int32_t vel[MCP_MAX_GP];
  int32_t not_vel[MCP_MAX_GP];
  double Ts;
  double var_scale[MCP_MAX_GP]; /* norm_list[g]^2 (Model_learning.py:220-221), 1 by default */
  mcp_gp gp[MCP_MAX_GP];
} mcp_model;

#define MCP_POLICY_PLAIN 0  /* Sum_of_gaussians                        policy_learning/Policy.py:153-265 */
#define MCP_POLICY_ANGLES 1 /* Sum_of_gaussians_with_angles            Policy.py:268-335  s=[x_na,cos,sin] */
#define MCP_POLICY_TRAJ 2   /* Sum_of_gaussians_with_target_trajectory Policy.py:338-403  s=[x, x*_t-x]    */

/* Measurement model of MC_PILCO4PMS.apply_policy (policy_learning/MC_PILCO.py:808-906): the particles evolve on their true
 * states, the policy is evaluated on a simulated measurement -- positions plus Gaussian noise (:881-885), velocities by
 * backward difference of the noisy positions (:888-891) passed through the first-order filter (b0 nv_t + b1 nv_{t-1} -
 * a1 mv_{t-1}) / a0 (:895-899); at t = 0 the measurement is the true state (:856).  n == 0: the policy sees the true state
 * (MC_PILCO.apply_policy). */
typedef struct mcp_meas {
  int32_t n;                      /* (position, velocity) pairs                                        */
  int32_t pos[MCP_MAX_STATE];     /* pos_indeces                                                       */
  int32_t vel[MCP_MAX_STATE];     /* vel_indeces                                                       */
  double std_pos[MCP_MAX_STATE];  /* std of the position measurement noise, std_meas_noise_sim[pos]    */
  double b0, b1, a0, a1;          /* scipy.signal.butter(1, fc)                                        */
  const double* pos_noise;        /* [T-1][M][n] standard normals (step t at row t-1), or NULL: Philox  */
  double* meas;                   /* [T][M][S] measured states: written by mcp_rollout_fwd, read by
                                     mcp_rollout_bwd (caller-owned, required when n > 0)               */
} mcp_meas;

typedef struct mcp_policy {
  int32_t kind;
  int32_t S;              /* state dim of the system                                   */
  int32_t P;              /* feature dim (state_dim of the RBF network)                */
  int32_t B, U;
  int32_t squash;         /* flg_squash                                                */
  int32_t n_angle, n_non_angle;
  int32_t angle[MCP_MAX_STATE];
  int32_t non_angle[MCP_MAX_STATE];
  int32_t traj_len;       /* rows of target_traj                                       */
  double p_drop;          /* dropout probability (0 -> no mask, no draw)               */
  const double* log_ls;   /* [P]     log_lengthscales                                  */
  const double* centers;  /* [B][P]                                                    */
  const double* weight;   /* [U][B]  f_linear.weight (no bias)                         */
  const double* u_max;    /* [U]                                                       */
  const double* target_traj; /* [traj_len][S] or NULL                                  */
  const double* bias;     /* [U]     f_linear.bias (flg_bias, Policy.py:203-212) or NULL: u = squash(W phi + bias); not dropped out */
  double* g_bias;         /* [U]     OUT of mcp_rollout_bwd when bias != NULL: dJ/dbias (this rank's particles); may be NULL */
  mcp_meas meas;          /* what the policy is evaluated on (n == 0: the true state)  */
} mcp_policy;

/* Where the rollout's random numbers come from.  Parity mode: the host draws them with the
 * reference's own torch calls (SURVEY 8c order) and passes buffers.  Performance mode:
 * eps==NULL / masks==NULL -> Philox4x32-10 keyed by (seed, call) and counted by GLOBAL particle
 * id (m + particle_offset), so a sharded run draws the same numbers as a single-GPU run.
 * Supported ranges of the addressing (csrc/mcp_device.h, philox_draw; restated and tested by tests/noise_truth.py): a time step t < 2^22 and a
 * global particle id < 2^40 -- one counter word holds the id's high word, t << 8 and the stream at bit 30, so particle 2^40 at t = 0 is particle
 * 0 at t = 1 and t = 2^22 is another stream's t = 0.  Every `call` of one seed draws other numbers (call + *call_dev is taken mod 2^64); the high
 * word of `call` is XORed into the key word that holds the seed's low word, so two SEEDS are independent of each other while call < 2^32. */
typedef struct mcp_noise {
  const double* eps;      /* [T-1][M][G] standard normals, or NULL                     */
  const uint8_t* masks;   /* [T][M][B]   dropout keep-masks {0,1}, or NULL (mcp_rollout_mlp_drop: [T][M][H], the hidden units) */
  uint64_t seed;
  uint64_t call;          /* increments once per rollout so draws never repeat         */
  int64_t particle_offset;
  const uint64_t* call_dev; /* optional DEVICE counter added to `call` when the kernels start (NULL: none): a rollout recorded into a HIP graph
                               draws fresh numbers on every replay when the graph also advances this word -- the by-value `call` is frozen
                               in the recorded kernel arguments (round 6: MC_PILCO.reinforce_policy replays its attempts) */
} mcp_noise;

/* PD law in closed loop -- Policy.PD_controller (policy_learning/Policy.py:406-449) with flg_trainable, evaluated inside the fused
 * rollout:  e = target_traj[t] - x_t;  a_k = sqrt_kp[k]^2 e[pos[k]] + sqrt_kd[k]^2 e[vel[k]];  u_t[k] = u_max[k] tanh(a_k / u_max[k])
 * (squash) or a_k.  The reference's layout is pos = 0..U-1, vel = S/2..S/2+U-1.  The entries of pos are distinct state components, and
 * so are those of vel.  The gains and the target are DEVICE pointers: an optimizer updates the gains in place. */
typedef struct mcp_pd_policy {
  int32_t U;                    /* inputs, == model->U                                        */
  int32_t squash;               /* flg_squash                                                 */
  int32_t pos[MCP_MAX_INPUT];   /* state component whose error sqrt_kp[k]^2 multiplies        */
  int32_t vel[MCP_MAX_INPUT];   /* state component whose error sqrt_kd[k]^2 multiplies        */
  double u_max[MCP_MAX_INPUT];  /* > 0 with squash                                            */
  const double* sqrt_kp;        /* [U]  sqrt_Kp_gains                                         */
  const double* sqrt_kd;        /* [U]  sqrt_Kd_gains                                         */
  const double* target_traj;    /* [target_rows][S]                                           */
  int32_t target_rows;          /* >= T                                                       */
} mcp_pd_policy;

/* Tanh multilayer perceptron in closed loop -- Policy.MLP_policy (this project's own class; the reference has none), evaluated inside the
 * fused rollout on the features of Sum_of_gaussians_with_angles in the order f = [x[non_angle], sin x[angle], cos x[angle]] (both lists
 * empty: f = x, P = S):
 *   h1 = tanh(W[0] f + b[0]);  h2 = tanh(W[1] h1 + b[1]) (n_hidden == 2);  a = W[2] h + b[2];  u[k] = u_max[k] tanh(a[k] / u_max[k]) (squash) or a[k]
 * Layer i is row-major [out][in]; W[2] / b[2] are ALWAYS the output layer, W[1] / b[1] are NULL with one hidden layer.  The weights are
 * DEVICE pointers: an optimizer updates them in place.  An index appears at most once in angle and non_angle together. */
#define MCP_MAX_HIDDEN 64 /* units of a hidden layer of mcp_mlp_policy */
typedef struct mcp_mlp_policy {
  int32_t S, U, P;                  /* == model->S, == model->U, n_non_angle + 2 n_angle (or S)    */
  int32_t n_hidden;                 /* 1 or 2                                                     */
  int32_t h[2];                     /* widths, 1 .. MCP_MAX_HIDDEN (h[1] ignored with one layer)  */
  int32_t n_angle, n_non_angle;     /* both 0: f = x                                              */
  int32_t angle[MCP_MAX_STATE];
  int32_t non_angle[MCP_MAX_STATE];
  int32_t squash;                   /* flg_squash                                                 */
  double u_max[MCP_MAX_INPUT];      /* > 0 with squash                                            */
  const double* W[3];               /* [h0][P] | [h1][h0] or NULL | [U][h_last]                   */
  const double* b[3];               /* [h0]    | [h1] or NULL     | [U]                           */
} mcp_mlp_policy;

/* Target-trajectory features of the tanh MLP -- the feature map of the reference's Sum_of_gaussians_with_target_trajectory (policy_in =
 * cat(x, x*_t - x), policy_learning/Policy.py:389-403) behind mcp_mlp_policy's own: the feature row of policy evaluation t (every row
 * 0 .. T - 1) is
 *   f_t = [x[non_angle], sin x[angle], cos x[angle], target[t][idx[i]] - x[idx[i]]  (i = 0 .. n - 1)]
 * so the descriptor's P = n_non_angle + 2 n_angle + n (without lists S + n) and W[0] is [h0][P] with the error columns LAST.  The error
 * is the plain difference target - x, not wrapped on angle components (as the reference and mcp_pd_policy have it).  The target is a
 * constant of the launch: no gradient. */
typedef struct mcp_mlp_track {
  int32_t n;                    /* error features; 0: none                       */
  int32_t idx[MCP_MAX_STATE];   /* distinct state components                     */
  int32_t rows;                 /* rows of target, >= T                          */
  const double* target;         /* DEVICE [rows][S]                              */
} mcp_mlp_track;

/* PD term of the RESIDUAL policy -- mcp_pd_policy's law added to the network's output ahead of the ONE squashing, so that a stabilising
 * PD controller (the UR5 launch script's) is kept and the network learns a correction on top of it:
 *   a[k] = (W[2] h + b[2])[k] + sqrt_kp[k]^2 (target[t][pos[k]] - x[pos[k]]) + sqrt_kd[k]^2 (target[t][vel[k]] - x[vel[k]])
 *   u[k] = u_max[k] tanh(a[k] / u_max[k]) (squash) or a[k]                 in every policy evaluation t = 0 .. T - 1, row T - 1 included
 * The gains are squared once per launch; the errors are plain differences, not wrapped; dropout never touches the term; in the measured
 * form x is the simulated measurement y_t here as everywhere else (as mcp_rollout_pd_meas has it).  The target is a constant of the
 * launch (no gradient) and may be the track's tensor or another. */
typedef struct mcp_mlp_pd {
  int32_t on;                   /* 0: no PD term                                                 */
  int32_t pos[MCP_MAX_INPUT];   /* distinct state components                                     */
  int32_t vel[MCP_MAX_INPUT];   /* distinct state components                                     */
  const double* sqrt_kp;        /* DEVICE [U]: an optimizer updates it in place                  */
  const double* sqrt_kd;        /* DEVICE [U]                                                    */
  const double* target;         /* DEVICE [rows][S]; may be the track's tensor or another        */
  int32_t rows;                 /* >= T                                                          */
} mcp_mlp_pd;

/* MEMORY of the tanh MLP -- the network reads the last h rows it was shown, so that it can learn its own estimator from them.  The fused
 * entries take it on the TRUE STATE only: with h > 1 and an active measurement model they return MCP_ERR_ARG (a measured form is not
 * built; MC_PILCO4PMS runs such a policy on its step loop).  With r_t the row the policy reads in evaluation t (the state x_t) and
 * phi the descriptor's own map [r[non_angle], sin r[angle], cos r[angle]] (or r), of width P0, the feature row of evaluation t (every row
 * 0 .. T - 1) is
 *   f_t = [phi(r_t), phi(r_{t-1}), ..., phi(r_{t-h+1}), target[t][idx[i]] - r_t[idx[i]]  (i = 0 .. n - 1)],   r_{t-j} := r_0 for t - j < 0
 * the NEWEST block first, the track's errors (of the current row only) last; rows before 0 REPEAT row 0 (no zero padding: f_0 is h copies
 * of phi(r_0)).  The descriptor's P = h P0 + track->n and W[0] is [h0][P].  The PD term and dropout are untouched: both see the current
 * row / the hidden units alone.  ADJOINT: block j of row t pulls on r_{max(t-j, 0)} through phi at THAT row, so row 0 collects the pull of
 * every block that was clamped onto it. */
#define MCP_MAX_HIST 4
typedef struct mcp_mlp_hist {
  int32_t h;                    /* 1 .. MCP_MAX_HIST; 1: no history */
} mcp_mlp_hist;

/* Integral term of the PD law in closed loop -- mcp_pd_policy's law with a clamped integral of the position error (anti-windup), the
 * first law here whose control depends on controller state carried across the steps.  The reference has no integral law: without this
 * term it is a stateful torch policy in the step loop of MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674; measured: :808-906).
 * For input k with p = pos[k], v = vel[k] of the mcp_pd_policy beside it, e_t = target_traj[t] - x_t (measured form: y_t in place of x_t):
 *   q_t[k] = I_{t-1}[k] + dt e_t[p],  I_{-1} = 0;      I_t[k] = min(max(q_t[k], -i_max[k]), +i_max[k])      (i_max[k] = +inf: no clamp)
 *   a_t[k] = (sqrt_kp[k]^2 e_t[p] + sqrt_kd[k]^2 e_t[v]) + sqrt_ki[k]^2 I_t[k];    u_t[k] = u_max[k] tanh(a_t[k] / u_max[k]) (squash) or a_t[k]
 * in every row t = 0 .. T - 1.  The PD products are mcp_rollout_pd's expression in its order and the integral product is added last, so
 * sqrt_ki == 0 (with a finite I) reproduces the PD launch bit for bit.  The errors are plain differences, not wrapped.  A NaN passes
 * through the clamp.  The clamp passes gradient iff |I_t[k]| < i_max[k] and blocks it where I_t sits on a bound; the forward launch
 * writes I to integ and the sweep reads it there, so the sweep never re-decides a clamp.  Adjoint, per row r from T - 1 down, with abar
 * the adjoint of a (mcp_rollout_pd_bwd's) and c_T = 0:
 *   Ibar_r[k] = sqrt_ki[k]^2 abar_r[k] + c_{r+1}[k];   c_r[k] = (|I_r[k]| < i_max[k]) ? Ibar_r[k] : 0
 *   lambda_r[pos[k]] -= dt c_r[k]  (beside - sqrt_kp[k]^2 abar_r[k]; measured form: on the measurement's adjoint, through the filter's)
 *   g_sqrt_ki[k] += 2 sqrt_ki[k] I_r[k] abar_r[k]
 * c is one double per (trajectory, input), kept in registers: no atomics, no sum across trajectories, the same bits run after run. */
typedef struct mcp_pid_term {
  int32_t on;                   /* 0: no integral term                                           */
  const double* sqrt_ki;        /* DEVICE [U]: an optimizer updates it in place                  */
  double i_max[MCP_MAX_INPUT];  /* > 0; +inf: no clamp                                           */
  double dt;                    /* > 0: the integration step (the class passes T_sampling)       */
  double* integ;                /* DEVICE [T][M][U]: I, written by the forward, read by the sweep */
} mcp_pid_term;

/* TIME-VARYING LINEAR FEEDBACK in closed loop -- Policy.TV_linear_controller (this project's own class; the reference has none): a
 * feedforward sequence plus per-step dense gains around a reference, the local controller of trajectory optimisation.  For row
 * t = 0 .. T - 1, with r_t the state x_t (measured form: the simulated measurement y_t of mcp_meas):
 *   e_t = target_traj[t] - r_t;   a_t[k] = (sum_s gain[t][k][s] e_t[s]) + ff[t][k]   (s ascending from 0.0, the feedforward added last)
 *   u_t[k] = u_max[k] tanh(a_t[k] / u_max[k]) (squash) or a_t[k]
 * The gains are plain (not squared) and dense over all S components; no index layout applies (S may be odd, U need not be S / 2).  The
 * errors are plain differences, not wrapped.  gain_rows == 1: one matrix [U][S] for every row.  ff_rows == 0: no feedforward (ff may be
 * NULL).  The three tensors are DEVICE pointers: an optimizer updates gain and ff in place; the target is a constant of the launch. */
typedef struct mcp_tvl_policy {
  int32_t U, S;                 /* == model->U, == model->S                                      */
  int32_t squash;               /* flg_squash                                                    */
  int32_t gain_rows;            /* 1: shared, else >= T                                          */
  int32_t ff_rows;              /* 0: no feedforward, else >= T                                  */
  int32_t target_rows;          /* >= T                                                          */
  double u_max[MCP_MAX_INPUT];  /* > 0 with squash                                               */
  const double* gain;           /* DEVICE [gain_rows][U][S]                                      */
  const double* ff;             /* DEVICE [ff_rows][U], or NULL with ff_rows == 0                */
  const double* target_traj;    /* DEVICE [target_rows][S]                                       */
} mcp_tvl_policy;

/* ---- library ------------------------------------------------------------------------ */
int mcp_abi_version(void);
const char* mcp_build_info(void);

/* ---- pretrain: Gram / Cholesky / inverse / alpha -------------------------------------- */
/* K[i][j] = k(X1_i, X2_j) (+ sigma_n2 on the diagonal when add_noise and X2==X1 semantics).
 * Replaces RBF.get_covariance (Stationary_GP.py:162-170), MPK_GP/Linear_GP.get_covariance
 * (Sparse_GP.py:426-441,625-646), Sum_Independent_GP.get_covariance (GP_prior.py:314-335). */
int mcp_cov_build(const mcp_kernel* kern, int N1, const double* X1, int N2, const double* X2, int add_noise,
                  double* K, int ldk, void* stream);
/* diag k(x_i,x_i) -- get_diag_covariance (Stationary_GP.py:172-181, Sparse_GP.py:443-453,658-668,
 * GP_prior.py:337-347). */
int mcp_cov_diag(const mcp_kernel* kern, int N, const double* X, int add_noise, double* diag, void* stream);
/* In place: A (symmetric, upper triangle read) -> U upper with A = U^T U; strictly-lower part
 * zeroed (from 600 rows on it serves as scratch on the way); logdet = 2 sum log U_ii.  N <= 8192.
 * torch.cholesky(K, upper=True) + log_det, GP_prior.py:106-107. */
int mcp_chol_factor(int N, double* A, int lda, double* logdet, uint32_t* status, void* stream);
/* Uinv = U^-1 (upper) and Kinv = Uinv Uinv^T.  torch.inverse(U), GP_prior.py:109-110.  Only the upper 16 x 16 blocks of Uinv are written
 * (and, beyond 1152 rows, its strictly-lower 128-row block rows are used as scratch and zeroed again): pass Uinv zero-filled for a clean lower
 * triangle.  N <= 16384. */
int mcp_chol_inverse(int N, const double* U, int ldu, double* Uinv, int ldi, double* Kinv, int ldk, void* stream);
/* out = A G A for a symmetric A [N][N] (K^-1) and any G [N][N]; scratch: N * N doubles; out, scratch, A, G distinct.  The chain rule through
 * torch.inverse in GP_prior.forward's autograd graph (GP_prior.py:109-110: d K^-1 = - K^-1 dK K^-1) for criteria other than the marginal
 * likelihood in GP_prior.fit_model (GP_prior.py:179-230).  N <= 16384. */
int mcp_sym_sandwich(int N, const double* A, int lda, const double* G, int ldg, double* out, int ldo, double* scratch, void* stream);
/* alpha = Kinv (Y - mean).  GP_prior.get_alpha, GP_prior.py:130-135. */
int mcp_gp_alpha(int N, const double* Kinv, int ldk, const double* Y, double mean, double* alpha, void* stream);
/* Greedy subset-of-data selection on the device, GP_prior.get_SOD (GP_prior.py:232-257):
 * idx_out[0..*n_out) receives the kept sample indices (ascending, bit-exact contract).
 * workspace: mcp_sod_workspace_bytes(N) -- W [N][N] and two running sums [N]; from 256 candidates on also the exchange area and the Gram matrix of
 * the form that runs across workgroups (one per 64 candidates, all resident; N <= 4096).  With 8 (N^2 + 2 N) bytes only, the call keeps to one
 * workgroup.  *n_out = -1: the workgroups never met (the device could not hold the grid) -- repeat with the smaller workspace. */
size_t mcp_sod_workspace_bytes(int N);
int mcp_sod_select(const mcp_kernel* kern, int N, const double* X, double threshold, int32_t* idx_out, int32_t* n_out,
                   void* workspace, size_t workspace_bytes, void* stream);
/* Gradient of the marginal likelihood  L = 1/2 ((Y-m)^T Kinv (Y-m) + logdet K)  w.r.t. the kernel's log-parameters --
 * what autograd computes through GP_prior.forward + Marginal_log_likelihood in GP_prior.fit_model (GP_prior.py:179-230,
 * gpr_lib/Likelihood/Gaussian_likelihood.py:15-24):  dL/dtheta = 1/2 tr((Kinv - alpha alpha^T) dK/dtheta).
 * grad [4D+3]: [0,D) d/d log lengthscale | D d/d log lambda | D+1  1/2 tr(Kinv - alpha alpha^T) (multiply by
 * d sigma_n^2/d sigma_n_log = 2 exp(2 sigma_n_log)) | [D+2,2D+3) MPK_1 Sigma_pos_par | [2D+3,3D+3), [3D+3,4D+3) the two
 * factors of MPK_2's Sigma_pos_par.  workspace: mcp_nll_workspace_bytes(N, D). */
size_t mcp_nll_workspace_bytes(int N, int D);
int mcp_nll_grad(const mcp_kernel* kern, int N, const double* X, const double* Kinv, int ldk, const double* alpha, double* grad,
                 void* workspace, size_t workspace_bytes, void* stream);
/* One epoch of hyper-parameter training for the G GPs of a model at once, from the optimizer's RAW parameters to their gradients and the
 * loss, without a host round trip -- what GP_prior.fit_model does per epoch through forward + Marginal_log_likelihood + autograd
 * (GP_prior.py:91-115,179-230; Gaussian_likelihood.py:15-24; Model_learning.train_gp_likelihood, Model_learning.py:398-421).  The GPs of
 * a model are independent (the reference trains them one after the other, Model_learning.py:149-161): every stage -- Gram, Cholesky,
 * U^-1, K^-1, alpha, gradient -- is ONE launch whose grid carries the GP index.  All GPs share the inputs X [N][D] and the kernel
 * structure: one squared-exponential term (lengthscales per dimension or, ard == 0, one shared) plus poly_deg = 0 / 1 / 2 Volterra
 * terms (MPK_1 with the offset feature, MPK_2 without), noise from the squared-exponential term.  mcp_nll_gp: device pointers to the
 * raw parameters as the reference stores them (log_lengthscales_par, log_lambda_par, sigma_n_log, mean_par, MPK Sigma_pos_par) and to
 * the gradient buffers (NULL: not wanted -- a frozen parameter).  16 < N <= 1152.  status: one word, OR of MCP_STATUS_NOT_SPD. */
typedef struct mcp_nll_gp {
  const double* log_ls;       /* [D], or [1] when ard == 0                                        */
  const double* log_lambda;   /* [1]                                                              */
  const double* sigma_n_log;  /* [1] or NULL: no noise parameter                                  */
  const double* mean;         /* [1] or NULL: zero prior mean                                     */
  const double* mpk1;         /* [D+1] MPK_1 Sigma_pos_par (log), or NULL                         */
  const double* mpk2;         /* [2D]  MPK_2 Sigma_pos_par (log): factor 0 | factor 1, or NULL    */
  const double* Y;            /* [N] targets                                                      */
  double y_scale;             /* the targets enter as Y * y_scale (1 / norm_list[g])              */
  double sigma_n_num2;        /* sigma_n_num^2                                                    */
  double* g_log_ls;           /* gradients w.r.t. the raw parameters, same shapes (NULL: skip)    */
  double* g_log_lambda;
  double* g_sigma_n_log;
  double* g_mean;
  double* g_mpk1;
  double* g_mpk2;
  double* loss;               /* [1]  1/2 ((Y-m)^T K^-1 (Y-m) + logdet K), or NULL                */
} mcp_nll_gp;
size_t mcp_nll_epoch_workspace_bytes(int G, int N, int D);
int mcp_nll_epoch(int G, const mcp_nll_gp* gps, int N, int D, int poly_deg, int ard, const double* X, uint32_t* status, void* workspace,
                  size_t workspace_bytes, void* stream);
/* Packs pretrain outputs into the mcp_gp layout (padding, transposes, aX). */
int mcp_gp_pack(int N, int D, const double* X, const double* alpha, const double* Kinv, int ldk, int Npad, double* Xt_out,
                double* X_out, double* alpha_out, double* Kinv_out, double* aX_out, void* stream);

/* ---- single-step GP posterior (GP_prior.get_estimate_from_alpha, GP_prior.py:137-155) -- */
/* mu[M], var[M] at test inputs Z [M][D]; Jmu/Jvar [M][D] = d mu/dz, d var/dz (NULL to skip). */
int mcp_posterior_fwd(const mcp_gp* gp, int M, const double* Z, double* mu, double* var, double* Jmu, double* Jvar,
                      uint32_t* status, void* stream);
/* gZ[m][d] = gmu[m]*Jmu[m][d] + gvar[m]*Jvar[m][d]  (adjoint of the above). */
int mcp_posterior_bwd(int M, int D, const double* gmu, const double* gvar, const double* Jmu, const double* Jvar, double* gZ,
                      void* stream);

/* ---- fused particle rollout (MC_PILCO.apply_policy, policy_learning/MC_PILCO.py:615-674:
 * T-loop of Model_learning.get_next_state (Model_learning.py:210-229,685-718) and the policy
 * forward (Policy.py:242-265,323-335,389-403)) ----------------------------------------- */
#define MCP_FWD_NO_GP_SHARDING 2 /* flag in mcp_rollout_fwd's particle_pred argument */
#define MCP_FWD_KT_PACKED 4      /* flags in the same argument: the workspace still holds the packed operand copies an EARLIER call built from    */
#define MCP_FWD_XJ_PACKED 8      /* this same model in this same workspace (KT: the lean small-swarm kernel's Kinv tiles; XJ: the wide classes'   */
                                 /* phase-J operands) -- the call does not rebuild them (8 us per rollout at the cart-pole size).  The caller's  */
                                 /* promise: nothing else wrote there and the model's arrays are unchanged.  Without the flags every call packs. */
size_t mcp_rollout_workspace_bytes(const mcp_model* model, const mcp_policy* policy, int M, int T);
/* x0 [M][S] -> states [T][M][S], inputs [T][M][U].  jac [T-1][M][G][D] (d delta_g/d z, sampling
 * included) is written when non-NULL and is what mcp_rollout_bwd consumes.
 * particle_pred: bit 0 clear -> delta = posterior mean (Model_learning.py:707-708); bit 1 (MCP_FWD_NO_GP_SHARDING) -> never launch
 * GP-sharded even though a workspace is passed (the repeat of a step that reported MCP_STATUS_SYNC: the workspace still carries the
 * packed operand copies of the wide / narrow kernels, only the hand-off between workgroups is given up).  T==1 evaluates the
 * policy only (Policy.forward); in that case `model` may be NULL.
 * workspace (optional, mcp_rollout_workspace_bytes): with it, small swarms run GP-sharded -- the G
 * workgroups of a particle cluster each evaluate one GP and hand each other the sampled increments
 * once per step through this buffer (zeroed by the call, on `stream`); results agree with the
 * unsharded launch to rounding.  MCP_STATUS_SYNC in `status` reports a hand-off that timed out
 * (the trajectories are then invalid).  Without a workspace the launch is never sharded.  For models with more
 * than 15 GP-input dimensions the workspace also takes the packed operand copies of the 16-particle kernel's
 * moment / Jacobian contraction (rebuilt by every call, on `stream`, unless MCP_FWD_XJ_PACKED says an earlier call's copy stands); without it
 * that phase keeps its slower form. */
int mcp_rollout_fwd(const mcp_model* model, const mcp_policy* policy, const mcp_noise* noise, int M, int T, int particle_pred,
                    const double* x0, double* states, double* inputs, double* jac, uint32_t* status, void* workspace,
                    size_t workspace_bytes, void* stream);
/* Open-loop rollout: M trajectories advanced T steps by the model alone, the input of step t read from `u` (the inputs recorded on
 * the system) -- no policy, no Jacobians, no workspace, one launch.  Replaces the step loop of MC_PILCO.rollout
 * (policy_learning/MC_PILCO.py:347-373) over Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 685-718).
 * x0 [M][S]; u [T-1][Mu][U] with Mu == M, or Mu == 1: one input sequence shared by every trajectory; states [T][M][S].
 * particle_pred bit 0 clear: delta = posterior mean, and unless `var` is asked for no Kinv is read (one workgroup per trajectory);
 * set: delta = mu + sqrt(var) eps with var = var_scale (k(z,z) - k^T Kinv k), eps from noise->eps [T-1][M][G] or Philox keyed by
 * (seed, call, m + particle_offset): trajectories [a, b) launched with particle_offset = a carry the bits of rows [a, b) of one launch
 * over all of them.  lengths (optional, [M], 1 <= len <= T, clamped): trajectory m is advanced to row len - 1, its later rows are
 * zeros and its inputs from row len - 1 on are never read.  mu / var (optional, [T-1][M][G]): the GP means and scaled variances of
 * every step (what get_next_state returns; rows beyond a length are not written).  status: MCP_STATUS_NAN | MCP_STATUS_NONPOS_VAR. */
int mcp_rollout_open(const mcp_model* model, const mcp_noise* noise, int M, int T, int particle_pred, const double* x0, const double* u,
                     int Mu, const int32_t* lengths, double* states, double* mu, double* var, uint32_t* status, void* stream);
/* The RECORDING form of mcp_rollout_open, for gradients through the open-loop rollout: the same arguments plus jac [T-1][M][G][D] =
 * d delta_g / d z with the sampling folded in (layout and meaning of mcp_rollout_fwd's record), which mcp_rollout_open_bwd consumes.
 * The states (and mu / var) carry the bits of mcp_rollout_open with the same arguments; jac is bitwise reproducible and independent of
 * the launch's other trajectories and of particle_offset sharding in the same way.  Rows of jac from len - 1 on are never written and
 * never read.  A sampled step whose variance is not positive raises MCP_STATUS_NONPOS_VAR and leaves inf / NaN in that trajectory's
 * rows, as mcp_rollout_fwd does.  Stands in for what autograd records through the step loop of MC_PILCO.rollout
 * (policy_learning/MC_PILCO.py:347-373) over Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_open_rec(const mcp_model* model, const mcp_noise* noise, int M, int T, int particle_pred, const double* x0, const double* u,
                         int Mu, const int32_t* lengths, double* states, double* mu, double* var, double* jac, uint32_t* status, void* stream);
/* Reverse-time sweep of the open-loop rollout: g_states [T][M][S] = dJ/dstates (required; rows beyond a trajectory's row len - 1 are
 * ignored) -> g_x0 [M][S] = dJ/dx0 and g_u [T-1][M][U] = dJ/du per trajectory (each may be NULL; rows of g_u from len - 1 on are zeros;
 * a shared input sequence's gradient is the caller's sum over M).  states, lengths, jac: what mcp_rollout_open_rec wrote / was given.
 * Only the model's index maps and Ts are read (no GP array).  No atomics: bitwise reproducible, a trajectory's results do not depend
 * on the others.  Replaces autograd's backward through the step loop of MC_PILCO.rollout (policy_learning/MC_PILCO.py:347-373) over
 * get_next_state and the integrators (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_open_bwd(const mcp_model* model, int M, int T, const double* states, const int32_t* lengths, const double* jac,
                         const double* g_states, double* g_x0, double* g_u, void* stream);
/* ONE time step of the model, for a closed loop whose policy the caller evaluates itself (any torch module): x [M][S], u [M][U] ->
 * x_next [M][S] in one launch, one workgroup per (tile of particles, GP), no workspace.  Replaces one Model_learning.get_next_state
 * (model_learning/Model_learning.py:210-229, 471-494, 685-718).  The arithmetic of a (particle, GP) is mcp_rollout_open's: a chain of
 * steps t = 0, 1, ... fed the inputs of a rollout carries the bits of that rollout's states (and of its mu / var).
 * noise->eps is THIS step's row [M][G]; NULL: Philox addressed as mcp_rollout_open addresses step t of a rollout (seed, call, call_dev,
 * m + particle_offset), so particles [a, b) launched with particle_offset = a carry the bits of rows [a, b) of one launch.
 * particle_pred bit 0 clear: the step is the posterior mean and reads no Kinv unless `var` is asked for.  mean / var (optional, [M][G]):
 * what get_next_state returns, var_scale applied.  jac (optional, [M][G][D]): the record d delta_g / dz with the sampling folded in, one
 * row of mcp_rollout_open_rec's, for mcp_model_step_bwd; x_next carries the same bits with and without it.  OUTPUTS NOT DIFFERENTIATED:
 * the record describes x_next alone -- no gradient is provided through mean and var.  status: MCP_STATUS_NAN (x, u, a moment or x_next is
 * not finite) | MCP_STATUS_NONPOS_VAR.  MCP_ERR_ARG: a NULL among model / noise / x / u / x_next / status, M <= 0, t < 0, a model
 * model_ok refuses; MCP_ERR_LIMIT: a dimension beyond MCP_MAX_*.  A refused call makes no HIP call. */
int mcp_model_step(const mcp_model* model, const mcp_noise* noise, int M, int t, int particle_pred, const double* x, const double* u,
                   double* x_next, double* mean, double* var, double* jac, uint32_t* status, void* stream);
/* The reverse of mcp_model_step: g_next [M][S] = dJ/dx_next -> g_x [M][S] = dJ/dx and g_u [M][U] = dJ/du (each may be NULL; both NULL:
 * MCP_OK without a launch) from x and the record jac of the forward call.  Only the model's index maps and Ts are read (no GP array).  No
 * atomics: bitwise reproducible, a particle's results do not depend on the others.  One row of mcp_rollout_open_bwd, the same order of
 * operations. */
int mcp_model_step_bwd(const mcp_model* model, int M, const double* x, const double* jac, const double* g_next, double* g_x, double* g_u,
                       void* stream);
/* Closed-loop rollout under the PD law, ONE launch: mcp_rollout_open's step with the input of step t computed from x_t inside the
 * kernel (mcp_pd_policy) instead of read from a buffer -- same phases, same noise addressing (eps [T-1][M][G] or Philox by seed, call,
 * m + particle_offset), same status flags; a NaN input raises MCP_STATUS_NAN.  states [T][M][S]; inputs [T][M][U], row T - 1 included
 * (no transition reads it; the reference stores it too and a cost may read it).  No ragged lengths.  jac NULL: nothing is recorded;
 * else jac [T-1][M][G][D] as mcp_rollout_open_rec writes it, input columns included, for mcp_rollout_pd_bwd; states and inputs carry the
 * same bits either way.  mu / var (optional, [T-1][M][G]) as in mcp_rollout_open.  T == 1 evaluates the policy only.
 * MCP_ERR_ARG: an index out of range or repeated, pd->U != model->U, target_rows < T, T < 1, a u_max <= 0 with squash; MCP_ERR_LIMIT
 * beyond MCP_MAX_*.  Replaces the loop of MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674) with PD_controller.forward
 * (policy_learning/Policy.py:437-449) over Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_pd(const mcp_model* model, const mcp_pd_policy* pd, const mcp_noise* noise, int M, int T, int particle_pred, const double* x0,
                   double* states, double* inputs, double* jac /* NULL: no record */, double* mu, double* var, uint32_t* status, void* stream);
/* Reverse-time sweep of mcp_rollout_pd: g_states [T][M][S] (required) and g_inputs [T][M][U] (optional) -> g_gains [M][2][U] =
 * dJ/d(sqrt_kp, sqrt_kd) PER TRAJECTORY (the sum over M is the caller's, in an order of its choosing) and g_x0 [M][S]; each may be
 * NULL.  states, inputs, jac: what mcp_rollout_pd wrote (jac may be NULL when T == 1).  Row T - 1 contributes through g_inputs alone.
 * No atomics: bitwise reproducible, a trajectory's results do not depend on the others.  Replaces autograd's backward (MC_PILCO.py:522)
 * through MC_PILCO.apply_policy's loop (policy_learning/MC_PILCO.py:615-674), PD_controller.forward (policy_learning/Policy.py:437-449)
 * and the integrators (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_pd_bwd(const mcp_model* model, const mcp_pd_policy* pd, int M, int T, const double* states, const double* inputs,
                       const double* jac, const double* g_states, const double* g_inputs, double* g_gains, double* g_x0, void* stream);
/* Closed-loop rollout under the tanh MLP (mcp_mlp_policy), ONE launch: mcp_rollout_pd with the descriptor exchanged -- the same step,
 * noise addressing, status flags (a NaN input raises MCP_STATUS_NAN; MCP_STATUS_NONPOS_VAR as there), T == 1 evaluates the policy only.
 * states [T][M][S]; inputs [T][M][U], row T - 1 included.  jac NULL: the plain launch; else the record [T-1][M][G][D] for
 * mcp_rollout_mlp_bwd.  The states carry the bits of mcp_rollout_open fed with the launch's own inputs[:T-1], and the plain launch those
 * of the recording launch.  The weights are copied to LDS (rows padded to an odd pitch) where they fit beside the step's layout, else read
 * from global memory.  MCP_ERR_ARG: a NULL pointer, M <= 0, T < 1, mlp->U != model->U, mlp->S != model->S, n_hidden outside 1..2, a
 * width < 1, an index out of range or listed twice, P != n_non_angle + 2 n_angle (P != S without lists), a missing layer pointer, a
 * u_max <= 0 with squash; MCP_ERR_LIMIT beyond MCP_MAX_* (P > MCP_MAX_PFEAT included) or MCP_MAX_HIDDEN; limits first, as for the PD law. */
int mcp_rollout_mlp(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_noise* noise, int M, int T, int particle_pred, const double* x0,
                    double* states, double* inputs, double* mu, double* var, double* jac /* NULL: no record */, uint32_t* status, void* stream);
/* Reverse-time sweep of mcp_rollout_mlp: g_states [T][M][S] (required) and g_inputs [T][M][U] (may be NULL) -> g_x0 [M][S] and
 * g_params [ceil(M/16)][n_param]: ONE PARTIAL SLAB PER WORKGROUP of 16 trajectories, laid out W0 | b0 | [W1 | b1] | Wout | bout (each
 * row-major as in the descriptor); the sum over the slabs is the caller's, in an order of its choosing.  No atomics, a fixed order of
 * sums: bitwise reproducible, and a slab depends on its own 16 trajectories alone.  Either output may be NULL; with both NULL the call
 * returns MCP_OK without a launch.  states, inputs, jac: what mcp_rollout_mlp wrote (jac may be NULL when T == 1).  Row T - 1 contributes
 * through g_inputs alone.  The activations are recomputed from states with the forward's own order of operations.  The argument checks of
 * the forward entry. */
int mcp_rollout_mlp_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, int M, int T, const double* states, const double* inputs,
                        const double* jac, const double* g_states, const double* g_inputs /* may be NULL */, double* g_params, double* g_x0,
                        void* stream);
/* mcp_rollout_pd with the PD law evaluated on a SIMULATED MEASUREMENT of the state (mcp_meas: noisy positions, backward-difference
 * velocities through the first-order filter; row 0 is measured true), ONE launch: the particles evolve on their true states,
 * e = target_traj[t] - y_t.  Per pair i (p = pos[i], v = vel[i]) and row t >= 1: np_t = x_t[p] + std_pos[i] n_{t,i}, nv_t = (np_t - np_{t-1}) / Ts,
 * y_t[v] = (b0 nv_t + b1 nv_{t-1} - a1 y_{t-1}[v]) / a0, y_t[p] = np_t; components in no pair are seen true.  n_{t,i} is
 * meas->pos_noise [T-1][M][n] (step t at row t - 1) or Philox by (seed, call, m + particle_offset) on the stream of mcp_rollout_fwd's
 * measurement model: a particle sees the same measurement noise whichever policy drives it.  meas->meas [T][M][S] receives y (every row;
 * a NaN in it raises MCP_STATUS_NAN) and is what mcp_rollout_pd_meas_bwd reads.  Ts is the model's (a delta-state model carries one for
 * this purpose alone).  Everything else -- states, inputs, jac, mu / var, eps addressing, status flags, T == 1 -- as mcp_rollout_pd; the
 * states carry the bits of mcp_rollout_open fed with the launch's own inputs, and the plain launch those of the recording launch.
 * meas->n == 0: mcp_rollout_pd itself (same kernels, same bits).  MCP_ERR_ARG beyond mcp_rollout_pd's: meas NULL, a pair index out of
 * range, pos or vel with a repeated entry, a component listed as both, n > 0 with meas->meas NULL, a0 == 0 or the model's Ts <= 0.
 * Replaces the loop of MC_PILCO4PMS.apply_policy (policy_learning/MC_PILCO.py:808-906) with PD_controller.forward
 * (policy_learning/Policy.py:437-449) over Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_pd_meas(const mcp_model* model, const mcp_pd_policy* pd, const mcp_meas* meas, const mcp_noise* noise, int M, int T,
                        int particle_pred, const double* x0, double* states, double* inputs, double* jac /* NULL: no record */, double* mu,
                        double* var, uint32_t* status, void* stream);
/* Reverse-time sweep of mcp_rollout_pd_meas: mcp_rollout_pd_bwd with the policy's adjoint taken on the measurement (meas->meas, as the
 * forward launch wrote it) and passed through the adjoint recursion of the filter -- two carries per (trajectory, pair), no atomics, no sum
 * across trajectories; g_gains [M][2][U] and g_x0 [M][S] as there.  meas->n == 0: mcp_rollout_pd_bwd itself.  The same argument checks as
 * the forward entry.  Replaces autograd's backward (MC_PILCO.py:522) through MC_PILCO4PMS.apply_policy's loop
 * (policy_learning/MC_PILCO.py:808-906), PD_controller.forward (policy_learning/Policy.py:437-449) and the integrators
 * (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_pd_meas_bwd(const mcp_model* model, const mcp_pd_policy* pd, const mcp_meas* meas, int M, int T, const double* states,
                            const double* inputs, const double* jac, const double* g_states, const double* g_inputs, double* g_gains,
                            double* g_x0, void* stream);
/* mcp_rollout_pd / mcp_rollout_pd_meas with the INTEGRAL TERM (mcp_pid_term: the law, its clamp and the derivative convention are stated
 * there), ONE launch.  meas NULL or n == 0: the law on the true state; else on the simulated measurement.  pid->integ [T][M][U] receives
 * I_t of every row.  Everything else -- states, inputs, jac, mu / var, noise addressing, status flags (a NaN gain or target row reaches
 * inputs and raises MCP_STATUS_NAN), T == 1, no ragged lengths -- as mcp_rollout_pd; the states carry the bits of mcp_rollout_open fed
 * with the launch's own inputs, and the plain launch those of the recording launch.  pid NULL or pid->on == 0: mcp_rollout_pd /
 * mcp_rollout_pd_meas on the same arguments (same kernels, same bits).  The checks of those entries in their order, then the term's:
 * sqrt_ki or integ NULL; dt not > 0 (a NaN included); an i_max[k], k < U, not > 0 (a NaN included; +inf is legal) -- each MCP_ERR_ARG.
 * Replaces a stateful torch policy (the reference has none) in the loop of MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674)
 * or MC_PILCO4PMS.apply_policy (:808-906) over Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_pid(const mcp_model* model, const mcp_pd_policy* pd, const mcp_pid_term* pid /* NULL or on == 0: no integral term */,
                    const mcp_meas* meas /* NULL or n == 0: the true state */, const mcp_noise* noise, int M, int T, int particle_pred,
                    const double* x0, double* states, double* inputs, double* jac /* NULL: no record */, double* mu, double* var,
                    uint32_t* status, void* stream);
/* Reverse-time sweep of mcp_rollout_pid: mcp_rollout_pd_bwd / mcp_rollout_pd_meas_bwd with the adjoint of the integral carried down the
 * rows (mcp_pid_term).  g_gains [M][3][U] = dJ/d(sqrt_kp, sqrt_kd, sqrt_ki) PER TRAJECTORY and g_x0 [M][S]; each may be NULL.  Reads
 * pid->integ as the forward launch wrote it.  No atomics: bitwise reproducible, a trajectory's results do not depend on the others.
 * pid NULL or pid->on == 0: mcp_rollout_pd_bwd / mcp_rollout_pd_meas_bwd on the same arguments, g_gains [M][2][U].  The same argument
 * checks as the forward entry.  Replaces autograd's backward (MC_PILCO.py:522) through the loops named there. */
int mcp_rollout_pid_bwd(const mcp_model* model, const mcp_pd_policy* pd, const mcp_pid_term* pid, const mcp_meas* meas, int M, int T,
                        const double* states, const double* inputs, const double* jac, const double* g_states, const double* g_inputs,
                        double* g_gains, double* g_x0, void* stream);
/* Closed-loop rollout under the time-varying linear feedback law (mcp_tvl_policy), ONE launch: mcp_rollout_pd / mcp_rollout_pd_meas with
 * the descriptor exchanged.  meas NULL or n == 0: the law on the true state; else on the simulated measurement (meas->meas [T][M][S]
 * receives y).  Everything else -- states, inputs (row T - 1 stored), jac, mu / var, noise addressing, status flags (a NaN input raises
 * MCP_STATUS_NAN), T == 1 evaluates the policy only, no ragged lengths -- as there; the states carry the bits of mcp_rollout_open fed
 * with the launch's own inputs[:T-1], and the plain launch (jac NULL) those of the recording launch.  Row t + 1 of gain, ff and the
 * target is brought into LDS while step t runs: nothing of the law is fetched from global memory between the step's barrier and u_t.
 * Limits first, as for the PD law: MCP_ERR_LIMIT beyond MCP_MAX_* (tvl->U, tvl->S included); MCP_ERR_ARG: a NULL required pointer,
 * M <= 0, T < 1, tvl->U / tvl->S not the model's, target_rows < T, gain_rows neither 1 nor >= T, ff_rows neither 0 nor >= T, ff_rows > 0
 * with ff NULL, a u_max <= 0 with squash, the measurement checks of mcp_rollout_pd_meas.  Replaces a torch policy in the loop of
 * MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674) or MC_PILCO4PMS.apply_policy (:808-906) over
 * Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_tvl(const mcp_model* model, const mcp_tvl_policy* tvl, const mcp_meas* meas /* NULL or n == 0: the true state */,
                    const mcp_noise* noise, int M, int T, int particle_pred, const double* x0, double* states, double* inputs,
                    double* jac /* NULL: no record */, double* mu, double* var, uint32_t* status, void* stream);
/* Reverse-time sweep of mcp_rollout_tvl: g_states [T][M][S] (required) and g_inputs [T][M][U] (may be NULL) -> g_x0 [M][S] and
 * g_part [ceil(M/16)][T][U][S+1]: ONE PARTIAL PER WORKGROUP of 16 trajectories and PER ROW -- columns 0 .. S - 1 are dJ/dgain[t][k][s],
 * column S is dJ/dff[t][k].  Every row 0 .. T - 1 of every slab is written (row T - 1 holds exact zeros when g_inputs is NULL; the absent
 * trajectories of a ragged last tile add nothing).  The sum over the slabs is the caller's, and so is the sum over the rows for a shared
 * gain.  No atomics; the 16 trajectories of a row are added in a fixed order: bitwise reproducible, and a slab depends on its own
 * trajectories alone.  Either output may be NULL; with both NULL the call returns MCP_OK without a launch.  states, inputs, jac: what
 * mcp_rollout_tvl wrote (jac may be NULL when T == 1); meas->meas as it wrote it.  The argument checks of the forward entry. */
int mcp_rollout_tvl_bwd(const mcp_model* model, const mcp_tvl_policy* tvl, const mcp_meas* meas, int M, int T, const double* states,
                        const double* inputs, const double* jac, const double* g_states, const double* g_inputs /* may be NULL */,
                        double* g_part, double* g_x0, void* stream);
/* mcp_rollout_mlp with the network evaluated on a SIMULATED MEASUREMENT of the state (mcp_meas, as mcp_rollout_pd_meas has it for the PD
 * law: noisy positions, backward-difference velocities through the first-order filter; row 0 is measured true), ONE launch: the particles
 * evolve on their true states, u_t = mlp(y_t).  Per pair i (p = pos[i], v = vel[i]) and row t >= 1: np_t = x_t[p] + std_pos[i] n_{t,i},
 * nv_t = (np_t - np_{t-1}) / Ts, y_t[v] = (b0 nv_t + b1 nv_{t-1} - a1 y_{t-1}[v]) / a0, y_t[p] = np_t; components in no pair are seen true.
 * n_{t,i} is meas->pos_noise [T-1][M][n] (step t at row t - 1) or Philox by (seed, call, m + particle_offset) on the stream of
 * mcp_rollout_fwd's measurement model: a particle sees the same measurement noise whichever policy drives it.  meas->meas [T][M][S] receives
 * y (every row; a NaN in it raises MCP_STATUS_NAN) and is what mcp_rollout_mlp_meas_bwd reads.  Ts is the model's.  Everything else --
 * states, inputs, jac, mu / var, eps addressing, status flags, T == 1, the weights' LDS copy -- as mcp_rollout_mlp; the states carry the bits
 * of mcp_rollout_open fed with the launch's own inputs[:T-1], and the plain launch those of the recording launch, meas->meas included.
 * meas->n == 0: mcp_rollout_mlp itself (same kernels, same bits).  Checks in this order: a NULL pointer (meas NULL included), M <= 0,
 * T < 1 -> MCP_ERR_ARG; MCP_MAX_* of the model -> MCP_ERR_LIMIT; the model; the descriptor as for mcp_rollout_mlp (its limits first); then
 * MCP_ERR_ARG for a pair index out of range, pos or vel with a repeated entry, a component listed as both, n > 0 with meas->meas NULL,
 * a0 == 0 (or NaN) or the model's Ts <= 0.  Replaces the loop of MC_PILCO4PMS.apply_policy (policy_learning/MC_PILCO.py:808-906; the
 * measurement :856-899) with Policy.MLP_policy over Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_mlp_meas(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_meas* meas, const mcp_noise* noise, int M, int T,
                         int particle_pred, const double* x0, double* states, double* inputs, double* mu, double* var,
                         double* jac /* NULL: no record */, uint32_t* status, void* stream);
/* Reverse-time sweep of mcp_rollout_mlp_meas: mcp_rollout_mlp_bwd with the activations recomputed from the measurement (meas->meas, as the
 * forward launch wrote it), the policy's adjoint taken on the measurement and passed through the adjoint recursion of the filter -- two
 * carries per (trajectory, pair), no atomics; g_params [ceil(M/16)][n_param] slabs and g_x0 [M][S] as there, bitwise reproducible, a slab
 * depending on its own 16 trajectories alone.  meas->n == 0: mcp_rollout_mlp_bwd itself.  The same argument checks as the forward entry
 * (the sweep looks at no GP operand).  Replaces autograd's backward (MC_PILCO.py:522) through MC_PILCO4PMS.apply_policy's loop
 * (policy_learning/MC_PILCO.py:808-906), Policy.MLP_policy and the integrators (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_mlp_meas_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_meas* meas, int M, int T, const double* states,
                             const double* inputs, const double* jac, const double* g_states, const double* g_inputs /* may be NULL */,
                             double* g_params, double* g_x0, void* stream);
/* mcp_rollout_mlp / mcp_rollout_mlp_meas with INVERTED DROPOUT on the hidden units, behind the activation (MC-PILCO's regulariser, which
 * the RBF policies have on their basis functions: mcp_policy.p_drop).  With s = 1 / (1 - p_drop):
 *   h_l[j] = keep[t][m][off_l + j] ? s tanh(pre_l[j]) : 0,   off_0 = 0, off_1 = h[0],   H = h[0] (+ h[1])
 * Features, the output layer and the squashing are never dropped.  One row of H decisions per policy evaluation: T rows, row T - 1
 * included.  noise->masks non-NULL: [T][M][H] keep-masks {0,1}, layer 0's units first; NULL: Philox by (seed, call, m + particle_offset, t)
 * on the stream of the RBF kernels' masks with the unit's index off_l + j in the basis function's place (a block of four may serve units of
 * both layers), kept where the word is >= p_drop 2^32: shard-invariant.  call_dev and particle_offset as everywhere.  meas NULL or
 * meas->n == 0: the network sees the true state.  Everything else -- outputs, status flags, T == 1, the tile ladder, the weights' LDS
 * copy -- as mcp_rollout_mlp_meas; the bit identities of mcp_rollout_mlp (mcp_rollout_open on the launch's own inputs; plain against
 * recording launch) hold.  p_drop == 0: the kernels of the entries without dropout on the same arguments, the same bits.  The argument
 * checks of mcp_rollout_mlp_meas in their order (a NULL meas allowed); p_drop outside [0, 1) or NaN is MCP_ERR_ARG, looked at with the
 * sizes -- before the limits. */
int mcp_rollout_mlp_drop(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_meas* meas /* NULL or n == 0: the true state */,
                         const mcp_noise* noise, double p_drop, int M, int T, int particle_pred, const double* x0, double* states, double* inputs,
                         double* mu, double* var, double* jac /* NULL: no record */, uint32_t* status, void* stream);
/* Reverse-time sweep of mcp_rollout_mlp_drop: mcp_rollout_mlp_meas_bwd with the forward's keep decisions, recomputed beside the
 * activations from the SAME noise descriptor (the mask buffer, or seed / call / particle_offset / call_dev) and p_drop: a dropped unit
 * passes no gradient, a kept one s (1 - tanh^2), to the parameter slabs and along the chain to g_x0 and the earlier rows alike.  g_params,
 * g_x0, the slab layout, reproducibility and the argument checks as there (a NULL meas allowed; p_drop as in the forward entry); noise may
 * be NULL only when p_drop == 0, which runs the kernels of the sweeps without dropout: the same bits. */
int mcp_rollout_mlp_drop_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_meas* meas, const mcp_noise* noise, double p_drop, int M,
                             int T, const double* states, const double* inputs, const double* jac, const double* g_states,
                             const double* g_inputs /* may be NULL */, double* g_params, double* g_x0, void* stream);
/* mcp_rollout_mlp_drop with TARGET-TRAJECTORY FEATURES (mcp_mlp_track): the network tracks -- in policy evaluation t it also sees the errors
 * target[t][idx[i]] - x_t[idx[i]], written behind the cosines (measured form: x is the simulated measurement y_t everywhere, errors
 * included: the network sees only the measurement).  mlp->P is the FULL feature width n_non_angle + 2 n_angle + track->n (without lists
 * S + track->n), at most MCP_MAX_PFEAT; W[0] is [h0][P], the error columns last.  Dropout, the output layer, the squashing, the noise
 * addressing, the status flags (a NaN in a target row reaches the inputs: MCP_STATUS_NAN), T == 1, the tile ladder and the weights' LDS
 * copy are mcp_rollout_mlp_drop's, and so are the bit identities (mcp_rollout_open on the launch's own inputs; plain against recording
 * launch).  track NULL or track->n == 0: mcp_rollout_mlp_drop itself on the same arguments (same kernels, same bits).  Checks in this
 * order: a NULL pointer, M <= 0, T < 1, p_drop -> MCP_ERR_ARG; MCP_MAX_* of the model -> MCP_ERR_LIMIT; the model -> MCP_ERR_ARG; the
 * descriptor's limits, track->n > MCP_MAX_STATE and P > MCP_MAX_PFEAT among them -> MCP_ERR_LIMIT; the descriptor's other errors, then
 * the track's -- n < 0, an idx entry out of range or repeated, rows < T, target NULL with n > 0, P != n_non_angle + 2 n_angle + n -- each
 * MCP_ERR_ARG; then the measurement's.  Replaces the loop of MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674; measured:
 * MC_PILCO4PMS.apply_policy, :808-906) with Policy.MLP_policy on the feature map of policy_learning/Policy.py:389-403 over
 * Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718). */
int mcp_rollout_mlp_track(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_track* track /* NULL or n == 0: no errors */,
                          const mcp_meas* meas /* NULL or n == 0: the true state */, const mcp_noise* noise, double p_drop, int M, int T,
                          int particle_pred, const double* x0, double* states, double* inputs, double* mu, double* var,
                          double* jac /* NULL: no record */, uint32_t* status, void* stream);
/* Reverse-time sweep of mcp_rollout_mlp_track: mcp_rollout_mlp_drop_bwd with the error features in the activation rows -- recomputed from
 * states (measured form: meas->meas) and target with the forward's statement, so g_W0 gets their columns through the same outer sums -- and
 * their pull on the state, lambda[idx[i]] -= fbar[n_non_angle + 2 n_angle + i] (measured form: the same term on the measurement, which
 * reaches the state through the filter's adjoint).  The parameter order and the slab layout are unchanged; n_param grows with P.  noise may
 * be NULL only when p_drop == 0.  track NULL or track->n == 0: mcp_rollout_mlp_drop_bwd itself.  The argument checks of the forward entry;
 * with neither output asked for MCP_OK without a launch.  Replaces autograd's backward (MC_PILCO.py:522) through the loops named above. */
int mcp_rollout_mlp_track_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_track* track, const mcp_meas* meas,
                              const mcp_noise* noise /* NULL ok iff p_drop == 0 */, double p_drop, int M, int T, const double* states,
                              const double* inputs, const double* jac, const double* g_states, const double* g_inputs /* may be NULL */,
                              double* g_params, double* g_x0, void* stream);
/* mcp_rollout_mlp_track with the PD TERM of mcp_mlp_pd added to the network's output ahead of the squashing (the residual policy
 * u = squash(PD(x, t) + net(x, t))): the RES forms of the tracking kernels -- the output threads read the two components of the row the
 * feature threads read (the state; measured form: the measurement y_t) and the two entries of res->target[t]; no barrier is added.  The
 * track (dropout, error features, measured form), the noise addressing, the status flags (a NaN gain or a NaN row of res->target reaches
 * the inputs: MCP_STATUS_NAN), T == 1, the tile ladder and the bit identities (mcp_rollout_open on the launch's own inputs; plain against
 * recording launch) are mcp_rollout_mlp_track's; track NULL or track->n == 0 is legal with the term (the network then sees no errors).
 * res NULL or res->on == 0: mcp_rollout_mlp_track itself on the same arguments (same kernels, same bits).  Checks in the order of
 * mcp_rollout_mlp_track up to and including the track's; then the residual's -- a pos / vel entry out of range, an entry repeated within
 * pos or within vel, sqrt_kp, sqrt_kd or target NULL, rows < T -- each MCP_ERR_ARG (more than MCP_MAX_INPUT inputs is already a limit of
 * the model); then the measurement's.  Replaces the loop of MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674; measured:
 * :808-906) with the sum of PD_controller.forward (policy_learning/Policy.py:406-449) and Policy.MLP_policy under one squashing. */
int mcp_rollout_mlp_res(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_track* track /* NULL or n == 0: no errors */,
                        const mcp_mlp_pd* res /* NULL or on == 0: no PD term */, const mcp_meas* meas /* NULL or n == 0: the true state */,
                        const mcp_noise* noise, double p_drop, int M, int T, int particle_pred, const double* x0, double* states,
                        double* inputs, double* mu, double* var, double* jac /* NULL: no record */, uint32_t* status, void* stream);
/* Reverse-time sweep of mcp_rollout_mlp_res: mcp_rollout_mlp_track_bwd with the PD term's pull on the state,
 *   lambda[pos[k]] -= sqrt_kp[k]^2 abar_k;   lambda[vel[k]] -= sqrt_kd[k]^2 abar_k      (measured form: the same pull on the measurement,
 *                                                                                         which reaches the state through the filter's adjoint)
 * and the gain gradients g_sqrt_kp[k] += 2 sqrt_kp[k] e[pos[k]] abar_k, g_sqrt_kd[k] += 2 sqrt_kd[k] e[vel[k]] abar_k, e = target[r] - x_r
 * (measured: y_r), abar the adjoint of the output layer's pre-activation; the network's deltas are unchanged.  With the term g_params is
 * [ceil(M / 16)][n_param + 2 U]: g_sqrt_kp [U] | g_sqrt_kd [U] behind bout in every slab, summed like the other entries (no atomics, a
 * fixed order, a slab from its own 16 trajectories alone, in parts where the layout asks for them).  The tail is written whenever g_params
 * is given (the descriptor has no switch for fixed gains: a caller with fixed gains ignores it); g_params NULL: nothing of it is computed.
 * res NULL or res->on == 0: mcp_rollout_mlp_track_bwd itself (slabs of n_param).  The argument checks of the forward entry. */
int mcp_rollout_mlp_res_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_track* track, const mcp_mlp_pd* res,
                            const mcp_meas* meas, const mcp_noise* noise /* NULL ok iff p_drop == 0 */, double p_drop, int M, int T,
                            const double* states, const double* inputs, const double* jac, const double* g_states,
                            const double* g_inputs /* may be NULL */, double* g_params, double* g_x0, void* stream);
/* mcp_rollout_mlp_res with MEMORY (mcp_mlp_hist): u_t = net(f_t) (+ the PD term), f_t the window of the last hist->h rows as stated at
 * mcp_mlp_hist -- newest block first, rows before 0 repeat row 0, the errors of the current row last; mlp->P = h P0 + track->n.  The HIST
 * forms of the residual kernels: per step the feature threads still compute ONE block, phi(r_t); the older blocks are the earlier steps'
 * block 0, moved one place down the feature row in LDS behind layer 0 (a thread per trajectory and column, no barrier added); at t = 0 the
 * feature threads write every block.  track NULL / n == 0, res NULL / on == 0 and p_drop == 0 are all legal; hist->h > 1 needs meas NULL
 * or meas->n == 0 (the true state): with an active measurement model the entry returns MCP_ERR_ARG.  Noise
 * addressing, inputs[T - 1], the status flags (a NaN anywhere in W[0] reaches the inputs: MCP_STATUS_NAN), T == 1, the tile ladder, the
 * weights' LDS copy and the bit identities (mcp_rollout_open on the launch's own inputs; plain against recording launch) are
 * mcp_rollout_mlp_res's.  hist NULL or hist->h == 1: mcp_rollout_mlp_res itself on the same arguments (same kernels, same bits).  Checks
 * in the order of mcp_rollout_mlp_res, the memory's with the descriptor's: hist->h > MCP_MAX_HIST or P > MCP_MAX_PFEAT is MCP_ERR_LIMIT
 * (with the descriptor's other limits, first); hist->h < 1 and P != h P0 + track->n are MCP_ERR_ARG; LAST, behind the track's, the PD term's
 * and the measurement's own checks (and in the sweep ahead of "nothing asked for"): hist->h > 1 with meas->n > 0 is MCP_ERR_ARG. */
int mcp_rollout_mlp_hist(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_hist* hist /* NULL or h == 1: no memory */,
                         const mcp_mlp_track* track /* NULL or n == 0: no errors */, const mcp_mlp_pd* res /* NULL or on == 0: no PD term */,
                         const mcp_meas* meas /* NULL or n == 0: the true state; n > 0 only with h == 1 */, const mcp_noise* noise,
                         double p_drop, int M, int T, int particle_pred, const double* x0, double* states, double* inputs, double* mu,
                         double* var, double* jac /* NULL: no record */, uint32_t* status, void* stream);
/* Reverse-time sweep of mcp_rollout_mlp_hist: mcp_rollout_mlp_res_bwd with the window in the activation rows (recomputed from rows
 * r .. r - h + 1 of states, clamped at 0, with the forward's functions: the forward's bits) and the ADJOINT of the window:
 * fbar = W0^T delta_1 has P columns; block j of row r pulls on row max(r - j, 0) through phi at that row, whose sines and cosines are
 * block j of row r's own activation row:   plain source i: fbar[j P0 + i];   angle source i: fbar[j P0 + nnp + i] cos - fbar[j P0 + nnp +
 * nap + i] sin.  The pulls of blocks j >= 1 are added, j ascending, into a ring pend[h][trajectory][S] in LDS at slot max(r - j, 0) mod h;
 * row r' adds slot r' mod h beside block 0's pull and clears it.  Row 0 collects every clamped block.  Slabs, g_x0, the gain gradients, the parts and the
 * fixed order of every sum as mcp_rollout_mlp_res_bwd.  hist NULL or hist->h == 1: mcp_rollout_mlp_res_bwd itself.  The argument checks
 * of the forward entry. */
int mcp_rollout_mlp_hist_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_hist* hist, const mcp_mlp_track* track,
                             const mcp_mlp_pd* res, const mcp_meas* meas, const mcp_noise* noise /* NULL ok iff p_drop == 0 */, double p_drop,
                             int M, int T, const double* states, const double* inputs, const double* jac, const double* g_states,
                             const double* g_inputs /* may be NULL */, double* g_params, double* g_x0, void* stream);
/* Reverse-time adjoint of the rollout: given dJ/dstates, dJ/dinputs (either may be NULL) returns
 * dJ/d{log_lengthscales [P], centers [B][P], f_linear.weight [U][B]} (overwritten, this rank's
 * particles only; with policy->bias also dJ/dbias into policy->g_bias) and optionally dJ/dx0 [M][S].  Replaces autograd's backward through
 * MC_PILCO.py:522. */
int mcp_rollout_bwd(const mcp_model* model, const mcp_policy* policy, const mcp_noise* noise, int M, int T,
                    const double* states, const double* inputs, const double* jac, const double* g_states,
                    const double* g_inputs, double* g_log_ls, double* g_centers, double* g_weight, double* g_x0,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- trajectory optimisation on the model: linearisation and the iLQR backward pass (the project's own: the reference has no
 * trajectory optimiser; mcp_tvl_policy is the controller these entries compute) --------------------------------------------------- */
#define MCP_LQR_MAX_T 2048 /* rows of one mcp_lqr_pass / mcp_linearize call: the pass keeps two doubles per row in LDS, within the 64 KiB a launch gets unasked */
/* Dense Jacobians of one model step along a recorded rollout: x_{t+1} ~ A_t dx + B_t da for t = 0 .. T - 2.  states [T][M][S] and jac
 * [T-1][M][G][D]: what mcp_rollout_open_rec (or a closed-loop recording launch) wrote -- the mean form's record is the nominal of the GP
 * mean model, a sampled form's has the sampling folded in.  A [T-1][M][S][S], B [T-1][M][S][U]; either may be NULL, both NULL: MCP_OK
 * without a launch.  With row J_g = jac[t][m][g], na = n_not_angle, z = [x[not_angle], sin x[angle], cos x[angle], u]:
 *   d delta_g / dx[not_angle[i]] = J_g[i];   d delta_g / dx[angle[j]] = J_g[na + j] cos x[angle[j]] - J_g[na + n_angle + j] sin x[angle[j]]
 *   d delta_g / du[k] = J_g[na + 2 n_angle + k]
 *   A = I + Ts E[not_vel[g], vel[g]] + sum_g (e_vel[g] + Ts/2 e_not_vel[g]) (d delta_g / dx)^T     (mcp_model's step maps; B alike, from d/du)
 * A row of a component that no GP integrates is zero, as the rollouts write that component.  du_da [T][M][U] (NULL: ones; row T - 1 is
 * not read) scales column k of B by du_da[t][m][k] -- the derivative of the squashing at the nominal, so that B refers to the pre-squash
 * variable a of mcp_tvl_policy.  The operations are those of mcp_model_step_bwd / mcp_rollout_open_bwd row by row: g^T A and g^T B agree
 * with those sweeps to rounding.  Only the model's index maps and Ts are read (no GP array).  MCP_ERR_ARG: model, states or jac NULL,
 * M <= 0, T < 2, a model whose scalars or index lists model_ok refuses; MCP_ERR_LIMIT: a dimension beyond MCP_MAX_*, T > MCP_LQR_MAX_T.
 * A refused call makes no HIP call.  Replaces torch.autograd.functional.jacobian through Model_learning.get_next_state
 * (model_learning/Model_learning.py:210-229, 471-494, 685-718), T - 1 times. */
int mcp_linearize(const mcp_model* model, int M, int T, const double* states, const double* jac, const double* du_da /* [T][M][U] or NULL = ones */,
                  double* A, double* B, void* stream);
/* The iLQR (Gauss-Newton) backward pass of M independent trajectories, ONE launch, one workgroup per trajectory.  states, jac, du_da as
 * for mcp_linearize (A_t and B_t are composed in LDS and never written).  lx [T][M][S], lu [T][M][U]: the stage cost's gradient along the
 * nominal; hxx [T][M][S], huu [T][M][U]: its DIAGONAL Hessians -- lu and huu in the pre-squash variable a (the caller's chain rule).
 * reg >= 0 is added to the diagonal of Quu.  gain [M][T][U][S] (slab m is an mcp_tvl_policy gain tensor), kff [M][T][U], dv [M][2]:
 *   row T - 1:  Vx = lx, Vxx = diag(hxx), gain = 0, kff = -lu / (huu + reg)
 *   row t = T - 2 .. 0:  Qx = lx + A^T Vx, Qu = lu + B^T Vx, Qxx = diag(hxx) + A^T Vxx A, Qux = B^T Vxx A,
 *     Quu = diag(huu) + B^T Vxx B + reg I = L L^T (Cholesky, its lower triangle read);  kff = -Quu^-1 Qu, gain = Quu^-1 Qux,
 *     Vx = Qx + Qux^T kff,  Vxx = (W + W^T) / 2 with W = Qxx - Qux^T gain
 *   dv[m] = (sum_t kff^T Qu, sum_t kff^T Quu kff), every row's term added in ascending t (row T - 1: Qu = lu, Quu = diag(huu + reg))
 * Sign convention: mcp_tvl_policy's law is a = gain (x* - x) + ff, so with x* the nominal states the update is ff <- a_nominal +
 * alpha kff and gain is used as written; the predicted change of the cost is alpha dv[0] + alpha^2 dv[1] / 2.
 * A pivot <= 0 (row T - 1: huu + reg <= 0) raises MCP_STATUS_NOT_SPD, a non-finite operand or pivot MCP_STATUS_NAN; that trajectory's
 * gain, kff and dv are then all NaN and the other trajectories are unaffected.  One thread per output element, every sum in index order,
 * no atomics on results: bitwise reproducible, and a trajectory's bits depend neither on M nor on the other trajectories.
 * MCP_ERR_ARG: a NULL pointer other than du_da, M <= 0, T < 2, reg negative or not finite (looked at with the sizes), a model as for
 * mcp_linearize; MCP_ERR_LIMIT as there.  A refused call makes no HIP call. */
int mcp_lqr_pass(const mcp_model* model, int M, int T, const double* states, const double* jac, const double* du_da /* [T][M][U] or NULL = ones */,
                 const double* lx, const double* lu, const double* hxx, const double* huu, double reg, double* gain, double* kff, double* dv,
                 uint32_t* status, void* stream);

/* ---- cost (policy_learning/Cost_function.py) ------------------------------------------ */
#define MCP_COST_CARTPOLE 0 /* cart_pole_cost, Cost_function.py:170-182                          */
#define MCP_COST_TRAJ 1     /* saturated_distance_from_trajectory, Cost_function.py:124-147      */
/* Target-state costs (Cost_function.py:39-101) over d = sum_i ((x[used[i]] - target[i]) / lengthscales[i])^2, i < n_used.
 * They reuse the trajectory cost's fields, with ONE difference: target_traj points at ONE row [n_used], indexed like
 * lengthscales (by position in `used`) and read at every t -- not MCP_COST_TRAJ's [T][S] rows indexed by state. */
#define MCP_COST_TARGET 2      /* saturated_distance_from_target: 1 - exp(-d)                    */
#define MCP_COST_TARGET_QUAD 3 /* distance_from_target: d                                        */
typedef struct mcp_cost {
  int32_t kind;
  int32_t S;
  int32_t angle_index, pos_index;       /* cart-pole                                    */
  double target_angle, target_pos;      /* target_state = [theta*, x*]                  */
  double ls_angle, ls_pos;              /* lengthscales = [l_theta, l_x]                */
  int32_t n_used;                       /* trajectory / target costs: used_indeces      */
  int32_t used[MCP_MAX_STATE];
  const double* target_traj;            /* [T][S]; MCP_COST_TARGET*: [n_used]           */
  const double* lengthscales;           /* [n_used]                                     */
} mcp_cost;
/* costs[t][m] = c(x_{t,m});  moments[t] = {mean_m c, sum_m (c-mean)^2} over THIS rank's M
 * particles (two-pass, as torch.mean/torch.std do; Cost_function.py:32-36). */
int mcp_cost_fwd(const mcp_cost* cost, int T, int M, const double* states, double* costs, double* moments, uint32_t* status,
                 void* stream);
/* Pools R ranks' moments [R][T][2] with counts[R] (host array) and writes out[0]=sum_t mean,
 * out[1]=sum_t unbiased std.  R==1 on a single GPU. */
int mcp_cost_finalize(int T, int R, const double* moments, const int64_t* counts, double* out, void* stream);
/* g_states[t][m][:] = (*g_cost) * gscale * d c/d x.  g_cost: DEVICE scalar with the upstream
 * gradient of the cost (NULL = 1), so no host synchronisation is needed; gscale = 1/M_total. */
int mcp_cost_bwd(const mcp_cost* cost, int T, int M, const double* states, const double* g_cost, double gscale, double* g_states,
                 void* stream);

/* Summable form of one rank's cost moments, for the SINGLE all-reduce of a particle-sharded step:
 * sums[t] = sum_m (c_tm - shift_t), sums[T+t] = sum_m (c_tm - shift_t)^2 over this rank's M particles, from the
 * moments of mcp_cost_fwd.  shift [T] (the same on every rank; NULL = 0; the previous step's pooled means are the
 * natural choice) keeps the pooled variance free of cancellation. */
int mcp_cost_sums(int T, int M, const double* moments, const double* shift, double* sums, void* stream);
/* sums [2T] added over all ranks (n_total particles) -> out[0] = sum_t mean_m c, out[1] = sum_t unbiased std_m c
 * (Cost_function.py:32-36 on the pooled swarm); mean_out [T] (optional) receives the pooled mean per time step. */
int mcp_cost_finalize_sums(int T, int64_t n_total, const double* sums, const double* shift, double* out, double* mean_out,
                           void* stream);

/* Control-effort and input-rate terms next to the state cost (the project's own extension: the reference's cost functions receive
 * inputs_sequence and ignore it).  With d_x the scaled state distance of `mcp_cost`, idx = used[0..n_used) (distinct) and
 *   d_u = sum_i ((u_t[idx[i]] - target[i]) / scales[i])^2                  (present when scales != NULL),
 *   d_r = sum_i ((u_t[idx[i]] - u_{t-1}[idx[i]]) / rate_scales[i])^2, t >= 1; 0 at t = 0   (present when rate_scales != NULL),
 *   f(d) = 1 - exp(-d)  (MCP_COST_CARTPOLE / _TRAJ / _TARGET),  f(d) = d  (MCP_COST_TARGET_QUAD):
 *   MCP_COST_U_ADD:   c = f(d_x) + d_u + d_r    (the penalty stays active where the state cost saturates)
 *   MCP_COST_U_JOINT: c = f(d_x + d_u + d_r)    (one saturated distance over states and inputs)
 * Row T-1 of the inputs takes part in both terms.  NULL descriptor, n_used == 0 or both scale pointers NULL: no input terms -- the
 * entries below run the kernels of mcp_cost_fwd / mcp_cost_bwd (the same bits) and `inputs` may be NULL. */
#define MCP_COST_U_ADD 0
#define MCP_COST_U_JOINT 1
typedef struct mcp_cost_inputs {
  int32_t U, mode, n_used;
  int32_t used[MCP_MAX_INPUT];
  const double* target;      /* [n_used] or NULL (= 0)            */
  const double* scales;      /* [n_used] l_i, or NULL: no effort  */
  const double* rate_scales; /* [n_used] r_i, or NULL: no rate    */
} mcp_cost_inputs;
/* costs[t][m] = c(x_{t,m}, u_{t,m}, u_{t-1,m}); moments and status as mcp_cost_fwd leaves them (mcp_cost_finalize, mcp_cost_sums and
 * mcp_cost_finalize_sums take them unchanged).  inputs [T][M][U].  Replaces the caller's torch ops of a generic
 * Expected_cost(lambda x, u, k: state_cost(x) + ((u - u*) / l)^2 + ((u_t - u_{t-1}) / r)^2) up to torch.mean / torch.std. */
int mcp_cost_u_fwd(const mcp_cost* cost, const mcp_cost_inputs* cin, int T, int M, const double* states, const double* inputs,
                   double* costs, double* moments, uint32_t* status, void* stream);
/* g_states[t][m][:] and g_inputs[t][m][:] = (*g_cost) * gscale * d(sum_t sum_m c)/d{x, u}_{t,m}: whole rows are written (zeros on the
 * components the cost does not read); the rate term couples u_t with u_{t-1} and u_{t+1} of the same particle, nothing else.  g_inputs
 * NULL: state gradient only; without input terms a g_inputs given is zero-filled on `stream` ([T][M][cin->U]: with a NULL descriptor its width
 * is unknown and it must be NULL).  No atomics: a particle's rows depend on
 * that particle alone.  Replaces autograd's backward through the torch ops named above; g_inputs is what the adjoint sweeps
 * (mcp_rollout_bwd, mcp_rollout_pd_bwd, mcp_rollout_mlp*_bwd, mcp_rollout_open_bwd) take as dJ/dinputs. */
int mcp_cost_u_bwd(const mcp_cost* cost, const mcp_cost_inputs* cin, int T, int M, const double* states, const double* inputs,
                   const double* g_cost, double gscale, double* g_states, double* g_inputs, void* stream);

/* Time-weighted, risk-sensitive objective over any of the costs above (the project's own extension: the reference minimises
 * sum_t mean_m c and only prints sum_t std_m c).  With mu_t / sigma_t the pooled mean / unbiased (n - 1) std over the n particles of the
 * swarm at step t:
 *   J = sum_t w_t (mu_t + kappa sigma_t)    (what is minimised; kappa > 0 cautious, kappa < 0 uncertainty-seeking: PILCO's cost.expl)
 *   S = sum_t w_t sigma_t                   (monitor; carries no gradient)
 *   dJ/dc_tm = w_t [1/n + kappa (c_tm - mu_t) / ((n - 1) sigma_t)]
 * -- unlike the reference's monitor, the kappa sigma term IS differentiated.  A row whose particles all have the same cost (sigma_t == 0,
 * e.g. t = 0 with a zero-variance x0) keeps the factor w_t / n: the sigma term of that row's gradient is dropped, where autograd through
 * torch.std gives NaN.  w: w_t >= 0, finite, not all zero (the caller's to ensure: it is device memory); kappa: any finite real;
 * kappa != 0 needs n >= 2 (MCP_ERR_ARG).  w == NULL, kappa == 0 is the plain expected cost. */
typedef struct mcp_objective {
  const double* w; /* DEVICE [T]; NULL: ones */
  double kappa;
} mcp_objective;
/* mcp_cost_finalize that also writes rows [T][2] = pooled (mean_t, unbiased std_t) and weights the sums: out[0] = J, out[1] = S.  The
 * same pooling over R ranks and the same reduction tree: obj NULL (= {NULL, 0}) gives mcp_cost_finalize's out, bit for bit. */
int mcp_cost_rows(int T, int R, const double* moments, const int64_t* counts, const mcp_objective* obj, double* rows, double* out,
                  void* stream);
/* mcp_cost_finalize_sums in the same way (the clamp of a negative variance and mean_out included). */
int mcp_cost_rows_sums(int T, int64_t n_total, const double* sums, const double* shift, const mcp_objective* obj, double* rows,
                       double* out, double* mean_out, void* stream);
/* g_states (and g_inputs, when cin has terms and g_inputs != NULL) of (*g_cost) * J for this process's M particles of a swarm of n_total
 * (n_total == M on one device).  costs: the [T][M] buffer mcp_cost_fwd / mcp_cost_u_fwd wrote (read, not recomputed); rows: from one of the
 * two calls above, of the WHOLE swarm (both are read only where kappa != 0, and must be given regardless).  cin NULL (or without terms): the state costs' gradient; g_inputs as for mcp_cost_u_bwd.  The
 * kernels are mcp_cost_bwd's / mcp_cost_u_bwd's with the scalar (*g_cost) * gscale replaced by (*g_cost) * dJ/dc_tm (gscale = 1 / n_total);
 * the rate term's neighbour factor a_{t+1} is built from dJ/dc_{t+1,m}.  obj NULL gives their bits.  One thread per (t, m), no atomics.
 * MCP_ERR_LIMIT: cin->U > MCP_MAX_INPUT;  MCP_ERR_ARG: a NULL pointer, T < 1, M < 1, n_total < M, a non-finite kappa, kappa != 0 with
 * n_total < 2, a bad descriptor. */
int mcp_cost_bwd_shaped(const mcp_cost* cost, const mcp_cost_inputs* cin, const mcp_objective* obj, int T, int M, int64_t n_total,
                        const double* states, const double* inputs, const double* costs, const double* rows, const double* g_cost,
                        double* g_states, double* g_inputs, void* stream);

/* ---- sampling MPC on the model: the MPPI rollout-cost and update (the project's own: the reference has no planner) -----------------
 * K candidate input sequences of H rows around a nominal a [H][U] (pre-squash), P model particles per candidate: trajectory m = k P + p,
 * M = K P.  Row t of trajectory m takes  u = squash(a[t] + sigma (.) xi(k, t, .)),  squash(v) = u_max tanh(v / u_max) (the closed-loop
 * kernels' own, mcp_pd_policy / mcp_tvl_policy) or v.  CANDIDATE 0 HAS xi = 0: the nominal is always among the candidates.  For k >= 1,
 * xi(k, t, u) = xi[(t K + k) U + u] from the buffer, or -- xi == NULL -- the standard normal of Philox stream MCP_STREAM_PLAN = 3
 * (csrc/mcp_device.h; streams 0..2: eps, masks, measurement noise) at (noise: seed, call, call_dev, particle_offset; particle = k, time
 * step t, index u): philox_normal(noise, k, t, u, MCP_STREAM_PLAN).  Nothing else of the perturbations is ever stored. */
#define MCP_MPPI_MAX_K 65536 /* candidates of one plan: the update's one workgroup walks them in a fixed order */
#define MCP_MPPI_MAX_M (1 << 30) /* K * P: trajectory indices (and a tile's past-the-end ones) stay inside an int32 */
typedef struct mcp_mppi {
  int32_t K, P, H;              /* candidates, particles per candidate, rows of the plan (H >= 2; H - 1 transitions) */
  int32_t U, squash;            /* inputs, == model->U; flg_squash                                                    */
  double u_max[MCP_MAX_INPUT];  /* > 0 with squash                                                                    */
  double sigma[MCP_MAX_INPUT];  /* >= 0, finite: std of the perturbation in the pre-squash variable a                 */
  double lambda;                /* temperature > 0, finite                                                            */
  double kappa;                 /* S_k = mean_p J + kappa * unbiased std_p J; != 0 needs P >= 2                        */
  int32_t t0;                   /* >= 0: row offset into the cost's target trajectory (receding horizon)              */
  const double* a;              /* DEVICE [H][U] nominal, pre-squash                                                  */
  const double* xi;             /* DEVICE [H][K][U] standard normals, or NULL: Philox                                 */
  const double* w;              /* DEVICE [H] time weights, or NULL: ones                                             */
} mcp_mppi;
/* Rolls the M = K P trajectories out from the ONE state x0 [S] through the model and reduces each to a single number, ONE launch:
 *   traj_cost[m] = sum_{t=0}^{H-1} w_t c(x_t, u_t, u_{t-1}),  added in ascending t from 0.0 in a register of the thread that owns m
 * with c = cost_u_point of (cost, cin) -- cost_point of cost where cin is NULL or has no terms -- evaluated at row t0 + t of the cost's
 * target (MCP_COST_TRAJ: target_traj must hold t0 + H rows); row H - 1 takes part and the rate term is 0 at t = 0, as in mcp_cost_u_fwd,
 * whose costs[t][m] these terms equal bit for bit.  The step is mcp_rollout_open's (csrc/rollout_open_phases.h: the same phases on the same
 * operands, the same tile ladder 16 -> 4 by LDS fit, one trajectory per workgroup in mean mode).  COMMON RANDOM NUMBERS: the GP
 * increment of trajectory m is drawn with particle id p = m mod P -- noise->eps is [H-1][P][G], Philox counts particle p +
 * particle_offset -- so every candidate meets the same model draws.  particle_pred bit 0 clear: the posterior-mean model (P may be 1, no
 * Kinv is read).  states [H][M][S] and inputs [H][M][U] are OPTIONAL (NULL: nothing of size [H][M] is written); inputs holds every row,
 * H - 1 included, and states carries the bits of mcp_rollout_open given those inputs (Mu == M) and the eps buffer repeated per
 * candidate; traj_cost does not depend on whether they are asked for.  status: MCP_STATUS_NAN for a non-finite state, input, GP moment
 * or trajectory cost, MCP_STATUS_NONPOS_VAR as mcp_rollout_open.  The nominal's H U doubles are kept in LDS.
 * MCP_ERR_ARG: model, mppi, mppi->a, cost, noise, x0, traj_cost or status NULL; K, P < 1 or H < 2; U != model->U (U < 1); lambda <= 0 or
 * not finite; a negative or non-finite sigma; u_max <= 0 with squash; kappa not finite, or != 0 with P < 2; t0 < 0; a model that model_ok
 * refuses; a bad cost descriptor (cin->U != U included).  MCP_ERR_LIMIT: a dimension beyond MCP_MAX_*, K > MCP_MPPI_MAX_K, K P >
 * MCP_MPPI_MAX_M, a plan whose rows do not fit the LDS beside the step's operands (H U > 20480 doubles is refused outright).  A refused call makes no HIP call.  Replaces, per
 * planning iteration, a torch materialisation of [H][M][U] inputs, mcp_rollout_open with Mu == M, mcp_cost_u_fwd and a sum over t. */
int mcp_mppi_rollout(const mcp_model* model, const mcp_mppi* mppi, const mcp_cost* cost, const mcp_cost_inputs* cin /* may be NULL */,
                     const mcp_noise* noise, int particle_pred, const double* x0, double* traj_cost, double* states /* or NULL */,
                     double* inputs /* or NULL */, uint32_t* status, void* stream);
/* The MPPI update from traj_cost [K P] (two launches, no atomics on results, no host synchronisation):
 *   cand_cost[k] = S_k = mean_p J + kappa std_p J   (J = traj_cost[k P + p]; the mean over ascending p, the unbiased std in two passes;
 *                                                    kappa == 0: the mean alone)
 *   S_min, argmin over the FINITE S_k (the lowest k among equals);  e_k = exp(-(S_k - S_min) / lambda), 0 for a non-finite S_k
 *   weights[k] = w_k = e_k / sum_k e_k;   a_new[t][u] = a[t][u] + sigma[u] sum_{k >= 1, w_k != 0} w_k xi(k, t, u)
 * with xi REGENERATED as above (candidate 0 contributes nothing).  stats [4] = S_min, argmin k (as a double), 1 / sum_k w_k^2 (the
 * effective sample size), sum_k w_k S_k over the finite candidates.  A non-finite S_k raises MCP_STATUS_NAN; if NO candidate is finite,
 * a_new = a, the weights are 0 and stats = NaN, -1, 0, NaN.  Every sum over k is taken by 256 threads, thread i adding k = i, i + 256, ...
 * in ascending order, then the 256 partial sums pairwise (i with i + 128, 64, ... 1): a fixed order, bitwise reproducible.
 * MCP_ERR_ARG: mppi, mppi->a, noise, traj_cost, a_new, cand_cost, weights, stats or status NULL, a_new == a, and the descriptor's refusals
 * above (U < 1 in place of U != model->U); MCP_ERR_LIMIT: U > MCP_MAX_INPUT, K > MCP_MPPI_MAX_K, K P > MCP_MPPI_MAX_M, H U > 20480 (a plan the
 * rollout cannot take).  A refused call
 * makes no HIP call.  Replaces torch's softmax over the candidates and an einsum over a [H][K][U] perturbation buffer. */
int mcp_mppi_update(const mcp_mppi* mppi, const mcp_noise* noise, const double* traj_cost, double* a_new /* [H][U], != a */,
                    double* cand_cost /* [K] */, double* weights /* [K] */, double* stats /* [4] */, uint32_t* status, void* stream);

/* ---- the planner's extension: a std per row, AR(1)-coloured perturbations, the input applied before row 0, the CEM update -------------
 * With n(k, t, u) the WHITE normal above (the xi buffer's entry, or the Philox normal), the perturbation of candidate k >= 1 is
 *   xi_0 = n_0,   xi_t = fma(beta, xi_{t-1}, c n_t),   c = sqrt(1 - beta^2) formed once on the host  (beta == 0: c == 1.0, xi_t has n_t's bits)
 * -- a xi buffer always holds the WHITE normals, the colouring happens in the kernels -- and row t takes
 *   u = squash(a[t] + s(t, .) (.) xi_t(k, .)),   s(t, u) = sigma_rows ? sigma_rows[t U + u] : mppi->sigma[u].
 * Candidate 0 keeps xi = 0.  The rows of sigma_rows live on the device: that they are >= 0 and finite is the CALLER's to check (ops.py does,
 * on the host values).  n_elite, alpha and sigma_min are read by mcp_cem_update alone. */
#define MCP_CEM_MAX_ELITE 1024 /* elites of one CEM update: they are sorted in the LDS of one workgroup */
typedef struct mcp_plan_ext {
  const double* sigma_rows;        /* DEVICE [H][U] std per row and input, or NULL: mppi->sigma for every row              */
  const double* u_prev;            /* DEVICE [U] post-squash input applied before row 0, or NULL (the rollout only)        */
  double beta;                     /* AR(1) coefficient in [0, 1); 0: white                                                */
  double alpha;                    /* CEM: smoothing in [0, 1) of mean and variance towards the previous ones              */
  double sigma_min[MCP_MAX_INPUT]; /* CEM: floor of the new std per input, >= 0 and finite                                 */
  int32_t n_elite;                 /* CEM: 1 .. min(K, MCP_CEM_MAX_ELITE)                                                  */
} mcp_plan_ext;
/* mcp_mppi_rollout under the extension: the same arguments with `ext` behind `mppi`.  ext NULL, or sigma_rows NULL, u_prev NULL and beta 0:
 * the call launches what mcp_mppi_rollout launches (the same kernel, rung and bits).  Otherwise the input threads of the same kernel read
 * s(t, u) from one more [H][U] block of LDS, carry xi in a register across the rows (still one row ahead of the step) and, with u_prev, the
 * rate term at t = 0 is taken against u_prev: c(x_0, u_0, u_prev) as mcp_cost_u_fwd forms row 1 of a run whose row 0 has u_prev as its
 * input.  Without a rate term u_prev changes no bit.  states carries mcp_rollout_open's bits given the launch's own inputs, as above.
 * Refusals in mcp_mppi_rollout's order; MCP_ERR_ARG also for beta outside [0, 1) (NaN included), MCP_ERR_LIMIT also for a plan whose
 * 2 H U + 2 PT U doubles do not fit the LDS beside the step's operands.  A refused call makes no HIP call. */
int mcp_plan_rollout(const mcp_model* model, const mcp_mppi* mppi, const mcp_plan_ext* ext /* may be NULL */, const mcp_cost* cost,
                     const mcp_cost_inputs* cin /* may be NULL */, const mcp_noise* noise, int particle_pred, const double* x0,
                     double* traj_cost, double* states /* or NULL */, double* inputs /* or NULL */, uint32_t* status, void* stream);
/* mcp_mppi_update under the extension: a_new[t][u] = a[t][u] + s(t, u) sum_{k >= 1, w_k != 0} w_k xi_t(k, u).  The sum is linear in n: the
 * weighted sums N_t[u] = sum_k w_k n(k, t, u) are formed per row exactly as mcp_mppi_update forms them, then ONE thread per input runs the
 * filter X_0 = N_0, X_t = fma(beta, X_{t-1}, c N_t) over the rows and a_new = a + s X (three launches; nothing is regenerated twice).
 * Weights, cand_cost, stats and status as mcp_mppi_update.  ext NULL, or sigma_rows NULL and beta 0 (u_prev is not read): mcp_mppi_update
 * itself, bit for bit.  Refusals as mcp_mppi_update, MCP_ERR_ARG also for beta outside [0, 1) and a_new == sigma_rows. */
int mcp_mppi_update_ext(const mcp_mppi* mppi, const mcp_plan_ext* ext /* may be NULL */, const mcp_noise* noise, const double* traj_cost,
                        double* a_new /* [H][U], != a */, double* cand_cost /* [K] */, double* weights /* [K] */, double* stats /* [4] */,
                        uint32_t* status, void* stream);
/* The CEM update from traj_cost [K P] around the nominal mppi->a and the current std s(t, u) of ext (two launches, no host
 * synchronisation, no atomics on floating-point results; mppi->lambda is checked and not read):
 *   cand_cost[k] = S_k as mcp_mppi_update forms it (kappa included); a non-finite S_k is never elite and raises MCP_STATUS_NAN
 *   the elites: the E' = min(n_elite, #finite) candidates with the smallest (S_k, k) -- ties go to the lower k, -0.0 == 0.0 --;
 *   elite[r], r < E', in that order (int32; -1 for E' <= r < n_elite).  Candidate 0 competes like any other and contributes xi = 0.
 *   One workgroup: a radix select on the 80-bit composite (order-preserving key of S_k, k), then a sort of the E' survivors in LDS.
 *   with xi regenerated for the elites alone (coloured as above):
 *     m[t][u] = (1 / E') sum_r xi_t(elite[r], u),   v[t][u] = (1 / E') sum_r (xi_t(elite[r], u) - m[t][u])^2   (two passes)
 *     a_new = alpha a + (1 - alpha) (a + s m),   sigma_new = max(sigma_min[u], sqrt(alpha s^2 + (1 - alpha) s^2 v))
 *   every sum over r: thread i adds the ranks i, i + 256, ... in ascending order, then the 256 partial sums pairwise as mcp_mppi_update's.
 *   The chains of a thread's at most four ranks live in registers across the rows: there is no workspace.
 * stats [4] = S_min, argmin k (= elite[0]), E', the mean cost of the elites.  No finite candidate: a_new = a, sigma_new = s, elite all -1,
 * stats = NaN, -1, 0, NaN.  MCP_ERR_ARG: a NULL pointer (ext included), the sizes of mcp_mppi_update, n_elite < 1; then MCP_ERR_LIMIT: its
 * limits, n_elite > MCP_CEM_MAX_ELITE, n_elite > K; then MCP_ERR_ARG: its values, beta or alpha outside [0, 1), a negative or non-finite
 * sigma_min[u < U], an output that is mppi->a, sigma_rows or the other output.  A refused call makes no HIP call.  Replaces torch's topk, a
 * gather from a [H][K][U] perturbation buffer and mean / var over the elites. */
int mcp_cem_update(const mcp_mppi* mppi, const mcp_plan_ext* ext, const mcp_noise* noise, const double* traj_cost, double* a_new /* [H][U] */,
                   double* sigma_new /* [H][U] */, double* cand_cost /* [K] */, int32_t* elite /* [n_elite] */, double* stats /* [4] */,
                   uint32_t* status, void* stream);

/* ---- the batched planner: B independent plans in the launches of one ----------------------------------------------------------------
 * B problems of the SAME shape (K, P, H, U), model, cost, time weights, t0, sigma, lambda, kappa and extension scalars, each with its own
 * start state, nominal and -- under the extension -- std rows and u_prev.  Batched operands are problem-major: mppi->a is [B][H][U],
 * ext->sigma_rows (when given) [B][H][U], ext->u_prev (when given) [B][U], every output carries a leading B.
 * THE CONTRACT: problem b's slice of every output carries the bits of the single-problem entry (mcp_plan_rollout, mcp_mppi_update_ext,
 * mcp_cem_update -- and through them the plain ones when ext is default) called on problem b's operands with
 * noise->particle_offset + b * particle_stride and the b-th xi / eps buffer.  status[b] receives problem b's flags alone; a problem with a
 * non-finite x0 or without a finite candidate keeps its nominal (and its CEM std) and reports stats NaN, -1, 0, NaN as the single-problem
 * entries do, and changes no bit of any other problem.
 * The rollout runs on a grid of (ceil(K P / PT), B) workgroups -- a tile never spans two problems; the tile ladder and the LDS fit rules
 * are the single-problem ones --, the weights / select / filter kernels on B workgroups, the mean kernel on (H, B), the CEM fit on (U, B):
 * the summation orders inside a problem are the single-problem kernels'. */
#define MCP_PLAN_MAX_B 4096
typedef struct mcp_plan_batch {
  int32_t B;                /* problems, 1 .. MCP_PLAN_MAX_B; B K P <= MCP_MPPI_MAX_M                                           */
  int32_t x0_per_particle;  /* 0: x0 is [B][S];  1: x0 is [B][P][S], trajectory m = k P + p of problem b starts at x0[b][p]     */
  int64_t particle_stride;  /* >= 0: problem b draws BOTH Philox streams (plan perturbations, particle id k; model increments,
                               particle id p) as the single-problem entry does with noise->particle_offset + b * particle_stride */
  int64_t xi_stride;        /* doubles between the problems' mppi->xi buffers: 0 (one [H][K][U] buffer for all) or >= H K U     */
  int64_t eps_stride;       /* the same for noise->eps: 0 or >= (H-1) P G                                                       */
} mcp_plan_batch;
/* mcp_plan_rollout for B problems in ONE launch.  x0: [B][S] or [B][P][S] (batch->x0_per_particle); traj_cost [B][K P]; states
 * [B][H][K P][S] and inputs [B][H][K P][U] optional; status uint32 [B].  MCP_ERR_ARG: a NULL pointer (batch included), B < 1, a negative
 * particle_stride, a non-zero xi_stride / eps_stride below the buffer's size, and every refusal of mcp_plan_rollout; MCP_ERR_LIMIT:
 * B > MCP_PLAN_MAX_B, B K P > MCP_MPPI_MAX_M and the limits of mcp_plan_rollout -- in that entry's one order (pointers; sizes; limits;
 * values; the LDS fit last).  A refused call makes no HIP call. */
int mcp_plan_batch_rollout(const mcp_model* model, const mcp_mppi* mppi, const mcp_plan_ext* ext /* may be NULL */, const mcp_plan_batch* batch,
                           const mcp_cost* cost, const mcp_cost_inputs* cin /* may be NULL */, const mcp_noise* noise, int particle_pred,
                           const double* x0, double* traj_cost, double* states /* or NULL */, double* inputs /* or NULL */, uint32_t* status,
                           void* stream);
/* mcp_mppi_update_ext for B problems: traj_cost [B][K P] -> a_new [B][H][U], cand_cost [B][K], weights [B][K], stats [B][4], status [B]
 * (two launches, three under sigma_rows or beta != 0).  batch->eps_stride and x0_per_particle are not read.  Refusals: the batch's as
 * above, then mcp_mppi_update_ext's. */
int mcp_plan_batch_update(const mcp_mppi* mppi, const mcp_plan_ext* ext /* may be NULL */, const mcp_plan_batch* batch, const mcp_noise* noise,
                          const double* traj_cost, double* a_new, double* cand_cost, double* weights, double* stats, uint32_t* status,
                          void* stream);
/* mcp_cem_update for B problems: a_new and sigma_new [B][H][U], cand_cost [B][K], elite int32 [B][n_elite], stats [B][4], status [B] (two
 * launches).  Refusals: the batch's as above, then mcp_cem_update's. */
int mcp_cem_batch_update(const mcp_mppi* mppi, const mcp_plan_ext* ext, const mcp_plan_batch* batch, const mcp_noise* noise,
                         const double* traj_cost, double* a_new, double* sigma_new, double* cand_cost, int32_t* elite, double* stats,
                         uint32_t* status, void* stream);

/* ---- the optimizer loop's bookkeeping on the device (MC_PILCO.reinforce_policy, policy_learning/MC_PILCO.py:475-607) ----------
 * The reference decides on the host, from torch.isnan(cost), whether a rollout counts, and so reads every step's cost back before
 * it can launch the next one.  These two entry points take the same decisions from device memory after each ATTEMPT (rollout +
 * cost + adjoint sweep), so the host may enqueue the next attempt at once and read the outcome (a small record) one attempt late:
 *   - an attempt FAILS when its cost is NaN (or flags / status say so: hand-off time-out, non-positive variance): nothing is
 *     updated, the next attempt is the retry (:479-501: "Cost is NaN: try sampling again", at most MCP_OPT_MAX_ATTEMPTS);
 *   - it is VOID while the loop waits for the host: after the tenth failure in a row (re-initialisation, :573-607), after the
 *     lr / exit condition fired (`pending`, :540-567), after step n_steps;
 *   - otherwise it COUNTS: parameters updated, cost_list / std_list [step] written, the cost-difference monitors advanced
 *     (ES1, ES2, diff_cost_ratio, :503-519), step += 1.
 * mcp_opt_state lives in device memory, zero-initialised (+ cost_prev = the warm-up cost, :462) by the caller; the caller resets
 * it (memset on the stream) when it builds a new optimizer or re-initialises the policy. */
#define MCP_OPT_MAX_ATTEMPTS 10
#define MCP_OPT_MAX_TENSORS 32
#define MCP_OPT_RECORD_DOUBLES 12
typedef struct mcp_opt_state {
  int64_t step;           /* optimizer steps taken since the last (re-)initialisation = next index of cost_list            */
  int64_t attempt;        /* failed attempts of the current step                                                          */
  int64_t pending;        /* 1: the lr / exit condition fired at the last counted attempt; cleared by the host            */
  int64_t adam_t;         /* steps of the CURRENT optimizer (Adam's bias correction); the host zeroes it with a new one   */
  int64_t total_attempts; /* every attempt seen, whatever became of it                                                    */
  double es2;             /* ES2_diff_cost                                                                                */
  double cost_prev;       /* cost_tm1                                                                                     */
} mcp_opt_state;
/* torch.optim.Adam's update (weight_decay 0, no amsgrad) of up to MCP_OPT_MAX_TENSORS parameter tensors in ONE launch, applied only
 * when the attempt counts (state == NULL: always, as step number `step` >= 1 of the optimizer -- GP training, where the host knows it;
 * with a state the step number is state->adam_t + 1).  params / grads / exp_avg / exp_avg_sq: HOST arrays of n_tensors device pointers,
 * numel their sizes; a NULL grad skips that tensor.  Must be enqueued BEFORE mcp_policy_step_commit of the same attempt (it reads
 * the state that call advances).  Without a state, a non-NULL `status` whose MCP_STATUS_NOT_SPD bit is set skips the update (GP
 * training: the epoch's Cholesky failed; the bit is sticky, so the parameters stay those of the last good epoch).
 * Replaces optimizer.step(), MC_PILCO.py:525 and GP_prior.py:209. */
int mcp_adam_step_guarded(int n_tensors, double* const* params, const double* const* grads, double* const* exp_avg,
                          double* const* exp_avg_sq, const int64_t* numel, double lr, double beta1, double beta2, double eps,
                          const mcp_opt_state* state, int64_t step, int n_steps, const double* cost, const double* flags,
                          const uint32_t* status, void* stream);
/* The loop's decisions for one attempt.  cost / std_cost: device scalars of the attempt; flags: optional device [3] doubles (> 0 =
 * NaN cost, hand-off time-out, non-positive variance -- the all-reduced form of a particle-sharded step), status: optional device
 * status word of the rollout (either or both may be NULL; a NaN cost always fails).  cost_list / std_list [n_steps], es1 / ratio
 * [n_steps + 1] (zero-initialised).  record (optional, device, MCP_OPT_RECORD_DOUBLES): [counted, void, step, attempts failed so
 * far, pending, cost, std, |ratio|, nan, time-out, non-positive variance, total attempts] for the host to read late. */
int mcp_policy_step_commit(mcp_opt_state* state, int n_steps, const double* cost, const double* std_cost, const double* flags,
                           const uint32_t* status, double* cost_list, double* std_list, double* es1, double* ratio,
                           double alpha_diff_cost, double min_step, double min_diff_cost, int num_min_diff_cost, double* record,
                           void* stream);

/* ---- particle sharding: the one collective of an optimizer step --------------------------
 * The reference is single-process (no collective anywhere); sharding the particles over the GPUs of a node adds ONE
 * exchange between `cost.backward()` and `optimizer.step()` (policy_learning/MC_PILCO.py:522-525): an in-place
 * all-reduce(sum) of the flat fp64 message [dJ/dlog_lengthscales | dJ/dcenters | dJ/dweight | mcp_cost_sums (2T) | flags].
 * Thin wrapper over RCCL (bound at run time; MCP_ERR_COMM when it cannot be loaded), ONE communicator per process created
 * once by mcp_comm_init and reused by every step.  Rank 0 obtains `id` (MCP_COMM_ID_BYTES) from mcp_comm_unique_id and
 * the host distributes it to the other ranks (any side channel: torch.distributed's store, MPI, a file). */
#define MCP_COMM_ID_BYTES 128
int mcp_comm_unique_id(void* id_out);
int mcp_comm_init(int world, int rank, const void* id);
int mcp_comm_world(void); /* 0 when no communicator exists */
int mcp_allreduce_grad(double* flat, size_t n, void* stream);
int mcp_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* MCPILCO_HIP_H */
