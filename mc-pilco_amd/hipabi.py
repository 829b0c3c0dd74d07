"""ctypes binding of libmcpilco_hip.so -- the C ABI declared in include/mcpilco_hip.h.

The library is the product's only compute path: if it is missing or does not load, importing
this module's ``lib()`` raises (there is no CPU fallback anywhere in the package).
PyTorch is used for device memory and streams only: tensors are passed as ``data_ptr()``
and launches go to ``torch.cuda.current_stream()``.
"""
import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmcpilco_hip.so")

MAX_GP, MAX_STATE, MAX_INPUT, MAX_GPDIM, MAX_PFEAT, MAX_BASIS, MAX_TRAIN = 8, 16, 8, 32, 32, 1024, 4096
MAX_BASIS_WIDE = 512  # B of a wide policy (P > 16 or U > 4): MCP_MAX_BASIS_WIDE
MAX_HIDDEN = 64  # units of a hidden layer of mcp_mlp_policy: MCP_MAX_HIDDEN
MAX_HIST = 4  # rows a policy with memory reads (mcp_mlp_hist.h): MCP_MAX_HIST
LQR_MAX_T = 2048  # rows of one mcp_lqr_pass / mcp_linearize call: MCP_LQR_MAX_T
MPPI_MAX_K = 65536  # candidates of one plan (mcp_mppi.K): MCP_MPPI_MAX_K
MPPI_MAX_M = 1 << 30  # trajectories of one plan (mcp_mppi.K * P): MCP_MPPI_MAX_M
CEM_MAX_ELITE = 1024  # elites of one CEM update (mcp_plan_ext.n_elite): MCP_CEM_MAX_ELITE
PLAN_MAX_B = 4096  # problems of one batched plan (mcp_plan_batch.B): MCP_PLAN_MAX_B
OK = 0
ERRORS = {-1: "MCP_ERR_ARG", -2: "MCP_ERR_LIMIT", -3: "MCP_ERR_WORKSPACE", -4: "MCP_ERR_LAUNCH", -5: "MCP_ERR_COMM"}
ABI_VERSION = 7
COMM_ID_BYTES = 128
STATUS_NAN, STATUS_NONPOS_VAR, STATUS_NOT_SPD, STATUS_SYNC = 1, 2, 4, 8
FWD_NO_GP_SHARDING = 2  # flag in mcp_rollout_fwd's particle_pred argument (MCP_FWD_NO_GP_SHARDING)
FWD_KT_PACKED, FWD_XJ_PACKED = 4, 8  # the workspace still holds the packed operand copies of an earlier call on the same model (MCP_FWD_*_PACKED)
POLICY_PLAIN, POLICY_ANGLES, POLICY_TRAJ = 0, 1, 2
COST_CARTPOLE, COST_TRAJ, COST_TARGET, COST_TARGET_QUAD = 0, 1, 2, 3
COST_U_ADD, COST_U_JOINT = 0, 1  # mcp_cost_inputs.mode: f(d_x) + d_u + d_r / f(d_x + d_u + d_r)

dptr = C.c_void_p


class Kernel(C.Structure):
    _fields_ = [("D", C.c_int32), ("poly_deg", C.c_int32), ("lam", C.c_double), ("sigma_n2", C.c_double), ("mean", C.c_double),
                ("inv_ls", dptr), ("w1", dptr), ("w20", dptr), ("w21", dptr), ("scal", dptr)]


class GP(C.Structure):
    _fields_ = [("kern", Kernel), ("N", C.c_int32), ("Npad", C.c_int32), ("Xt", dptr), ("X", dptr), ("alpha", dptr), ("Kinv", dptr),
                ("aX", dptr)]


class Model(C.Structure):
    _fields_ = [("S", C.c_int32), ("U", C.c_int32), ("G", C.c_int32), ("D", C.c_int32), ("n_angle", C.c_int32),
                ("n_not_angle", C.c_int32), ("angle", C.c_int32 * MAX_STATE), ("not_angle", C.c_int32 * MAX_STATE),
                ("vel", C.c_int32 * MAX_GP), ("not_vel", C.c_int32 * MAX_GP), ("Ts", C.c_double), ("var_scale", C.c_double * MAX_GP),
                ("gp", GP * MAX_GP)]


class Meas(C.Structure):
    _fields_ = [("n", C.c_int32), ("pos", C.c_int32 * MAX_STATE), ("vel", C.c_int32 * MAX_STATE), ("std_pos", C.c_double * MAX_STATE),
                ("b0", C.c_double), ("b1", C.c_double), ("a0", C.c_double), ("a1", C.c_double), ("pos_noise", dptr), ("meas", dptr)]


class Policy(C.Structure):
    _fields_ = [("kind", C.c_int32), ("S", C.c_int32), ("P", C.c_int32), ("B", C.c_int32), ("U", C.c_int32), ("squash", C.c_int32),
                ("n_angle", C.c_int32), ("n_non_angle", C.c_int32), ("angle", C.c_int32 * MAX_STATE),
                ("non_angle", C.c_int32 * MAX_STATE), ("traj_len", C.c_int32), ("p_drop", C.c_double), ("log_ls", dptr),
                ("centers", dptr), ("weight", dptr), ("u_max", dptr), ("target_traj", dptr), ("bias", dptr), ("g_bias", dptr), ("meas", Meas)]


class Noise(C.Structure):
    _fields_ = [("eps", dptr), ("masks", dptr), ("seed", C.c_uint64), ("call", C.c_uint64), ("particle_offset", C.c_int64), ("call_dev", dptr)]


class PDPolicy(C.Structure):
    _fields_ = [("U", C.c_int32), ("squash", C.c_int32), ("pos", C.c_int32 * MAX_INPUT), ("vel", C.c_int32 * MAX_INPUT),
                ("u_max", C.c_double * MAX_INPUT), ("sqrt_kp", dptr), ("sqrt_kd", dptr), ("target_traj", dptr), ("target_rows", C.c_int32)]


class MLPPolicy(C.Structure):
    _fields_ = [("S", C.c_int32), ("U", C.c_int32), ("P", C.c_int32), ("n_hidden", C.c_int32), ("h", C.c_int32 * 2), ("n_angle", C.c_int32),
                ("n_non_angle", C.c_int32), ("angle", C.c_int32 * MAX_STATE), ("non_angle", C.c_int32 * MAX_STATE), ("squash", C.c_int32),
                ("u_max", C.c_double * MAX_INPUT), ("W", dptr * 3), ("b", dptr * 3)]


class MLPTrack(C.Structure):
    """mcp_mlp_track: the error features target[t][idx[i]] - x[idx[i]] of the tracking entries, behind the cosines (n == 0: none)."""
    _fields_ = [("n", C.c_int32), ("idx", C.c_int32 * MAX_STATE), ("rows", C.c_int32), ("target", dptr)]


class MLPResidual(C.Structure):
    """mcp_mlp_pd: the PD term sqrt_kp[k]^2 e[pos[k]] + sqrt_kd[k]^2 e[vel[k]], e = target[t] - x, added to the network's output ahead of
    the squashing by the residual entries (on == 0: none)."""
    _fields_ = [("on", C.c_int32), ("pos", C.c_int32 * MAX_INPUT), ("vel", C.c_int32 * MAX_INPUT), ("sqrt_kp", dptr), ("sqrt_kd", dptr),
                ("target", dptr), ("rows", C.c_int32)]


class MLPHist(C.Structure):
    """mcp_mlp_hist: the network reads the features of the last h rows, newest block first (rows before 0 repeat row 0); h == 1: no memory."""
    _fields_ = [("h", C.c_int32)]


class PIDTerm(C.Structure):
    """mcp_pid_term: the clamped integral I_t = clamp(I_{t-1} + dt e[pos[k]], +-i_max[k]) of the position error and its product
    sqrt_ki[k]^2 I_t[k] behind the PD law's two, of the integral entries (on == 0: none); integ [T][M][U] is written by the rollout and read
    by the sweep."""
    _fields_ = [("on", C.c_int32), ("sqrt_ki", dptr), ("i_max", C.c_double * MAX_INPUT), ("dt", C.c_double), ("integ", dptr)]


class TVLPolicy(C.Structure):
    """mcp_tvl_policy: the time-varying linear feedback law a_t = gain[t] (target[t] - r_t) + ff[t] (gain_rows == 1: one matrix for all
    rows; ff_rows == 0: no feedforward)."""
    _fields_ = [("U", C.c_int32), ("S", C.c_int32), ("squash", C.c_int32), ("gain_rows", C.c_int32), ("ff_rows", C.c_int32),
                ("target_rows", C.c_int32), ("u_max", C.c_double * MAX_INPUT), ("gain", dptr), ("ff", dptr), ("target_traj", dptr)]


class OptState(C.Structure):
    _fields_ = [("step", C.c_int64), ("attempt", C.c_int64), ("pending", C.c_int64), ("adam_t", C.c_int64), ("total_attempts", C.c_int64),
                ("es2", C.c_double), ("cost_prev", C.c_double)]


OPT_MAX_ATTEMPTS, OPT_MAX_TENSORS, OPT_RECORD_DOUBLES = 10, 32, 12


class NllGP(C.Structure):
    _fields_ = [("log_ls", dptr), ("log_lambda", dptr), ("sigma_n_log", dptr), ("mean", dptr), ("mpk1", dptr), ("mpk2", dptr), ("Y", dptr),
                ("y_scale", C.c_double), ("sigma_n_num2", C.c_double), ("g_log_ls", dptr), ("g_log_lambda", dptr), ("g_sigma_n_log", dptr),
                ("g_mean", dptr), ("g_mpk1", dptr), ("g_mpk2", dptr), ("loss", dptr)]


class Cost(C.Structure):
    _fields_ = [("kind", C.c_int32), ("S", C.c_int32), ("angle_index", C.c_int32), ("pos_index", C.c_int32),
                ("target_angle", C.c_double), ("target_pos", C.c_double), ("ls_angle", C.c_double), ("ls_pos", C.c_double),
                ("n_used", C.c_int32), ("used", C.c_int32 * MAX_STATE), ("target_traj", dptr), ("lengthscales", dptr)]


class CostInputs(C.Structure):
    """mcp_cost_inputs: the control-effort and input-rate terms next to a state cost (scales NULL: no effort; rate_scales NULL: no rate)."""
    _fields_ = [("U", C.c_int32), ("mode", C.c_int32), ("n_used", C.c_int32), ("used", C.c_int32 * MAX_INPUT), ("target", dptr),
                ("scales", dptr), ("rate_scales", dptr)]


class Objective(C.Structure):
    """mcp_objective: the time weights (device [T]; NULL: ones) and the risk parameter kappa of J = sum_t w_t (mean_t + kappa std_t)."""
    _fields_ = [("w", dptr), ("kappa", C.c_double)]


class MPPI(C.Structure):
    """mcp_mppi: K candidates x P model particles over H rows around the pre-squash nominal ``a`` [H][U]; u = squash(a + sigma xi), xi from the
    buffer [H][K][U] or (NULL) from Philox stream 3; S_k = mean_p J + kappa std_p J, weights exp(-(S_k - S_min) / lambda)."""
    _fields_ = [("K", C.c_int32), ("P", C.c_int32), ("H", C.c_int32), ("U", C.c_int32), ("squash", C.c_int32),
                ("u_max", C.c_double * MAX_INPUT), ("sigma", C.c_double * MAX_INPUT), ("lam", C.c_double), ("kappa", C.c_double),
                ("t0", C.c_int32), ("a", dptr), ("xi", dptr), ("w", dptr)]


class PlanExt(C.Structure):
    """mcp_plan_ext: the planner's extension -- a std per row (``sigma_rows`` [H][U], NULL: mcp_mppi.sigma), the AR(1) coefficient ``beta`` of
    the perturbations, the input applied before row 0 (``u_prev`` [U], NULL: none), and what the CEM update alone reads: ``n_elite``, the
    smoothing ``alpha``, the std's floor ``sigma_min`` per input."""
    _fields_ = [("sigma_rows", dptr), ("u_prev", dptr), ("beta", C.c_double), ("alpha", C.c_double), ("sigma_min", C.c_double * MAX_INPUT),
                ("n_elite", C.c_int32)]


class PlanBatch(C.Structure):
    """mcp_plan_batch: B problems of one shape in the launches of one plan -- ``x0_per_particle`` (x0 [B][P][S] instead of [B][S]), the Philox
    particle ids of problem b shifted by b * ``particle_stride``, the doubles between the problems' xi / eps buffers (0: one shared buffer)."""
    _fields_ = [("B", C.c_int32), ("x0_per_particle", C.c_int32), ("particle_stride", C.c_int64), ("xi_stride", C.c_int64),
                ("eps_stride", C.c_int64)]


class Dispatch(C.Structure):
    """include/mcpilco_hip_debug.h: struct mcp_dispatch -- the request a call carries (all zero = automatic) and what it reports back."""
    _fields_ = [("fwd_particles", C.c_int32), ("gp_sharding", C.c_int32), ("fwd_lean", C.c_int32), ("policy_split", C.c_int32), ("row_split", C.c_int32),
                ("cluster_map", C.c_int32), ("fwd_no_xlds", C.c_int32),
                ("fwd_gb", C.c_int32), ("bwd_particles", C.c_int32), ("bwd_lean", C.c_int32), ("bwd_pipe", C.c_int32), ("stamp_block", C.c_uint32),
                ("fwd_stamps", dptr), ("bwd_stamps", dptr), ("ran_particles", C.c_int32), ("ran_gp_sharded", C.c_int32), ("ran_fwd_lean", C.c_int32),
                ("ran_bwd_lean", C.c_int32), ("ran_row_split", C.c_int32), ("ran_bwd_pipe", C.c_int32)]


class FwdPlan(C.Structure):
    """include/mcpilco_hip_debug.h: struct mcp_fwd_plan -- what mcp_rollout_fwd_plan answers (the launch plan of a forward call)."""
    _fields_ = [(k, C.c_int32) for k in ("family", "particles", "xlds", "gb", "ncmax", "lds_bytes", "npad_max", "maxdeg", "launches", "particles_per_launch",
                                         "gsh_cs", "gsh_rs", "gsh_map", "policy_split", "ws_xch", "ws_xj", "ws_kt", "ws_uxch", "ws_rxch", "ws_total", "use_xj", "use_kt", "zero_xch", "zero_uxch", "zero_rxch", "pack_kt",
                                         "pack_xj", "ran_particles", "ran_gp_sharded", "ran_fwd_lean", "ran_row_split")]


class BwdPlan(C.Structure):
    """include/mcpilco_hip_debug.h: struct mcp_bwd_plan -- what mcp_rollout_bwd_plan answers."""
    _fields_ = [(k, C.c_int32) for k in ("lean", "pfm", "um", "maxnt", "particles", "threads", "pipe", "launches", "slabs", "ran_bwd_lean", "ran_bwd_pipe")]


class NllPlan(C.Structure):
    """include/mcpilco_hip_debug.h: struct mcp_nll_plan -- what mcp_nll_epoch_plan answers (workspace map in doubles, gradient form)."""
    _fields_ = [(k, C.c_int64) for k in ("first_gp", "per_gp", "total", "K", "Uinv", "Kinv", "alpha", "r", "slab", "grad", "inv_ls", "w1", "w20", "w21",
                                         "scal", "logdet", "grad_form", "rows_per_wg", "slab_rows", "lds_bytes")]


NLL_GRAD_ROWS, NLL_GRAD_ROW_PER_WG = 1, 2  # mcp_nll_plan.grad_form
FWD_SMALL_SHARDED, FWD_LEAN, FWD_TILE_SHARDED, FWD_TILE, FWD_SMALL = 1, 2, 3, 4, 5  # mcp_fwd_plan.family

# The dispatch request of THIS PROCESS's calls through `ops` (all zero: automatic).  It lives here, in the host layer -- the library keeps no
# dispatch state; tests and tools set its fields through the `mcp_debug_*` methods of `lib()` (the names the library itself exported until
# round 4), every `ops` call passes it along and finds in it what ran.
DISPATCH = Dispatch()

_SIGS = {
    "mcp_abi_version": (C.c_int, []),
    "mcp_build_info": (C.c_char_p, []),
    "mcp_cov_build": (C.c_int, [C.POINTER(Kernel), C.c_int, dptr, C.c_int, dptr, C.c_int, dptr, C.c_int, dptr]),
    "mcp_cov_diag": (C.c_int, [C.POINTER(Kernel), C.c_int, dptr, C.c_int, dptr, dptr]),
    "mcp_chol_factor": (C.c_int, [C.c_int, dptr, C.c_int, dptr, dptr, dptr]),
    "mcp_chol_inverse": (C.c_int, [C.c_int, dptr, C.c_int, dptr, C.c_int, dptr, C.c_int, dptr]),
    "mcp_sym_sandwich": (C.c_int, [C.c_int, dptr, C.c_int, dptr, C.c_int, dptr, C.c_int, dptr, dptr]),
    "mcp_gp_alpha": (C.c_int, [C.c_int, dptr, C.c_int, dptr, C.c_double, dptr, dptr]),
    "mcp_sod_workspace_bytes": (C.c_size_t, [C.c_int]),
    "mcp_sod_select": (C.c_int, [C.POINTER(Kernel), C.c_int, dptr, C.c_double, dptr, dptr, dptr, C.c_size_t, dptr]),
    "mcp_nll_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mcp_nll_grad": (C.c_int, [C.POINTER(Kernel), C.c_int, dptr, dptr, C.c_int, dptr, dptr, dptr, C.c_size_t, dptr]),
    "mcp_gp_pack": (C.c_int, [C.c_int, C.c_int, dptr, dptr, dptr, C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_posterior_fwd": (C.c_int, [C.POINTER(GP), C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_posterior_fwd_ex": (C.c_int, [C.POINTER(GP), C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, C.POINTER(Dispatch)]),
    "mcp_posterior_bwd": (C.c_int, [C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_workspace_bytes": (C.c_size_t, [C.POINTER(Model), C.POINTER(Policy), C.c_int, C.c_int]),
    "mcp_rollout_fwd": (C.c_int, [C.POINTER(Model), C.POINTER(Policy), C.POINTER(Noise), C.c_int, C.c_int, C.c_int, dptr, dptr, dptr,
                                  dptr, dptr, dptr, C.c_size_t, dptr]),
    "mcp_rollout_open": (C.c_int, [C.POINTER(Model), C.POINTER(Noise), C.c_int, C.c_int, C.c_int, dptr, dptr, C.c_int, dptr, dptr, dptr, dptr,
                                   dptr, dptr]),
    "mcp_rollout_open_rec": (C.c_int, [C.POINTER(Model), C.POINTER(Noise), C.c_int, C.c_int, C.c_int, dptr, dptr, C.c_int, dptr, dptr, dptr, dptr,
                                       dptr, dptr, dptr]),
    "mcp_rollout_open_bwd": (C.c_int, [C.POINTER(Model), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_model_step": (C.c_int, [C.POINTER(Model), C.POINTER(Noise), C.c_int, C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_model_step_bwd": (C.c_int, [C.POINTER(Model), C.c_int, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_pd": (C.c_int, [C.POINTER(Model), C.POINTER(PDPolicy), C.POINTER(Noise), C.c_int, C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr,
                                 dptr, dptr, dptr]),
    "mcp_rollout_pd_bwd": (C.c_int, [C.POINTER(Model), C.POINTER(PDPolicy), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_mlp": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(Noise), C.c_int, C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr,
                                  dptr, dptr, dptr]),
    "mcp_rollout_mlp_bwd": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_pd_meas": (C.c_int, [C.POINTER(Model), C.POINTER(PDPolicy), C.POINTER(Meas), C.POINTER(Noise), C.c_int, C.c_int, C.c_int, dptr, dptr,
                                      dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_pd_meas_bwd": (C.c_int, [C.POINTER(Model), C.POINTER(PDPolicy), C.POINTER(Meas), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr,
                                          dptr, dptr]),
    "mcp_rollout_pid": (C.c_int, [C.POINTER(Model), C.POINTER(PDPolicy), C.POINTER(PIDTerm), C.POINTER(Meas), C.POINTER(Noise), C.c_int, C.c_int,
                                  C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_pid_bwd": (C.c_int, [C.POINTER(Model), C.POINTER(PDPolicy), C.POINTER(PIDTerm), C.POINTER(Meas), C.c_int, C.c_int, dptr, dptr, dptr,
                                      dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_tvl": (C.c_int, [C.POINTER(Model), C.POINTER(TVLPolicy), C.POINTER(Meas), C.POINTER(Noise), C.c_int, C.c_int, C.c_int, dptr, dptr,
                                  dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_tvl_bwd": (C.c_int, [C.POINTER(Model), C.POINTER(TVLPolicy), C.POINTER(Meas), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr,
                                      dptr, dptr]),
    "mcp_linearize": (C.c_int, [C.POINTER(Model), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_lqr_pass": (C.c_int, [C.POINTER(Model), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, C.c_double, dptr, dptr, dptr, dptr,
                               dptr]),
    "mcp_rollout_mlp_meas": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(Meas), C.POINTER(Noise), C.c_int, C.c_int, C.c_int, dptr, dptr,
                                       dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_mlp_meas_bwd": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(Meas), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr,
                                           dptr, dptr, dptr]),
    "mcp_rollout_mlp_drop": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(Meas), C.POINTER(Noise), C.c_double, C.c_int, C.c_int,
                                       C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_mlp_drop_bwd": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(Meas), C.POINTER(Noise), C.c_double, C.c_int, C.c_int,
                                           dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_mlp_track": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(MLPTrack), C.POINTER(Meas), C.POINTER(Noise), C.c_double,
                                        C.c_int, C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_mlp_track_bwd": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(MLPTrack), C.POINTER(Meas), C.POINTER(Noise),
                                            C.c_double, C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_mlp_res": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(MLPTrack), C.POINTER(MLPResidual), C.POINTER(Meas),
                                      C.POINTER(Noise), C.c_double, C.c_int, C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_mlp_res_bwd": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(MLPTrack), C.POINTER(MLPResidual), C.POINTER(Meas),
                                          C.POINTER(Noise), C.c_double, C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_rollout_mlp_hist": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(MLPHist), C.POINTER(MLPTrack), C.POINTER(MLPResidual),
                                       C.POINTER(Meas), C.POINTER(Noise), C.c_double, C.c_int, C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr,
                                       dptr, dptr]),
    "mcp_rollout_mlp_hist_bwd": (C.c_int, [C.POINTER(Model), C.POINTER(MLPPolicy), C.POINTER(MLPHist), C.POINTER(MLPTrack), C.POINTER(MLPResidual),
                                           C.POINTER(Meas), C.POINTER(Noise), C.c_double, C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr,
                                           dptr, dptr]),
    "mcp_rollout_bwd":(C.c_int, [C.POINTER(Model), C.POINTER(Policy), C.POINTER(Noise), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr,
                                  dptr, dptr, dptr, dptr, dptr, C.c_size_t, dptr]),
    "mcp_rollout_fwd_ex": (C.c_int, [C.POINTER(Model), C.POINTER(Policy), C.POINTER(Noise), C.c_int, C.c_int, C.c_int, dptr, dptr, dptr,
                                     dptr, dptr, dptr, C.c_size_t, dptr, C.POINTER(Dispatch)]),
    "mcp_rollout_bwd_ex": (C.c_int, [C.POINTER(Model), C.POINTER(Policy), C.POINTER(Noise), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr,
                                     dptr, dptr, dptr, dptr, dptr, C.c_size_t, dptr, C.POINTER(Dispatch)]),
    "mcp_rollout_fwd_plan": (C.c_int, [C.POINTER(Model), C.POINTER(Policy), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(Dispatch),
                                       C.POINTER(FwdPlan)]),
    "mcp_rollout_bwd_plan": (C.c_int, [C.POINTER(Model), C.POINTER(Policy), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(Dispatch),
                                       C.POINTER(BwdPlan)]),
    "mcp_cost_fwd": (C.c_int, [C.POINTER(Cost), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr]),
    "mcp_cost_finalize": (C.c_int, [C.c_int, C.c_int, dptr, C.POINTER(C.c_int64), dptr, dptr]),
    "mcp_cost_bwd": (C.c_int, [C.POINTER(Cost), C.c_int, C.c_int, dptr, dptr, C.c_double, dptr, dptr]),
    "mcp_cost_u_fwd": (C.c_int, [C.POINTER(Cost), C.POINTER(CostInputs), C.c_int, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_cost_u_bwd": (C.c_int, [C.POINTER(Cost), C.POINTER(CostInputs), C.c_int, C.c_int, dptr, dptr, dptr, C.c_double, dptr, dptr, dptr]),
    "mcp_cost_sums": (C.c_int, [C.c_int, C.c_int, dptr, dptr, dptr, dptr]),
    "mcp_cost_finalize_sums": (C.c_int, [C.c_int, C.c_int64, dptr, dptr, dptr, dptr, dptr]),
    "mcp_cost_rows": (C.c_int, [C.c_int, C.c_int, dptr, C.POINTER(C.c_int64), C.POINTER(Objective), dptr, dptr, dptr]),
    "mcp_cost_rows_sums": (C.c_int, [C.c_int, C.c_int64, dptr, dptr, C.POINTER(Objective), dptr, dptr, dptr, dptr]),
    "mcp_cost_bwd_shaped": (C.c_int, [C.POINTER(Cost), C.POINTER(CostInputs), C.POINTER(Objective), C.c_int, C.c_int, C.c_int64, dptr, dptr,
                                      dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_mppi_rollout": (C.c_int, [C.POINTER(Model), C.POINTER(MPPI), C.POINTER(Cost), C.POINTER(CostInputs), C.POINTER(Noise), C.c_int, dptr, dptr,
                                   dptr, dptr, dptr, dptr]),
    "mcp_mppi_update": (C.c_int, [C.POINTER(MPPI), C.POINTER(Noise), dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_plan_rollout": (C.c_int, [C.POINTER(Model), C.POINTER(MPPI), C.POINTER(PlanExt), C.POINTER(Cost), C.POINTER(CostInputs), C.POINTER(Noise),
                                   C.c_int, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_mppi_update_ext": (C.c_int, [C.POINTER(MPPI), C.POINTER(PlanExt), C.POINTER(Noise), dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_cem_update": (C.c_int, [C.POINTER(MPPI), C.POINTER(PlanExt), C.POINTER(Noise), dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_plan_batch_rollout": (C.c_int, [C.POINTER(Model), C.POINTER(MPPI), C.POINTER(PlanExt), C.POINTER(PlanBatch), C.POINTER(Cost),
                                         C.POINTER(CostInputs), C.POINTER(Noise), C.c_int, dptr, dptr, dptr, dptr, dptr, dptr]),
    "mcp_plan_batch_update": (C.c_int, [C.POINTER(MPPI), C.POINTER(PlanExt), C.POINTER(PlanBatch), C.POINTER(Noise), dptr, dptr, dptr, dptr, dptr,
                                        dptr, dptr]),
    "mcp_cem_batch_update": (C.c_int, [C.POINTER(MPPI), C.POINTER(PlanExt), C.POINTER(PlanBatch), C.POINTER(Noise), dptr, dptr, dptr, dptr, dptr,
                                       dptr, dptr, dptr]),
    "mcp_adam_step_guarded": (C.c_int, [C.c_int, C.POINTER(dptr), C.POINTER(dptr), C.POINTER(dptr), C.POINTER(dptr), C.POINTER(C.c_int64), C.c_double,
                                        C.c_double, C.c_double, C.c_double, dptr, C.c_int64, C.c_int, dptr, dptr, dptr, dptr]),
    "mcp_nll_epoch_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mcp_nll_epoch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, dptr, dptr, dptr, C.c_size_t, dptr]),
    "mcp_nll_epoch_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(NllPlan)]),
    "mcp_policy_step_commit": (C.c_int, [dptr, C.c_int, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr, C.c_double, C.c_double, C.c_double, C.c_int,
                                         dptr, dptr]),
    "mcp_comm_unique_id": (C.c_int, [C.c_char_p]),
    "mcp_comm_init": (C.c_int, [C.c_int, C.c_int, C.c_char_p]),
    "mcp_comm_world": (C.c_int, []),
    "mcp_allreduce_grad": (C.c_int, [dptr, C.c_size_t, dptr]),
    "mcp_comm_destroy": (C.c_int, []),
}
PLAN_QUERIES = ("mcp_rollout_fwd_plan", "mcp_rollout_bwd_plan", "mcp_nll_epoch_plan")
EXPORTED_DEBUG = [k for k in _SIGS if k.endswith("_ex") or k in PLAN_QUERIES]  # include/mcpilco_hip_debug.h
EXPORTED = [k for k in _SIGS if k not in EXPORTED_DEBUG]                       # include/mcpilco_hip.h

_lib = None


def lib():
    """The loaded library; raises RuntimeError when it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libmcpilco_hip.so is missing (%s): build it with `python mc-pilco_amd/build.py` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(handle, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if handle.mcp_abi_version() != ABI_VERSION:
            raise RuntimeError("libmcpilco_hip.so ABI version mismatch")
        _lib = _Lib(handle)
    return _lib


class _Lib:
    """The loaded library plus the `mcp_debug_*` names as HOST-SIDE accessors of DISPATCH (what the library exported as process-wide setters
    until round 4): tests and tools keep their calls, the state they set is this module's, and it reaches the kernels with each call."""

    def __init__(self, handle):
        self._h = handle

    def __getattr__(self, name):
        return getattr(self._h, name)

    # forward rollout: particles per workgroup 1 / 2 / 4 / 16, 0 = automatic
    def mcp_debug_set_particles_per_wg(self, p):
        DISPATCH.fwd_particles = int(p)

    def mcp_debug_last_particles_per_wg(self):
        return int(DISPATCH.ran_particles)

    def mcp_debug_set_bwd_particles(self, pb):
        DISPATCH.bwd_particles = int(pb)

    def mcp_debug_set_stamp_buffer(self, p):
        DISPATCH.fwd_stamps = p

    def mcp_debug_set_stamp_block(self, b):
        DISPATCH.stamp_block = max(0, int(b))

    def mcp_debug_set_fwd_mode(self, xlds, gb):  # xlds 0: never stage the small operands in LDS; gb: GPs per pass (0 = as many as fit)
        DISPATCH.fwd_no_xlds = 1 if int(xlds) == 0 else 0
        DISPATCH.fwd_gb = int(gb)

    def mcp_debug_set_bwd_stamp_buffer(self, p):
        DISPATCH.bwd_stamps = p

    def mcp_debug_last_bwd_pipe(self):
        return int(DISPATCH.ran_bwd_pipe)

    def mcp_debug_set_bwd_pipe(self, mode):  # -1 / 1 wherever it applies, 0 never
        DISPATCH.bwd_pipe = 1 if int(mode) == 0 else 0

    def mcp_debug_set_gp_sharding(self, mode):  # -1 automatic, 0 never, 1 whenever the grid fits the device
        DISPATCH.gp_sharding = {-1: 0, 0: 1, 1: 2}[int(mode)]

    def mcp_debug_set_policy_split(self, mode):  # -1 automatic, 0 off, 1 whenever the shape allows
        DISPATCH.policy_split = {-1: 0, 0: 1, 1: 2}[int(mode)]

    def mcp_debug_set_row_split(self, mode):  # -1 automatic, 0 off, 1 / 2 two row parts whenever the shape allows, 3 three
        DISPATCH.row_split = {-1: 0, 0: 1, 1: 2, 2: 2, 3: 3}[int(mode)]

    def mcp_debug_set_cluster_map(self, mode):  # -1 automatic, 0 the workgroups of a tile on one XCD, 1 row part major
        DISPATCH.cluster_map = {-1: 0, 0: 1, 1: 2}[int(mode)]

    def mcp_debug_last_row_split(self):
        return int(DISPATCH.ran_row_split)

    def mcp_debug_last_gp_sharded(self):
        return int(DISPATCH.ran_gp_sharded)

    def mcp_debug_set_fwd_lean(self, mode):  # -1 / 1 wherever it applies, 0 never
        DISPATCH.fwd_lean = 1 if int(mode) == 0 else 0

    def mcp_debug_last_fwd_lean(self):
        return int(DISPATCH.ran_fwd_lean)

    def mcp_debug_set_bwd_lean(self, mode):  # -1 automatic, 0 never
        DISPATCH.bwd_lean = 1 if int(mode) == 0 else 0

    def mcp_debug_last_bwd_lean(self):
        return int(DISPATCH.ran_bwd_lean)


def check(rc, what):
    if rc != OK:
        raise RuntimeError("%s failed: %s" % (what, ERRORS.get(rc, rc)))


def ptr(t):
    """Device pointer of a contiguous CUDA(HIP) tensor, or None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libmcpilco_hip operates on GPU memory only (got a %s tensor); there is no CPU path" % t.device)
    if not t.is_contiguous():
        raise RuntimeError("non-contiguous tensor passed to the HIP ABI")
    return C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """The current HIP stream of the current device (every launch goes there).  Through torch's raw-handle getter where this build has
    it: ``torch.cuda.current_stream()`` builds a Stream object per call, ~11 us -- 3-5 of them per optimizer step / training epoch."""
    if _raw_stream is not None and _cur_device is not None:
        return C.c_void_p(_raw_stream(_cur_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f64(t, device):
    return torch.as_tensor(t, dtype=torch.float64).to(device).contiguous()
