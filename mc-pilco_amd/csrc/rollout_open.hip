// Fused rollouts for gfx950 (MI355X) whose inputs do not come out of the RBF policy, and their reverse-time sweeps.  M trajectories are
// advanced T steps through an mcp_model in ONE launch; the forms differ in where the input of step t comes from and in what is kept:
//   open loop          mcp_rollout_open         u_t is read from a buffer (the inputs recorded on the system)
//   recording          mcp_rollout_open_rec     the same, and the Jacobians of the increments are recorded for mcp_rollout_open_bwd
//   feedback           mcp_rollout_pd           u_t is the PD law on x_t (struct OpenArgsPd); with jac the record for mcp_rollout_pd_bwd
//   measured feedback  mcp_rollout_pd_meas      the PD law on a simulated measurement of x_t (struct OpenArgsPdMeas); mcp_rollout_pd_meas_bwd
//   integral feedback  mcp_rollout_pid          either feedback form with a clamped integral of the position error in the law (struct
//                                               OpenArgsPid); mcp_rollout_pid_bwd
//   time-varying law   mcp_rollout_tvl          either feedback form with a dense gain row and a feedforward per step in the PD law's place
//                                               (struct OpenArgsTvl); mcp_rollout_tvl_bwd
// All forward forms are one kernel template, rollout_open_kernel<PT, MAXDEG, NEEDVAR, NEEDJAC, FB, PMS, PID, TVL>, the sweeps one,
// rollout_open_bwd_kernel<FB, PMS, PID, TVL>.  The host path is the same for every entry point: checks (rollout_common.h: model_within_limits,
// model_ok / model_lists_ok, meas_model_check -- for the closed loops in closed_loop_checks' one order; here: pd_policy_check), one fill of
// the arguments' base part per direction (open_fill, open_bwd_fill over sweep_fill_model), one ladder of tiles (launch_open_tiles) -- a refused call makes no HIP call.
//
// The open-loop form replaces the step loop of MC_PILCO.rollout (policy_learning/MC_PILCO.py:347-373) over Model_learning.get_next_state
// (model_learning/Model_learning.py:210-229, 685-718; GP_prior.get_estimate_from_alpha, GP_prior.py:137-155): per step G posterior
// launches plus indexing, concatenation and a Normal(...).rsample() -- here no workspace, no hand-off between workgroups.  Without a
// record a step is three phases:
//
//   K   k[j][p] = k(z_p, X_j)          thread j, all particles of the tile; the weighted distance in the reference's own expanded form
//                                      |z/l|^2 + |X_j/l|^2 - 2 sum_d (z_d/l_d^2) X_jd (Stationary_GP.py:65-109), as in the closed-loop
//                                      kernels: the open-loop check then rounds like the model the policy is optimised on; the
//                                      posterior mean sum_j alpha_j k_j is accumulated on the way (wave sums, one LDS slot per wave)
//   V   q_p = k_p^T Kinv k_p           only when a variance is needed (sampling, or the caller asks for it):
//                                      v_mfma_f64_16x16x4_f64, A = 32 x 4 panel of Kinv (one 16-byte load per lane feeds the even / odd
//                                      row MFMAs), B = k[j..j+3][particles] from LDS; 32-row blocks are dealt to the 8 waves, the
//                                      product v = Kinv k is never stored: every lane multiplies its accumulators by k and sums
//   F   mu, var, sample, integrate     thread (particle, state component); the thread of a position recomputes its GP's increment
//                                      (same operations, same bits) instead of waiting for the velocity's thread
//
// Mean mode without variances touches no Kinv: one workgroup per trajectory, X^T and alpha of every GP in LDS where they fit, two
// workgroup barriers per step.  With variances a workgroup owns a tile of 16 trajectories so that Kinv is streamed once per step for
// all of them; the k panel ([Npad][16] doubles) must fit the LDS, so beyond ~1000 training points the tile shrinks to 4 (fits up to
// MCP_MAX_TRAIN).  Phase K walks X^T once per group of 4 trajectories of the tile (register budget of the polynomial terms).
//
// The RECORDING form (template NEEDJAC, mcp_rollout_open_rec) also writes jac [T-1][M][G][D] = d delta_g / dz with the sampling folded
// in -- layout and meaning of the closed-loop kernels' record (mcp_rollout_fwd) -- for the reverse-time sweep at the end of this file
// (rollout_open_bwd_kernel, mcp_rollout_open_bwd).  Phases K, V and F are the same instructions in both forms (the library is built
// without floating-point contraction), so the states carry the same bits; the recording form adds
//   V'  v = Kinv k is KEPT: a second [Npad][pitch] panel next to k (where the two do not fit, the tile shrinks 16 -> 4 -> 1)
//   J   R_c = [X^T; 1] W_c  on v_mfma_f64_16x16x4_f64, one column per trajectory of the tile:
//         d delta/dz = sum_j beta_j dk_j/dz + w dk(z,z)/dz,   beta_j = alpha_j - 2 w v_j,   w = var_scale eps / (2 sigma)  (0: mean)
//         W_0 = beta kse | W_1 = beta (degree >= 1) | W_2 = beta pb, W_3 = beta pa (degree 2);  lane (kk, n) recomputes kse / pa / pb of
//         training row j0 + kk for trajectory n (phase K's arithmetic: a twentieth of phase V at the cart-pole size) instead of keeping
//         three more panels; the 8 waves take interleaved 4-row steps, their partial R meet in LDS (over the k panel, dead after V)
//   J'  thread (trajectory, d): adds the waves' parts in wave order, applies the kernel's factors, writes jac
// A variance that is not positive follows the closed-loop phase F: w = eps / (2 sqrt(var)) is formed as it comes (inf / NaN rows of
// jac for that trajectory alone) and MCP_STATUS_NONPOS_VAR is raised.  Rows of jac from len - 1 on are NEVER WRITTEN and never read.
// The arguments' base part (OpenArgs, open_fill), the LDS layout (open_layout) and phases K, V, J, J' are in rollout_open_phases.h: model_step.hip
// runs the same step, one per launch, and rollout_mlp.hip the same loop under the tanh-MLP policy.
#include <type_traits>

#include "rollout_open_phases.h"

using namespace mcp;

// FEEDBACK form (template FB, mcp_rollout_pd): the input of step t is not read from a buffer, it is the PD law on the state the step
// starts from (Policy.PD_controller.forward, policy_learning/Policy.py:437-449, inside MC_PILCO.apply_policy's loop, MC_PILCO.py:615-674):
//   e = target_traj[t] - x_t;   a_k = sqrt_kp[k]^2 e[pos[k]] + sqrt_kd[k]^2 e[vel[k]];   u_t[k] = u_max[k] tanh(a_k / u_max[k])  (or a_k)
// The threads that fetch the inputs in the open-loop form compute them from the xs row the state threads have just published -- one more
// LDS barrier per step, in this form only -- and store them to inputs [T][M][U]; row T - 1 is computed and stored although no transition
// reads it.  Everything after that (phases K, V, J, F, the noise addressing) is the open-loop step on the same operands.
struct OpenArgsPd : OpenArgs {
  mcp_pd_policy pd;
  double* inputs;  // [T][M][U]
};
// MEASURED feedback form (template PMS with FB, mcp_rollout_pd_meas): the PD law reads a simulated measurement y_t of x_t instead of x_t
// (MC_PILCO4PMS.apply_policy, policy_learning/MC_PILCO.py:856-899; mcp_meas in include/mcpilco_hip.h).  Per pair i, p = pos[i], v = vel[i]:
//   row 0      np_0 = x_0[p],  nv_0 = mv_0 = x_0[v]                                   (the true state)
//   row t >= 1 np_t = x_t[p] + std_i n_{t,i};  nv_t = (np_t - np_{t-1}) / Ts;  mv_t = (b0 nv_t + b1 nv_{t-1} - a1 mv_{t-1}) / a0
//   y_t = x_t with y[p] = np_t, y[v] = mv_t;   e = target_traj[t] - y_t
// The state thread of a measured position keeps np, nv, mv of its pair in registers (x_0[v] read once from x0) and writes y[p] and y[v]
// into an LDS row beside xs; the threads of the components in no pair write their own value, the thread of a measured velocity writes
// nothing; the input threads read that row behind the barrier the feedback form already has.  n_{t,i} is addressed as in the closed-loop
// kernels (pos_noise[((t-1) M + m) n + i], or Philox stream MCP_STREAM_POS by global particle id): a particle sees the same measurement
// noise whichever policy drives it.  meas.meas [T][M][S] is written for every row (the sweep reads it).
struct OpenArgsPdMeas : OpenArgsPd {
  mcp_meas ms;
};
// INTEGRAL form (template PID with FB, with or without PMS, mcp_rollout_pid): the law gains a clamped integral of the position error, the
// first control here that depends on controller state carried across the steps (the reference has no such law: this replaces a stateful
// torch policy in the loop of MC_PILCO.apply_policy, policy_learning/MC_PILCO.py:615-674, measured: :856-899).  With e as above (on y_t in
// the measured form), p = pos[k], I_{-1} = 0:
//   q_t = I_{t-1}[k] + dt e[p];   I_t[k] = min(max(q_t, -i_max[k]), +i_max[k]);   a_k = (sqrt_kp[k]^2 e[p] + sqrt_kd[k]^2 e[vel[k]]) + sqrt_ki[k]^2 I_t[k]
// The input thread (up, uk) keeps I in a register across the step loop, forms it from the row it already reads behind the barrier the
// feedback form already has, and stores it to pid.integ [T][M][U] beside inputs (the sweep reads it and never re-decides a clamp).  The PD
// products stay the PD form's expression and the integral product is added last: sqrt_ki == 0 reproduces the PD launch bit for bit.  The
// clamp is written as two comparisons: a NaN passes through, as through torch.clamp.
template <bool PMS>
struct OpenArgsPid : std::conditional<PMS, OpenArgsPdMeas, OpenArgsPd>::type {
  mcp_pid_term pid;
};
// TIME-VARYING LINEAR form (template TVL with FB, with or without PMS, mcp_rollout_tvl): the law is a dense row of gains and a feedforward
// per step (Policy.TV_linear_controller; the reference has no such class: this replaces a torch policy in the loops named above).  With e
// as above (on y_t in the measured form):
//   a_k = (sum_s gain[t][k][s] e[s]) + ff[t][k]       (s ascending from 0.0, the feedforward last)
// The input thread (up, uk) forms the dot behind the barrier the feedback form already has, from the row it already reads and from LDS
// alone: row t of gain | ff | target ([U][S] | [U] | [S] doubles) sits in one half of a double buffer (the layout's `ext` region) and row
// t + 1 is brought into the other half by the LAST threads of the workgroup (the state and input threads are the first) right behind the
// barrier that opens phase K of step t -- a step ahead, off the stretch between the feedback barrier and u_t, and without a barrier of
// its own: the write of step t and the reads of steps t - 1 and t + 1 are separated by the step's existing barriers.  Registers were the
// other way; the variance forms of this kernel sit at their register bound, the buffer costs none.  The base parts' pd carries U, squash,
// u_max and the target; its gains and index lists are not read.
struct TvlRows {
  const double* gain;  // [gain_rows][U][S]
  const double* ff;    // [ff_rows][U] or NULL
  int gain_rows, ff_rows;
};
#define TVL_ROW(U, S) ((U) * (S) + (U) + (S))
template <bool PMS>
struct OpenArgsTvl : std::conditional<PMS, OpenArgsPdMeas, OpenArgsPd>::type {
  TvlRows tv;
};
template <bool FB, bool PMS = false, bool PID = false, bool TVL = false>
struct OpenArgsOf {
  typedef OpenArgs type;
};
template <bool PMS>
struct OpenArgsOf<true, PMS, false, true> {
  typedef OpenArgsTvl<PMS> type;
};
template <>
struct OpenArgsOf<true, false, false> {
  typedef OpenArgsPd type;
};
template <>
struct OpenArgsOf<true, true, false> {
  typedef OpenArgsPdMeas type;
};
template <bool PMS>
struct OpenArgsOf<true, PMS, true> {
  typedef OpenArgsPid<PMS> type;
};

// row t of the time-varying law into one half of its LDS buffer: gain[t] (row 0 of a shared gain) | ff[t] (zeros without one) | target[t]
__device__ __forceinline__ void tvl_stage_row(const TvlRows& tv, const double* target, int t, int U, int S, double* dst, int tid) {
  const int US = U * S;
  for (int it = RF_NT - 1 - tid; it < TVL_ROW(U, S); it += RF_NT) {
    double v;
    if (it < US)
      v = tv.gain[(tv.gain_rows == 1 ? (size_t)0 : (size_t)t * US) + it];
    else if (it < US + U)
      v = tv.ff_rows ? tv.ff[(size_t)t * U + (it - US)] : 0.0;
    else
      v = target[(size_t)t * S + (it - US - U)];
    dst[it] = v;
  }
}

template <int PT, int MAXDEG, bool NEEDVAR, bool NEEDJAC, bool FB = false, bool PMS = false, bool PID = false, bool TVL = false>
__global__ __launch_bounds__(RF_NT) void rollout_open_kernel(typename OpenArgsOf<FB, PMS, PID, TVL>::type a) {
  static_assert(FB || !PMS, "the measurement model belongs to the feedback form");
  static_assert(FB || !PID, "the integral term belongs to the feedback form");
  static_assert((FB && !PID) || !TVL, "the time-varying law is a feedback form of its own");
  extern __shared__ double smem[];
  const mcp_model& md = a.model;
  const int S = md.S, U = md.U, G = md.G, D = md.D, M = a.M, T = a.T;
  const int nna = md.n_not_angle, na = md.n_angle;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const OpenLayout L = open_layout(PT, NEEDVAR, S, D, G, a.NpadMax, NEEDJAC, a.na, PMS, TVL ? 2 * TVL_ROW(U, S) : 0);
  double* xs = smem + L.xs;
  double* z = smem + L.z;
  double* red = smem + L.red;  // [2][G][RF_NW][PT]
  GpL* gpl = reinterpret_cast<GpL*>(smem + L.gpl);
  double* kpar = smem + L.kpar;
  double* panel = smem + L.panel;
  double* vpan = smem + L.vpan;  // (recording form)
  double* wjl = smem + L.wj;
  double* redj = smem + L.redj;
  const mcp_noise nzl = noise_of_launch(a.nz);
  const int m0 = blockIdx.x * PT;

  stage_gp_tables(md.gp, md.var_scale, G, D, gpl, kpar, tid);
  if (L.xl) {  // mean mode: the small operands of phase K come from LDS for the whole launch
    const int NP = a.NpadMax;
    for (int g = 0; g < G; ++g) {
      const mcp_gp& gp = md.gp[g];
      for (int it = tid; it < D * NP; it += RF_NT) {
        const int d = it / NP, j = it - d * NP;
        smem[L.xt + (g * D + d) * NP + j] = j < gp.Npad ? gp.Xt[(size_t)d * gp.Npad + j] : 0.0;
      }
      for (int j = tid; j < NP; j += RF_NT) smem[L.al + g * NP + j] = j < gp.Npad ? gp.alpha[j] : 0.0;
    }
  }
  __syncthreads();
  // thread (p, s) owns state component s of trajectory p of the tile; the next PT * U threads fetch the inputs
  const bool own = tid < PT * S;
  const int op = own ? tid / S : 0, os = own ? tid - op * S : 0;
  const int ut = tid - PT * S;
  const bool isu = ut >= 0 && ut < PT * U;
  const int up = isu ? ut / U : 0, uk = isu ? ut - up * U : 0;
  const int tp = own ? op : up;
  const int om = imin(m0 + tp, M - 1);
  const bool ovalid = m0 + tp < M;
  const int len = a.lengths ? imin(imax(a.lengths[om], 1), T) : T;
  int tl = 1;  // the longest trajectory of the tile (uniform)
  for (int p = 0; p < PT; ++p) tl = imax(tl, a.lengths ? imin(imax(a.lengths[imin(m0 + p, M - 1)], 1), T) : T);
  double xn = own ? a.x0[(size_t)om * S + os] : 0.0;
  int zi_plain = -1, zi_ang = -1, g_vel = -1, g_pos = -1, vel_of_pos = 0;
  if (own) {
    for (int i = 0; i < nna; ++i)
      if (md.not_angle[i] == os) zi_plain = i;
    for (int i = 0; i < na; ++i)
      if (md.angle[i] == os) zi_ang = i;
    for (int g = 0; g < G; ++g) {
      if (md.vel[g] == os) g_vel = g;
      if (md.not_vel[g] == os) {
        g_pos = g;
        vel_of_pos = md.vel[g];
      }
    }
  }
  const int og = g_pos >= 0 ? g_pos : g_vel;  // the GP whose increment this component integrates
  const double Ts = md.Ts;
  unsigned bad = 0;
  int cur = 0;
  // feedback form: the gains (squared once, as the reference squares them in every evaluation), bound and state components of input uk
  double kp2 = 0.0, kd2 = 0.0, umax = 1.0;
  int ipos = 0, ivel = 0;
  if constexpr (FB && !TVL) {
    if (isu) {
      const double kp = a.pd.sqrt_kp[uk], kd = a.pd.sqrt_kd[uk];
      kp2 = kp * kp;
      kd2 = kd * kd;
      umax = a.pd.u_max[uk];
      ipos = a.pd.pos[uk];
      ivel = a.pd.vel[uk];
    }
  }
  // integral form: the squared gain, the bound, the step and the integral of input uk (I_{-1} = 0)
  double ki2 = 0.0, imax = 0.0, idt = 0.0, integ = 0.0;
  if constexpr (PID) {
    if (isu) {
      const double ki = a.pid.sqrt_ki[uk];
      ki2 = ki * ki;
      imax = a.pid.i_max[uk];
      idt = a.pid.dt;
    }
  }
  // measured feedback form: the pair of this state component (pm_pos: it is the pair's position and carries the filter; pm_vel: it is
  // the pair's velocity and leaves its slot of the measurement row to the position's thread)
  int pm_pos = -1, pm_vel = -1, pm_vc = 0;
  double pm_std = 0.0, pm_np = 0.0, pm_nv = 0.0, pm_mv = 0.0;
  if constexpr (PMS) {
    if (own) {
      for (int i = 0; i < a.ms.n; ++i) {
        if (a.ms.vel[i] == os) pm_vel = i;
        if (a.ms.pos[i] == os) {
          pm_pos = i;
          pm_vc = a.ms.vel[i];
          pm_std = a.ms.std_pos[i];
        }
      }
      if (pm_pos >= 0) pm_nv = pm_mv = a.x0[(size_t)om * S + pm_vc];
    }
  }
  // time-varying form: the bound of input uk; row 0 of the law into the first half of its buffer
  double* tvr = smem + L.ext;
  (void)tvr;
  if constexpr (TVL) {
    if (isu) umax = a.pd.u_max[uk];
    tvl_stage_row(a.tv, a.pd.target_traj, 0, U, S, tvr, tid);
  }
  lds_barrier();

  for (int t = 0; t < T; ++t) {
    // ---- phase S: publish x_t and its GP features; rows beyond a trajectory's length are zeros -----------------------
    if (own) {
      xs[cur * PT * S + op * S + os] = xn;
      if (ovalid) {
        a.states[((size_t)t * M + m0 + op) * S + os] = t < len ? xn : 0.0;
        if (t < len && is_bad(xn)) bad |= MCP_STATUS_NAN;
      }
    }
    if constexpr (PMS) {  // y_t: the measurement of the row just formed (MC_PILCO.py:856-899)
      if (own && pm_vel < 0) {
        double* yr = smem + L.ym + op * S;
        double npos = xn, mv = 0.0;
        if (pm_pos >= 0) {
          if (t == 0) {
            mv = pm_mv;  // (row 0: the true velocity, which also starts both histories)
          } else {
            const double nn = a.ms.pos_noise ? a.ms.pos_noise[((size_t)(t - 1) * M + om) * a.ms.n + pm_pos]
                                             : philox_normal(nzl, om, t, pm_pos, MCP_STREAM_POS);
            npos = fma(pm_std, nn, xn);
            const double nv = (npos - pm_np) / Ts;
            mv = (a.ms.b0 * nv + a.ms.b1 * pm_nv - a.ms.a1 * pm_mv) / a.ms.a0;
            pm_nv = nv;
            pm_mv = mv;
          }
          pm_np = npos;
          yr[pm_vc] = mv;
        }
        yr[os] = npos;
        if (ovalid) {
          double* mr = a.ms.meas + ((size_t)t * M + m0 + op) * S;
          mr[os] = npos;
          if (pm_pos >= 0) mr[pm_vc] = mv;
          if (is_bad(npos) || is_bad(mv)) bad |= MCP_STATUS_NAN;
        }
      }
    }
    double ufb = 0.0;
    if constexpr (FB) {  // u_t from the row just published (every row, the last one included: it is stored, and a cost may read it)
      lds_barrier();
      if (isu) {
        const double* xr = PMS ? smem + L.ym + up * S : xs + cur * PT * S + up * S;
        const double* tg = a.pd.target_traj + (size_t)t * S;
        double av;
        if constexpr (TVL) {  // the dense row: gain, feedforward and target of step t from LDS alone
          const double* gr = tvr + (t & 1) * TVL_ROW(U, S);
          const double* gk = gr + uk * S;
          const double* tgr = gr + U * S + U;
          double acc = 0.0;
          for (int s = 0; s < S; ++s) acc += gk[s] * (tgr[s] - xr[s]);
          av = acc + gr[U * S + uk];
        } else {
          av = kp2 * (tg[ipos] - xr[ipos]) + kd2 * (tg[ivel] - xr[ivel]);
        }
        if constexpr (PID) {
          const double q = integ + idt * (tg[ipos] - xr[ipos]);
          integ = q < -imax ? -imax : (q > imax ? imax : q);
          av = av + ki2 * integ;
          if (ovalid) a.pid.integ[((size_t)t * M + m0 + up) * U + uk] = integ;
        }
        ufb = a.pd.squash ? umax * fast_tanh(av / umax) : av;
        if (ovalid) {
          a.inputs[((size_t)t * M + m0 + up) * U + uk] = ufb;
          if (is_bad(ufb)) bad |= MCP_STATUS_NAN;
        }
      }
    }
    // (this path skips the barrier below, which is also what separates the input threads' read of the measurement row of step t from its
    //  rewrite in step t + 1: harmless while the feedback form has no ragged lengths -- tl == T, the path is the last row's alone)
    if (t + 1 >= tl) continue;  // (uniform) nothing of this tile goes further: only the zero rows are left to write
    if (own) {
      double* zp = z + op * D;
      if (zi_plain >= 0) zp[zi_plain] = xn;
      if (zi_ang >= 0) {
        double sn, cs;
        sincos_fast(xn, &sn, &cs);
        zp[nna + zi_ang] = sn;
        zp[nna + na + zi_ang] = cs;
      }
    }
    if constexpr (FB) {
      if (isu) z[up * D + nna + 2 * na + uk] = ufb;
    } else if (isu) {  // inputs beyond a trajectory's last transition are never read
      const double uv = (t + 1 < len) ? a.u[((size_t)t * a.Mu + (a.Mu == 1 ? 0 : om)) * U + uk] : 0.0;
      z[up * D + nna + 2 * na + uk] = uv;
      if (ovalid && t + 1 < len && is_bad(uv)) bad |= MCP_STATUS_NAN;
    }
    lds_barrier();
    if constexpr (TVL) tvl_stage_row(a.tv, a.pd.target_traj, t + 1, U, S, tvr + ((t + 1) & 1) * TVL_ROW(U, S), tid);  // (t + 1 < T here)
    // ---- phases K (and V) per GP ---------------------------------------------------------------------------------------
    for (int g = 0; g < G; ++g) {
      const GpL gp = gpl[g];
      // X^T and alpha of GP g: their LDS copies (row pitch NpadMax) where the launch staged them, else global memory (the GP's own Npad)
      const double* Xt = L.xl ? smem + L.xt + g * D * a.NpadMax : gp.Xt;
      const double* al = L.xl ? smem + L.al + g * a.NpadMax : gp.alpha;
      open_phase_k<PT, MAXDEG, NEEDVAR>(gp, kpar + g * KP_STRIDE(D), D, z, panel, red + g * RF_NW * PT, tid, wv, lane, Xt, al,
                                        L.xl ? a.NpadMax : gp.Npad);
      if (NEEDJAC && !NEEDVAR)  // the mean chain: beta = alpha, nothing of phase K is needed -- no barrier in between
        open_phase_j<PT, MAXDEG, false>(gp, kpar + g * KP_STRIDE(D), D, z, nullptr, 0.0, redj + g * L.redj_gp, a.na, wv, lane, Xt, al,
                                        L.xl ? a.NpadMax : gp.Npad);
      if (NEEDVAR) {
        lds_barrier();
        const int Npad = __builtin_amdgcn_readfirstlane(gp.Npad);
        double q = 0.0;
        for (int I0 = 32 * wv; I0 < Npad; I0 += 32 * RF_NW) q += open_v_block<PT, NEEDJAC>(gp.Kinv, Npad, I0, panel, vpan, lane);
        q = fold_kk(q);
        if (lane < PT) red[(G + g) * RF_NW * PT + wv * PT + lane] = q;
        lds_barrier();  // the panel is rewritten by the next GP (recording form: by phase J's partial sums)
        if (NEEDJAC) {
          const int nn = (lane & 15) < PT ? (lane & 15) : 0;
          const double wjs = open_wjs<PT, MAXDEG>(a, nzl, gp, kpar + g * KP_STRIDE(D), D, G, g, t, imin(m0 + nn, M - 1), z + nn * D, red, nn);
          if (wv == 0 && lane < PT) wjl[lane] = wjs;
          open_phase_j<PT, MAXDEG, true>(gp, kpar + g * KP_STRIDE(D), D, z, vpan, wjs, redj, a.na, wv, lane, Xt, al, gp.Npad);
          lds_barrier();
          open_jac_store<PT, MAXDEG, true>(a, gp, kpar + g * KP_STRIDE(D), g, t, m0, z, wjl, redj, a.na, tid);
          lds_barrier();  // the next GP's phase K writes the panel again
        }
      }
    }
    if (!NEEDVAR) lds_barrier();
    if (NEEDJAC && !NEEDVAR)
      for (int g = 0; g < G; ++g) open_jac_store<PT, MAXDEG, false>(a, gpl[g], kpar + g * KP_STRIDE(D), g, t, m0, z, nullptr, redj + g * L.redj_gp, a.na, tid);
    // ---- phase F: moments, sample, integrate   v' = v + delta ;  q' = q + Ts v + Ts/2 delta   (Model_learning.py:711-716) ----
    if (own) {
      const double* xc = xs + cur * PT * S + op * S;
      double nx = 0.0;
      if (og >= 0) {
        const GpL& gp = gpl[og];
        const double* kp = kpar + og * KP_STRIDE(D);
        const double* zp = z + op * D;
        double mu = gp.mean;
#pragma unroll
        for (int w = 0; w < RF_NW; ++w) mu += red[og * RF_NW * PT + w * PT + op];
        double var = 0.0, dv = mu;
        if (NEEDVAR) {
          double ktv = 0.0;
#pragma unroll
          for (int w = 0; w < RF_NW; ++w) ktv += red[(G + og) * RF_NW * PT + w * PT + op];
          double kzz = gp.lambda;
          if (MAXDEG >= 1 && gp.deg >= 1) {
            double p1 = kp[KP_W1(D) + D];
            for (int d = 0; d < D; ++d) p1 = fma(kp[KP_W1(D) + d] * zp[d], zp[d], p1);
            kzz += p1;
            if (MAXDEG >= 2 && gp.deg >= 2) {
              double Sa = 0.0, Sb = 0.0;
              for (int d = 0; d < D; ++d) {
                const double zz = zp[d] * zp[d];
                Sa = fma(kp[KP_W20(D) + d], zz, Sa);
                Sb = fma(kp[KP_W21(D) + d], zz, Sb);
              }
              kzz = fma(Sa, Sb, kzz);
            }
          }
          var = (kzz - ktv) * gp.var_scale;
          if (a.sample) {
            const double e = nzl.eps ? nzl.eps[((size_t)t * M + om) * G + og] : philox_normal(nzl, om, t, og);
            dv = fma(sqrt(var), e, mu);
          }
        }
        if (og == g_vel && ovalid && t + 1 < len) {  // every GP has exactly one velocity component: its thread reports
          const size_t o = ((size_t)t * M + m0 + op) * G + og;
          if (a.mu) a.mu[o] = mu;
          if (NEEDVAR && a.var) a.var[o] = var;
          if (a.sample && var <= 0.0) bad |= MCP_STATUS_NONPOS_VAR;  // (finite and not positive: a NaN variance is MCP_STATUS_NAN)
          if (is_bad(mu) || is_bad(var)) bad |= MCP_STATUS_NAN;
        }
        nx = og == g_pos ? xc[os] + Ts * xc[vel_of_pos] + 0.5 * Ts * dv : xc[os] + dv;
      }
      xn = nx;
    }
    if ((NEEDVAR && MAXDEG >= 1) || NEEDJAC) lds_barrier();  // k(z, z) above (and phase J') read z, which the next step's phase S rewrites
    cur ^= 1;
  }
  if (bad) atomicOr(a.status, bad);
}

// ---- host path of the forward entry points: checks -> fill -> ladder -----------------------------------------------------------------
// (an entry checks its own pointers and sizes, then the limits, the model, its descriptors -- every refusal before any HIP call --, fills
// the base part of the arguments with open_fill, adds what is its own and hands them to the one ladder of tiles, launch_open_tiles)
template <int PT, int MAXDEG, bool NEEDVAR, bool NEEDJAC, bool FB, bool PMS, bool PID, bool TVL = false>
static int launch_open(const typename OpenArgsOf<FB, PMS, PID, TVL>::type& a, hipStream_t st) {
  const OpenLayout L = open_layout(PT, NEEDVAR, a.model.S, a.model.D, a.model.G, a.NpadMax, NEEDJAC, a.na, PMS, TVL ? 2 * TVL_ROW(a.model.U, a.model.S) : 0);
  const size_t lds = (size_t)L.total * sizeof(double);
  if (lds > MCP_LDS_LIMIT) return MCP_ERR_LIMIT;
  MCP_ENSURE_MAX_LDS((rollout_open_kernel<PT, MAXDEG, NEEDVAR, NEEDJAC, FB, PMS, PID, TVL>));
  hipLaunchKernelGGL((rollout_open_kernel<PT, MAXDEG, NEEDVAR, NEEDJAC, FB, PMS, PID, TVL>), dim3((a.M + PT - 1) / PT), dim3(RF_NT), lds, st, a);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}
template <int PT, bool NEEDVAR, bool NEEDJAC, bool FB, bool PMS, bool PID, bool TVL = false>
static int launch_open_deg(const typename OpenArgsOf<FB, PMS, PID, TVL>::type& a, int maxdeg, hipStream_t st) {
  return maxdeg == 0 ? launch_open<PT, 0, NEEDVAR, NEEDJAC, FB, PMS, PID, TVL>(a, st) : launch_open<PT, 2, NEEDVAR, NEEDJAC, FB, PMS, PID, TVL>(a, st);
}
// The ladder of tiles, the same for every form (the feedback and its integral add nothing to the LDS layout, the measurement one row [PT][S], the time-varying law two rows of at most 152 doubles); a.jac: the
// recording form.  The mean chain (no sampling, no variance asked for) touches no Kinv: one trajectory per workgroup.  With a variance:
//   no record  16 trajectories per workgroup, 4 where the k panel of 16 does not fit (at every compiled limit at once -- S = 16, D = 32, G = 8,
//              Npad = 4096 -- that layout takes 148 KB of the 160, so nothing within MCP_MAX_* is refused)
//   record     two panels: 16 up to Npad ~ 500, 4 up to ~ 2000, beyond that one (at every compiled limit at once: 2 x 32 KB of panels, 85 KB
//              in all; the recording mean chain: 85 KB, X^T then stays in global memory)
template <bool FB, bool PMS, bool PID = false, bool TVL = false>
static int launch_open_tiles(const typename OpenArgsOf<FB, PMS, PID, TVL>::type& a, int maxdeg, bool wantvar, hipStream_t st) {
  if (!a.jac) {
    if (!a.sample && !wantvar) return launch_open_deg<1, false, false, FB, PMS, PID, TVL>(a, maxdeg, st);
    int rc = launch_open_deg<16, true, false, FB, PMS, PID, TVL>(a, maxdeg, st);
    if (rc == MCP_ERR_LIMIT) rc = launch_open_deg<4, true, false, FB, PMS, PID, TVL>(a, maxdeg, st);
    return rc;
  }
  if (!a.sample && !wantvar) return launch_open_deg<1, false, true, FB, PMS, PID, TVL>(a, maxdeg, st);
  int rc = launch_open_deg<16, true, true, FB, PMS, PID, TVL>(a, maxdeg, st);
  if (rc == MCP_ERR_LIMIT) rc = launch_open_deg<4, true, true, FB, PMS, PID, TVL>(a, maxdeg, st);
  if (rc == MCP_ERR_LIMIT) rc = launch_open_deg<1, true, true, FB, PMS, PID, TVL>(a, maxdeg, st);
  return rc;
}

// what mcp_rollout_open and mcp_rollout_open_rec share (jac: the recording form)
static int open_dispatch(const mcp_model* model, const mcp_noise* noise, int M, int T, int particle_pred, const double* x0, const double* u, int Mu,
                         const int32_t* lengths, double* states, double* mu, double* var, double* jac, uint32_t* status, void* stream) {
  if (!model || !noise || !x0 || !u || !states || !status) return MCP_ERR_ARG;
  if (M <= 0 || T < 2 || (Mu != 1 && Mu != M)) return MCP_ERR_ARG;
  if (!model_within_limits(model)) return MCP_ERR_LIMIT;
  if (!model_ok(model)) return MCP_ERR_ARG;
  OpenArgs a;
  const int maxdeg = open_fill(a, model, noise, M, T, particle_pred, x0, u, Mu, lengths, states, mu, var, jac, status);
  return launch_open_tiles<false, false>(a, maxdeg, var != nullptr, (hipStream_t)stream);
}

extern "C" int mcp_rollout_open(const mcp_model* model, const mcp_noise* noise, int M, int T, int particle_pred, const double* x0, const double* u,
                                int Mu, const int32_t* lengths, double* states, double* mu, double* var, uint32_t* status, void* stream) {
  return open_dispatch(model, noise, M, T, particle_pred, x0, u, Mu, lengths, states, mu, var, nullptr, status, stream);
}

// the recording form (same reference lines as mcp_rollout_open; the record is what autograd would keep of MC_PILCO.py:347-373)
extern "C" int mcp_rollout_open_rec(const mcp_model* model, const mcp_noise* noise, int M, int T, int particle_pred, const double* x0, const double* u,
                                    int Mu, const int32_t* lengths, double* states, double* mu, double* var, double* jac, uint32_t* status,
                                    void* stream) {
  if (!jac) return MCP_ERR_ARG;
  return open_dispatch(model, noise, M, T, particle_pred, x0, u, Mu, lengths, states, mu, var, jac, status, stream);
}

// ---- feedback form: checks, entry -------------------------------------------------------------------------------------------------------
// the descriptor against the model and the horizon (host fields only: the gains and the target are device memory).  pos / vel hold distinct
// components each: the sweep keeps one input per state component and role
static int pd_policy_check(const mcp_model* model, const mcp_pd_policy* pd, int T) {
  if (pd->U < 1 || pd->U > MCP_MAX_INPUT) return pd->U > MCP_MAX_INPUT ? MCP_ERR_LIMIT : MCP_ERR_ARG;
  if (pd->U != model->U || pd->target_rows < T || !pd->sqrt_kp || !pd->sqrt_kd || !pd->target_traj) return MCP_ERR_ARG;
  for (int k = 0; k < pd->U; ++k) {
    if (pd->pos[k] < 0 || pd->pos[k] >= model->S || pd->vel[k] < 0 || pd->vel[k] >= model->S) return MCP_ERR_ARG;
    if (pd->squash && !(pd->u_max[k] > 0.0)) return MCP_ERR_ARG;
    for (int j = 0; j < k; ++j)
      if (pd->pos[j] == pd->pos[k] || pd->vel[j] == pd->vel[k]) return MCP_ERR_ARG;
  }
  return MCP_OK;
}

// the integral term (host fields and the two pointers), looked at behind every check of the PD entries.  pid NULL or on == 0: no term
static inline bool pid_active(const mcp_pid_term* pid) { return pid && pid->on != 0; }
static int pid_term_check(const mcp_pid_term* pid, int U) {
  if (!pid_active(pid)) return MCP_OK;
  if (!pid->sqrt_ki || !pid->integ) return MCP_ERR_ARG;
  if (!(pid->dt > 0.0)) return MCP_ERR_ARG;  // (a NaN is refused too)
  for (int k = 0; k < U; ++k)
    if (!(pid->i_max[k] > 0.0)) return MCP_ERR_ARG;  // (+inf: no clamp)
  return MCP_OK;
}
// the arguments of an integral form: those of the feedback form it extends, and the term
template <class PidArgs, class Args>
static PidArgs pd_with_pid(const Args& a, const mcp_pid_term* pid) {
  PidArgs d;
  static_cast<Args&>(d) = a;
  d.pid = *pid;
  return d;
}

// Closed-loop rollout under the PD law: replaces the loop of MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674) with
// Policy.PD_controller.forward (policy_learning/Policy.py:437-449) as the policy, over Model_learning.get_next_state
// (model_learning/Model_learning.py:210-229, 471-494, 685-718).  jac != NULL: the recording form (what autograd would keep of that loop).
// pid (NULL or on == 0: none): the integral forms of the same kernels.
static int pd_dispatch(const mcp_model* model, const mcp_pd_policy* pd, const mcp_meas* ms, const mcp_noise* noise, int M, int T, int particle_pred,
                       const double* x0, double* states, double* inputs, double* jac, double* mu, double* var, uint32_t* status, void* stream,
                       const mcp_pid_term* pid = nullptr) {
  int crc = closed_loop_checks(model && pd && noise && x0 && states && inputs && status, M, T, model, ms, false,
                               [&] { return pd_policy_check(model, pd, T); });
  if (crc == MCP_OK) crc = pid_term_check(pid, pd->U);
  if (crc != MCP_OK) return crc;
  OpenArgsPdMeas a;
  // (T == 1: the policy alone -- no transition, nothing to record)
  const int maxdeg = open_fill(a, model, noise, M, T, particle_pred, x0, nullptr, M, nullptr, states, mu, var, T == 1 ? nullptr : jac, status);
  a.pd = *pd;
  a.inputs = inputs;
  hipStream_t st = (hipStream_t)stream;
  if (pid_active(pid)) {
    if (!meas_active(ms)) return launch_open_tiles<true, false, true>(pd_with_pid<OpenArgsPid<false>, OpenArgsPd>(a, pid), maxdeg, var != nullptr, st);
    a.ms = *ms;
    return launch_open_tiles<true, true, true>(pd_with_pid<OpenArgsPid<true>, OpenArgsPdMeas>(a, pid), maxdeg, var != nullptr, st);
  }
  if (!meas_active(ms)) return launch_open_tiles<true, false>(a, maxdeg, var != nullptr, st);  // (the base part of `a`: mcp_rollout_pd's own kernels)
  a.ms = *ms;
  return launch_open_tiles<true, true>(a, maxdeg, var != nullptr, st);
}

extern "C" int mcp_rollout_pd(const mcp_model* model, const mcp_pd_policy* pd, const mcp_noise* noise, int M, int T, int particle_pred,
                              const double* x0, double* states, double* inputs, double* jac, double* mu, double* var, uint32_t* status,
                              void* stream) {
  return pd_dispatch(model, pd, nullptr, noise, M, T, particle_pred, x0, states, inputs, jac, mu, var, status, stream);
}

// Closed-loop rollout under the PD law evaluated on a simulated measurement: replaces the loop of MC_PILCO4PMS.apply_policy
// (policy_learning/MC_PILCO.py:808-906: noisy positions, backward-difference velocities, the first-order filter) with
// Policy.PD_controller.forward (policy_learning/Policy.py:437-449) as the policy, over Model_learning.get_next_state
// (model_learning/Model_learning.py:210-229, 471-494, 685-718).  meas->n == 0: mcp_rollout_pd's kernels on the same arguments.
extern "C" int mcp_rollout_pd_meas(const mcp_model* model, const mcp_pd_policy* pd, const mcp_meas* meas, const mcp_noise* noise, int M, int T,
                                   int particle_pred, const double* x0, double* states, double* inputs, double* jac, double* mu, double* var,
                                   uint32_t* status, void* stream) {
  if (!meas) return MCP_ERR_ARG;
  return pd_dispatch(model, pd, meas, noise, M, T, particle_pred, x0, states, inputs, jac, mu, var, status, stream);
}

// Closed-loop rollout under the PD law with the integral term (mcp_pid_term; the law and its clamp: OpenArgsPid above), on the true state
// (meas NULL or n == 0) or on the simulated measurement: replaces a stateful torch policy in the loop of MC_PILCO.apply_policy
// (policy_learning/MC_PILCO.py:615-674) or MC_PILCO4PMS.apply_policy (:808-906) over Model_learning.get_next_state
// (model_learning/Model_learning.py:210-229, 471-494, 685-718) -- the reference has no integral law.  pid NULL or on == 0: mcp_rollout_pd /
// mcp_rollout_pd_meas on the same arguments.
extern "C" int mcp_rollout_pid(const mcp_model* model, const mcp_pd_policy* pd, const mcp_pid_term* pid, const mcp_meas* meas, const mcp_noise* noise,
                               int M, int T, int particle_pred, const double* x0, double* states, double* inputs, double* jac, double* mu,
                               double* var, uint32_t* status, void* stream) {
  return pd_dispatch(model, pd, meas, noise, M, T, particle_pred, x0, states, inputs, jac, mu, var, status, stream, pid);
}

// ---- time-varying linear form: checks, entry ---------------------------------------------------------------------------------------------
// the descriptor against the model and the horizon (host fields and the pointers' presence), limits first as for the PD law
static int tvl_policy_check(const mcp_model* model, const mcp_tvl_policy* tv, int T) {
  if (tv->U > MCP_MAX_INPUT || tv->S > MCP_MAX_STATE) return MCP_ERR_LIMIT;
  if (tv->U < 1 || tv->U != model->U || tv->S != model->S || tv->target_rows < T || !tv->gain || !tv->target_traj) return MCP_ERR_ARG;
  if (tv->gain_rows != 1 && tv->gain_rows < T) return MCP_ERR_ARG;
  if (tv->ff_rows != 0 && (tv->ff_rows < T || !tv->ff)) return MCP_ERR_ARG;
  for (int k = 0; k < tv->U; ++k)
    if (tv->squash && !(tv->u_max[k] > 0.0)) return MCP_ERR_ARG;
  return MCP_OK;
}
// what the kernels read of the descriptor through the feedback form's pd (U, squash, u_max, the target; no gains, no index lists)
static mcp_pd_policy tvl_as_pd(const mcp_tvl_policy* tv) {
  mcp_pd_policy pd;
  memset(&pd, 0, sizeof(pd));
  pd.U = tv->U, pd.squash = tv->squash, pd.target_traj = tv->target_traj, pd.target_rows = tv->target_rows;
  for (int k = 0; k < MCP_MAX_INPUT; ++k) pd.u_max[k] = tv->u_max[k];
  return pd;
}

// Closed-loop rollout under the time-varying linear feedback law (the law and how its rows reach the step: OpenArgsTvl above), on the true
// state (meas NULL or n == 0) or on the simulated measurement: replaces a torch policy (Policy.TV_linear_controller; the reference has no
// such law) in the loop of MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674) or MC_PILCO4PMS.apply_policy (:808-906) over
// Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718).
extern "C" int mcp_rollout_tvl(const mcp_model* model, const mcp_tvl_policy* tvl, const mcp_meas* meas, const mcp_noise* noise, int M, int T,
                               int particle_pred, const double* x0, double* states, double* inputs, double* jac, double* mu, double* var,
                               uint32_t* status, void* stream) {
  const int crc = closed_loop_checks(model && tvl && noise && x0 && states && inputs && status, M, T, model, meas, false,
                                     [&] { return tvl_policy_check(model, tvl, T); });
  if (crc != MCP_OK) return crc;
  OpenArgsTvl<true> a;
  const int maxdeg = open_fill(a, model, noise, M, T, particle_pred, x0, nullptr, M, nullptr, states, mu, var, T == 1 ? nullptr : jac, status);
  a.pd = tvl_as_pd(tvl);
  a.inputs = inputs;
  a.tv.gain = tvl->gain, a.tv.ff = tvl->ff, a.tv.gain_rows = tvl->gain_rows, a.tv.ff_rows = tvl->ff_rows;
  hipStream_t st = (hipStream_t)stream;
  if (meas_active(meas)) {
    a.ms = *meas;
    return launch_open_tiles<true, true, false, true>(a, maxdeg, var != nullptr, st);
  }
  OpenArgsTvl<false> b;
  static_cast<OpenArgsPd&>(b) = a;
  b.tv = a.tv;
  return launch_open_tiles<true, false, false, true>(b, maxdeg, var != nullptr, st);
}

// ---------------------------------------------------------------------------------------
// Reverse-time sweep of the open-loop rollout: what autograd's backward does through the step loop of MC_PILCO.rollout
// (MC_PILCO.py:347-373) over get_next_state (Model_learning.py:210-229, 471-494, 685-718), from the record alone.
//   lambda_{len-1} = g_states[len-1];   g_u[t] = (dx_{t+1}/du_t)^T lambda_{t+1};   lambda_t = g_states[t] + (dx_{t+1}/dx_t)^T lambda_{t+1}
// One step backwards, with gd_g the adjoint of GP g's increment and gz = sum_g gd_g jac[t][m][g][:] that of its input z:
//   gd_g  = sum over the components s that integrate GP g of  lambda'[s]  (a velocity, or a delta-state component: not_vel == -1)
//                                                          or  Ts/2 lambda'[s]  (the position not_vel[g])
//   lambda[s] = g_states[t][s] + lambda'[s] (s is integrated at all) + Ts lambda'[not_vel[g]] (s = vel[g] of a position) + gz through
//               z = [x_not_angle, sin, cos, u]: gz[i] | gz[sin_i] cos x - gz[cos_i] sin x;     g_u[t][k] = gz[nna + 2 na + k]
// The same uniform test as rollout_bwd.hip separates the model families: not_vel[g] < 0 has no Ts term.
// Trajectories are independent: a workgroup of two waves owns OB_PT of them, no atomics, no sums across trajectories.  Wave 1 is the
// LOADER: while wave 0 runs the chain of row r it brings row r - 1 of the record (jac, the states for the angles, g_states) into the
// other half of a double buffer, coalesced -- jac[t][m0 .. m0 + OB_PT) is one contiguous block.  Wave 0, lane (p = l & 15, q = l >> 4):
// trajectory p, every fourth g / d / s; its three stages meet in LDS, ordered within the wave (no workgroup barrier on the chain).
// Ragged lengths: row len - 1 starts the sweep, later rows of g_states are never read, g_u rows from len - 1 on are zeros.
// ---------------------------------------------------------------------------------------
#define OB_PT 16
#define OB_NT 128

struct OpenBwdArgs {
  int S, U, G, D, nna, na, M, T;
  int angle[MCP_MAX_STATE], not_angle[MCP_MAX_STATE], vel[MCP_MAX_GP], not_vel[MCP_MAX_GP];
  double Ts;
  const double* states;
  const double* jac;
  const double* g_states;
  const int32_t* lengths;
  double* g_x0;
  double* g_u;
};
// FEEDBACK form of the sweep (template FB, mcp_rollout_pd_bwd): u_t = pd(x_t) closes the loop, so the adjoint of the input goes back into
// the state of the same row and into the gains.  Per row r, after stage B (row T - 1 has no record: only the upstream term):
//   gu_k = gz[nna + 2 na + k] + g_inputs[r][k];     abar_k = gu_k (1 - (u_k / u_max_k)^2)  with squashing, gu_k without
//   lambda[pos[k]] -= sqrt_kp[k]^2 abar_k;  lambda[vel[k]] -= sqrt_kd[k]^2 abar_k                      (stage C, tables kpos / kvel)
//   g_sqrt_kp[k] += 2 sqrt_kp[k] e[pos[k]] abar_k;  g_sqrt_kd[k] += 2 sqrt_kd[k] e[vel[k]] abar_k,  e = target_traj[r] - x_r
// Lane (p, q) keeps the sums of trajectory p's inputs q and q + 4 in registers and stores them once: g_gains [M][2][U], no atomics, no
// sum across trajectories.  The loader also brings inputs[r], g_inputs[r], the state of EVERY row and target_traj[r].
struct OpenBwdArgsPd : OpenBwdArgs {
  mcp_pd_policy pd;
  const double* inputs;    // [T][M][U]
  const double* g_inputs;  // [T][M][U] or NULL
  double* g_gains;         // [M][2][U] or NULL
};
// MEASURED feedback form of the sweep (template PMS with FB, mcp_rollout_pd_meas_bwd): the PD law read y_r (ms.meas, brought by the loader),
// so stage B' takes e = target_traj[r] - y_r and stage C receives the policy's pull ON THE MEASUREMENT,
//   ybar_r[s] = - sqrt_kp[k]^2 abar_k (pos[k] == s) - sqrt_kd[k]^2 abar_k (vel[k] == s),
// through the adjoint of the filter.  Per (trajectory, pair) two carries, both zero behind the last row, kept in LDS at the pair's position
// component (the same lane writes and reads them, row after row):
//   mvbar_r = ybar_r[v] - (a1/a0) mvbar_{r+1};   nvbar_r = (b0/a0) mvbar_r + (b1/a0) mvbar_{r+1};   npbar_r = ybar_r[p] + (nvbar_r - nvbar_{r+1}) / Ts
//   r >= 1: lambda_r[p] += npbar_r (the true velocity gets nothing from the policy)
//   r == 0: lambda_0[p] += ybar_0[p] - nvbar_1 / Ts;   lambda_0[v] += ybar_0[v] + ((b1 - a1)/a0) mvbar_1     (row 0 is measured true)
// Components in no pair: lambda_r[s] += ybar_r[s], as in the plain feedback form.
struct OpenBwdArgsPdMeas : OpenBwdArgsPd {
  mcp_meas ms;
};
// INTEGRAL form of the sweep (template PID with FB, with or without PMS, mcp_rollout_pid_bwd): I_r feeds a_r and I_{r+1}, so its adjoint
// is a carry c down the rows, one double per (trajectory, input), zero behind the last row, in the registers of the chain lane that
// keeps that input's gain sums.  Per row r, in stage B' behind abar (I_r: pid.integ, brought by the loader like inputs[r]):
//   Ibar_k = sqrt_ki[k]^2 abar_k + c_k;   c_k = (|I_r[k]| < i_max[k]) ? Ibar_k : 0;   g_sqrt_ki[k] += 2 sqrt_ki[k] I_r[k] abar_k
// (the clamp passes gradient iff I_r sits strictly inside its bounds; the forward's stored I decides, never a recomputation), and in
// stage C beside the proportional pull:  lambda[pos[k]] -= dt c_k  (measured form: on ybar[pos[k]], through the filter adjoint unchanged).
// The lane leaves c_k to stage C in the slot of the integral's row buffer it has just read.  g_gains is [M][3][U]: kp | kd | ki.
template <bool PMS>
struct OpenBwdArgsPid : std::conditional<PMS, OpenBwdArgsPdMeas, OpenBwdArgsPd>::type {
  mcp_pid_term pid;
};
// TIME-VARYING LINEAR form of the sweep (template TVL with FB, with or without PMS, mcp_rollout_tvl_bwd): stage B' is the feedback form's
// (abar through the squashing); stage C takes the dense pull
//   lambda_r[s] -= sum_k gain[r][k][s] abar_k       (measured form: on ybar_r[s], through the filter's adjoint unchanged)
// with gain[r] brought by the loader beside the row.  The parameter gradient is PER ROW: one partial per workgroup,
//   g_part[tile][r][k][s] = sum_p abar[p][k] e_r[p][s]  (s < S),   g_part[tile][r][k][S] = sum_p abar[p][k],   e_r = target_traj[r] - x_r (or y_r)
// over the tile's valid trajectories p in a fixed order.  The sum lives in WAVE 1, behind the chain: abar is double-buffered by row
// parity, and in the iteration in which wave 0 runs row r the loader first reduces row r + 1 out of the buffer half it is about to refill
// (16 entries (k, s) at a time, each quarter of the wave adding four trajectories and the quarters meeting by the row / half swaps:
// (p 0-3 + p 4-7) + (p 8-11 + p 12-15), a fixed tree), then loads row r - 1 into it; row 0 is reduced behind the loop.  A reduction across
// the 16 lanes p of wave 0 would put U (S + 1) / 4 four-step lane reductions on every row of the serial chain instead.  One lane per
// entry adding all 16 trajectories was measured first: the loader then finishes behind the chain (sweep 0.69 against the PD twin's 0.47 ms
// at M = 400, T = 150, profiles/NOTES.md part AE).
template <bool PMS>
struct OpenBwdArgsTvl : std::conditional<PMS, OpenBwdArgsPdMeas, OpenBwdArgsPd>::type {
  const double* gain;  // [gain_rows][U][S]
  int gain_rows;
  double* g_part;      // [tiles][T][U][S + 1] or NULL
};
template <bool FB, bool PMS = false, bool PID = false, bool TVL = false>
struct OpenBwdArgsOf {
  typedef OpenBwdArgs type;
};
template <bool PMS>
struct OpenBwdArgsOf<true, PMS, false, true> {
  typedef OpenBwdArgsTvl<PMS> type;
};
template <>
struct OpenBwdArgsOf<true, false, false> {
  typedef OpenBwdArgsPd type;
};
template <>
struct OpenBwdArgsOf<true, true, false> {
  typedef OpenBwdArgsPdMeas type;
};
template <bool PMS>
struct OpenBwdArgsOf<true, PMS, true> {
  typedef OpenBwdArgsPid<PMS> type;
};
#define OB_KMAX ((MCP_MAX_INPUT + 3) / 4)  // inputs per lane of the chain wave

struct OpenBwdLayout {
  int rec, xs, gs, lam, gd, gz, tab, total;  // offsets in doubles
  int rp;                                    // pitch of a trajectory's record row (odd: bank spread)
  int ul, gul, tgl, abl, ktab, gnl;          // feedback form: inputs | g_inputs | target row (double buffers) | abar | kpos, kvel | gains^2
  int yml, car, mtab;                        // measured feedback form: measurement rows (double buffer) | the filter's carries | pvel, ppos
  int itl, gil;                              // integral form: the integral's rows (double buffer; stage B' leaves the carry there) | sqrt_ki^2, i_max
  int gnr;                                   // time-varying form: the gain rows [2][U][S] (double buffer); abar is [2][OB_PT][U] there
};
__host__ __device__ inline OpenBwdLayout open_bwd_layout(int S, int G, int D, bool fb = false, int U = 0, bool pms = false, bool pid = false,
                                                         bool tvl = false) {
  OpenBwdLayout L;
  int o = 0;
  auto take = [&](int n) {
    int r = o;
    o += (n + 1) & ~1;
    return r;
  };
  L.rp = (G * D) | 1;
  L.rec = take(2 * OB_PT * L.rp);
  L.xs = take(2 * OB_PT * S);
  L.gs = take(2 * OB_PT * S);
  L.lam = take(2 * OB_PT * S);
  L.gd = take(OB_PT * G);
  L.gz = take(OB_PT * D);
  L.tab = take((5 * MCP_MAX_STATE + OB_PT) / 2 + 2);  // ints: og | ispos | velof | zplain | zang (per state component), len (per trajectory)
  L.ul = fb ? take(2 * OB_PT * U) : 0;
  L.gul = fb ? take(2 * OB_PT * U) : 0;
  L.tgl = fb ? take(2 * S) : 0;
  L.abl = fb ? take((tvl ? 2 : 1) * OB_PT * U) : 0;
  L.ktab = fb ? take(MCP_MAX_STATE) : 0;  // ints: kpos | kvel (per state component: the input that reads it as position / velocity, or -1)
  L.gnl = fb ? take(2 * MCP_MAX_INPUT) : 0;  // sqrt_kp^2 | sqrt_kd^2
  L.yml = pms ? take(2 * OB_PT * S) : 0;
  L.car = pms ? take(2 * OB_PT * S) : 0;     // [trajectory][position component]: mvbar | nvbar of the row behind
  L.mtab = pms ? take(MCP_MAX_STATE) : 0;    // ints: pvel (per state component: the velocity of the pair it is the position of, or -1) | ppos (the converse)
  L.itl = pid ? take(2 * OB_PT * U) : 0;
  L.gil = pid ? take(2 * MCP_MAX_INPUT) : 0;  // the gain table's second half: sqrt_ki^2 | i_max
  L.gnr = tvl ? take(2 * U * S) : 0;
  L.total = o;
  return L;
}

template <bool FB, bool PMS = false, bool PID = false, bool TVL = false>
__global__ __launch_bounds__(OB_NT) void rollout_open_bwd_kernel(typename OpenBwdArgsOf<FB, PMS, PID, TVL>::type a) {
  static_assert(FB || !PMS, "the measurement model belongs to the feedback form");
  static_assert(FB || !PID, "the integral term belongs to the feedback form");
  static_assert((FB && !PID) || !TVL, "the time-varying law is a feedback form of its own");
  extern __shared__ double smem[];
  const int S = a.S, U = a.U, G = a.G, D = a.D, M = a.M, T = a.T, nna = a.nna, na = a.na;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const OpenBwdLayout L = open_bwd_layout(S, G, D, FB, U, PMS, PID, TVL);
  const int GD = G * D, RP = L.rp;
  double* rec = smem + L.rec;
  double* xsl = smem + L.xs;
  double* gsl = smem + L.gs;
  double* lam = smem + L.lam;
  double* gdl = smem + L.gd;
  double* gzl = smem + L.gz;
  int* ogt = reinterpret_cast<int*>(smem + L.tab);
  int* post = ogt + MCP_MAX_STATE;
  int* velof = post + MCP_MAX_STATE;
  int* zplain = velof + MCP_MAX_STATE;
  int* zang = zplain + MCP_MAX_STATE;
  int* lenl = zang + MCP_MAX_STATE;
  double* ull = smem + L.ul;   // (feedback form)
  double* gul = smem + L.gul;
  double* tgl = smem + L.tgl;
  double* abl = smem + L.abl;
  int* kpos = reinterpret_cast<int*>(smem + L.ktab);
  int* kvel = kpos + MCP_MAX_STATE;
  double* gnl = smem + L.gnl;
  double* yml = smem + L.yml;  // (measured feedback form)
  double* car = smem + L.car;
  int* pvel = reinterpret_cast<int*>(smem + L.mtab);
  int* ppos = pvel + MCP_MAX_STATE;
  double* itl = smem + L.itl;  // (integral form)
  double* gil = smem + L.gil;
  double* gnr = smem + L.gnr;  // (time-varying form)
  (void)gnr;
  const int m0 = blockIdx.x * OB_PT;

  if (tid < S) {  // which GP a component integrates, as the forward kernel decides it
    const int s = tid;
    int g_vel = -1, g_pos = -1, zp = -1, za = -1;
    for (int g = 0; g < G; ++g) {
      if (a.vel[g] == s) g_vel = g;
      if (a.not_vel[g] == s) g_pos = g;
    }
    for (int i = 0; i < nna; ++i)
      if (a.not_angle[i] == s) zp = i;
    for (int i = 0; i < na; ++i)
      if (a.angle[i] == s) za = i;
    ogt[s] = g_pos >= 0 ? g_pos : g_vel;
    post[s] = g_pos >= 0 ? 1 : 0;
    velof[s] = g_pos >= 0 ? a.vel[g_pos] : -1;
    zplain[s] = zp;
    zang[s] = za;
    if constexpr (FB && !TVL) {
      int kp = -1, kv = -1;
      for (int k = 0; k < U; ++k) {
        if (a.pd.pos[k] == s) kp = k;
        if (a.pd.vel[k] == s) kv = k;
      }
      kpos[s] = kp;
      kvel[s] = kv;
    }
    if constexpr (PMS) {
      int pv = -1, pp = -1;
      for (int i = 0; i < a.ms.n; ++i) {
        if (a.ms.pos[i] == s) pv = a.ms.vel[i];
        if (a.ms.vel[i] == s) pp = a.ms.pos[i];
      }
      pvel[s] = pv;
      ppos[s] = pp;
    }
  }
  if constexpr (FB && !TVL) {
    if (tid >= 64 + OB_PT && tid < 64 + OB_PT + U) {
      const int k = tid - 64 - OB_PT;
      const double kp = a.pd.sqrt_kp[k], kd = a.pd.sqrt_kd[k];
      gnl[k] = kp * kp;
      gnl[MCP_MAX_INPUT + k] = kd * kd;
      if constexpr (PID) {
        const double ki = a.pid.sqrt_ki[k];
        gil[k] = ki * ki;
        gil[MCP_MAX_INPUT + k] = a.pid.i_max[k];
      }
    }
  }
  if (tid >= 64 && tid < 64 + OB_PT) {
    const int p = tid - 64;
    lenl[p] = m0 + p < M ? (a.lengths ? imin(imax(a.lengths[m0 + p], 1), T) : T) : 0;
  }
  for (int it = tid; it < 2 * OB_PT * S; it += OB_NT) lam[it] = 0.0;
  if constexpr (PMS)
    for (int it = tid; it < 2 * OB_PT * S; it += OB_NT) car[it] = 0.0;
  if constexpr (TVL)  // (the absent trajectories of a ragged tile never write their abar)
    for (int it = tid; it < 2 * OB_PT * U; it += OB_NT) abl[it] = 0.0;
  __syncthreads();
  int tl = 1;
  for (int p = 0; p < OB_PT; ++p) tl = imax(tl, lenl[p]);
  if (a.g_u) {  // rows from len - 1 on: zeros
    for (int p = 0; p < OB_PT; ++p) {
      const int len = lenl[p];
      if (len == 0) continue;
      for (int it = (len - 1) * U + tid; it < (T - 1) * U; it += OB_NT) {
        const int t = it / U, k = it - t * U;
        a.g_u[((size_t)t * M + m0 + p) * U + k] = 0.0;
      }
    }
  }

  // the loader's work for one row (64 lanes): g_states[r] where r <= len - 1; states[r] and jac[r] where r < len - 1
  auto load_row = [&](int r, int b, int l) {
    for (int it = l; it < OB_PT * S; it += 64) {
      const int p = it / S, s = it - p * S;
      const int len = lenl[p];
      if (r <= len - 1) gsl[(b * OB_PT + p) * S + s] = a.g_states[((size_t)r * M + m0 + p) * S + s];
      if (r < len - (FB ? 0 : 1)) xsl[(b * OB_PT + p) * S + s] = a.states[((size_t)r * M + m0 + p) * S + s];
      if constexpr (PMS)
        if (r <= len - 1) yml[(b * OB_PT + p) * S + s] = a.ms.meas[((size_t)r * M + m0 + p) * S + s];
    }
    if constexpr (FB) {
      for (int it = l; it < OB_PT * U; it += 64) {
        const int p = it / U, k = it - p * U;
        if (r <= lenl[p] - 1) {
          ull[(b * OB_PT + p) * U + k] = a.inputs[((size_t)r * M + m0 + p) * U + k];
          gul[(b * OB_PT + p) * U + k] = a.g_inputs ? a.g_inputs[((size_t)r * M + m0 + p) * U + k] : 0.0;
          if constexpr (PID) itl[(b * OB_PT + p) * U + k] = a.pid.integ[((size_t)r * M + m0 + p) * U + k];
        }
      }
      for (int s = l; s < S; s += 64) tgl[b * S + s] = a.pd.target_traj[(size_t)r * S + s];
      if constexpr (TVL)
        for (int it = l; it < U * S; it += 64) gnr[b * U * S + it] = a.gain[(a.gain_rows == 1 ? (size_t)0 : (size_t)r * U * S) + it];
    }
    for (int it = l; it < OB_PT * GD; it += 64) {
      const int p = it / GD, e = it - p * GD;
      if (r < lenl[p] - 1) rec[(b * OB_PT + p) * RP + e] = a.jac[((size_t)r * M + m0 + p) * GD + e];
    }
  };

  // time-varying form, the loader's other work (64 lanes): the row's partial of the parameter gradient, from the row's buffer half `bb`
  // and the abar of its parity -- the tile's valid trajectories are added in a fixed tree
  auto reduce_row = [&](int r, int bb, int l) {
    if constexpr (TVL) {
      if (!a.g_part) return;
      const int npv = imin(OB_PT, M - m0);
      const double* ab = abl + (r & 1) * OB_PT * U;
      const double* er = (PMS ? yml : xsl) + bb * OB_PT * S;
      double* out = a.g_part + ((size_t)blockIdx.x * T + r) * U * (S + 1);
      const int pq = 4 * (l >> 4);  // this quarter of the wave adds trajectories pq .. pq + 3; the quarters meet by the row / half swaps
      for (int i0 = 0; i0 < U * (S + 1); i0 += 16) {  // (uniform: the swaps want every lane)
        const int it = i0 + (l & 15);
        const bool on = it < U * (S + 1);
        const int k = on ? it / (S + 1) : 0, s = on ? it - k * (S + 1) : 0;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int p = pq + i;
          const double v = s < S ? ab[p * U + k] * (tgl[bb * S + s] - er[p * S + s]) : ab[p * U + k];
          acc += p < npv ? v : 0.0;  // (an absent trajectory's row of the buffer was never written)
        }
        acc = sum_xor32(sum_xor16(acc));  // (p 0-3 + p 4-7) + (p 8-11 + p 12-15), the same bits in every quarter
        if (on && l < 16) out[it] = acc;
      }
    }
  };

  int b = 0, lc = 0;
  // feedback form: this lane's inputs q, q + 4, ... of trajectory p and the running sums of their gain gradients
  double fkp[OB_KMAX], fkd[OB_KMAX], fum[OB_KMAX], gkp[OB_KMAX], gkd[OB_KMAX];
  int fpos[OB_KMAX], fvel[OB_KMAX];
  if constexpr (TVL) {
#pragma unroll
    for (int i = 0; i < OB_KMAX; ++i) {
      const int k = (lane >> 4) + 4 * i;
      fum[i] = k < U ? a.pd.u_max[k] : 1.0;
    }
  }
  if constexpr (FB && !TVL) {
#pragma unroll
    for (int i = 0; i < OB_KMAX; ++i) {
      const int k = (lane >> 4) + 4 * i;
      fkp[i] = k < U ? a.pd.sqrt_kp[k] : 0.0;
      fkd[i] = k < U ? a.pd.sqrt_kd[k] : 0.0;
      fum[i] = k < U ? a.pd.u_max[k] : 1.0;
      fpos[i] = k < U ? a.pd.pos[k] : 0;
      fvel[i] = k < U ? a.pd.vel[k] : 0;
      gkp[i] = gkd[i] = 0.0;
    }
  }
  // integral form: sqrt_ki of the same inputs, the sums of its gradient and the carry c (zero behind the last row)
  double fki[OB_KMAX], gki[OB_KMAX], cin[OB_KMAX];
  if constexpr (PID) {
#pragma unroll
    for (int i = 0; i < OB_KMAX; ++i) {
      const int k = (lane >> 4) + 4 * i;
      fki[i] = k < U ? a.pid.sqrt_ki[k] : 0.0;
      gki[i] = cin[i] = 0.0;
    }
  }
  if (wv == 1) load_row(tl - 1, 0, lane);
  __syncthreads();
  for (int r = tl - 1; r >= 0; --r) {
    if (wv == 1) {
      if (r < tl - 1) reduce_row(r + 1, b ^ 1, lane);  // (before that half is refilled)
      if (r > 0) load_row(r - 1, b ^ 1, lane);
    } else {
      const int p = lane & 15, q = lane >> 4;
      const int len = lenl[p];
      const double* lamc = lam + (lc * OB_PT + p) * S;
      double* lamn = lam + ((lc ^ 1) * OB_PT + p) * S;
      const double* rc = rec + (b * OB_PT + p) * RP;
      const double* xc = xsl + (b * OB_PT + p) * S;
      const double* gc = gsl + (b * OB_PT + p) * S;
      const bool active = r < len - 1;
      const double* ec = PMS ? yml + (b * OB_PT + p) * S : xc;  // what the PD law read of row r
      (void)ec;
      // stage A: the adjoints of the increments
      for (int g = q; g < G; g += 4) {
        double acc = 0.0;
        for (int s = 0; s < S; ++s)
          if (ogt[s] == g) acc += post[s] ? 0.5 * a.Ts * lamc[s] : lamc[s];
        gdl[p * G + g] = acc;
      }
      wave_lds_sync();
      // stage B: through the record to the GP input
      if (active) {
        for (int d = q; d < D; d += 4) {
          double acc = 0.0;
          for (int g = 0; g < G; ++g) acc = fma(gdl[p * G + g], rc[g * D + d], acc);
          gzl[p * D + d] = acc;
        }
      }
      wave_lds_sync();
      if constexpr (FB) {  // stage B': through the squashing to the PD law's argument; the gains' sums
        if (r <= len - 1) {
          const double* tg = tgl + b * S;
#pragma unroll
          for (int i = 0; i < OB_KMAX; ++i) {
            const int k = q + 4 * i;
            if (k < U) {
              double gu = gul[(b * OB_PT + p) * U + k];
              if (active) gu += gzl[p * D + nna + 2 * na + k];
              double ab = gu;
              if (a.pd.squash) {
                const double th = ull[(b * OB_PT + p) * U + k] / fum[i];
                ab = gu * (1.0 - th * th);
              }
              abl[(TVL ? (r & 1) * OB_PT * U : 0) + p * U + k] = ab;
              if constexpr (!TVL) {
                gkp[i] += 2.0 * fkp[i] * (tg[fpos[i]] - ec[fpos[i]]) * ab;
                gkd[i] += 2.0 * fkd[i] * (tg[fvel[i]] - ec[fvel[i]]) * ab;
              }
              if constexpr (PID) {
                double* ir = itl + (b * OB_PT + p) * U + k;
                const double iv = *ir;
                const double ib = gil[k] * ab + cin[i];
                cin[i] = fabs(iv) < gil[MCP_MAX_INPUT + k] ? ib : 0.0;
                gki[i] += 2.0 * fki[i] * iv * ab;
                *ir = cin[i];  // (to stage C)
              }
            }
          }
        }
        wave_lds_sync();
      }
      // stage C: the integrator and the feature map
      for (int s = q; s < S; s += 4) {
        double v = 0.0;
        if (r == len - 1) {
          v = gc[s];
        } else if (active) {
          v = gc[s];
          if (ogt[s] >= 0) v += lamc[s];
          for (int s2 = 0; s2 < S; ++s2)
            if (velof[s2] == s) v = fma(a.Ts, lamc[s2], v);
          if (zplain[s] >= 0) v += gzl[p * D + zplain[s]];
          if (zang[s] >= 0) {
            double sn, cs;
            sincos_fast(xc[s], &sn, &cs);
            v += gzl[p * D + nna + zang[s]] * cs - gzl[p * D + nna + na + zang[s]] * sn;
          }
        }
        // time-varying form: the dense pull of the law on component c of the row it read
        auto tvl_pull = [&](int c) {
          const double* gr = gnr + b * U * S + c;
          const double* ab = abl + (r & 1) * OB_PT * U + p * U;
          double y = 0.0;
          for (int k = 0; k < U; ++k) y -= gr[k * S] * ab[k];
          return y;
        };
        (void)tvl_pull;
        if constexpr (TVL && !PMS) {
          if (r <= len - 1) v += tvl_pull(s);
        }
        if constexpr (FB && !PMS && !TVL) {
          if (r <= len - 1) {
            const int kp = kpos[s], kv = kvel[s];
            if (kp >= 0) v -= gnl[kp] * abl[p * U + kp];
            if constexpr (PID)
              if (kp >= 0) v -= a.pid.dt * itl[(b * OB_PT + p) * U + kp];
            if (kv >= 0) v -= gnl[MCP_MAX_INPUT + kv] * abl[p * U + kv];
          }
        }
        if constexpr (PMS) {
          if (r <= len - 1) {
            auto ybar = [&](int c) {  // the policy's pull on component c of the measurement
              if constexpr (TVL) return tvl_pull(c);
              const int kp = kpos[c], kv = kvel[c];
              double y = 0.0;
              if (kp >= 0) y -= gnl[kp] * abl[p * U + kp];
              if constexpr (PID)
                if (kp >= 0) y -= a.pid.dt * itl[(b * OB_PT + p) * U + kp];
              if (kv >= 0) y -= gnl[MCP_MAX_INPUT + kv] * abl[p * U + kv];
              return y;
            };
            const int pv = pvel[s], pp = ppos[s];
            if (pv >= 0) {  // a measured position: the filter's adjoint of its pair
              double* cr = car + (p * S + s) * 2;
              const double mvn = cr[0], nvn = cr[1];
              if (r >= 1) {
                const double mvb = ybar(pv) - (a.ms.a1 / a.ms.a0) * mvn;
                const double nvb = (a.ms.b0 / a.ms.a0) * mvb + (a.ms.b1 / a.ms.a0) * mvn;
                v += ybar(s) + (nvb - nvn) / a.Ts;
                cr[0] = mvb;
                cr[1] = nvb;
              } else {
                v += ybar(s) - nvn / a.Ts;
              }
            } else if (pp >= 0) {  // a measured velocity: seen true in row 0 only, where it also started both histories
              if (r == 0) v += ybar(s) + ((a.ms.b1 - a.ms.a1) / a.ms.a0) * car[(p * S + pp) * 2];
            } else {
              v += ybar(s);
            }
          }
        }
        lamn[s] = v;
      }
      if (active && a.g_u)
        for (int k = q; k < U; k += 4) a.g_u[((size_t)r * M + m0 + p) * U + k] = gzl[p * D + nna + 2 * na + k];
      wave_lds_sync();
      lc ^= 1;
    }
    __syncthreads();
    b ^= 1;
  }
  if (wv == 0 && a.g_x0) {
    const int p = lane & 15, q = lane >> 4;
    if (lenl[p] > 0)
      for (int s = q; s < S; s += 4) a.g_x0[(size_t)(m0 + p) * S + s] = lam[(lc * OB_PT + p) * S + s];
  }
  if constexpr (TVL) {
    if (wv == 1) reduce_row(0, b ^ 1, lane);  // (row 0's abar came out of the last iteration)
  }
  if constexpr (FB && !TVL) {
    if (wv == 0 && a.g_gains) {
      const int p = lane & 15, q = lane >> 4;
      if (lenl[p] > 0) {
#pragma unroll
        for (int i = 0; i < OB_KMAX; ++i) {
          const int k = q + 4 * i;
          if (k < U) {
            a.g_gains[((size_t)(m0 + p) * (PID ? 3 : 2) + 0) * U + k] = gkp[i];
            a.g_gains[((size_t)(m0 + p) * (PID ? 3 : 2) + 1) * U + k] = gkd[i];
            if constexpr (PID) a.g_gains[((size_t)(m0 + p) * 3 + 2) * U + k] = gki[i];
          }
        }
      }
    }
  }
}

// ---- host path of the sweeps: checks -> fill -> launch ---------------------------------------------------------------------------------
// (the sweeps run from the record: they check the model's scalars and index lists, model_lists_ok, and never look at a GP descriptor)
static void open_bwd_fill(OpenBwdArgs& a, const mcp_model* model, int M, int T, const double* states, const int32_t* lengths, const double* jac,
                          const double* g_states, double* g_x0, double* g_u) {
  sweep_fill_model(a, model, M, T);
  a.states = states;
  a.jac = jac;
  a.g_states = g_states;
  a.lengths = lengths;
  a.g_x0 = g_x0;
  a.g_u = g_u;
}
// (at every compiled limit at once the layout takes 72 KB, the feedback form 89 KB, the measured form 98 KB, the integral 2 KB more, the time-varying law 3 KB more)
template <bool FB, bool PMS, bool PID = false, bool TVL = false>
static int launch_open_bwd(const typename OpenBwdArgsOf<FB, PMS, PID, TVL>::type& a, hipStream_t st) {
  const OpenBwdLayout L = open_bwd_layout(a.S, a.G, a.D, FB, a.U, PMS, PID, TVL);
  const size_t lds = (size_t)L.total * sizeof(double);
  if (lds > MCP_LDS_LIMIT) return MCP_ERR_LIMIT;
  MCP_ENSURE_MAX_LDS((rollout_open_bwd_kernel<FB, PMS, PID, TVL>));
  hipLaunchKernelGGL((rollout_open_bwd_kernel<FB, PMS, PID, TVL>), dim3((a.M + OB_PT - 1) / OB_PT), dim3(OB_NT), lds, st, a);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_rollout_open_bwd(const mcp_model* model, int M, int T, const double* states, const int32_t* lengths, const double* jac,
                                    const double* g_states, double* g_x0, double* g_u, void* stream) {
  if (!model || !states || !jac || !g_states) return MCP_ERR_ARG;
  if (M <= 0 || T < 2) return MCP_ERR_ARG;
  if (!model_within_limits(model, false)) return MCP_ERR_LIMIT;
  if (!model_lists_ok(model)) return MCP_ERR_ARG;
  if (!g_x0 && !g_u) return MCP_OK;  // nothing asked for
  OpenBwdArgs a;
  memset(&a, 0, sizeof(a));
  open_bwd_fill(a, model, M, T, states, lengths, jac, g_states, g_x0, g_u);
  return launch_open_bwd<false, false>(a, (hipStream_t)stream);
}

// Reverse-time sweep of the closed loop under the PD law: replaces autograd's backward (MC_PILCO.py:522) through the loop of
// MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674), Policy.PD_controller.forward (policy_learning/Policy.py:437-449) and
// get_next_state with its integrators (model_learning/Model_learning.py:210-229, 471-494, 685-718), from the record alone.
static int pd_bwd_dispatch(const mcp_model* model, const mcp_pd_policy* pd, const mcp_meas* ms, int M, int T, const double* states,
                           const double* inputs, const double* jac, const double* g_states, const double* g_inputs, double* g_gains, double* g_x0,
                           void* stream, const mcp_pid_term* pid = nullptr) {
  int crc = closed_loop_checks(model && pd && states && inputs && g_states && (jac || T <= 1), M, T, model, ms, true,
                               [&] { return pd_policy_check(model, pd, T); });
  if (crc == MCP_OK) crc = pid_term_check(pid, pd->U);
  if (crc != MCP_OK) return crc;
  if (!g_x0 && !g_gains) return MCP_OK;  // nothing asked for
  OpenBwdArgsPdMeas a;
  memset(&a, 0, sizeof(a));
  open_bwd_fill(a, model, M, T, states, nullptr, jac, g_states, g_x0, nullptr);
  a.pd = *pd;
  a.inputs = inputs;
  a.g_inputs = g_inputs;
  a.g_gains = g_gains;
  hipStream_t st = (hipStream_t)stream;
  if (pid_active(pid)) {
    if (!meas_active(ms)) return launch_open_bwd<true, false, true>(pd_with_pid<OpenBwdArgsPid<false>, OpenBwdArgsPd>(a, pid), st);
    a.ms = *ms;
    return launch_open_bwd<true, true, true>(pd_with_pid<OpenBwdArgsPid<true>, OpenBwdArgsPdMeas>(a, pid), st);
  }
  if (meas_active(ms)) {
    a.ms = *ms;
    return launch_open_bwd<true, true>(a, st);
  }
  return launch_open_bwd<true, false>(a, st);  // (the base part of `a`: mcp_rollout_pd_bwd's own kernel)
}

extern "C" int mcp_rollout_pd_bwd(const mcp_model* model, const mcp_pd_policy* pd, int M, int T, const double* states, const double* inputs,
                                  const double* jac, const double* g_states, const double* g_inputs, double* g_gains, double* g_x0,
                                  void* stream) {
  return pd_bwd_dispatch(model, pd, nullptr, M, T, states, inputs, jac, g_states, g_inputs, g_gains, g_x0, stream);
}

// Reverse-time sweep of the closed loop under the PD law on the simulated measurement: replaces autograd's backward (MC_PILCO.py:522)
// through the loop of MC_PILCO4PMS.apply_policy (policy_learning/MC_PILCO.py:808-906, the filter recursion included),
// Policy.PD_controller.forward (policy_learning/Policy.py:437-449) and get_next_state with its integrators
// (model_learning/Model_learning.py:210-229, 471-494, 685-718), from the record and meas->meas alone.  meas->n == 0: mcp_rollout_pd_bwd's kernel.
extern "C" int mcp_rollout_pd_meas_bwd(const mcp_model* model, const mcp_pd_policy* pd, const mcp_meas* meas, int M, int T, const double* states,
                                       const double* inputs, const double* jac, const double* g_states, const double* g_inputs, double* g_gains,
                                       double* g_x0, void* stream) {
  if (!meas) return MCP_ERR_ARG;
  return pd_bwd_dispatch(model, pd, meas, M, T, states, inputs, jac, g_states, g_inputs, g_gains, g_x0, stream);
}

// Reverse-time sweep of mcp_rollout_pid (the carry of the integral's adjoint: OpenBwdArgsPid above): replaces autograd's backward
// (MC_PILCO.py:522) through the same loops with a stateful torch policy in them.  g_gains [M][3][U].  pid NULL or on == 0:
// mcp_rollout_pd_bwd / mcp_rollout_pd_meas_bwd on the same arguments (g_gains [M][2][U]).
extern "C" int mcp_rollout_pid_bwd(const mcp_model* model, const mcp_pd_policy* pd, const mcp_pid_term* pid, const mcp_meas* meas, int M, int T,
                                   const double* states, const double* inputs, const double* jac, const double* g_states, const double* g_inputs,
                                   double* g_gains, double* g_x0, void* stream) {
  return pd_bwd_dispatch(model, pd, meas, M, T, states, inputs, jac, g_states, g_inputs, g_gains, g_x0, stream, pid);
}

// Reverse-time sweep of mcp_rollout_tvl (the dense pull and the per-row partials: OpenBwdArgsTvl above): replaces autograd's backward
// (MC_PILCO.py:522) through the loops named at the forward entry with a torch policy in them.  g_part [ceil(M/16)][T][U][S+1].
extern "C" int mcp_rollout_tvl_bwd(const mcp_model* model, const mcp_tvl_policy* tvl, const mcp_meas* meas, int M, int T, const double* states,
                                   const double* inputs, const double* jac, const double* g_states, const double* g_inputs, double* g_part,
                                   double* g_x0, void* stream) {
  const int crc = closed_loop_checks(model && tvl && states && inputs && g_states && (jac || T <= 1), M, T, model, meas, true,
                                     [&] { return tvl_policy_check(model, tvl, T); });
  if (crc != MCP_OK) return crc;
  if (!g_x0 && !g_part) return MCP_OK;  // nothing asked for
  OpenBwdArgsTvl<true> a;
  memset(&a, 0, sizeof(a));
  open_bwd_fill(a, model, M, T, states, nullptr, jac, g_states, g_x0, nullptr);
  a.pd = tvl_as_pd(tvl);
  a.inputs = inputs;
  a.g_inputs = g_inputs;
  a.gain = tvl->gain, a.gain_rows = tvl->gain_rows, a.g_part = g_part;
  hipStream_t st = (hipStream_t)stream;
  if (meas_active(meas)) {
    a.ms = *meas;
    return launch_open_bwd<true, true, false, true>(a, st);
  }
  OpenBwdArgsTvl<false> b;
  static_cast<OpenBwdArgsPd&>(b) = a;
  b.gain = a.gain, b.gain_rows = a.gain_rows, b.g_part = a.g_part;
  return launch_open_bwd<true, false, false, true>(b, st);
}
