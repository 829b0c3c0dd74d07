// Sampling MPC on the model for gfx950 (MI355X): the MPPI rollout-cost and update, mcp_mppi_rollout / mcp_mppi_update (the project's own:
// the reference has no planner).  One planning iteration is three launches and no buffer of size [H][M]:
//   mppi_rollout_kernel<PT, MAXDEG, NEEDVAR>   the open-loop step loop of rollout_open.hip over the shared phases of rollout_open_phases.h
//                                              (K, V and the statements of F: the same operations on the same operands, so a trajectory
//                                              carries mcp_rollout_open's bits), with two differences:
//       input    u_t is not read from a buffer: the LAST PT * U threads of the workgroup form  squash(a[t] + sigma xi(k, t, .))  from the
//                nominal rows in LDS (the layout's `ext` region) and a perturbation that is read, or drawn from Philox stream
//                MCP_STREAM_PLAN, ONE ROW AHEAD: u_{t+1} is formed behind the barrier that opens phase K of step t and kept in a
//                register -- the inputs do not depend on the state, so nothing of them sits on the step's serial chain.  Those threads
//                have the highest training indices of phase K (none below Npad ~ 370): the draw hides behind the others' kernel rows.
//       cost     the PT threads in front of them each own a trajectory of the tile: behind the same barrier the thread reads x_t from
//                the published xs row and u_t, u_{t-1} from a two-row LDS buffer, evaluates cost_u_point / cost_point (cost_point.h: the
//                cost kernels' own text) at target row t0 + t and adds w_t c to a running sum in a register; one store per trajectory
//                at the end.  states / inputs are written only when the caller asks.
//     Common random numbers: the GP increment of trajectory m = k P + p is drawn with particle id p (eps [H-1][P][G], or Philox).
//   mppi_weights_kernel   one workgroup: S_k per candidate, the minimum over the finite ones, the softmax weights, the statistics
//   mppi_mean_kernel      one workgroup per row t: a_new[t] = a[t] + sigma sum_k w_k xi(k, t, .), the perturbations regenerated
// Every sum of the update runs in a fixed order (mppi_block_sum); no atomics on results.
// Under mcp_plan_ext (mcp_plan_rollout, mcp_mppi_update_ext, mcp_cem_update):
//   mppi_rollout_kernel<.., EXT = true>   the same kernel with the input threads reading the std of row t from one more [H][U] block of the
//                                         `ext` region, carrying the AR(1) perturbation xi_t = fma(beta, xi_{t-1}, c n_t) in a register -- still
//                                         one row ahead, off the chain -- and staging u_prev in the row -1 slot of the two-row input buffer.
//                                         EXT is a template flag and the extended form has its own argument type: the EXT = false
//                                         instantiations are the kernels mcp_mppi_rollout always launched.
//   mppi_mean_kernel<RAW> + mppi_filter_kernel   the weighted sums of the WHITE normals per row, then the AR(1) filter over those H U sums
//   cem_select_kernel, cem_fit_kernel     the elite set (an on-device radix select and an LDS sort) and the fit of mean and std to it
// Under mcp_plan_batch (mcp_plan_batch_rollout, mcp_plan_batch_update, mcp_cem_batch_update): B problems of one shape in the launches of one.
//   mppi_rollout_kernel<.., BATCH = true>   a grid of (tiles, B): workgroup (., b) is a workgroup of the single-problem launch on problem b's
//                                           operands (PlanProb); a tile never spans two problems
//   *_batch_kernel                          the update kernels' bodies on B workgroups (weights, select, filter), (H, B) (mean), (U, B) (fit)
//   Problem b's slice of every output carries the bits of the single-problem entry: nothing is reduced across problems.
#include "cost_point.h"
#include "rollout_open_phases.h"

#include <type_traits>

using namespace mcp;

struct MppiArgs : OpenArgs {
  mcp_mppi mp;
  mcp_cost cost;
  mcp_cost_inputs cin;
  int has_cin;
  double* traj_cost;  // [M]
  double* inputs;     // [H][M][U] or NULL
};

// what mcp_plan_rollout's own form takes on top (mcp_plan_ext): a separate argument type, so that the plain form's kernel argument -- and
// with it its code and resource numbers -- is what it was before the extension existed
struct PlanArgs : MppiArgs {
  const double* sigma_rows;  // [H][U] or NULL: mp.sigma per row
  const double* u_prev;      // [U] or NULL
  double beta, cnew;         // xi_t = fma(beta, xi_{t-1}, cnew n_t), cnew = sqrt(1 - beta^2) formed once on the host
};
template <bool EXT>
using MppiKernelArgs = typename std::conditional<EXT, PlanArgs, MppiArgs>::type;

// doubles of the layout's `ext` region: the nominal [H][U] | u_t, u_{t-1} of the tile's trajectories [2][PT][U] | -- the extended form only --
// the std of every row [H][U]
__host__ __device__ inline int mppi_extra(int PT, int H, int U, bool ext = false) { return H * U + 2 * PT * U + (ext ? H * U : 0); }

// xi(k, t, u): 0 for the nominal's candidate, else the buffer's entry or the Philox normal
__device__ __forceinline__ double mppi_xi(const mcp_mppi& mp, const mcp_noise& nzl, int k, int t, int u) {
  if (k == 0) return 0.0;
  return mp.xi ? mp.xi[((size_t)t * mp.K + k) * mp.U + u] : philox_normal(nzl, k, t, u, MCP_STREAM_PLAN);
}

// ---- the batched forms (mcp_plan_batch_rollout, mcp_plan_batch_update, mcp_cem_batch_update) ------------------------------------------------
// BATCH is a template flag like EXT.  With BATCH = false every operand is the kernel argument itself and `pb` is never read: the rollout's
// BATCH = false instantiations are the kernels mcp_mppi_rollout / mcp_plan_rollout always launched (the batched form has its own argument
// type), and the update kernels keep their names and arguments over bodies they share with thin batched kernels.  With BATCH = true the
// problem b is a grid coordinate and the operands that differ between problems come from `pb`: the arguments moved to problem b's slices.
// `BATCH ? pb.x : arg.x` is decided where the template is instantiated.
struct PlanProb {
  const double *x0, *a, *xi, *sigma_rows, *u_prev;
  double *traj_cost, *states, *inputs;
  uint32_t* status;
  int x0_per_particle;
  mcp_noise nz;
};
// the noise of problem b: the launch's (the device counter folded in: the bodies' own noise_of_launch finds none) at particle_offset +
// b * particle_stride, with the b-th eps buffer
__device__ __forceinline__ mcp_noise noise_of_problem(const mcp_noise& nz, const mcp_plan_batch& bt, size_t b) {
  mcp_noise r = noise_of_launch(nz);
  r.call_dev = nullptr;
  r.particle_offset += (int64_t)b * bt.particle_stride;
  if (r.eps) r.eps += b * (size_t)bt.eps_stride;
  return r;
}
// mppi_xi over the problem's own buffer
__device__ __forceinline__ double plan_xi(const mcp_mppi& mp, const double* xi, const mcp_noise& nzl, int k, int t, int u) {
  if (k == 0) return 0.0;
  return xi ? xi[((size_t)t * mp.K + k) * mp.U + u] : philox_normal(nzl, k, t, u, MCP_STREAM_PLAN);
}

// sin and cos of a state angle with sincos_fast's bits, lane by lane.  sincos_fast sends the WHOLE wave through the library routine when one
// lane is outside its range (NaN / inf included), and the two routines differ in the last bit here and there: a candidate lost to a NaN
// perturbation would move the states of the healthy trajectories that share its wave -- and with them their costs and the plan.  A
// planner drops such a candidate and keeps the rest, so the rest must not depend on it: lanes outside the range go through the library
// routine alone, the others see a wave that is inside it.  On a wave without such a lane these are sincos_fast's (and so
// mcp_rollout_open's) bits.
__device__ __forceinline__ void mppi_sincos(double x, double* sp, double* cp) {
  const bool far = !(fabs(x) < 1.0e5);
  sincos_fast(far ? 0.0 : x, sp, cp);
  if (__builtin_expect(far, 0)) sincos(x, sp, cp);
}

// the batched rollout's arguments: the single-problem form's with the batch descriptor behind them, on a grid of (tiles, B) -- workgroup
// (., b) is a workgroup of the single-problem launch on problem b's operands
template <bool EXT>
struct PlanBatchArgs : MppiKernelArgs<EXT> {
  mcp_plan_batch bt;
};
template <bool EXT, bool BATCH>
using LaunchArgs = typename std::conditional<BATCH, PlanBatchArgs<EXT>, MppiKernelArgs<EXT>>::type;

// problem b of a batched rollout
template <bool EXT>
__device__ __forceinline__ PlanProb rollout_problem(const PlanBatchArgs<EXT>& a, size_t b) {
  const size_t M = a.M, T = a.T, S = a.model.S, U = a.model.U;
  PlanProb pb;
  pb.x0_per_particle = a.bt.x0_per_particle;
  pb.x0 = a.x0 + b * (a.bt.x0_per_particle ? (size_t)a.mp.P * S : S);
  pb.a = a.mp.a + b * T * U;
  pb.xi = a.mp.xi ? a.mp.xi + b * (size_t)a.bt.xi_stride : nullptr;
  pb.sigma_rows = pb.u_prev = nullptr;
  if constexpr (EXT) {
    pb.sigma_rows = a.sigma_rows ? a.sigma_rows + b * T * U : nullptr;
    pb.u_prev = a.u_prev ? a.u_prev + b * U : nullptr;
  }
  pb.traj_cost = a.traj_cost + b * M;
  pb.states = a.states ? a.states + b * T * M * S : nullptr;
  pb.inputs = a.inputs ? a.inputs + b * T * M * U : nullptr;
  pb.status = a.status + b;
  pb.nz = noise_of_problem(a.nz, a.bt, b);
  return pb;
}

template <int PT, int MAXDEG, bool NEEDVAR, bool EXT, bool BATCH = false>
__global__ __launch_bounds__(RF_NT) void mppi_rollout_kernel(LaunchArgs<EXT, BATCH> a) {
  extern __shared__ double smem[];
  PlanProb pb;
  if constexpr (BATCH) pb = rollout_problem<EXT>(a, blockIdx.y);
  const mcp_model& md = a.model;
  const int S = md.S, U = md.U, G = md.G, D = md.D, M = a.M, T = a.T, P = a.mp.P;
  const int nna = md.n_not_angle, na = md.n_angle;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const OpenLayout L = open_layout(PT, NEEDVAR, S, D, G, a.NpadMax, false, 0, false, mppi_extra(PT, T, U, EXT));
  double* xs = smem + L.xs;
  double* z = smem + L.z;
  double* red = smem + L.red;  // [2][G][RF_NW][PT]
  GpL* gpl = reinterpret_cast<GpL*>(smem + L.gpl);
  double* kpar = smem + L.kpar;
  double* panel = smem + L.panel;
  double* nom = smem + L.ext;   // [T][U]
  double* ub = nom + T * U;     // [2][PT][U]
  double* srow = ub + 2 * PT * U;  // [T][U], the extended form only
  const mcp_noise nzl = noise_of_launch(BATCH ? pb.nz : a.nz);
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
  for (int it = tid; it < T * U; it += RF_NT) nom[it] = (BATCH ? pb.a : a.mp.a)[it];
  if constexpr (EXT && BATCH) {  // (two loops: one load per loop, so that no pointer into the arguments meets a device pointer in a phi --
                                 // the compiler then keeps a private copy of the whole argument block)
    if (pb.sigma_rows) {
      for (int it = tid; it < T * U; it += RF_NT) srow[it] = pb.sigma_rows[it];
    } else {
      for (int it = tid; it < T * U; it += RF_NT) srow[it] = a.mp.sigma[it % U];
    }
  } else if constexpr (EXT) {
    for (int it = tid; it < T * U; it += RF_NT) srow[it] = a.sigma_rows ? a.sigma_rows[it] : a.mp.sigma[it % U];
  }
  __syncthreads();
  // thread (p, s) owns state component s of trajectory p of the tile; the LAST PT * U threads form the inputs, the PT in front of them
  // each own a trajectory's cost (PT (S + U + 1) <= 400 of the 512 threads at every compiled limit: the three sets are disjoint)
  const bool own = tid < PT * S;
  const int op = own ? tid / S : 0, os = own ? tid - op * S : 0;
  const int ut = RF_NT - 1 - tid;
  const bool isu = ut < PT * U;
  const int up = isu ? ut / U : 0, uk = isu ? ut - up * U : 0;
  const int ct = ut - PT * U;
  const bool isc = ct >= 0 && ct < PT;
  const int tp = own ? op : (isu ? up : (isc ? ct : 0));
  const int om = imin(m0 + tp, M - 1);
  const bool ovalid = m0 + tp < M;
  const int kc = om / P;       // the candidate
  const int pp = om - kc * P;  // the model particle: the id the GP increments are drawn with
  double xn = own ? (BATCH ? pb.x0 : a.x0)[os] : 0.0;
  if constexpr (BATCH)
    if (own && pb.x0_per_particle) xn = pb.x0[pp * S + os];  // a start state per model particle
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
  // the input of row 0 (and, in the loop, of row t + 1 a step ahead): the law of the closed-loop kernels' squashing
  double sig = 0.0, umax = 1.0, ucur = 0.0;
  double xic = 0.0;  // (the extended form) the coloured perturbation of the row in ucur, carried across the rows
  bool has_up = false;
  if (isu) {
    umax = a.mp.u_max[uk];
    if constexpr (EXT) {
      xic = BATCH ? plan_xi(a.mp, pb.xi, nzl, kc, 0, uk) : mppi_xi(a.mp, nzl, kc, 0, uk);  // xi_0 = n_0
      sig = srow[uk];
      const double* u_prev = BATCH ? pb.u_prev : a.u_prev;
      if (u_prev) ub[(PT + up) * U + uk] = u_prev[uk];  // row -1 has the slot of the odd rows: rewritten by row 1, two barriers on
    } else {
      sig = a.mp.sigma[uk];
      xic = BATCH ? plan_xi(a.mp, pb.xi, nzl, kc, 0, uk) : mppi_xi(a.mp, nzl, kc, 0, uk);
    }
    const double av = nom[uk] + sig * xic;
    ucur = a.mp.squash ? umax * fast_tanh(av / umax) : av;
  }
  if constexpr (EXT) has_up = (BATCH ? pb.u_prev : a.u_prev) != nullptr;
  double jsum = 0.0;  // the trajectory's running cost
  lds_barrier();

  for (int t = 0; t < T; ++t) {
    const bool more = t + 1 < T;
    // ---- phase S: publish x_t, u_t and the GP features -------------------------------------------------------------------
    if (own) {
      xs[cur * PT * S + op * S + os] = xn;
      if (ovalid) {
        double* states = BATCH ? pb.states : a.states;
        if (states) states[((size_t)t * M + m0 + op) * S + os] = xn;
        if (is_bad(xn)) bad |= MCP_STATUS_NAN;
      }
      if (more) {
        double* zp = z + op * D;
        if (zi_plain >= 0) zp[zi_plain] = xn;
        if (zi_ang >= 0) {
          double sn, cs;
          mppi_sincos(xn, &sn, &cs);
          zp[nna + zi_ang] = sn;
          zp[nna + na + zi_ang] = cs;
        }
      }
    }
    if (isu) {
      ub[((t & 1) * PT + up) * U + uk] = ucur;
      if (more) z[up * D + nna + 2 * na + uk] = ucur;
      if (ovalid) {
        double* inputs = BATCH ? pb.inputs : a.inputs;
        if (inputs) inputs[((size_t)t * M + m0 + up) * U + uk] = ucur;
        if (is_bad(ucur)) bad |= MCP_STATUS_NAN;
      }
    }
    lds_barrier();
    // ---- the row's cost, in the thread that owns the trajectory (rows t and t - 1 of ub; the next write of either slot is two barriers away) ----
    if (isc) {
      const double* xr = xs + cur * PT * S + ct * S;
      const double* ur = ub + ((t & 1) * PT + ct) * U;
      const double* upr = (t > 0 || (EXT && has_up)) ? ub + (((t + 1) & 1) * PT + ct) * U : nullptr;
      const double c = a.has_cin ? cost_u_point(a.cost, a.cin, xr, ur, upr, a.mp.t0 + t) : cost_point(a.cost, xr, a.mp.t0 + t, nullptr);
      jsum += a.mp.w ? a.mp.w[t] * c : c;
    }
    if (!more) break;  // (uniform)
    if (isu) {         // u_{t+1}, a row ahead
      double av;
      if constexpr (EXT) {
        xic = fma(a.beta, xic, a.cnew * (BATCH ? plan_xi(a.mp, pb.xi, nzl, kc, t + 1, uk) : mppi_xi(a.mp, nzl, kc, t + 1, uk)));
        av = nom[(t + 1) * U + uk] + srow[(t + 1) * U + uk] * xic;
      } else {
        av = nom[(t + 1) * U + uk] + sig * (BATCH ? plan_xi(a.mp, pb.xi, nzl, kc, t + 1, uk) : mppi_xi(a.mp, nzl, kc, t + 1, uk));
      }
      ucur = a.mp.squash ? umax * fast_tanh(av / umax) : av;
    }
    // ---- phases K (and V) per GP ---------------------------------------------------------------------------------------
    for (int g = 0; g < G; ++g) {
      const GpL gp = gpl[g];
      const double* Xt = L.xl ? smem + L.xt + g * D * a.NpadMax : gp.Xt;
      const double* al = L.xl ? smem + L.al + g * a.NpadMax : gp.alpha;
      open_phase_k<PT, MAXDEG, NEEDVAR>(gp, kpar + g * KP_STRIDE(D), D, z, panel, red + g * RF_NW * PT, tid, wv, lane, Xt, al,
                                        L.xl ? a.NpadMax : gp.Npad);
      if (NEEDVAR) {
        lds_barrier();
        const int Npad = __builtin_amdgcn_readfirstlane(gp.Npad);
        double q = 0.0;
        for (int I0 = 32 * wv; I0 < Npad; I0 += 32 * RF_NW) q += open_v_block<PT, false>(gp.Kinv, Npad, I0, panel, nullptr, lane);
        q = fold_kk(q);
        if (lane < PT) red[(G + g) * RF_NW * PT + wv * PT + lane] = q;
        lds_barrier();  // the panel is rewritten by the next GP
      }
    }
    if (!NEEDVAR) lds_barrier();
    // ---- phase F: moments, sample, integrate   v' = v + delta ;  q' = q + Ts v + Ts/2 delta   (rollout_open.hip's statements) ----
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
            const double e = nzl.eps ? nzl.eps[((size_t)t * P + pp) * G + og] : philox_normal(nzl, pp, t, og);
            dv = fma(sqrt(var), e, mu);
          }
        }
        if (og == g_vel && ovalid) {  // every GP has exactly one velocity component: its thread reports
          if (a.sample && var <= 0.0) bad |= MCP_STATUS_NONPOS_VAR;  // (finite and not positive: a NaN variance is MCP_STATUS_NAN)
          if (is_bad(mu) || is_bad(var)) bad |= MCP_STATUS_NAN;
        }
        nx = og == g_pos ? xc[os] + Ts * xc[vel_of_pos] + 0.5 * Ts * dv : xc[os] + dv;
      }
      xn = nx;
    }
    if (NEEDVAR && MAXDEG >= 1) lds_barrier();  // k(z, z) above reads z, which the next step's phase S rewrites
    cur ^= 1;
  }
  if (isc && ovalid) {
    (BATCH ? pb.traj_cost : a.traj_cost)[m0 + ct] = jsum;
    if (is_bad(jsum)) bad |= MCP_STATUS_NAN;
  }
  if (bad) atomicOr(BATCH ? pb.status : a.status, bad);
}

// ---- the update ---------------------------------------------------------------------------------------------------------------------------
#define MU_NT 256

// the sum of the workgroup's MU_NT values in a fixed order (i with i + 128, 64, ... 1), in every thread; `red`: MU_NT doubles of LDS
__device__ __forceinline__ double mppi_block_sum(double v, double* red, int tid) {
  __syncthreads();  // (the buffer's previous readers)
  red[tid] = v;
  __syncthreads();
  for (int s = MU_NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// Every update kernel is a body over ONE problem's operands and two thin kernels: the single-problem one hands it its arguments, the batched one
// (grid y, or x where the single-problem kernel is one workgroup: the problem b) its arguments moved to problem b's slices.
__device__ __forceinline__ void mppi_weights_body(const mcp_mppi& mp, const double* __restrict__ traj_cost, double* __restrict__ cand_cost,
                                                  double* __restrict__ weights, double* __restrict__ stats, uint32_t* __restrict__ status) {
  __shared__ double red[MU_NT];
  __shared__ double mins[MU_NT];
  __shared__ int mink[MU_NT];
  const int tid = threadIdx.x, K = mp.K, P = mp.P;
  // S_k, and this thread's minimum over the finite ones (ascending k: the lowest k among equals)
  double smin = 0.0;
  int kmin = -1;
  bool nonfinite = false;
  for (int k = tid; k < K; k += MU_NT) {
    const double* J = traj_cost + (size_t)k * P;
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += J[p];
    double Sk = s / (double)P;
    if (mp.kappa != 0.0) {
      double q = 0.0;
      for (int p = 0; p < P; ++p) {
        const double d = J[p] - Sk;
        q = fma(d, d, q);
      }
      Sk += mp.kappa * sqrt(q / (double)(P - 1));
    }
    cand_cost[k] = Sk;
    if (is_bad(Sk)) {
      nonfinite = true;
    } else if (kmin < 0 || Sk < smin) {
      smin = Sk;
      kmin = k;
    }
  }
  mins[tid] = smin;
  mink[tid] = kmin;
  __syncthreads();
  for (int s = MU_NT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const int ko = mink[tid + s];
      const double so = mins[tid + s];
      const int km = mink[tid];
      if (ko >= 0 && (km < 0 || so < mins[tid] || (so == mins[tid] && ko < km))) {
        mins[tid] = so;
        mink[tid] = ko;
      }
    }
    __syncthreads();
  }
  smin = mins[0];
  kmin = mink[0];
  if (nonfinite) atomicOr(status, MCP_STATUS_NAN);
  if (kmin < 0) {  // no finite candidate: the mean kernel then leaves a_new = a
    for (int k = tid; k < K; k += MU_NT) weights[k] = 0.0;
    if (tid == 0) {
      const double nanv = __longlong_as_double(0x7ff8000000000000ll);
      stats[0] = nanv, stats[1] = -1.0, stats[2] = 0.0, stats[3] = nanv;
    }
    return;
  }
  double es = 0.0;
  for (int k = tid; k < K; k += MU_NT) {
    const double Sk = cand_cost[k];
    const double e = is_bad(Sk) ? 0.0 : exp(-(Sk - smin) / mp.lambda);
    weights[k] = e;  // (this thread's own entries: read back below by the same thread)
    es += e;
  }
  const double esum = mppi_block_sum(es, red, tid);
  double w2 = 0.0, ws = 0.0;
  for (int k = tid; k < K; k += MU_NT) {
    const double w = weights[k] / esum;
    weights[k] = w;
    w2 = fma(w, w, w2);
    if (w != 0.0) ws = fma(w, cand_cost[k], ws);
  }
  w2 = mppi_block_sum(w2, red, tid);
  ws = mppi_block_sum(ws, red, tid);
  if (tid == 0) stats[0] = smin, stats[1] = (double)kmin, stats[2] = 1.0 / w2, stats[3] = ws;
}
__global__ __launch_bounds__(MU_NT) void mppi_weights_kernel(mcp_mppi mp, const double* __restrict__ traj_cost, double* __restrict__ cand_cost,
                                                             double* __restrict__ weights, double* __restrict__ stats,
                                                             uint32_t* __restrict__ status) {
  mppi_weights_body(mp, traj_cost, cand_cost, weights, stats, status);
}
__global__ __launch_bounds__(MU_NT) void mppi_weights_batch_kernel(mcp_mppi mp, const double* __restrict__ traj_cost, double* __restrict__ cand_cost,
                                                                   double* __restrict__ weights, double* __restrict__ stats,
                                                                   uint32_t* __restrict__ status) {
  const size_t b = blockIdx.x;
  mppi_weights_body(mp, traj_cost + b * (size_t)mp.K * mp.P, cand_cost + b * mp.K, weights + b * mp.K, stats + 4 * b, status + b);
}

// the nominal and the xi buffer of problem b of a batched update (what its bodies read of a PlanProb)
__device__ __forceinline__ PlanProb update_problem(const mcp_mppi& mp, const mcp_plan_batch& bt, size_t b) {
  PlanProb pb;
  pb.a = mp.a + b * (size_t)mp.H * mp.U;
  pb.xi = mp.xi ? mp.xi + b * (size_t)bt.xi_stride : nullptr;
  return pb;
}

// one workgroup per row t: a_new[t][u] = a[t][u] + sigma[u] sum_{k >= 1, w_k != 0} w_k xi(k, t, u); RAW (mcp_mppi_update_ext): the weighted
// sum N_t[u] of the WHITE normals alone is left in a_new[t][u] for mppi_filter_kernel
template <bool RAW, bool BATCH>
__device__ __forceinline__ void mppi_mean_body(const mcp_mppi& mp, const mcp_noise& nz, const PlanProb& pb, const double* __restrict__ weights,
                                               double* __restrict__ a_new) {
  __shared__ double red[MU_NT];
  const int tid = threadIdx.x, t = blockIdx.x, K = mp.K, U = mp.U;
  const mcp_noise nzl = noise_of_launch(nz);
  for (int u = 0; u < U; ++u) {
    double acc = 0.0;
    for (int k = tid; k < K; k += MU_NT) {
      const double w = weights[k];
      if (k >= 1 && w != 0.0) acc = fma(w, BATCH ? plan_xi(mp, pb.xi, nzl, k, t, u) : mppi_xi(mp, nzl, k, t, u), acc);
    }
    acc = mppi_block_sum(acc, red, tid);
    if (tid == 0) a_new[(size_t)t * U + u] = RAW ? acc : (BATCH ? pb.a : mp.a)[(size_t)t * U + u] + mp.sigma[u] * acc;
  }
}
template <bool RAW>
__global__ __launch_bounds__(MU_NT) void mppi_mean_kernel(mcp_mppi mp, mcp_noise nz, const double* __restrict__ weights, double* __restrict__ a_new) {
  mppi_mean_body<RAW, false>(mp, nz, PlanProb{}, weights, a_new);
}
template <bool RAW>
__global__ __launch_bounds__(MU_NT) void mppi_mean_batch_kernel(mcp_mppi mp, mcp_noise nz, mcp_plan_batch bt, const double* __restrict__ weights,
                                                                double* __restrict__ a_new) {
  const size_t b = blockIdx.y;
  mppi_mean_body<RAW, true>(mp, noise_of_problem(nz, bt, b), update_problem(mp, bt, b), weights + b * mp.K, a_new + b * (size_t)mp.H * mp.U);
}

// The perturbation sum is linear in the white normals, so the AR(1) filter runs over the H U weighted sums instead of over every candidate:
// thread u walks the rows, X_0 = N_0, X_t = fma(beta, X_{t-1}, cnew N_t), a_new[t][u] = a[t][u] + s(t, u) X_t (in place of N_t).
template <bool BATCH>
__device__ __forceinline__ void mppi_filter_body(const mcp_mppi& mp, const double* anom, const double* __restrict__ sigma_rows, double beta, double cnew,
                                                 double* __restrict__ a_new) {
  const int u = threadIdx.x, U = mp.U;
  if (u >= U) return;
  double x = 0.0;
  for (int t = 0; t < mp.H; ++t) {
    const size_t i = (size_t)t * U + u;
    const double n = a_new[i];
    x = t == 0 ? n : fma(beta, x, cnew * n);
    a_new[i] = (BATCH ? anom : mp.a)[i] + (sigma_rows ? sigma_rows[i] : mp.sigma[u]) * x;
  }
}
__global__ __launch_bounds__(MCP_MAX_INPUT) void mppi_filter_kernel(mcp_mppi mp, const double* __restrict__ sigma_rows, double beta, double cnew,
                                                                    double* __restrict__ a_new) {
  mppi_filter_body<false>(mp, nullptr, sigma_rows, beta, cnew, a_new);
}
__global__ __launch_bounds__(MCP_MAX_INPUT) void mppi_filter_batch_kernel(mcp_mppi mp, const double* __restrict__ sigma_rows, double beta, double cnew,
                                                                          double* __restrict__ a_new) {
  const size_t o = (size_t)blockIdx.x * mp.H * mp.U;
  mppi_filter_body<true>(mp, mp.a + o, sigma_rows ? sigma_rows + o : nullptr, beta, cnew, a_new + o);
}

// ---- the CEM update: mcp_cem_update ---------------------------------------------------------------------------------------------------------
//   cem_select_kernel   one workgroup: S_k as mppi_weights_kernel forms it; E' = min(n_elite, #finite); a radix select (ten passes of eight
//                       bits, most significant first) on the 80-bit composite (order-preserving key of S_k, k) finds its E'-th smallest
//                       value -- the composite is unique, so exactly E' candidates lie at or below it --; they are gathered in LDS in any
//                       order and sorted there (bitonic, 1024 slots): unique keys make the result independent of the gathering order.
//                       Integer LDS atomics count; no floating-point result goes through an atomic.
//   cem_fit_kernel      one workgroup per input u: thread i owns the ranks i, i + 256, ... (at most CEM_SLOTS) and carries their AR(1)
//                       chains in registers across the rows; per row the mean, then -- the values still in registers -- the squared
//                       deviations from it: no [H][E][U] scratch.
#define CEM_SLOTS (MCP_CEM_MAX_ELITE / MU_NT)

// the order of the finite doubles as unsigned integers (-0.0 counts as 0.0: equal costs tie, and ties go to the lower k)
__device__ __forceinline__ unsigned long long cem_key(double s) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(s == 0.0 ? 0.0 : s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// digit p (0 .. 9, most significant first) of the composite (key, k), k < 65536
__device__ __forceinline__ int cem_digit(unsigned long long key, int k, int p) { return p < 8 ? (int)((key >> (56 - 8 * p)) & 255u) : ((k >> (8 * (9 - p))) & 255); }
// whether the digits above p equal the threshold's
__device__ __forceinline__ bool cem_match(unsigned long long key, int k, unsigned long long tkey, int tk, int p) {
  if (p == 0) return true;
  if (p < 8) return (key >> (64 - 8 * p)) == (tkey >> (64 - 8 * p));
  return key == tkey && (p == 8 || (k >> 8) == (tk >> 8));
}

__device__ __forceinline__ void cem_select_body(const mcp_mppi& mp, int n_elite, const double* __restrict__ traj_cost, double* __restrict__ cand_cost,
                                                int32_t* __restrict__ elite, double* __restrict__ stats, uint32_t* __restrict__ status) {
  __shared__ double red[MU_NT];
  __shared__ unsigned long long skey[MCP_CEM_MAX_ELITE];
  __shared__ int sk[MCP_CEM_MAX_ELITE];
  __shared__ int hist[MU_NT], scan[MU_NT];
  __shared__ int nfin, sel, need, nsurv;
  const int tid = threadIdx.x, K = mp.K, P = mp.P;
  if (tid == 0) nfin = 0, nsurv = 0;
  __syncthreads();
  int fin = 0;
  bool nonfinite = false;
  for (int k = tid; k < K; k += MU_NT) {  // (mppi_weights_kernel's statements)
    const double* J = traj_cost + (size_t)k * P;
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += J[p];
    double Sk = s / (double)P;
    if (mp.kappa != 0.0) {
      double q = 0.0;
      for (int p = 0; p < P; ++p) {
        const double d = J[p] - Sk;
        q = fma(d, d, q);
      }
      Sk += mp.kappa * sqrt(q / (double)(P - 1));
    }
    cand_cost[k] = Sk;  // (read back below by this thread alone)
    if (is_bad(Sk))
      nonfinite = true;
    else
      ++fin;
  }
  if (fin) atomicAdd(&nfin, fin);
  if (nonfinite) atomicOr(status, MCP_STATUS_NAN);
  __syncthreads();
  const int E = imin(n_elite, nfin);
  for (int r = E + tid; r < n_elite; r += MU_NT) elite[r] = -1;
  if (E == 0) {  // (uniform) no finite candidate: cem_fit_kernel then leaves a_new = a, sigma_new = s
    if (tid == 0) {
      const double nanv = __longlong_as_double(0x7ff8000000000000ll);
      stats[0] = nanv, stats[1] = -1.0, stats[2] = 0.0, stats[3] = nanv;
    }
    return;
  }
  // the E-th smallest composite, digit by digit
  unsigned long long tkey = 0;
  int tk = 0;
  if (tid == 0) need = E;
  for (int p = 0; p < 10; ++p) {
    hist[tid] = 0;
    __syncthreads();
    for (int k = tid; k < K; k += MU_NT) {
      const double Sk = cand_cost[k];
      if (is_bad(Sk)) continue;
      const unsigned long long key = cem_key(Sk);
      if (cem_match(key, k, tkey, tk, p)) atomicAdd(&hist[cem_digit(key, k, p)], 1);
    }
    __syncthreads();
    scan[tid] = hist[tid];
    __syncthreads();
    for (int off = 1; off < MU_NT; off <<= 1) {  // inclusive prefix counts over the 256 digits
      const int v = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int want = need;
    __syncthreads();
    if (scan[tid] - hist[tid] < want && want <= scan[tid]) {  // exactly one digit
      sel = tid;
      need = want - (scan[tid] - hist[tid]);
    }
    __syncthreads();
    if (p < 8)
      tkey |= (unsigned long long)sel << (56 - 8 * p);
    else
      tk |= sel << (8 * (9 - p));
  }
  // gather the E candidates at or below it, then sort them by (key, k)
  for (int r = tid; r < MCP_CEM_MAX_ELITE; r += MU_NT) skey[r] = ~0ull, sk[r] = 0x7fffffff;
  __syncthreads();
  for (int k = tid; k < K; k += MU_NT) {
    const double Sk = cand_cost[k];
    if (is_bad(Sk)) continue;
    const unsigned long long key = cem_key(Sk);
    if (key < tkey || (key == tkey && k <= tk)) {
      const int slot = atomicAdd(&nsurv, 1);
      if (slot < MCP_CEM_MAX_ELITE) skey[slot] = key, sk[slot] = k;  // (exactly E <= MCP_CEM_MAX_ELITE of them: the guard never bites)
    }
  }
  __syncthreads();
  int n2 = 2;  // the power of two the E slots fit in (the slots behind them hold the largest composite)
  while (n2 < E) n2 <<= 1;
  for (int len = 2; len <= n2; len <<= 1)
    for (int j = len >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += MU_NT) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & len) == 0;
          const unsigned long long ki = skey[i], kl = skey[l];
          const int ci = sk[i], cl = sk[l];
          const bool gt = ki > kl || (ki == kl && ci > cl);
          if (gt == up) skey[i] = kl, skey[l] = ki, sk[i] = cl, sk[l] = ci;
        }
      }
      __syncthreads();
    }
  double cs = 0.0;
  for (int r = tid; r < E; r += MU_NT) {
    elite[r] = sk[r];
    cs += cand_cost[sk[r]];
  }
  cs = mppi_block_sum(cs, red, tid);
  if (tid == 0) stats[0] = cand_cost[sk[0]], stats[1] = (double)sk[0], stats[2] = (double)E, stats[3] = cs / (double)E;
}
__global__ __launch_bounds__(MU_NT) void cem_select_kernel(mcp_mppi mp, int n_elite, const double* __restrict__ traj_cost, double* __restrict__ cand_cost,
                                                           int32_t* __restrict__ elite, double* __restrict__ stats, uint32_t* __restrict__ status) {
  cem_select_body(mp, n_elite, traj_cost, cand_cost, elite, stats, status);
}
__global__ __launch_bounds__(MU_NT) void cem_select_batch_kernel(mcp_mppi mp, int n_elite, const double* __restrict__ traj_cost,
                                                                 double* __restrict__ cand_cost, int32_t* __restrict__ elite, double* __restrict__ stats,
                                                                 uint32_t* __restrict__ status) {
  const size_t b = blockIdx.x;
  cem_select_body(mp, n_elite, traj_cost + b * (size_t)mp.K * mp.P, cand_cost + b * mp.K, elite + b * (size_t)n_elite, stats + 4 * b, status + b);
}

template <bool BATCH>
__device__ __forceinline__ void cem_fit_body(const mcp_mppi& mp, const mcp_noise& nz, const mcp_plan_ext& ex, const PlanProb& pb, double cnew,
                                             const int32_t* __restrict__ elite, const double* __restrict__ stats, double* __restrict__ a_new,
                                             double* __restrict__ sigma_new) {
  __shared__ double red[MU_NT];
  const int tid = threadIdx.x, u = blockIdx.x, U = mp.U, H = mp.H;
  const mcp_noise nzl = noise_of_launch(nz);
  const double* sigma_rows = BATCH ? pb.sigma_rows : ex.sigma_rows;
  const double beta = ex.beta, alpha = ex.alpha, sigma_min = ex.sigma_min[u];
  const int E = imin((int)stats[2], ex.n_elite);  // (E' of cem_select_kernel, earlier on the stream)
  if (E <= 0) {
    for (int t = tid; t < H; t += MU_NT) {
      const size_t i = (size_t)t * U + u;
      a_new[i] = (BATCH ? pb.a : mp.a)[i];
      sigma_new[i] = sigma_rows ? sigma_rows[i] : mp.sigma[u];
    }
    return;
  }
  int ks[CEM_SLOTS];
  double xi[CEM_SLOTS];
#pragma unroll
  for (int j = 0; j < CEM_SLOTS; ++j) {
    const int r = tid + j * MU_NT;
    ks[j] = r < E ? elite[r] : -1;
    xi[j] = 0.0;
  }
  const double inv = (double)E;
  for (int t = 0; t < H; ++t) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < CEM_SLOTS; ++j)
      if (ks[j] >= 0) {  // ascending rank
        const double n = BATCH ? plan_xi(mp, pb.xi, nzl, ks[j], t, u) : mppi_xi(mp, nzl, ks[j], t, u);
        xi[j] = t == 0 ? n : fma(beta, xi[j], cnew * n);
        acc += xi[j];
      }
    const double mean = mppi_block_sum(acc, red, tid) / inv;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < CEM_SLOTS; ++j)
      if (ks[j] >= 0) {
        const double d = xi[j] - mean;
        q = fma(d, d, q);
      }
    const double v = mppi_block_sum(q, red, tid) / inv;
    if (tid == 0) {
      const size_t i = (size_t)t * U + u;
      const double s = sigma_rows ? sigma_rows[i] : mp.sigma[u], a = (BATCH ? pb.a : mp.a)[i];
      a_new[i] = alpha * a + (1.0 - alpha) * (a + s * mean);
      const double s2 = s * s;
      sigma_new[i] = fmax(sigma_min, sqrt(alpha * s2 + (1.0 - alpha) * s2 * v));
    }
  }
}
__global__ __launch_bounds__(MU_NT) void cem_fit_kernel(mcp_mppi mp, mcp_noise nz, mcp_plan_ext ex, double cnew, const int32_t* __restrict__ elite,
                                                        const double* __restrict__ stats, double* __restrict__ a_new, double* __restrict__ sigma_new) {
  cem_fit_body<false>(mp, nz, ex, PlanProb{}, cnew, elite, stats, a_new, sigma_new);
}
__global__ __launch_bounds__(MU_NT) void cem_fit_batch_kernel(mcp_mppi mp, mcp_noise nz, mcp_plan_ext ex, mcp_plan_batch bt, double cnew,
                                                              const int32_t* __restrict__ elite, const double* __restrict__ stats,
                                                              double* __restrict__ a_new, double* __restrict__ sigma_new) {
  const size_t b = blockIdx.y, hu = (size_t)mp.H * mp.U;
  PlanProb pb = update_problem(mp, bt, b);
  pb.sigma_rows = ex.sigma_rows ? ex.sigma_rows + b * hu : nullptr;
  cem_fit_body<true>(mp, noise_of_problem(nz, bt, b), ex, pb, cnew, elite + b * (size_t)ex.n_elite, stats + 4 * b, a_new + b * hu, sigma_new + b * hu);
}

// ---- host path: checks -> fill -> ladder (a refused call makes no HIP call) ----------------------------------------------------------------
static inline bool mppi_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// the descriptor's own refusals, behind the entry's pointers: the sizes and the compiled limits (the entries' one order: MCP_ERR_ARG for what
// is missing or not positive, then MCP_ERR_LIMIT), and -- behind the model's checks in the rollout -- the values
static int mppi_sizes(const mcp_mppi* mp) {
  if (!mp->a || mp->K < 1 || mp->P < 1 || mp->H < 2 || mp->U < 1 || mp->t0 < 0) return MCP_ERR_ARG;
  if (mp->U > MCP_MAX_INPUT || mp->K > MCP_MPPI_MAX_K || (int64_t)mp->K * mp->P > MCP_MPPI_MAX_M) return MCP_ERR_LIMIT;
  if ((int64_t)mp->H * mp->U > MCP_LDS_LIMIT / (int)sizeof(double)) return MCP_ERR_LIMIT;  // (the nominal alone would not fit: no layout is tried)
  return MCP_OK;
}
static int mppi_values(const mcp_mppi* mp) {
  if (!(mp->lambda > 0.0) || !mppi_finite(mp->lambda) || !mppi_finite(mp->kappa) || (mp->kappa != 0.0 && mp->P < 2)) return MCP_ERR_ARG;
  for (int k = 0; k < mp->U; ++k) {
    if (!(mp->sigma[k] >= 0.0) || !mppi_finite(mp->sigma[k])) return MCP_ERR_ARG;
    if (mp->squash && !(mp->u_max[k] > 0.0)) return MCP_ERR_ARG;
  }
  return MCP_OK;
}

// the descriptor of a batched call, behind mppi_sizes: its limits (MCP_ERR_LIMIT), and -- with the plan's values -- its strides (G: the
// model's GPs, for the eps buffer; < 0: an update, which reads no eps)
static int plan_batch_limits(const mcp_plan_batch* bt, const mcp_mppi* mp) {
  return (bt->B > MCP_PLAN_MAX_B || (int64_t)bt->B * mp->K * mp->P > MCP_MPPI_MAX_M) ? MCP_ERR_LIMIT : MCP_OK;
}
static int plan_batch_values(const mcp_plan_batch* bt, const mcp_mppi* mp, int G) {
  if (bt->particle_stride < 0) return MCP_ERR_ARG;
  if (bt->xi_stride != 0 && bt->xi_stride < (int64_t)mp->H * mp->K * mp->U) return MCP_ERR_ARG;
  if (G >= 0 && bt->eps_stride != 0 && bt->eps_stride < (int64_t)(mp->H - 1) * mp->P * G) return MCP_ERR_ARG;
  return MCP_OK;
}

template <int PT, int MAXDEG, bool NEEDVAR, bool EXT, bool BATCH = false>
static int launch_mppi(const LaunchArgs<EXT, BATCH>& a, hipStream_t st) {
  const OpenLayout L = open_layout(PT, NEEDVAR, a.model.S, a.model.D, a.model.G, a.NpadMax, false, 0, false, mppi_extra(PT, a.T, a.model.U, EXT));
  const size_t lds = (size_t)L.total * sizeof(double);
  if (lds > MCP_LDS_LIMIT) return MCP_ERR_LIMIT;
  dim3 grid((a.M + PT - 1) / PT);
  if constexpr (BATCH) grid.y = a.bt.B;  // (tiles of ONE problem, problems): a tile never spans two problems
  MCP_ENSURE_MAX_LDS((mppi_rollout_kernel<PT, MAXDEG, NEEDVAR, EXT, BATCH>));
  hipLaunchKernelGGL((mppi_rollout_kernel<PT, MAXDEG, NEEDVAR, EXT, BATCH>), grid, dim3(RF_NT), lds, st, a);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}
template <int PT, bool NEEDVAR, bool EXT, bool BATCH = false>
static int launch_mppi_deg(const LaunchArgs<EXT, BATCH>& a, int maxdeg, hipStream_t st) {
  return maxdeg == 0 ? launch_mppi<PT, 0, NEEDVAR, EXT, BATCH>(a, st) : launch_mppi<PT, 2, NEEDVAR, EXT, BATCH>(a, st);
}

// the nominal's rows (the extended form: and the std's) beside the largest layout of a rung must fit the LDS: looked at BEFORE the first
// launch attempt's HIP calls
static bool mppi_fits(const MppiArgs& a, int PT, bool needvar, bool ext = false) {
  const OpenLayout L = open_layout(PT, needvar, a.model.S, a.model.D, a.model.G, a.NpadMax, false, 0, false, mppi_extra(PT, a.T, a.model.U, ext));
  return (size_t)L.total * sizeof(double) <= MCP_LDS_LIMIT;
}

// the ladder of rollout_open.hip's forward form without a record: the mean chain one trajectory per workgroup, with variances 16, then 4
template <bool EXT, bool BATCH = false>
static int mppi_ladder(const LaunchArgs<EXT, BATCH>& a, int maxdeg, hipStream_t st) {
  if (!a.sample) return mppi_fits(a, 1, false, EXT) ? launch_mppi_deg<1, false, EXT, BATCH>(a, maxdeg, st) : MCP_ERR_LIMIT;
  if (mppi_fits(a, 16, true, EXT)) return launch_mppi_deg<16, true, EXT, BATCH>(a, maxdeg, st);
  return mppi_fits(a, 4, true, EXT) ? launch_mppi_deg<4, true, EXT, BATCH>(a, maxdeg, st) : MCP_ERR_LIMIT;
}

// the extension's own refusals (MCP_ERR_ARG; the device rows of sigma_rows are the caller's to check): what the rollout and the MPPI update
// read of it, and what the CEM update alone reads
static bool plan_ext_default(const mcp_plan_ext* e) { return !e || (!e->sigma_rows && !e->u_prev && e->beta == 0.0); }
static int plan_ext_values(const mcp_plan_ext* e) { return (e && !(e->beta >= 0.0 && e->beta < 1.0)) ? MCP_ERR_ARG : MCP_OK; }

// the checks of the rollout entries in their one order, then the fill (batch: the batched entry's descriptor, checked with the plan's sizes,
// limits and values; NULL: a single-problem entry)
static int mppi_rollout_fill(MppiArgs& a, int* maxdeg, const mcp_model* model, const mcp_mppi* mppi, const mcp_plan_ext* ext, const mcp_cost* cost,
                             const mcp_cost_inputs* cin, const mcp_noise* noise, int particle_pred, const double* x0, double* traj_cost,
                             double* states, double* inputs, uint32_t* status, const mcp_plan_batch* batch = nullptr) {
  if (!model || !mppi || !cost || !noise || !x0 || !traj_cost || !status) return MCP_ERR_ARG;
  if (batch && batch->B < 1) return MCP_ERR_ARG;
  const int src = mppi_sizes(mppi);
  if (src != MCP_OK) return src;
  if (batch && plan_batch_limits(batch, mppi) != MCP_OK) return MCP_ERR_LIMIT;
  if (!model_within_limits(model)) return MCP_ERR_LIMIT;
  if (!model_ok(model) || mppi->U != model->U || mppi_values(mppi) != MCP_OK || plan_ext_values(ext) != MCP_OK) return MCP_ERR_ARG;
  if (batch && plan_batch_values(batch, mppi, model->G) != MCP_OK) return MCP_ERR_ARG;
  if (!cost_ok(cost) || cost->S != model->S || !cost_inputs_ok(cin) || (cin && cin->U != model->U)) return MCP_ERR_ARG;
  *maxdeg = open_fill(a, model, noise, mppi->K * mppi->P, mppi->H, particle_pred, x0, nullptr, 0, nullptr, states, nullptr, nullptr, nullptr, status);
  a.mp = *mppi;
  a.cost = *cost;
  a.has_cin = cost_inputs_none(cin) ? 0 : 1;
  if (a.has_cin)
    a.cin = *cin;
  else
    memset(&a.cin, 0, sizeof(a.cin));
  a.traj_cost = traj_cost;
  a.inputs = inputs;
  return MCP_OK;
}

extern "C" int mcp_mppi_rollout(const mcp_model* model, const mcp_mppi* mppi, const mcp_cost* cost, const mcp_cost_inputs* cin, const mcp_noise* noise,
                                int particle_pred, const double* x0, double* traj_cost, double* states, double* inputs, uint32_t* status,
                                void* stream) {
  MppiArgs a;
  int maxdeg = 0;
  const int rc = mppi_rollout_fill(a, &maxdeg, model, mppi, nullptr, cost, cin, noise, particle_pred, x0, traj_cost, states, inputs, status);
  return rc != MCP_OK ? rc : mppi_ladder<false>(a, maxdeg, (hipStream_t)stream);
}

extern "C" int mcp_plan_rollout(const mcp_model* model, const mcp_mppi* mppi, const mcp_plan_ext* ext, const mcp_cost* cost,
                                const mcp_cost_inputs* cin, const mcp_noise* noise, int particle_pred, const double* x0, double* traj_cost,
                                double* states, double* inputs, uint32_t* status, void* stream) {
  PlanArgs a;
  int maxdeg = 0;
  const int rc = mppi_rollout_fill(a, &maxdeg, model, mppi, ext, cost, cin, noise, particle_pred, x0, traj_cost, states, inputs, status);
  if (rc != MCP_OK) return rc;
  if (plan_ext_default(ext)) return mppi_ladder<false>(a, maxdeg, (hipStream_t)stream);  // mcp_mppi_rollout's own launch
  a.sigma_rows = ext->sigma_rows;
  a.u_prev = ext->u_prev;
  a.beta = ext->beta;
  a.cnew = sqrt(1.0 - ext->beta * ext->beta);  // (beta == 0: exactly 1)
  return mppi_ladder<true>(a, maxdeg, (hipStream_t)stream);
}

extern "C" int mcp_mppi_update(const mcp_mppi* mppi, const mcp_noise* noise, const double* traj_cost, double* a_new, double* cand_cost,
                               double* weights, double* stats, uint32_t* status, void* stream) {
  if (!mppi || !noise || !traj_cost || !a_new || !cand_cost || !weights || !stats || !status) return MCP_ERR_ARG;
  const int rc = mppi_sizes(mppi);
  if (rc != MCP_OK) return rc;
  if (mppi_values(mppi) != MCP_OK || a_new == mppi->a) return MCP_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mppi_weights_kernel, dim3(1), dim3(MU_NT), 0, st, *mppi, traj_cost, cand_cost, weights, stats, status);
  MCP_LAUNCH_CHECK();
  hipLaunchKernelGGL(mppi_mean_kernel<false>, dim3(mppi->H), dim3(MU_NT), 0, st, *mppi, *noise, weights, a_new);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_mppi_update_ext(const mcp_mppi* mppi, const mcp_plan_ext* ext, const mcp_noise* noise, const double* traj_cost, double* a_new,
                                   double* cand_cost, double* weights, double* stats, uint32_t* status, void* stream) {
  if (plan_ext_default(ext) && plan_ext_values(ext) == MCP_OK)
    return mcp_mppi_update(mppi, noise, traj_cost, a_new, cand_cost, weights, stats, status, stream);  // (u_prev is the rollout's alone)
  if (!mppi || !noise || !traj_cost || !a_new || !cand_cost || !weights || !stats || !status) return MCP_ERR_ARG;
  const int rc = mppi_sizes(mppi);
  if (rc != MCP_OK) return rc;
  if (mppi_values(mppi) != MCP_OK || plan_ext_values(ext) != MCP_OK || a_new == mppi->a || a_new == ext->sigma_rows) return MCP_ERR_ARG;
  if (!ext->sigma_rows && ext->beta == 0.0) return mcp_mppi_update(mppi, noise, traj_cost, a_new, cand_cost, weights, stats, status, stream);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mppi_weights_kernel, dim3(1), dim3(MU_NT), 0, st, *mppi, traj_cost, cand_cost, weights, stats, status);
  MCP_LAUNCH_CHECK();
  hipLaunchKernelGGL(mppi_mean_kernel<true>, dim3(mppi->H), dim3(MU_NT), 0, st, *mppi, *noise, weights, a_new);
  MCP_LAUNCH_CHECK();
  hipLaunchKernelGGL(mppi_filter_kernel, dim3(1), dim3(MCP_MAX_INPUT), 0, st, *mppi, ext->sigma_rows, ext->beta, sqrt(1.0 - ext->beta * ext->beta), a_new);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cem_update(const mcp_mppi* mppi, const mcp_plan_ext* ext, const mcp_noise* noise, const double* traj_cost, double* a_new,
                              double* sigma_new, double* cand_cost, int32_t* elite, double* stats, uint32_t* status, void* stream) {
  if (!mppi || !ext || !noise || !traj_cost || !a_new || !sigma_new || !cand_cost || !elite || !stats || !status) return MCP_ERR_ARG;
  if (ext->n_elite < 1) return MCP_ERR_ARG;  // (a size: with the plan's, ahead of every limit)
  const int rc = mppi_sizes(mppi);
  if (rc != MCP_OK) return rc;
  if (ext->n_elite > MCP_CEM_MAX_ELITE || ext->n_elite > mppi->K) return MCP_ERR_LIMIT;
  if (mppi_values(mppi) != MCP_OK || plan_ext_values(ext) != MCP_OK || !(ext->alpha >= 0.0 && ext->alpha < 1.0)) return MCP_ERR_ARG;
  for (int k = 0; k < mppi->U; ++k)
    if (!(ext->sigma_min[k] >= 0.0) || !mppi_finite(ext->sigma_min[k])) return MCP_ERR_ARG;
  if (a_new == mppi->a || a_new == ext->sigma_rows || sigma_new == mppi->a || sigma_new == ext->sigma_rows || a_new == sigma_new) return MCP_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cem_select_kernel, dim3(1), dim3(MU_NT), 0, st, *mppi, ext->n_elite, traj_cost, cand_cost, elite, stats, status);
  MCP_LAUNCH_CHECK();
  hipLaunchKernelGGL(cem_fit_kernel, dim3(mppi->U), dim3(MU_NT), 0, st, *mppi, *noise, *ext, sqrt(1.0 - ext->beta * ext->beta), elite, stats, a_new,
                     sigma_new);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

// ---- the batched entries: the single-problem entries' checks with the batch descriptor's among them, the same decisions, the batched kernels ----
extern "C" int mcp_plan_batch_rollout(const mcp_model* model, const mcp_mppi* mppi, const mcp_plan_ext* ext, const mcp_plan_batch* batch,
                                      const mcp_cost* cost, const mcp_cost_inputs* cin, const mcp_noise* noise, int particle_pred, const double* x0,
                                      double* traj_cost, double* states, double* inputs, uint32_t* status, void* stream) {
  if (!batch) return MCP_ERR_ARG;
  PlanBatchArgs<true> a;
  int maxdeg = 0;
  const int rc = mppi_rollout_fill(a, &maxdeg, model, mppi, ext, cost, cin, noise, particle_pred, x0, traj_cost, states, inputs, status, batch);
  if (rc != MCP_OK) return rc;
  a.bt = *batch;
  if (plan_ext_default(ext)) {  // the plain kernel's batched form, as mcp_plan_rollout takes the plain kernel
    PlanBatchArgs<false> p;
    static_cast<MppiArgs&>(p) = a;
    p.bt = *batch;
    return mppi_ladder<false, true>(p, maxdeg, (hipStream_t)stream);
  }
  a.sigma_rows = ext->sigma_rows;
  a.u_prev = ext->u_prev;
  a.beta = ext->beta;
  a.cnew = sqrt(1.0 - ext->beta * ext->beta);
  return mppi_ladder<true, true>(a, maxdeg, (hipStream_t)stream);
}

extern "C" int mcp_plan_batch_update(const mcp_mppi* mppi, const mcp_plan_ext* ext, const mcp_plan_batch* batch, const mcp_noise* noise,
                                     const double* traj_cost, double* a_new, double* cand_cost, double* weights, double* stats, uint32_t* status,
                                     void* stream) {
  if (!mppi || !batch || !noise || !traj_cost || !a_new || !cand_cost || !weights || !stats || !status) return MCP_ERR_ARG;
  if (batch->B < 1) return MCP_ERR_ARG;
  const int rc = mppi_sizes(mppi);
  if (rc != MCP_OK) return rc;
  if (plan_batch_limits(batch, mppi) != MCP_OK) return MCP_ERR_LIMIT;
  if (mppi_values(mppi) != MCP_OK || plan_ext_values(ext) != MCP_OK || plan_batch_values(batch, mppi, -1) != MCP_OK) return MCP_ERR_ARG;
  if (a_new == mppi->a || (ext && a_new == ext->sigma_rows)) return MCP_ERR_ARG;
  const bool coloured = ext && (ext->sigma_rows || ext->beta != 0.0);  // (else mcp_mppi_update's two kernels, as mcp_mppi_update_ext decides)
  hipStream_t st = (hipStream_t)stream;
  const dim3 rows(mppi->H, batch->B);
  hipLaunchKernelGGL(mppi_weights_batch_kernel, dim3(batch->B), dim3(MU_NT), 0, st, *mppi, traj_cost, cand_cost, weights, stats, status);
  MCP_LAUNCH_CHECK();
  if (!coloured) {
    hipLaunchKernelGGL(mppi_mean_batch_kernel<false>, rows, dim3(MU_NT), 0, st, *mppi, *noise, *batch, weights, a_new);
    MCP_LAUNCH_CHECK();
    return MCP_OK;
  }
  hipLaunchKernelGGL(mppi_mean_batch_kernel<true>, rows, dim3(MU_NT), 0, st, *mppi, *noise, *batch, weights, a_new);
  MCP_LAUNCH_CHECK();
  hipLaunchKernelGGL(mppi_filter_batch_kernel, dim3(batch->B), dim3(MCP_MAX_INPUT), 0, st, *mppi, ext->sigma_rows, ext->beta,
                     sqrt(1.0 - ext->beta * ext->beta), a_new);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cem_batch_update(const mcp_mppi* mppi, const mcp_plan_ext* ext, const mcp_plan_batch* batch, const mcp_noise* noise,
                                    const double* traj_cost, double* a_new, double* sigma_new, double* cand_cost, int32_t* elite, double* stats,
                                    uint32_t* status, void* stream) {
  if (!mppi || !ext || !batch || !noise || !traj_cost || !a_new || !sigma_new || !cand_cost || !elite || !stats || !status) return MCP_ERR_ARG;
  if (ext->n_elite < 1 || batch->B < 1) return MCP_ERR_ARG;
  const int rc = mppi_sizes(mppi);
  if (rc != MCP_OK) return rc;
  if (ext->n_elite > MCP_CEM_MAX_ELITE || ext->n_elite > mppi->K || plan_batch_limits(batch, mppi) != MCP_OK) return MCP_ERR_LIMIT;
  if (mppi_values(mppi) != MCP_OK || plan_ext_values(ext) != MCP_OK || !(ext->alpha >= 0.0 && ext->alpha < 1.0)) return MCP_ERR_ARG;
  for (int k = 0; k < mppi->U; ++k)
    if (!(ext->sigma_min[k] >= 0.0) || !mppi_finite(ext->sigma_min[k])) return MCP_ERR_ARG;
  if (plan_batch_values(batch, mppi, -1) != MCP_OK) return MCP_ERR_ARG;
  if (a_new == mppi->a || a_new == ext->sigma_rows || sigma_new == mppi->a || sigma_new == ext->sigma_rows || a_new == sigma_new) return MCP_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cem_select_batch_kernel, dim3(batch->B), dim3(MU_NT), 0, st, *mppi, ext->n_elite, traj_cost, cand_cost, elite, stats, status);
  MCP_LAUNCH_CHECK();
  hipLaunchKernelGGL(cem_fit_batch_kernel, dim3(mppi->U, batch->B), dim3(MU_NT), 0, st, *mppi, *noise, *ext, *batch, sqrt(1.0 - ext->beta * ext->beta),
                     elite, stats, a_new, sigma_new);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}
