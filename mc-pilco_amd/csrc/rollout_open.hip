// Fused OPEN-LOOP rollout for gfx950 (MI355X): M trajectories are advanced T steps through an mcp_model, the input of step t
// is read from a buffer (the inputs recorded on the system) instead of coming out of a policy.
//
// Replaces the step loop of MC_PILCO.rollout (policy_learning/MC_PILCO.py:347-373) over Model_learning.get_next_state
// (model_learning/Model_learning.py:210-229, 685-718; GP_prior.get_estimate_from_alpha, GP_prior.py:137-155): per step G posterior
// launches plus indexing, concatenation and a Normal(...).rsample() -- here ONE launch, no workspace, no hand-off between
// workgroups.  There is no policy and no Jacobian (nothing is differentiated), so a step is three phases:
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
#include "rollout_fwd_shared.h"

using namespace mcp;

typedef double v4d __attribute__((ext_vector_type(4)));

#define RO_VU 4  // 4-row MFMA steps per register batch of phase V

struct OpenArgs {
  mcp_model model;
  mcp_noise nz;
  int M, T, sample, Mu, NpadMax;
  const double* x0;
  const double* u;
  const int32_t* lengths;
  double* states;
  double* mu;
  double* var;
  uint32_t* status;
};

struct OpenLayout {
  int xs, z, red, gpl, kpar, panel, xt, al, total;  // offsets in doubles
  int xl;                                           // X^T and alpha of every GP staged in LDS (row pitch NpadMax)
};

#define RO_KR(PT) ((PT) == 16 ? 18 : (PT))  // row pitch of the k panel (16 particles: + 2 pad, bank spread of the phase-K stores)

__host__ __device__ inline OpenLayout open_layout(int PT, bool needvar, int S, int D, int G, int NpadMax) {
  OpenLayout L;
  int o = 0;
  auto take = [&](int n) {
    int r = o;
    o += (n + 1) & ~1;
    return r;
  };
  L.xs = take(2 * PT * S);
  L.z = take(PT * D);
  L.red = take(2 * G * RF_NW * PT);  // per-wave partial sums: alpha^T k | k^T Kinv k
  L.gpl = take(G * GPL_DOUBLES);
  L.kpar = take(G * KP_STRIDE(D));
  L.panel = needvar ? take(NpadMax * RO_KR(PT)) : 0;
  const int xneed = G * (D + 1) * NpadMax + 4;
  L.xl = (!needvar && o + xneed <= MCP_LDS_LIMIT / 8) ? 1 : 0;
  L.xt = L.xl ? take(G * D * NpadMax) : 0;
  L.al = L.xl ? take(G * NpadMax) : 0;
  L.total = o;
  return L;
}

// ---------------------------------------------------------------------------------------
// phase V: this wave's share of  q[n] = sum_i k[i][n] (Kinv k)[i][n]  over one 32-row block of Kinv
//   A operand  lane (m = l&15, kk = l>>4) : Kinv[j0+kk][I0 + 2m], Kinv[j0+kk][I0 + 2m + 1]   (Kinv symmetric: row j0+kk)
//   B operand  lane (kk = l>>4, n = l&15) : k[j0+kk][n]
//   acc_e[r] / acc_o[r] : v[I0 + 2((l>>4)+4r) (+1)][n = l&15]
// Columns of the product are independent: with fewer than 16 particles the lanes of the missing columns read column 0 and their
// result is never used.  In the last block of an Npad that is not a multiple of 32 the missing row pairs read column 0 of Kinv and
// are left out of the sum.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void open_v_load(v2d (&A)[RO_VU], double (&B)[RO_VU], gptr2_t ap, size_t astep, const double* bp, int kr) {
#pragma unroll
  for (int u = 0; u < RO_VU; ++u) {
    A[u] = ap[(size_t)u * astep];
    B[u] = bp[u * 4 * kr];
  }
}
__device__ __forceinline__ void open_v_mfma(const v2d (&A)[RO_VU], const double (&B)[RO_VU], v4d& acc_e, v4d& acc_o) {
#pragma unroll
  for (int u = 0; u < RO_VU; ++u) {
    acc_e = __builtin_amdgcn_mfma_f64_16x16x4f64(A[u].x, B[u], acc_e, 0, 0, 0);
    acc_o = __builtin_amdgcn_mfma_f64_16x16x4f64(A[u].y, B[u], acc_o, 0, 0, 0);
  }
}
template <int PT>
__device__ __forceinline__ double open_v_block(const double* Kinv, int Npad, int I0, const double* panel, int lane) {
  constexpr int KR = RO_KR(PT);
  const int m = lane & 15, kk = lane >> 4;
  const int nn = m < PT ? m : 0;
  const int col = I0 + 2 * m;
  gptr2_t a0 = (gptr2_t)((gptr_t)Kinv + (size_t)kk * Npad + (col < Npad ? col : 0));
  const size_t astep = (size_t)4 * Npad / 2;  // 4 rows, in v2d units
  const size_t abatch = (size_t)RO_VU * astep;
  const int bbatch = RO_VU * 4 * KR;
  const double* b0 = panel + kk * KR + nn;
  const int nb = Npad >> 4;  // batches of 16 rows (Npad is a multiple of 16)
  v4d acc_e = (v4d){0.0, 0.0, 0.0, 0.0}, acc_o = acc_e;
  v2d A0[RO_VU], A1[RO_VU];
  double B0[RO_VU], B1[RO_VU];
  open_v_load(A0, B0, a0, astep, b0, KR);
  for (int b = 0; b + 1 < nb; b += 2) {
    open_v_load(A1, B1, a0 + (size_t)(b + 1) * abatch, astep, b0 + (b + 1) * bbatch, KR);
    open_v_mfma(A0, B0, acc_e, acc_o);
    const int b2 = imin(b + 2, nb - 1);  // past the end: reload the last batch rather than branch
    open_v_load(A0, B0, a0 + (size_t)b2 * abatch, astep, b0 + b2 * bbatch, KR);
    open_v_mfma(A1, B1, acc_e, acc_o);
  }
  if (nb & 1) open_v_mfma(A0, B0, acc_e, acc_o);
  double q = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = I0 + 2 * (kk + 4 * r);
    if (row < Npad) {  // (Npad is even: row + 1 is inside too)
      q = fma(acc_e[r], panel[row * KR + nn], q);
      q = fma(acc_o[r], panel[(row + 1) * KR + nn], q);
    }
  }
  return q;
}

// ---------------------------------------------------------------------------------------
// phase K for one GP: k(z_p, X_j) for thread j and the PT particles of the tile, PC particles at a time
// ---------------------------------------------------------------------------------------
template <int PT, int MAXDEG, bool NEEDVAR>
__device__ __forceinline__ void open_phase_k(const GpL& gp, const double* kp, int D, const double* z, double* panel, double* red_mu, int tid, int wv,
                                             int lane, const double* Xt, const double* al, int pitch) {
  constexpr int PC = PT < 4 ? PT : 4;
  constexpr int KR = RO_KR(PT);
  const int N = gp.N, Npad = gp.Npad;
  const int deg = MAXDEG == 0 ? 0 : gp.deg;
  const double lam = gp.lambda;
  const double w1D = (MAXDEG >= 1 && deg >= 1) ? kp[KP_W1(D) + D] : 0.0;
  double mtot[PT];
#pragma unroll
  for (int p = 0; p < PT; ++p) mtot[p] = 0.0;
  for (int j = tid; j < Npad; j += RF_NT) {
    const double aj = al[j];  // zero on the padding rows
    const bool live = j < N;
#pragma unroll
    for (int pc = 0; pc < PT; pc += PC) {
      double se[PC], p1[PC], pa[PC], pb[PC], szz[PC];
      double sxx = 0.0;
#pragma unroll
      for (int q = 0; q < PC; ++q) se[q] = p1[q] = pa[q] = pb[q] = szz[q] = 0.0;
      for (int d = 0; d < D; ++d) {
        const double x = Xt[(size_t)d * pitch + j];
        const double il = kp[KP_INVLS(D) + d];
        const double w1 = MAXDEG >= 1 ? kp[KP_W1(D) + d] : 0.0;
        const double wa = MAXDEG >= 2 ? kp[KP_W20(D) + d] : 0.0, wb = MAXDEG >= 2 ? kp[KP_W21(D) + d] : 0.0;
        const double tx = il * x;
        sxx = fma(tx, tx, sxx);
#pragma unroll
        for (int q = 0; q < PC; ++q) {
          const double zz = z[(pc + q) * D + d];
          const double il2z = il * il * zz;
          se[q] = fma(-2.0 * il2z, x, se[q]);
          szz[q] = fma(il2z, zz, szz[q]);
          if (MAXDEG >= 1) p1[q] = fma(w1 * zz, x, p1[q]);
          if (MAXDEG >= 2) {
            const double ab = zz * x;
            pa[q] = fma(wa, ab, pa[q]);
            pb[q] = fma(wb, ab, pb[q]);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < PC; ++q) {
        double k = lam * exp(-((szz[q] + sxx) + se[q]));
        if (MAXDEG >= 1 && deg >= 1) {
          k += p1[q] + w1D;
          if (MAXDEG >= 2 && deg >= 2) k = fma(pa[q], pb[q], k);
        }
        if (!live) k = 0.0;
        mtot[pc + q] = fma(aj, k, mtot[pc + q]);
        if (NEEDVAR) panel[j * KR + pc + q] = k;
      }
    }
  }
  wave_sum_multi<PT>(mtot);
  if (lane == 0) {
#pragma unroll
    for (int p = 0; p < PT; ++p) red_mu[wv * PT + p] = mtot[p];
  }
}

template <int PT, int MAXDEG, bool NEEDVAR>
__global__ __launch_bounds__(RF_NT) void rollout_open_kernel(OpenArgs a) {
  extern __shared__ double smem[];
  const mcp_model& md = a.model;
  const int S = md.S, U = md.U, G = md.G, D = md.D, M = a.M, T = a.T;
  const int nna = md.n_not_angle, na = md.n_angle;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const OpenLayout L = open_layout(PT, NEEDVAR, S, D, G, a.NpadMax);
  double* xs = smem + L.xs;
  double* z = smem + L.z;
  double* red = smem + L.red;  // [2][G][RF_NW][PT]
  GpL* gpl = reinterpret_cast<GpL*>(smem + L.gpl);
  double* kpar = smem + L.kpar;
  double* panel = smem + L.panel;
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
    if (isu) {  // inputs beyond a trajectory's last transition are never read
      const double uv = (t + 1 < len) ? a.u[((size_t)t * a.Mu + (a.Mu == 1 ? 0 : om)) * U + uk] : 0.0;
      z[up * D + nna + 2 * na + uk] = uv;
      if (ovalid && t + 1 < len && is_bad(uv)) bad |= MCP_STATUS_NAN;
    }
    lds_barrier();
    // ---- phases K (and V) per GP ---------------------------------------------------------------------------------------
    for (int g = 0; g < G; ++g) {
      const GpL gp = gpl[g];
      // X^T and alpha of GP g: their LDS copies (row pitch NpadMax) where the launch staged them, else global memory (the GP's own Npad)
      const double* Xt = L.xl ? smem + L.xt + g * D * a.NpadMax : gp.Xt;
      const double* al = L.xl ? smem + L.al + g * a.NpadMax : gp.alpha;
      open_phase_k<PT, MAXDEG, NEEDVAR>(gp, kpar + g * KP_STRIDE(D), D, z, panel, red + g * RF_NW * PT, tid, wv, lane, Xt, al,
                                        L.xl ? a.NpadMax : gp.Npad);
      if (NEEDVAR) {
        lds_barrier();
        const int Npad = __builtin_amdgcn_readfirstlane(gp.Npad);
        double q = 0.0;
        for (int I0 = 32 * wv; I0 < Npad; I0 += 32 * RF_NW) q += open_v_block<PT>(gp.Kinv, Npad, I0, panel, lane);
        q = fold_kk(q);
        if (lane < PT) red[(G + g) * RF_NW * PT + wv * PT + lane] = q;
        lds_barrier();  // the panel is rewritten by the next GP
      }
    }
    if (!NEEDVAR) lds_barrier();
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
    if (NEEDVAR && MAXDEG >= 1) lds_barrier();  // k(z, z) above read z, which the next step's phase S rewrites
    cur ^= 1;
  }
  if (bad) atomicOr(a.status, bad);
}

template <int PT, int MAXDEG, bool NEEDVAR>
static int launch_open(const OpenArgs& a, hipStream_t st) {
  const OpenLayout L = open_layout(PT, NEEDVAR, a.model.S, a.model.D, a.model.G, a.NpadMax);
  const size_t lds = (size_t)L.total * sizeof(double);
  if (lds > MCP_LDS_LIMIT) return MCP_ERR_LIMIT;
  MCP_ENSURE_MAX_LDS(rollout_open_kernel<PT, MAXDEG, NEEDVAR>);
  hipLaunchKernelGGL((rollout_open_kernel<PT, MAXDEG, NEEDVAR>), dim3((a.M + PT - 1) / PT), dim3(RF_NT), lds, st, a);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}
template <int PT, bool NEEDVAR>
static int launch_open_deg(const OpenArgs& a, int maxdeg, hipStream_t st) {
  return maxdeg == 0 ? launch_open<PT, 0, NEEDVAR>(a, st) : launch_open<PT, 2, NEEDVAR>(a, st);
}

extern "C" int mcp_rollout_open(const mcp_model* model, const mcp_noise* noise, int M, int T, int particle_pred, const double* x0, const double* u,
                                int Mu, const int32_t* lengths, double* states, double* mu, double* var, uint32_t* status, void* stream) {
  if (!model || !noise || !x0 || !u || !states || !status) return MCP_ERR_ARG;
  if (M <= 0 || T < 2 || (Mu != 1 && Mu != M)) return MCP_ERR_ARG;
  if (model->S > MCP_MAX_STATE || model->U > MCP_MAX_INPUT || model->G > MCP_MAX_GP || model->D > MCP_MAX_GPDIM) return MCP_ERR_LIMIT;
  for (int g = 0; g < model->G && g < MCP_MAX_GP; ++g)
    if (model->gp[g].N > MCP_MAX_TRAIN) return MCP_ERR_LIMIT;
  if (!model_ok(model)) return MCP_ERR_ARG;
  OpenArgs a;
  a.model = *model;
  a.nz = *noise;
  a.M = M;
  a.T = T;
  a.sample = particle_pred & 1;
  a.Mu = Mu;
  a.NpadMax = 0;
  int maxdeg = 0;
  for (int g = 0; g < model->G; ++g) {
    a.NpadMax = imax(a.NpadMax, model->gp[g].Npad);
    maxdeg = imax(maxdeg, model->gp[g].kern.poly_deg);
  }
  a.x0 = x0;
  a.u = u;
  a.lengths = lengths;
  a.states = states;
  a.mu = mu;
  a.var = var;
  a.status = status;
  hipStream_t st = (hipStream_t)stream;
  if (!a.sample && !var) return launch_open_deg<1, false>(a, maxdeg, st);  // the mean chain: no Kinv
  int rc = launch_open_deg<16, true>(a, maxdeg, st);
  // the k panel of 16 trajectories does not fit the LDS: 4 per workgroup (at every compiled limit at once -- S = 16, D = 32, G = 8, Npad = 4096 --
  // that layout takes 148 KB of the 160, so nothing within MCP_MAX_* is refused)
  if (rc == MCP_ERR_LIMIT) rc = launch_open_deg<4, true>(a, maxdeg, st);
  return rc;
}
