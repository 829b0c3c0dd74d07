// The step of the open-loop rollouts, shared by rollout_open.hip (T steps of a tile in one launch, the GPs one after the other) and
// model_step.hip (one step per launch, one workgroup per (tile, GP)) and rollout_mlp.hip (the loop under the tanh-MLP policy): the arguments'
// base part and its fill, the loop's LDS layout, phases K, V, J and J'.  All
// sources instantiate the same functions and the library is built without floating-point contraction, so a (particle, GP) carries the
// same bits whichever of them runs it.
#pragma once
#include "rollout_fwd_shared.h"

namespace mcp {

#define RO_VU 4  // 4-row MFMA steps per register batch of phase V

struct OpenArgs {
  mcp_model model;
  mcp_noise nz;
  int M, T, sample, Mu, NpadMax;
  int na;       // recording form: weight columns of phase J per trajectory (1 / 2 / 4 by the model's highest polynomial degree)
  double* jac;  // recording form: [T-1][M][G][D]
  const double* x0;
  const double* u;
  const int32_t* lengths;
  double* states;
  double* mu;
  double* var;
  uint32_t* status;
};

#define RO_KR(PT) ((PT) == 16 ? 18 : (PT))  // row pitch of the k panel (16 particles: + 2 pad, bank spread of the phase-K stores)

// the LDS layout of a tile's step loop (rollout_open.hip, rollout_mlp.hip)
struct OpenLayout {
  int xs, z, red, gpl, kpar, panel, xt, al, total;  // offsets in doubles
  int vpan, redj, wj, redj_gp;                      // recording form: v panel | partial sums of phase J (stride per GP) | w per trajectory
  int xl;                                           // X^T and alpha of every GP staged in LDS (row pitch NpadMax)
  int ym;                                           // measured feedback form: the measurement row [PT][S]
  int ext;                                          // a form's own region of `extra` doubles (rollout_mlp.hip: features, activations, weights)
};

__host__ __device__ inline OpenLayout open_layout(int PT, bool needvar, int S, int D, int G, int NpadMax, bool needjac = false, int na = 0,
                                                  bool pms = false, int extra = 0) {
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
  // phase J's partial sums [wave][column][D + 1][PT]: with variances one GP at a time, over the k panel (dead once phase V is through);
  // the mean chain runs J beside K for every GP before its one barrier, so each GP has its own
  const int rj = needjac ? RF_NW * na * (D + 1) * PT : 0;
  L.panel = needvar ? take(imax(NpadMax * RO_KR(PT), rj)) : 0;
  L.vpan = (needvar && needjac) ? take(NpadMax * RO_KR(PT)) : 0;
  L.wj = (needvar && needjac) ? take(PT) : 0;
  L.redj_gp = needvar ? 0 : rj;
  L.redj = needvar ? L.panel : (needjac ? take(G * rj) : 0);
  L.ym = pms ? take(PT * S) : 0;
  L.ext = extra > 0 ? take(extra) : 0;
  const int xneed = G * (D + 1) * NpadMax + 4;
  L.xl = (!needvar && o + xneed <= MCP_LDS_LIMIT / 8) ? 1 : 0;
  L.xt = L.xl ? take(G * D * NpadMax) : 0;
  L.al = L.xl ? take(G * NpadMax) : 0;
  L.total = o;
  return L;
}

// orders this wave's LDS stores before its later LDS loads (the DS queue of a wave is in order; this drains it and stops the compiler)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }


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
template <int PT, bool STOREV>
__device__ __forceinline__ double open_v_block(const double* Kinv, int Npad, int I0, const double* panel, double* vpan, int lane) {
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
      if (STOREV && m < PT) {  // recording form: every (row, trajectory) of v comes out of exactly one lane of one wave
        vpan[row * KR + m] = acc_e[r];
        vpan[(row + 1) * KR + m] = acc_o[r];
      }
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

// ---------------------------------------------------------------------------------------
// recording form.  w = var_scale eps / (2 sigma) of trajectory p of the tile at GP g (0 without sampling): the variance from the
// same sums as phase F
// ---------------------------------------------------------------------------------------
template <int PT, int MAXDEG>
__device__ __forceinline__ double open_wjs(const OpenArgs& a, const mcp_noise& nzl, const GpL& gp, const double* kp, int D, int G, int g, int t,
                                           int om, const double* zp, const double* red, int p) {
  if (!a.sample) return 0.0;
  double ktv = 0.0;
#pragma unroll
  for (int w = 0; w < RF_NW; ++w) ktv += red[(G + g) * RF_NW * PT + w * PT + p];
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
  const double var = (kzz - ktv) * gp.var_scale;
  const double e = nzl.eps ? nzl.eps[((size_t)t * a.M + om) * G + g] : philox_normal(nzl, om, t, g);
  return e / (2.0 * sqrt(var)) * gp.var_scale;
}

// phase J for one GP:  R_c[r][n] = sum_j [X^T; 1][r][j] W_c[j][n]  over this wave's 4-row steps of the training index
//   A operand  lane (m = l&15, kk = l>>4) : [X^T; 1][16 db + m][j0 + kk]
//   B operand  lane (kk = l>>4, n = l&15) : W_c[j0 + kk][n], formed in the lane
//   acc[db][c][r] : R_c[16 db + (l>>4) + 4r][n = l&15]
// Padding rows of the training index carry alpha = v = 0.  Lanes of trajectories the tile does not have repeat column 0, unused.
template <int PT, int MAXDEG, bool NEEDVAR>
__device__ __forceinline__ void open_phase_j(const GpL& gp, const double* kp, int D, const double* z, const double* vpan, double wjs, double* redj,
                                             int na, int wv, int lane, const double* Xt, const double* al, int pitch) {
  constexpr int KR = RO_KR(PT);
  constexpr int NAX = MAXDEG == 0 ? 1 : 4;
  const int m = lane & 15, kk = lane >> 4;
  const int nn = m < PT ? m : 0;
  const int Npad = gp.Npad, rows = D + 1, ndb = (rows + 15) >> 4;
  const int deg = MAXDEG == 0 ? 0 : gp.deg;
  const double lam = gp.lambda;
  const double* zp = z + nn * D;
  v4d acc[3][NAX];
#pragma unroll
  for (int db = 0; db < 3; ++db)
#pragma unroll
    for (int c = 0; c < NAX; ++c) acc[db][c] = (v4d){0.0, 0.0, 0.0, 0.0};
  for (int j0 = 4 * wv; j0 < Npad; j0 += 4 * RF_NW) {
    const int j = j0 + kk;
    double se = 0.0, szz = 0.0, sxx = 0.0, pa = 0.0, pb = 0.0;
    for (int d = 0; d < D; ++d) {
      const double x = Xt[(size_t)d * pitch + j];
      const double il = kp[KP_INVLS(D) + d];
      const double zz = zp[d];
      const double tx = il * x;
      sxx = fma(tx, tx, sxx);
      const double il2z = il * il * zz;
      se = fma(-2.0 * il2z, x, se);
      szz = fma(il2z, zz, szz);
      if (MAXDEG >= 2) {
        const double ab = zz * x;
        pa = fma(kp[KP_W20(D) + d], ab, pa);
        pb = fma(kp[KP_W21(D) + d], ab, pb);
      }
    }
    const double kse = lam * exp(-((szz + sxx) + se));
    double beta = al[j];
    if (NEEDVAR) beta = fma(-2.0 * wjs, vpan[j * KR + nn], beta);
    double B[NAX];
    B[0] = beta * kse;
    if (MAXDEG >= 1) {
      B[1] = beta;
      B[2] = beta * pb;
      B[3] = beta * pa;
    }
#pragma unroll
    for (int db = 0; db < 3; ++db) {
      if (db < ndb) {
        const int r = 16 * db + m;
        const double A = r < D ? Xt[(size_t)r * pitch + j] : (r == D ? 1.0 : 0.0);
#pragma unroll
        for (int c = 0; c < NAX; ++c)
          if (c == 0 || (c == 1 && deg >= 1) || (c >= 2 && deg >= 2)) acc[db][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(A, B[c], acc[db][c], 0, 0, 0);
      }
    }
  }
  if (m < PT) {
#pragma unroll
    for (int db = 0; db < 3; ++db)
#pragma unroll
      for (int c = 0; c < NAX; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * db + kk + 4 * r;
          if (db < ndb && row < rows && c < na) redj[((wv * na + c) * rows + row) * PT + m] = acc[db][c][r];
        }
  }
}

// phase J': thread (trajectory p, feature d) of one GP: the waves' parts in wave order, the kernel's factors, the store
//   d delta/dz_d = -2/l_d^2 (z_d R_0[D] - R_0[d]) + w1_d R_1[d] + w20_d R_2[d] + w21_d R_3[d] + w d k(z,z)/dz_d
template <int PT, int MAXDEG, bool NEEDVAR>
__device__ __forceinline__ void open_jac_store(const OpenArgs& a, const GpL& gp, const double* kp, int g, int t, int m0, const double* z,
                                               const double* wjl, const double* redj, int na, int tid) {
  const int D = a.model.D, G = a.model.G, rows = D + 1;
  const int deg = MAXDEG == 0 ? 0 : gp.deg;
  for (int it = tid; it < PT * D; it += RF_NT) {
    const int p = it / D, d = it - p * D;
    const int mm = m0 + p;
    if (mm >= a.M) continue;
    const int len = a.lengths ? imin(imax(a.lengths[mm], 1), a.T) : a.T;
    if (t + 1 >= len) continue;
    double R[4] = {0.0, 0.0, 0.0, 0.0}, R0D = 0.0;
    for (int w = 0; w < RF_NW; ++w) {
      R0D += redj[((w * na + 0) * rows + D) * PT + p];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < na && (c == 0 || (c == 1 && deg >= 1) || (c >= 2 && deg >= 2))) R[c] += redj[((w * na + c) * rows + d) * PT + p];
    }
    const double* zp = z + p * D;
    const double il = kp[KP_INVLS(D) + d];
    const double wjs = NEEDVAR ? wjl[p] : 0.0;
    double J = -2.0 * (il * il) * (zp[d] * R0D - R[0]);
    if (MAXDEG >= 1 && deg >= 1) {
      const double w1 = kp[KP_W1(D) + d];
      J += w1 * R[1];
      if (NEEDVAR) J += wjs * (2.0 * w1 * zp[d]);
      if (MAXDEG >= 2 && deg >= 2) {
        const double wa = kp[KP_W20(D) + d], wb = kp[KP_W21(D) + d];
        J += wa * R[2] + wb * R[3];
        if (NEEDVAR) {
          double Sa = 0.0, Sb = 0.0;
          for (int e = 0; e < D; ++e) {
            const double zz = zp[e] * zp[e];
            Sa = fma(kp[KP_W20(D) + e], zz, Sa);
            Sb = fma(kp[KP_W21(D) + e], zz, Sb);
          }
          J += wjs * (2.0 * zp[d] * (wa * Sb + wb * Sa));
        }
      }
    }
    a.jac[(((size_t)t * a.M + mm) * G + g) * D + d] = J;
  }
}

// the base part of the arguments, for every form (u, Mu, lengths: the open-loop form's own; jac != NULL: the recording form); returns the
// highest polynomial degree of the model's kernels
static inline int open_fill(OpenArgs& a, const mcp_model* model, const mcp_noise* noise, int M, int T, int particle_pred, const double* x0, const double* u,
                     int Mu, const int32_t* lengths, double* states, double* mu, double* var, double* jac, uint32_t* status) {
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
  a.na = jac ? (maxdeg == 0 ? 1 : maxdeg == 1 ? 2 : 4) : 0;
  a.jac = jac;
  a.x0 = x0;
  a.u = u;
  a.lengths = lengths;
  a.states = states;
  a.mu = mu;
  a.var = var;
  a.status = status;
  return maxdeg;
}

}  // namespace mcp
