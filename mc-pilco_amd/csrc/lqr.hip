// Trajectory optimisation on the learned model for gfx950 (MI355X): the dense linearisation of a recorded rollout and the iLQR
// (Gauss-Newton) backward pass over it.
//   mcp_linearize   A [T-1][M][S][S], B [T-1][M][S][U] from the record jac [T-1][M][G][D] of mcp_rollout_open_rec, one launch
//   mcp_lqr_pass    gain [M][T][U][S], kff [M][T][U], dv [M][2] of M independent trajectories, one launch, one workgroup per trajectory
// Both run from the record: the model's index maps and Ts are read, no GP array (as mcp_model_step_bwd).  The reference has no trajectory
// optimiser; on the device the same recursion in torch is T x a dozen launches per pass.
//
// One row of the linearisation, in the terms of model_step_bwd_kernel (model_step.hip): component r of the next state integrates GP
// ogt[r] with the factor 1 (a velocity, a delta-state component) or Ts / 2 (a position), a position also takes Ts x its velocity, and the
// increment's derivative reaches component c through z = [x_not_angle, sin, cos, u]:
//   A[r][c] = [r == c] + Ts [velof[r] == c] + coef[r] (J[zplain[c]] + J[sin_c] cos x_c - J[cos_c] sin x_c),   J = jac[t][m][ogt[r]]
//   B[r][k] = coef[r] J[nna + 2 na + k] du_da[k]
// A row of the next state that no GP integrates is zero (the rollouts write such a component as zero).
//
// The pass keeps Vxx, Vx, A, B and the Q blocks of one trajectory in LDS and walks the rows T - 2 .. 0; a row is six phases between
// LDS-only barriers, one thread per output element, every sum in index order from its first term: nothing depends on the other
// trajectories of the launch, on M or on the run.  Row t - 1 of jac / states / du_da / the cost rows is in flight in two registers per
// thread while row t computes, and is written to the other half of a two-row staging area in phase 3.  The Cholesky factor of Quu (U <= 8)
// is one thread's, in registers; the U x (S + 1) right-hand sides [Qu | Qux] are solved one thread per column.
#include "rollout_common.h"

using namespace mcp;

#define LQ_NT 256
#define LZ_NT 128
#define LQ_SS (MCP_MAX_STATE * MCP_MAX_STATE)
#define LQ_SU (MCP_MAX_STATE * MCP_MAX_INPUT)
#define LQ_UU (MCP_MAX_INPUT * MCP_MAX_INPUT)

struct LqrArgs {
  int S, U, G, D, nna, na, M, T;
  int angle[MCP_MAX_STATE], not_angle[MCP_MAX_STATE], vel[MCP_MAX_GP], not_vel[MCP_MAX_GP];
  double Ts;
  double reg;
  const double *states, *jac, *du_da, *lx, *lu, *hxx, *huu;
  double *gain, *kff, *dv, *A, *B;
  uint32_t* status;
};

// which GP a component integrates and where it enters z, as model_step_bwd_kernel decides it
struct LqrTab {
  int ogt[MCP_MAX_STATE], post[MCP_MAX_STATE], velof[MCP_MAX_STATE], zplain[MCP_MAX_STATE], zang[MCP_MAX_STATE];
};

__device__ __forceinline__ void lqr_tables(const LqrArgs& a, LqrTab* tb, int s) {
  int g_vel = -1, g_pos = -1, zp = -1, za = -1;
  for (int g = 0; g < a.G; ++g) {
    if (a.vel[g] == s) g_vel = g;
    if (a.not_vel[g] == s) g_pos = g;
  }
  for (int i = 0; i < a.nna; ++i)
    if (a.not_angle[i] == s) zp = i;
  for (int i = 0; i < a.na; ++i)
    if (a.angle[i] == s) za = i;
  tb->ogt[s] = g_pos >= 0 ? g_pos : g_vel;
  tb->post[s] = g_pos >= 0 ? 1 : 0;
  tb->velof[s] = g_pos >= 0 ? a.vel[g_pos] : -1;
  tb->zplain[s] = zp;
  tb->zang[s] = za;
}

// jr: the record's row [G][D] of this (t, m); cs / sn [S]: cos / sin of the angle components
__device__ __forceinline__ double lqr_a_elem(const LqrArgs& a, const LqrTab* tb, const double* jr, const double* cs, const double* sn, int r, int c) {
  const int g = tb->ogt[r];
  if (g < 0) return 0.0;
  double v = r == c ? 1.0 : 0.0;
  if (tb->velof[r] == c) v += a.Ts;
  const double* J = jr + g * a.D;
  double dd = 0.0;
  if (tb->zplain[c] >= 0) dd += J[tb->zplain[c]];
  if (tb->zang[c] >= 0) dd += J[a.nna + tb->zang[c]] * cs[c] - J[a.nna + a.na + tb->zang[c]] * sn[c];
  return v + (tb->post[r] ? 0.5 * a.Ts * dd : dd);
}

__device__ __forceinline__ double lqr_b_elem(const LqrArgs& a, const LqrTab* tb, const double* jr, const double* du, int r, int k) {
  const int g = tb->ogt[r];
  if (g < 0) return 0.0;
  const double j = jr[g * a.D + a.nna + 2 * a.na + k];
  return (tb->post[r] ? 0.5 * a.Ts * j : j) * du[k];
}

// ---------------------------------------------------------------------------------------
// mcp_linearize: a workgroup per (t, m), grid-strided
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(LZ_NT) void lqr_linearize_kernel(LqrArgs a) {
  __shared__ LqrTab tb;
  __shared__ double cs[MCP_MAX_STATE], sn[MCP_MAX_STATE], du[MCP_MAX_INPUT];
  const int S = a.S, U = a.U, tid = threadIdx.x;
  if (tid < S) lqr_tables(a, &tb, tid);
  __syncthreads();
  const size_t items = (size_t)(a.T - 1) * a.M;
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {  // it = t M + m
    if (tid < S) {
      double s = 0.0, c = 0.0;
      if (tb.zang[tid] >= 0) sincos_fast(a.states[it * S + tid], &s, &c);
      cs[tid] = c, sn[tid] = s;
    }
    if (tid < U) du[tid] = a.du_da ? a.du_da[it * U + tid] : 1.0;
    __syncthreads();
    const double* jr = a.jac + it * a.G * a.D;
    if (a.A)
      for (int e = tid; e < S * S; e += LZ_NT) a.A[it * S * S + e] = lqr_a_elem(a, &tb, jr, cs, sn, e / S, e % S);
    if (a.B)
      for (int e = tid; e < S * U; e += LZ_NT) a.B[it * S * U + e] = lqr_b_elem(a, &tb, jr, du, e / U, e % U);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------
// mcp_lqr_pass
// ---------------------------------------------------------------------------------------
// one staged row: the record's row, cos / sin of the state's angle components, du_da, and the four cost rows
#define LQ_ST_JAC 0
#define LQ_ST_CS (MCP_MAX_GP * MCP_MAX_GPDIM)
#define LQ_ST_SN (LQ_ST_CS + MCP_MAX_STATE)
#define LQ_ST_DU (LQ_ST_SN + MCP_MAX_STATE)
#define LQ_ST_LX (LQ_ST_DU + MCP_MAX_INPUT)
#define LQ_ST_LU (LQ_ST_LX + MCP_MAX_STATE)
#define LQ_ST_HXX (LQ_ST_LU + MCP_MAX_INPUT)
#define LQ_ST_HUU (LQ_ST_HXX + MCP_MAX_STATE)
#define LQ_ST_ROW (LQ_ST_HUU + MCP_MAX_INPUT)

__global__ __launch_bounds__(LQ_NT) void lqr_pass_kernel(LqrArgs a) {
  extern __shared__ double dvt[];  // [T][2]: (kff^T Qu, kff^T Quu kff) of every row, added in ascending order at the end (T <= MCP_LQR_MAX_T)
  __shared__ double Vxx[LQ_SS], Am[LQ_SS], VA[LQ_SS], Qxx[LQ_SS], Bm[LQ_SU], VB[LQ_SU], Qux[LQ_SU], Quu[LQ_UU], Lc[LQ_UU];
  __shared__ double X[MCP_MAX_INPUT * (MCP_MAX_STATE + 1)], Vx[MCP_MAX_STATE], Qx[MCP_MAX_STATE], Qu[MCP_MAX_INPUT], rinv[MCP_MAX_INPUT];
  __shared__ double stage[2][LQ_ST_ROW];
  __shared__ LqrTab tb;
  __shared__ unsigned flag_nan, flag_spd;
  const int S = a.S, U = a.U, M = a.M, T = a.T, GD = a.G * a.D, S1 = S + 1;
  const int tid = threadIdx.x, m = blockIdx.x;
  const double nanv = __longlong_as_double(0x7ff8000000000000ll);

  // the small operands of a row, one per thread: x [S] | du_da [U] | lx [S] | lu [U] | hxx [S] | huu [U]
  int seg = -1, off = 0;
  {
    int q = tid;
    const int w[6] = {S, U, S, U, S, U};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (seg < 0 && q < w[i]) seg = i, off = q;
      q -= w[i];
    }
  }
  const double* sbase = seg == 0 ? a.states : seg == 1 ? a.du_da : seg == 2 ? a.lx : seg == 3 ? a.lu : seg == 4 ? a.hxx : a.huu;
  const int swid = (seg & 1) ? U : S;
  double pj = 0.0, ps = 0.0;
  // rows 0 .. T - 2 take part with everything; row T - 1 with its cost rows alone (no transition leaves it: jac has no such row)
  auto load_row = [&](int t) {
    const bool dyn = t < T - 1;
    if (dyn && tid < GD) pj = a.jac[((size_t)t * M + m) * GD + tid];
    if (seg >= (dyn ? 0 : 2)) ps = sbase ? sbase[((size_t)t * M + m) * swid + off] : 1.0;  // (du_da NULL: ones)
  };
  auto stage_row = [&](int t) {
    double* st = stage[t & 1];
    const bool dyn = t < T - 1;
    bool bad = false;
    if (dyn && tid < GD) st[LQ_ST_JAC + tid] = pj, bad = is_bad(pj);
    if (seg >= (dyn ? 0 : 2)) {
      bad = bad || is_bad(ps);
      if (seg == 0) {
        double s = 0.0, c = 0.0;
        if (tb.zang[off] >= 0) sincos_fast(ps, &s, &c);
        st[LQ_ST_CS + off] = c, st[LQ_ST_SN + off] = s;
      } else {
        st[(seg == 1 ? LQ_ST_DU : seg == 2 ? LQ_ST_LX : seg == 3 ? LQ_ST_LU : seg == 4 ? LQ_ST_HXX : LQ_ST_HUU) + off] = ps;
      }
    }
    if (bad) flag_nan = 1u;
  };

  if (tid < S) lqr_tables(a, &tb, tid);
  if (tid == 0) flag_nan = 0u, flag_spd = 0u;
  load_row(T - 1);
  __syncthreads();
  stage_row(T - 1);
  load_row(T - 2);
  lds_barrier();
  // ---- row T - 1:  Vx = lx, Vxx = diag(hxx), gain = 0, kff = -lu / (huu + reg) ----
  {
    const double* st = stage[(T - 1) & 1];
    for (int e = tid; e < S * S; e += LQ_NT) Vxx[e] = (e / S == e % S) ? st[LQ_ST_HXX + e / S] : 0.0;
    if (tid < S) Vx[tid] = st[LQ_ST_LX + tid];
    for (int e = tid; e < U * S; e += LQ_NT) a.gain[((size_t)m * T + (T - 1)) * U * S + e] = 0.0;
    if (tid == 0) {
      double d0 = 0.0, d1 = 0.0;
      for (int k = 0; k < U; ++k) {
        const double den = st[LQ_ST_HUU + k] + a.reg, lu = st[LQ_ST_LU + k];
        if (is_bad(den)) flag_nan = 1u;
        else if (den <= 0.0) flag_spd = 1u;
        const double kf = -lu / den;
        a.kff[((size_t)m * T + (T - 1)) * U + k] = kf;
        d0 = fma(kf, lu, d0);
        d1 = fma(kf, den * kf, d1);
      }
      dvt[2 * (T - 1)] = d0, dvt[2 * (T - 1) + 1] = d1;
    }
  }
  stage_row(T - 2);
  if (T >= 3) load_row(T - 3);
  lds_barrier();

  for (int t = T - 2; t >= 0; --t) {
    if (flag_nan | flag_spd) break;  // (written before the last barrier: the same answer in every thread)
    const double* st = stage[t & 1];
    // ---- phase 2: A, B of row t ----
    for (int e = tid; e < S * S; e += LQ_NT) Am[e] = lqr_a_elem(a, &tb, st + LQ_ST_JAC, st + LQ_ST_CS, st + LQ_ST_SN, e / S, e % S);
    for (int e = tid; e < S * U; e += LQ_NT) Bm[e] = lqr_b_elem(a, &tb, st + LQ_ST_JAC, st + LQ_ST_DU, e / U, e % U);
    lds_barrier();
    // ---- phase 3: VA = Vxx A, VB = Vxx B, Qx = lx + A^T Vx, Qu = lu + B^T Vx; row t - 1 goes to the other half of the staging area ----
    for (int e = tid; e < S * S + S * U + S + U; e += LQ_NT) {
      if (e < S * S) {
        const int i = e / S, j = e % S;
        double acc = 0.0;
        for (int k = 0; k < S; ++k) acc = fma(Vxx[i * S + k], Am[k * S + j], acc);
        VA[e] = acc;
      } else if (e < S * S + S * U) {
        const int f = e - S * S, i = f / U, j = f % U;
        double acc = 0.0;
        for (int k = 0; k < S; ++k) acc = fma(Vxx[i * S + k], Bm[k * U + j], acc);
        VB[f] = acc;
      } else if (e < S * S + S * U + S) {
        const int i = e - S * S - S * U;
        double acc = 0.0;
        for (int k = 0; k < S; ++k) acc = fma(Am[k * S + i], Vx[k], acc);
        Qx[i] = st[LQ_ST_LX + i] + acc;
      } else {
        const int i = e - S * S - S * U - S;
        double acc = 0.0;
        for (int k = 0; k < S; ++k) acc = fma(Bm[k * U + i], Vx[k], acc);
        Qu[i] = st[LQ_ST_LU + i] + acc;
      }
    }
    if (t >= 1) {
      stage_row(t - 1);
      if (t >= 2) load_row(t - 2);
    }
    lds_barrier();
    // ---- phase 4: Qxx = diag(hxx) + A^T VA, Qux = B^T VA, Quu = diag(huu) + B^T VB + reg I ----
    for (int e = tid; e < S * S + U * S + U * U; e += LQ_NT) {
      if (e < S * S) {
        const int i = e / S, j = e % S;
        double acc = 0.0;
        for (int k = 0; k < S; ++k) acc = fma(Am[k * S + i], VA[k * S + j], acc);
        Qxx[e] = i == j ? st[LQ_ST_HXX + i] + acc : acc;
      } else if (e < S * S + U * S) {
        const int f = e - S * S, i = f / S, j = f % S;
        double acc = 0.0;
        for (int k = 0; k < S; ++k) acc = fma(Bm[k * U + i], VA[k * S + j], acc);
        Qux[f] = acc;
      } else {
        const int f = e - S * S - U * S, i = f / U, j = f % U;
        double acc = 0.0;
        for (int k = 0; k < S; ++k) acc = fma(Bm[k * U + i], VB[k * U + j], acc);
        Quu[f] = i == j ? (st[LQ_ST_HUU + i] + acc) + a.reg : acc;
      }
    }
    lds_barrier();
    // ---- phase 5a: Quu = L L^T, one thread, the factor in registers (the lower triangle of Quu is read) ----
    if (tid == 0) {
      double L[MCP_MAX_INPUT][MCP_MAX_INPUT];
      unsigned fn = 0u, fs = 0u;
#pragma unroll
      for (int j = 0; j < MCP_MAX_INPUT; ++j) {
        if (j < U) {
          double p = Quu[j * U + j];
#pragma unroll
          for (int k = 0; k < j; ++k) p = fma(-L[j][k], L[j][k], p);
          if (!(fn | fs)) {  // (the first bad pivot decides: the ones behind it are its NaN)
            if (is_bad(p)) fn = 1u;
            else if (p <= 0.0) fs = 1u;
          }
          const double d = sqrt(p), ri = 1.0 / d;
          L[j][j] = d;
          rinv[j] = ri;
          Lc[j * U + j] = d;
#pragma unroll
          for (int i = j + 1; i < MCP_MAX_INPUT; ++i) {
            if (i < U) {
              double v = Quu[i * U + j];
#pragma unroll
              for (int k = 0; k < j; ++k) v = fma(-L[i][k], L[j][k], v);
              L[i][j] = v * ri;
              Lc[i * U + j] = L[i][j];
            }
          }
        }
      }
      if (fn) flag_nan = 1u;
      if (fs) flag_spd = 1u;
    }
    lds_barrier();
    // ---- phase 5b: L L^T X = [Qu | Qux], one thread per column ----
    if (tid < S1) {
      double y[MCP_MAX_INPUT];
#pragma unroll
      for (int k = 0; k < MCP_MAX_INPUT; ++k) {
        if (k < U) {
          double v = tid == 0 ? Qu[k] : Qux[k * S + tid - 1];
#pragma unroll
          for (int j = 0; j < k; ++j) v = fma(-Lc[k * U + j], y[j], v);
          y[k] = v * rinv[k];
        }
      }
#pragma unroll
      for (int k = MCP_MAX_INPUT - 1; k >= 0; --k) {
        if (k < U) {
          double v = y[k];
#pragma unroll
          for (int j = k + 1; j < MCP_MAX_INPUT; ++j)
            if (j < U) v = fma(-Lc[j * U + k], y[j], v);
          y[k] = v * rinv[k];
          X[k * S1 + tid] = y[k];
        }
      }
    }
    lds_barrier();
    // ---- phase 6: kff = -X[:, 0], gain = X[:, 1:], Vx = Qx + Qux^T kff, Vxx = (W + W^T) / 2 with W = Qxx - Qux^T gain, the row's dv terms ----
    for (int e = tid; e < U * S; e += LQ_NT) a.gain[((size_t)m * T + t) * U * S + e] = X[(e / S) * S1 + 1 + e % S];
    if (tid < U) a.kff[((size_t)m * T + t) * U + tid] = -X[tid * S1];
    for (int e = tid; e < S * S; e += LQ_NT) {
      const int i = e / S, j = e % S;
      double wij = Qxx[i * S + j], wji = Qxx[j * S + i];
      for (int k = 0; k < U; ++k) {
        wij = fma(-Qux[k * S + i], X[k * S1 + 1 + j], wij);
        wji = fma(-Qux[k * S + j], X[k * S1 + 1 + i], wji);
      }
      Vxx[e] = 0.5 * (wij + wji);
    }
    if (tid >= LQ_NT - S) {  // (the last wave: the first is the busiest)
      const int i = tid - (LQ_NT - S);
      double acc = Qx[i];
      for (int k = 0; k < U; ++k) acc = fma(Qux[k * S + i], -X[k * S1], acc);
      Vx[i] = acc;
    }
    if (tid == LQ_NT - 64) {
      double d0 = 0.0, d1 = 0.0;
      for (int k = 0; k < U; ++k) {
        const double kf = -X[k * S1];
        double qk = 0.0;
        for (int j = 0; j < U; ++j) qk = fma(Quu[k * U + j], -X[j * S1], qk);
        d0 = fma(kf, Qu[k], d0);
        d1 = fma(kf, qk, d1);
      }
      dvt[2 * t] = d0, dvt[2 * t + 1] = d1;
    }
    lds_barrier();
  }
  __syncthreads();  // (also orders this workgroup's earlier global stores ahead of the NaN fill below)
  const unsigned bits = (flag_nan ? MCP_STATUS_NAN : 0u) | (flag_spd ? MCP_STATUS_NOT_SPD : 0u);
  if (bits) {
    for (size_t e = tid; e < (size_t)T * U * S; e += LQ_NT) a.gain[(size_t)m * T * U * S + e] = nanv;
    for (size_t e = tid; e < (size_t)T * U; e += LQ_NT) a.kff[(size_t)m * T * U + e] = nanv;
    if (tid < 2) a.dv[(size_t)m * 2 + tid] = nanv;
    if (tid == 0) atomicOr(a.status, bits);
  } else if (tid < 2) {
    double acc = 0.0;
    for (int t = 0; t < T; ++t) acc += dvt[2 * t + tid];
    a.dv[(size_t)m * 2 + tid] = acc;
  }
}

// ---- host path: checks -> fill -> launch (a refused call makes no HIP call) ------------------------------------------------------------
static int lqr_checks(bool ptrs, const mcp_model* model, int M, int T) {
  if (!ptrs || M <= 0 || T < 2) return MCP_ERR_ARG;
  if (!model_within_limits(model, false) || T > MCP_LQR_MAX_T) return MCP_ERR_LIMIT;
  return model_lists_ok(model) ? MCP_OK : MCP_ERR_ARG;  // (what model_ok asks of the scalars and index lists: no GP descriptor is looked at)
}

static void lqr_fill(LqrArgs& a, const mcp_model* model, int M, int T, const double* states, const double* jac, const double* du_da) {
  memset(&a, 0, sizeof(a));
  sweep_fill_model(a, model, M, T);
  a.states = states, a.jac = jac, a.du_da = du_da;
}

extern "C" int mcp_linearize(const mcp_model* model, int M, int T, const double* states, const double* jac, const double* du_da, double* A,
                             double* B, void* stream) {
  const int rc = lqr_checks(model && states && jac, model, M, T);
  if (rc != MCP_OK) return rc;
  if (!A && !B) return MCP_OK;  // nothing asked for
  LqrArgs a;
  lqr_fill(a, model, M, T, states, jac, du_da);
  a.A = A, a.B = B;
  const size_t items = (size_t)(T - 1) * M;
  hipLaunchKernelGGL(lqr_linearize_kernel, dim3((unsigned)(items < 65536 ? items : 65536)), dim3(LZ_NT), 0, (hipStream_t)stream, a);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_lqr_pass(const mcp_model* model, int M, int T, const double* states, const double* jac, const double* du_da, const double* lx,
                            const double* lu, const double* hxx, const double* huu, double reg, double* gain, double* kff, double* dv,
                            uint32_t* status, void* stream) {
  const bool reg_ok = reg >= 0.0 && reg <= 1.79769313486231570815e308;  // not negative, infinite or NaN: looked at with the sizes
  const int rc = lqr_checks(model && states && jac && lx && lu && hxx && huu && gain && kff && dv && status && reg_ok, model, M, T);
  if (rc != MCP_OK) return rc;
  LqrArgs a;
  lqr_fill(a, model, M, T, states, jac, du_da);
  a.lx = lx, a.lu = lu, a.hxx = hxx, a.huu = huu, a.reg = reg;
  a.gain = gain, a.kff = kff, a.dv = dv, a.status = status;
  hipLaunchKernelGGL(lqr_pass_kernel, dim3(M), dim3(LQ_NT), (size_t)2 * T * sizeof(double), (hipStream_t)stream, a);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}
