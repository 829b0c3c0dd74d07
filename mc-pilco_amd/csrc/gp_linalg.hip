// Dense linear algebra of the GP pretrain and training paths for gfx950 (mcp_chol_factor, mcp_chol_inverse, mcp_sym_sandwich): the
// Cholesky factorisation in three forms (the LDS kernel for N <= 16 and short panel tails, the left-looking MFMA kernel of one workgroup,
// panels across the chip from 600 rows), U^-1 and K^-1 = U^-1 U^-T in three forms (one wave per column for N <= 16, block columns in one
// launch pair up to 1152 rows, block forward substitution beyond), and the transposed-left product tn_gemm_kernel.
// Replaces torch.cholesky / torch.inverse of GP_prior.forward (gpr_lib/GP_prior/GP_prior.py:106-110; once per GP per trial in
// Model_learning.pretrain_gp, once per EPOCH in GP_prior.fit_model, GP_prior.py:179-230) and the chain rule through K^-1 of its autograd
// graph.  launch_chol_left and launch_inverse_mfma also serve the batched training epoch of gp_nll.hip (gp_launch.h).
#include <type_traits>

#include "gp_launch.h"
#include "mcp_device.h"

using namespace mcp;

// ---------------------------------------------------------------------------------------
// Cholesky A = U^T U, upper, in place, one workgroup, blocked right-looking (NB = 16):
//   per block row kb:  (1) 16x16 diagonal block factored in LDS by wave 0,
//                      (2) row panel U[kb:kb+16, kb+16:N] = U_kk^-T A[...]  (thread per column),
//                          kept in LDS for (3) the trailing update A[i][j] -= sum_m U[m][i] U[m][j].
// ---------------------------------------------------------------------------------------
#define CH_NB 16
#define CH_NT 1024

__global__ __launch_bounds__(CH_NT) void chol_factor_kernel(int N, double* __restrict__ A, int lda, double* __restrict__ logdet,
                                                            uint32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* dg = smem;                     // [NB][NB+1] diagonal block
  double* pn = smem + CH_NB * (CH_NB + 1);  // [NB][N] row panel
  const int tid = threadIdx.x;
  double ld_acc = 0.0;  // thread 0 only
  uint32_t bad = 0;

  for (int kb = 0; kb < N; kb += CH_NB) {
    const int nb = min(CH_NB, N - kb);
    // (1) diagonal block -> LDS, factor with the first nb lanes of wave 0
    if (tid < CH_NB * CH_NB) {
      int r = tid / CH_NB, c = tid % CH_NB;
      dg[r * (CH_NB + 1) + c] = (r < nb && c < nb && c >= r) ? A[(size_t)(kb + r) * lda + kb + c] : 0.0;
    }
    __syncthreads();
    if (tid < MCP_WAVE) {
      volatile double* dgv = dg;  // single-wave section: LDS accesses must stay in program order
      for (int k = 0; k < nb; ++k) {
        double d = dgv[k * (CH_NB + 1) + k];
        if (!(d > 0.0)) bad |= MCP_STATUS_NOT_SPD;
        double sd = sqrt(d);
        if (tid == 0) ld_acc += log(sd);
        // scale row k, then rank-1 update of the rows below (lanes <-> columns)
        double ukc = 0.0;
        if (tid < nb && tid >= k) {
          ukc = (tid == k) ? sd : dgv[k * (CH_NB + 1) + tid] / sd;
          dgv[k * (CH_NB + 1) + tid] = ukc;
        }
        __builtin_amdgcn_wave_barrier();
        if (tid < nb && tid > k) {
          for (int r = k + 1; r <= tid; ++r) dgv[r * (CH_NB + 1) + tid] = dgv[r * (CH_NB + 1) + tid] - dgv[k * (CH_NB + 1) + r] * ukc;
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    __syncthreads();
    // write the factored diagonal block back (and zero below the diagonal)
    if (tid < CH_NB * CH_NB) {
      int r = tid / CH_NB, c = tid % CH_NB;
      if (r < nb && c < nb) A[(size_t)(kb + r) * lda + kb + c] = (c >= r) ? dg[r * (CH_NB + 1) + c] : 0.0;
    }
    const int j0 = kb + nb;
    const int nc = N - j0;
    // (2) panel solve: column j of the panel solves U_kk^T x = a  (forward substitution)
    for (int c = tid; c < nc; c += CH_NT) {
      double x[CH_NB];
#pragma unroll
      for (int r = 0; r < CH_NB; ++r) {
        if (r < nb) {
          double s = A[(size_t)(kb + r) * lda + j0 + c];
          for (int m = 0; m < r; ++m) s = fma(-dg[m * (CH_NB + 1) + r], x[m], s);
          x[r] = s / dg[r * (CH_NB + 1) + r];
          A[(size_t)(kb + r) * lda + j0 + c] = x[r];
          pn[(size_t)r * nc + c] = x[r];
        }
      }
    }
    __syncthreads();
    // (3) trailing update over the upper triangle (i <= j)
    //     4x4 register tiles: per panel row m a thread reads 4 + 4 panel values from LDS for 16 multiply-adds (one element per
    //     thread needed 2 LDS reads per multiply-add and made the phase instruction bound); only tiles on or above the diagonal
    const int nts = (nc + 3) >> 2;
    for (int t = tid; t < nts * nts; t += CH_NT) {
      const int ti = t / nts, tj = t - ti * nts;
      if (tj < ti) continue;
      const int i0 = 4 * ti, jj0 = 4 * tj;
      double acc[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int i = imin(i0 + r, nc - 1), j = imin(jj0 + c, nc - 1);
          acc[r][c] = A[(size_t)(j0 + i) * lda + j0 + j];
        }
#pragma unroll
      for (int m = 0; m < CH_NB; ++m) {
        if (m < nb) {
          double pi[4], pj[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pi[r] = pn[(size_t)m * nc + imin(i0 + r, nc - 1)];
            pj[r] = pn[(size_t)m * nc + imin(jj0 + r, nc - 1)];
          }
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = fma(-pi[r], pj[c], acc[r][c]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int i = i0 + r, j = jj0 + c;
          if (i < nc && j < nc && j >= i) A[(size_t)(j0 + i) * lda + j0 + j] = acc[r][c];
        }
    }
    __syncthreads();
  }
  // zero the strictly-lower part that lies outside the diagonal blocks
  for (int idx = tid; idx < N * N; idx += CH_NT) {
    int r = idx / N, c = idx % N;
    if (c < r && (c / CH_NB) != (r / CH_NB)) A[(size_t)r * lda + c] = 0.0;
  }
  if (tid == 0) *logdet = 2.0 * ld_acc;
  if (bad) atomicOr(status, bad);
}

// Uinv = U^-1 for N <= 1024 (mcp_chol_inverse runs it for N <= 16): one WAVE per column j.  Back substitution
// x_i = (delta_ij - sum_{i<m<=j} U[i][m] x_m) / U[i][i], i = j .. 0: lane l keeps x_m for m = l (mod 64) in registers, the row of U is
// one coalesced read per 64 columns (the next row is fetched while the current dot product is reduced), the dot product a wave64 DPP
// sum.  N columns run in parallel.
#define TW_KM 16  // 64 * TW_KM >= N
__global__ __launch_bounds__(256) void tri_inverse_wave_kernel(int N, const double* __restrict__ U, int ldu, double* __restrict__ Ui, int ldi) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);  // this wave's column
  if (j >= N) return;
  double x[TW_KM];
#pragma unroll
  for (int k = 0; k < TW_KM; ++k) x[k] = 0.0;
  const int kj = j >> 6;  // register slots 0..kj can hold a nonzero
  double urow[TW_KM], unext[TW_KM];
  auto load_row = [&](double (&r)[TW_KM], int i) {
#pragma unroll
    for (int k = 0; k < TW_KM; ++k) {
      const int m = k * 64 + lane;
      r[k] = (k <= kj && i >= 0 && m <= j) ? U[(size_t)i * ldu + m] : 0.0;
    }
  };
  load_row(urow, j);
  for (int i = j; i >= 0; --i) {
    load_row(unext, i - 1);
    double part = 0.0, uii = 0.0;
#pragma unroll
    for (int k = 0; k < TW_KM; ++k) {
      if (k <= kj) {
        const int m = k * 64 + lane;
        if (m > i) part = fma(urow[k], x[k], part);  // x_m is still 0 for m > j
        if (m == i) uii = urow[k];
      }
    }
    const double dot = wave_sum(part);
    const double d = wave_sum(uii);  // the diagonal element, from the lane that owns column i
    const double xi = ((i == j ? 1.0 : 0.0) - dot) / d;
#pragma unroll
    for (int k = 0; k < TW_KM; ++k)
      if (k * 64 + lane == i) x[k] = xi;
#pragma unroll
    for (int k = 0; k < TW_KM; ++k) urow[k] = unext[k];
  }
  // column j of the result: rows <= j from the registers, zeros below
#pragma unroll
  for (int k = 0; k < TW_KM; ++k) {
    const int m = k * 64 + lane;
    if (m < N) Ui[(size_t)m * ldi + j] = m <= j ? x[k] : 0.0;
  }
}

// ---------------------------------------------------------------------------------------
// MFMA-blocked forms of the two kernels above (GP_prior.forward's torch.cholesky / torch.inverse, GP_prior.py:106-110, once per GP
// per trial in pretrain and once per EPOCH in GP_prior.fit_model, GP_prior.py:179-230).  Every 16x16 block product runs on
// v_mfma_f64_16x16x4_f64:
//   A operand  lane l -> A[i = l & 15][k = l >> 4],   B operand  lane l -> B[k = l >> 4][j = l & 15],
//   accumulator register r of lane l -> D[(l >> 4) + 4 r][l & 15]          (so register u of an accumulator IS the B operand of
//   step u of a following product: D2 = A2 * D needs no data movement).
// The 16x16 diagonal blocks are factored / inverted by ONE wave in registers: lane c holds column c (the LDS form of chol_factor_kernel
// spends ~13 k cycles per block in volatile round trips).
// Measured at N = 300 (tools/time_fit_model.py, rocprofv3): see DESIGN.md 4.5.
// ---------------------------------------------------------------------------------------
#define CM_NT 512  // (1024 threads = 128 registers: the in-register diagonal block of wave 0 spills 26 of them)
typedef double __attribute__((address_space(1))) * gdp_t;         // explicit global pointers: a noinline device function would otherwise
typedef const double __attribute__((address_space(1))) * gcdp_t;  // address its pointer arguments as flat (64-bit address per lane and load)
// arguments of a non-kernel function arrive in vector registers even when they are uniform: back to scalars
__device__ __forceinline__ int uniform_int(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ gdp_t uniform_ptr(gdp_t p) {
  const unsigned long long a = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return (gdp_t)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ double lane_get(double v, int l) {  // l: a compile-time constant after unrolling
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// the value of lane R of each 16-lane row, in every lane of that row (DPP row_newbcast: stays in the vector registers -- the 136
// scalars a 16x16 block needs through v_readlane overflowed the scalar file into v_writelane / v_readlane spill pairs)
template <int R>
__device__ __forceinline__ double row_get(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x150 + R, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x150 + R, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
// Column steps k = K..15 of the in-register Cholesky of a 16x16 block (lane c: column c in x[]; rows below the diagonal are scratch)
// with the inverse riding along: after step k row k of U is final, which is all that row k of L^-1 = U^-T needs,
//   Linv[k][c] = (delta_kc - sum_{m < k} U[m][k] Linv[m][c]) / U[k][k]          (lane c: v[m] = Linv[m][c] = Uinv[c][m]),
// k independent FMAs that fill the stalls of the step's dependent chain (rsq, Newton steps, the pivot row) instead of a second
// serial pass of sixteen rows after it.
template <int K>
struct Chol16Col {
  template <int Rr>
  static __device__ __forceinline__ void update(double uk, double (&x)[16]) {
    if constexpr (Rr < 16) {
      x[Rr] = fma(-row_get<Rr>(uk), uk, x[Rr]);
      update<Rr + 1>(uk, x);
    }
  }
  template <int M>
  static __device__ __forceinline__ void dotl(const double (&x)[16], const double (&v)[16], double& s0, double& s1) {
    if constexpr (M < K) {
      if constexpr (M & 1)
        s1 = fma(-row_get<K>(x[M]), v[M], s1);
      else
        s0 = fma(-row_get<K>(x[M]), v[M], s0);
      dotl<M + 1>(x, v, s0, s1);
    }
  }
  static __device__ __forceinline__ void run(double (&x)[16], double (&v)[16], int c, uint32_t& bad) {
    const double dk = row_get<K>(x[K]);
    if (!(dk > 0.0)) bad |= MCP_STATUS_NOT_SPD;
    // sqrt(dk) and 1 / sqrt(dk) together (v_rsq_f64 seed, coupled Goldschmidt step, two Newton steps each): the pivots of a Gram
    // matrix are far from the denormal / overflow ranges the library forms rescale for, and a pivot <= 0 or NaN still gives NaN
    const double y = __builtin_amdgcn_rsq(dk);
    double g = dk * y, h = 0.5 * y;
    const double r0 = fma(-h, g, 0.5);
    g = fma(g, r0, g);
    h = fma(h, r0, h);
    g = fma(fma(-g, g, dk), h, g);
    g = fma(fma(-g, g, dk), h, g);
    double is = h + h;
    is = fma(is, fma(-g, is, 1.0), is);
    is = fma(is, fma(-g, is, 1.0), is);
    const double uk = c == K ? g : (c > K ? x[K] * is : 0.0);
    x[K] = uk;
    update<K + 1>(uk, x);
    double s0 = c == K ? 1.0 : 0.0, s1 = 0.0;
    dotl<0>(x, v, s0, s1);
    double vk = (s0 + s1) * is;
    asm volatile("" : "+v"(vk));  // (pins the step's work before the scheduling fence below)
    v[K] = vk;
    __builtin_amdgcn_sched_barrier(0);  // (or the scheduler hoists every broadcast of every step to the top and spills a hundred registers)
    if constexpr (K < 15) Chol16Col<K + 1>::run(x, v, c, bad);
  }
};

// lane c (= lane & 15; the four 16-lane rows of the wave work redundantly) holds column c of an upper-triangular 16x16 block in
// x[0..15] (x[r] = U[r][c], 0 below the diagonal).  Returns column c of U^-1 in w[].  inv_d[r] = 1 / U[r][r].
__device__ __forceinline__ void tri16_inverse(const double (&x)[16], const double (&inv_d)[16], int c, double (&w)[16]) {
#pragma unroll
  for (int m = 0; m < 16; ++m) w[m] = 0.0;
#pragma unroll
  for (int r = 15; r >= 0; --r) {
    double s = (r == c) ? 1.0 : 0.0;
#pragma unroll
    for (int m = r + 1; m < 16; ++m) s = fma(-lane_get(x[r], m), w[m], s);  // U[r][m] w[m]  (w[m] = 0 for m > c)
    w[r] = s * inv_d[r];
  }
}

// The factorization LEFT-looking (round 4), one workgroup per matrix: block row I of U is finished in one go,
//   T_IJ = A_IJ - sum_{k < I} U_kI^T U_kJ,   U_II = chol(T_II),   U_IJ = U_II^-T T_IJ   (J > I),
// so every 16x16 tile of the matrix is written ONCE (a right-looking form reads, updates and writes every trailing tile in every
// block step: a store -> barrier -> load chain per step that its MFMAs wait behind), the sums over k stream finished, read-only
// rows with their loads two k-steps ahead, and the one serial chain -- factoring and inverting the diagonal block, wave 0 -- runs
// BESIDE the other waves' sums, which do not need it until their last four MFMAs:
//   wave 0:       T_II = P_I - U_(I-1)I^T U_(I-1)I  (P_I and the tile both wait in LDS, see below) -> columns in registers -> U_II, W_I = U_II^-1
//   tile waves:   tiles J = I + 1 + hw + 6 s, up to CL_GS at a time in the same k loop (their loads overlap), T_IJ kept in registers
//   wave 1 also:  P_(I+1) = A_(I+1)(I+1) - sum_{k < I} U_k(I+1)^T U_k(I+1): all of the NEXT diagonal block's sum that can be had
//                 before this row is finished; both of its MFMA operands are the B operand of the wave's tile J = I + 1 -- no loads
//                 (in the last block rows, where some waves have no tile, the first of those does it instead)
//   barrier;  U_IJ = W_I^T T_IJ (register u of T IS the B operand of step u), wave 1 leaves U_I(I+1) in LDS for the next row;  barrier.
// The chain per block row is then: 4 MFMAs, two LDS round trips, the 16 column steps, the inverse, two barriers and one tile product.
// CL_MAXS tile slots per tile wave, up to CL_GS of them in one k loop (registers).
// the role of wave 0 (a function of its own: its registers are then allocated apart from the tile role's)
__device__ __noinline__ void chol_left_diag_role(int N_, gdp_t A_, int lda_, double* __restrict__ logdet, uint32_t* __restrict__ status,
                                                 double* ui, double* dg, double (*dgp)[256], double* nt) {
  const int N = uniform_int(N_), lda = uniform_int(lda_);
  const gdp_t A = uniform_ptr(A_);
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, li = lane & 15;
  const int NBK = (N + 15) >> 4;
  {
    double ld_acc = 0.0;
    uint32_t bad = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // P_0 = A_00 (identity beyond N), no tile above it
      const int row = kq + 4 * r;
      dgp[0][row * 16 + li] = (row < N && li < N) ? A[(size_t)row * lda + li] : (row == li ? 1.0 : 0.0);
      nt[row * 16 + li] = 0.0;
    }
    for (int I = 0; I < NBK; ++I) {
      int kb = I << 4;
      asm volatile("" : "+s"(kb));  // (or the sixteen store addresses of the block become 64-bit induction variables, spilled and reloaded every row)
      const int nb = min(16, N - kb);
      v4d acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = dgp[I & 1][(kq + 4 * r) * 16 + li];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double av = nt[(4 * u + kq) * 16 + li];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-av, av, acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) dg[(kq + 4 * r) * 16 + li] = acc[r];
      __builtin_amdgcn_wave_barrier();
      int c = li;
      asm volatile("" : "+v"(c));  // (or sixty loop-invariant masks and constants of c are hoisted out of the row loop and spilled)
      double x[16], w[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const double v = dg[r * 16 + c];
        x[r] = r <= c ? v : 0.0;
      }
      Chol16Col<0>::run(x, w, c, bad);  // w[m] = Uinv[c][m]
      if (lane < 16 && c < nb) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (r < nb) A[(size_t)(kb + r) * lda + kb + c] = r <= c ? x[r] : 0.0;  // (zeros below the diagonal, as torch.cholesky(upper=True) returns)
        double dcc = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) dcc = r == c ? x[r] : dcc;
        ld_acc += log(dcc);
      }
      if (lane < 16) {
#pragma unroll
        for (int m = 0; m < 16; ++m) ui[c * 16 + m] = w[m];
      }
      __syncthreads();  // (the tile role's two barriers of the row)
      __syncthreads();
    }
    const double tot = wave_sum(lane < 16 ? ld_acc : 0.0);
    if (lane == 0) *logdet = 2.0 * tot;
    if (bad) atomicOr(status, bad);
  }
}

// the k loop of NA tiles of one wave:  acc[q] = sum_{k < I} U_kI^T U_kJq.  The loads are unconditional (a lane beyond column N reads a
// valid address of no consequence: its sums reach only outputs that are never stored; rows are always inside, off-diagonal tiles
// exist only in full block rows).  Operands of NS consecutive k-steps wait in NS register sets that take turns: the loads of a set are
// issued right after its MFMAs, NS k-steps before they are needed.
// WITH_P: tile 0 of the group is J = I + 1, whose B operand U_k(I+1) is both operands of the next diagonal block's sum
// accp = sum_{k < I} U_k(I+1)^T U_k(I+1)  (four more MFMAs per k-step, no more loads; okc: this lane's column of that block is inside N).
template <int NA, bool WITH_P, bool PANEL>
__device__ __forceinline__ void chol_left_sums(gcdp_t A, int lda, int I, unsigned aoff, const double* panel, const unsigned (&off)[NA], v4d (&acc)[NA],
                                               v4d& accp, bool okc) {
  // register sets in flight (a wave with one tile has only its loads to wait for; deeper measured slower: every row starts with NS
  // sets of loads whether it has that many k-steps or not)
  constexpr int NS = NA == 1 ? 6 : (NA == 2 ? 4 : 3);
  const int kmax = max(I - 1, 0);
  double av[PANEL ? 1 : NS][4], bv[NS][NA][4];
  auto fetch = [&](int set, int k) {
    gcdp_t rp = A + (size_t)(16 * min(k, kmax)) * lda;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if constexpr (!PANEL) av[set][u] = (rp + (size_t)(4 * u) * lda)[aoff];
#pragma unroll
      for (int q = 0; q < NA; ++q) bv[set][q][u] = (rp + (size_t)(4 * u) * lda)[off[q]];
    }
  };
  auto mult = [&](int set, int k) {
    if constexpr (PANEL) {  // the A operand of the whole row waits in LDS (aoff: this lane's element of a 4-row slab there)
#pragma unroll
      for (int u = 0; u < 4; ++u) av[0][u] = panel[(16 * k + 4 * u) * 16 + aoff];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double a = av[PANEL ? 0 : set][u];
#pragma unroll
      for (int q = 0; q < NA; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv[set][q][u], acc[q], 0, 0, 0);
      if constexpr (WITH_P) {
        const double v = okc ? bv[set][0][u] : 0.0;
        accp = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, accp, 0, 0, 0);
      }
    }
  };
#pragma unroll
  for (int q = 0; q < NA; ++q) acc[q] = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int st = 0; st < NS; ++st) fetch(st, st);
  // whole rounds without a branch (a conditional step would make the number of loads in flight unknown to the compiler's wait-count
  // bookkeeping, which then waits for all of them: one memory latency per k-step), then the last I % NS steps
  int k = 0;
  for (; k + NS <= I; k += NS) {
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      mult(st, k + st);
      fetch(st, k + st + NS);
    }
  }
#pragma unroll
  for (int st = 0; st < NS - 1; ++st)
    if (k + st < I) mult(st, k + st);  // (uniform)
}

// the same sum for a wave that has no tile in the row (the last five block rows): accp = sum_{k < I} U_k(I+1)^T U_k(I+1), own loads
__device__ __forceinline__ void chol_left_psum(gcdp_t A, int lda, int I, unsigned offn, bool okc, v4d& accp) {
  constexpr int NS = 6;
  const int kmax = max(I - 1, 0);
  double pv[NS][4];
  auto fetch = [&](int set, int k) {
    gcdp_t rp = A + (size_t)(16 * min(k, kmax)) * lda;
#pragma unroll
    for (int u = 0; u < 4; ++u) pv[set][u] = (rp + (size_t)(4 * u) * lda)[offn];
  };
  auto mult = [&](int set) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double v = okc ? pv[set][u] : 0.0;
      accp = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, accp, 0, 0, 0);
    }
  };
#pragma unroll
  for (int st = 0; st < NS; ++st) fetch(st, st);
  int k = 0;
  for (; k + NS <= I; k += NS) {
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      mult(st);
      fetch(st, k + st + NS);
    }
  }
#pragma unroll
  for (int st = 0; st < NS - 1; ++st)
    if (k + st < I) mult(st);  // (uniform)
}

// tile t (J = I + t) of slot s of tile wave hw: the first six tiles go round once, then wave hw = 0 -- which carries the next diagonal
// block's sum with its first tile -- sits out one turn:  hw 0: 1, 12, 18, ...;  hw 1..5: 1 + hw, 6 + hw, 12 + hw, ...
__device__ __forceinline__ int chol_left_tile_of(int hw, int s) { return s == 0 ? 1 + hw : (hw == 0 ? 6 + 6 * s : hw + 6 * s); }

// The role of the six tile waves 1, 2, 3, 5, 6, 7 (helper index hw = 0..5; wave 4 shares its SIMD with wave 0, whose double-precision
// FMAs wait behind any MFMA issued there -- fp64 MFMA and VALU share the DP units -- so it only keeps the barriers company):
// slots s in groups of CL_GS, each group's k loop instantiated for the number of tiles it really has.
template <int CL_MAXS, int CL_GS, bool PANEL>
__device__ __noinline__ void chol_left_tile_role(int N_, gdp_t A_, int lda_, int wv_, const double* ui, double (*dgp)[256], double* nt, double* panels) {
  const int N = uniform_int(N_), lda = uniform_int(lda_), wv = uniform_int(wv_);
  const gdp_t A = uniform_ptr(A_);
  static_assert(CL_MAXS % CL_GS == 0 && CL_GS <= 4, "slots come in whole groups");
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, li = lane & 15;
  const int NBK = (N + 15) >> 4;
  const int hw = wv < 4 ? wv - 1 : wv - 2;
  const unsigned lrow = (unsigned)(kq * lda);
  const int pstride = 16 * (NBK << 4);  // doubles per LDS panel
  v4d T[CL_MAXS];
  // the original entries A_IJ of this wave's tiles of block row I: loaded a row ahead (behind the previous row's stores, in front of
  // its second barrier), so that their latency is not part of the row
  auto load_tiles = [&](int I) {
    const int kb = I << 4, ntile = NBK - I;
#pragma unroll
    for (int s = 0; s < CL_MAXS; ++s) {
      const int t = chol_left_tile_of(hw, s);
      if (t < ntile) {  // (uniform)
        const unsigned o = lrow + (unsigned)min(kb + 16 * t + li, N - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) T[s][r] = (A + (size_t)(kb + 4 * r) * lda)[o];
      }
    }
  };
  if (wv != 4) load_tiles(0);
  for (int I = 0; I < NBK; ++I) {
    int kb = I << 4;
    asm volatile("" : "+s"(kb));  // (keeps the per-slot addresses from becoming spilled 64-bit induction variables of the row loop)
    const int ntile = NBK - I;
    if (wv != 4) {
      // the mirror tiles below the diagonal: zeros, as torch.cholesky(upper=True) returns (nothing reads them; stored here, the stores
      // drain behind the k loops instead of in front of the row's second barrier)
#pragma unroll
      for (int s = 0; s < CL_MAXS; ++s) {
        const int t = chol_left_tile_of(hw, s);
        if (t < ntile) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int mrow = kb + 16 * t + kq + 4 * r;
            if (mrow < N) A[(size_t)mrow * lda + kb + li] = 0.0;
          }
        }
      }
      const unsigned aoff = PANEL ? (unsigned)(kq * 16 + li) : lrow + (unsigned)min(kb + li, N - 1);
      const double* panel = panels + (I & 1) * pstride;
      // P_(I+1): with six or more tiles in the row every wave has one, and the sum rides in wave hw = 0's first k loop on the operand
      // that is there anyway; with fewer, the first wave WITHOUT a tile takes it as a job of its own
      const bool okc = kb + 16 + li < N;
      const int p_owner = ntile - 1 >= 6 ? 0 : ntile - 1;  // (the last row, ntile = 1, has no next block: owner 0 finds no tile)
      double an[4] = {0.0, 0.0, 0.0, 0.0};
      if (hw == p_owner && ntile > 1) {
        const int cn = kb + 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = kq + 4 * r, rown = kb + 16 + row;
          an[r] = (cn < N && rown < N) ? A[(size_t)rown * lda + cn] : (row == li ? 1.0 : 0.0);  // identity beyond N
        }
      }
      if (hw == p_owner && p_owner > 0) {
        v4d accp = {0.0, 0.0, 0.0, 0.0};
        chol_left_psum(A, lda, I, lrow + (unsigned)(okc ? kb + 16 + li : 0), okc, accp);
#pragma unroll
        for (int r = 0; r < 4; ++r) dgp[(I + 1) & 1][(kq + 4 * r) * 16 + li] = an[r] - accp[r];
      }
#pragma unroll
      for (int g0 = 0; g0 < CL_MAXS; g0 += CL_GS) {
        int na = 0;  // (uniform) tiles of this group
#pragma unroll
        for (int q = 0; q < CL_GS; ++q) na += chol_left_tile_of(hw, g0 + q) < ntile ? 1 : 0;
        if (na > 0) {
          unsigned off[CL_GS];
#pragma unroll
          for (int q = 0; q < CL_GS; ++q) {
            const int t = chol_left_tile_of(hw, g0 + q);
            off[q] = lrow + (unsigned)min(kb + 16 * (t < ntile ? t : 0) + li, N - 1);
          }
          v4d accp = {0.0, 0.0, 0.0, 0.0};
          const bool with_p = g0 == 0 && hw == 0 && p_owner == 0;  // (this group holds tile 1)
          auto run = [&](auto na_c) {
            constexpr int NA = decltype(na_c)::value;
            unsigned o[NA];
            v4d acc[NA];
#pragma unroll
            for (int q = 0; q < NA; ++q) o[q] = off[q];
            if (with_p)
              chol_left_sums<NA, true, PANEL>(A, lda, I, aoff, panel, o, acc, accp, okc);
            else
              chol_left_sums<NA, false, PANEL>(A, lda, I, aoff, panel, o, acc, accp, okc);
#pragma unroll
            for (int q = 0; q < NA; ++q) T[g0 + q] -= acc[q];
          };
          if (na == 1) run(std::integral_constant<int, 1>());
          if constexpr (CL_GS >= 2) {
            if (na == 2) run(std::integral_constant<int, 2>());
          }
          if constexpr (CL_GS >= 3) {
            if (na == 3) run(std::integral_constant<int, 3>());
          }
          if constexpr (CL_GS >= 4) {
            if (na == 4) run(std::integral_constant<int, 4>());
          }
          if (with_p) {  // P_(I+1)
#pragma unroll
            for (int r = 0; r < 4; ++r) dgp[(I + 1) & 1][(kq + 4 * r) * 16 + li] = an[r] - accp[r];
          }
        }
      }
    }
    if constexpr (PANEL) {
      // the column panel U[0 : 16 I][block column I + 1], the A operand of every tile of the NEXT row, into the other LDS buffer (these rows
      // are final; the last sixteen, U_I(I+1), follow from wave 1 below): one pass by the seven waves here while the chain finishes
      if (I + 1 < NBK) {
        double* pn = panels + ((I + 1) & 1) * pstride;
        const int cnt = kb * 16, c0 = kb + 16;
        for (int base = (wv - 1) * 64 + lane; base < cnt; base += 8 * 448) {
          double v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int idx = base + e * 448, r = idx >> 4, c = c0 + (idx & 15);
            v[e] = (idx < cnt && c < N) ? A[(size_t)r * lda + c] : 0.0;
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int idx = base + e * 448;
            if (idx < cnt) pn[idx] = v[e];
          }
        }
      }
    }
    __syncthreads();
    if (wv != 4) {
      double wa[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) wa[u] = ui[(4 * u + kq) * 16 + li];
#pragma unroll
      for (int s = 0; s < CL_MAXS; ++s) {
        const int t = chol_left_tile_of(hw, s);
        if (t < ntile) {  // (uniform)
          const int col = kb + 16 * t + li;
          v4d o = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int u = 0; u < 4; ++u) o = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[u], T[s][u], o, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = kb + kq + 4 * r;
            if (col < N) A[(size_t)row * lda + col] = o[r];
            if (t == 1) {
              nt[(kq + 4 * r) * 16 + li] = col < N ? o[r] : 0.0;
              if constexpr (PANEL) (panels + ((I + 1) & 1) * pstride)[(kb + kq + 4 * r) * 16 + li] = col < N ? o[r] : 0.0;
            }
          }
        }
      }
      if (I + 1 < NBK) load_tiles(I + 1);
    }
    __syncthreads();
  }
}

#define CL_LDS_FIXED 1280  // doubles
template <int CL_MAXS, int CL_GS, bool PANEL>
__global__ __launch_bounds__(CM_NT) void chol_left_mfma_kernel(int N, double* __restrict__ A, int lda, double* __restrict__ logdet,
                                                               uint32_t* __restrict__ status, size_t a_stride, size_t ld_stride) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* ui = smem;                                   // [256]    W_I (row m, column r at ui[m * 16 + r])
  double* dg = smem + 256;                             // [256]    T_II on its way from accumulator layout to one column per lane
  double(*dgp)[256] = (double(*)[256])(smem + 512);    // [2][256] P_I (row I & 1), accumulator layout unfolded: [row][column]
  double* nt = smem + 1024;                            // [256]    U_(I-1)I
  double* panels = smem + CL_LDS_FIXED;                // PANEL: two column panels [16 NBK][16] (this row's and the next one's)
  A += (size_t)blockIdx.x * a_stride;
  logdet += (size_t)blockIdx.x * ld_stride;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // two roles with the same two barriers per block row
  if (wv == 0)
    chol_left_diag_role(N, (gdp_t)A, lda, logdet, status, ui, dg, dgp, nt);
  else
    chol_left_tile_role<CL_MAXS, CL_GS, PANEL>(N, (gdp_t)A, lda, wv, ui, dgp, nt, panels);
}

int mcp::launch_chol_left(int N, double* A, int lda, double* logdet, uint32_t* status, int batch, size_t a_stride, size_t ld_stride, hipStream_t st) {
  const size_t fixed_lds = sizeof(double) * CL_LDS_FIXED, panel_lds = fixed_lds + sizeof(double) * 2 * 16 * (size_t)(((N + 15) >> 4) << 4);
  if (N <= 400) {  // 1 + 6 * 4 tiles in the first block row
    MCP_ENSURE_MAX_LDS((chol_left_mfma_kernel<4, 4, true>));
    hipLaunchKernelGGL((chol_left_mfma_kernel<4, 4, true>), dim3(batch), dim3(CM_NT), panel_lds, st, N, A, lda, logdet, status, a_stride, ld_stride);
  } else if (N <= 576) {  // (two panels of 16 x 576 doubles: 144 KiB, + 10 KiB, of the 160)
    MCP_ENSURE_MAX_LDS((chol_left_mfma_kernel<8, 2, true>));
    hipLaunchKernelGGL((chol_left_mfma_kernel<8, 2, true>), dim3(batch), dim3(CM_NT), panel_lds, st, N, A, lda, logdet, status, a_stride, ld_stride);
  } else if (N <= 784) {  // 1 + 6 * 8
    hipLaunchKernelGGL((chol_left_mfma_kernel<8, 2, false>), dim3(batch), dim3(CM_NT), fixed_lds, st, N, A, lda, logdet, status, a_stride, ld_stride);
  } else {  // 1 + 6 * 12 >= 72 (N <= 1152)
    hipLaunchKernelGGL((chol_left_mfma_kernel<12, 2, false>), dim3(batch), dim3(CM_NT), fixed_lds, st, N, A, lda, logdet, status, a_stride, ld_stride);
  }
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

// Round 4: U^-1 by BLOCK COLUMNS.  Column J of X = U^-1 depends on U alone:  X[J][J] = W_J = U_JJ^-1,  X[I][J] = - W_I sum_{K = I+1..J} U[I][K]
// X[K][J]  for I = J-1 .. 0 -- a serial chain over I inside a column, no dependence between columns.  So: one launch inverts the
// diagonal blocks (one wave each), a second one gives every block column its own workgroup, which keeps the column's finished blocks in
// LDS (the B operands of its later products): NBK x G workgroups in flight instead of one (a one-workgroup block-diagonal sweep: NBK
// stages of at most NBK / 8 tile products per wave behind a barrier each -- 0.52 ms at N = 400).
__global__ __launch_bounds__(64) void tri_diag_inverse_kernel(int N, const double* __restrict__ U, int ldu, double* __restrict__ Ui, int ldi,
                                                              size_t u_stride, size_t ui_stride) {
  U += (size_t)blockIdx.y * u_stride;
  Ui += (size_t)blockIdx.y * ui_stride;
  const int lane = threadIdx.x, c = lane & 15, kb = (int)blockIdx.x << 4, nb = min(16, N - kb);
  double x[16], inv_d[16], w[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) x[r] = (r <= c && c < nb) ? U[(size_t)(kb + r) * ldu + kb + c] : (r == c ? 1.0 : 0.0);
#pragma unroll
  for (int r = 0; r < 16; ++r) inv_d[r] = 1.0 / lane_get(x[r], r);
  tri16_inverse(x, inv_d, c, w);
  if (lane < 16 && c < nb) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (r < nb) Ui[(size_t)(kb + r) * ldi + kb + c] = r <= c ? w[r] : 0.0;
  }
}
// One block column per workgroup of FOUR waves.  Step I of the chain is a sum of J - I block products followed by one closing
// product: the products of a step are dealt to the four waves (item m = J - K of the step to wave m mod 4, oldest blocks first, so that the
// one product that needs the block finished in the previous step, K = I + 1, is the last of its wave), partial sums meet in LDS, wave 0
// adds them and closes the step while the others are already in the next one.  Per step two LDS-only barriers (s_waitcnt lgkmcnt(0) +
// s_barrier: the prefetched global operands stay in flight across them; __syncthreads would drain them twice per step).
// The chain of the last column, 171 products at N = 300, becomes 18 steps of ceil(n / 4) products + close.
#define TC4_PF 4
__global__ __launch_bounds__(256) void tri_inverse_cols4_kernel(int N, const double* __restrict__ U, int ldu, double* __restrict__ Ui, int ldi,
                                                                size_t u_stride, size_t ui_stride) {
  extern __shared__ __attribute__((aligned(16))) double xs[];  // [J + 1][256] finished blocks | [3][256] partial sums of waves 1..3
  U += (size_t)blockIdx.y * u_stride;
  Ui += (size_t)blockIdx.y * ui_stride;
  const int NBK = (N + 15) >> 4;
  const int J = NBK - 1 - (int)blockIdx.x;  // (the longest columns start first)
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, li = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = 16 * J + li;
  double* part = xs + (J + 1) * 256;
  if (w == 0) {  // X[J][J] = W_J (written by tri_diag_inverse_kernel)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * J + kq + 4 * r;
      xs[J * 256 + (kq + 4 * r) * 16 + li] = (row < N && col < N) ? Ui[(size_t)row * ldi + col] : 0.0;
    }
  }
  const gcdp_t Ug = (gcdp_t)U, Wg = (gcdp_t)Ui;
  // this wave's stream of items: per step I = J-1 .. 0 the products m = w, w + 4, ... < n = J - I (block K = J - m), then, wave 0 only, the
  // closing item (m = -1 stands for it).  Steps in which the wave has no product (n <= w) have no item.
  int If = J - 1, mf = w;  // fetch position
  auto skip_empty = [&](int& I, int& m) {
    while (I >= 0 && m >= 0 && m >= J - I) {  // no (more) product of mine in step I
      if (w == 0) {
        m = -1;  // the closing item comes next
        return;
      }
      --I;
      m = w;
    }
  };
  skip_empty(If, mf);
  double buf[TC4_PF][4];
  auto fetch = [&](double (&dst)[4]) {
    const bool live = If >= 0;  // (past the end of the stream: block (0, 0) of U, never used)
    const int I = live ? If : 0;
    const bool closing = live && mf < 0;
    const gcdp_t base = closing ? Wg : Ug;  // (uniform)
    const int ld = closing ? ldi : ldu, kc = live ? (closing ? I : J - mf) : 0;
    const unsigned rowoff = (unsigned)((16 * I + li) * ld);  // A[i = li][k]: block row 16 I + i (< N: I < J)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ac = 16 * kc + 4 * u + kq;
      const double v = base[rowoff + (unsigned)min(ac, N - 1)];
      dst[u] = ac < N ? v : 0.0;
    }
    if (live) {  // (scalar bookkeeping)
      if (mf < 0) {
        --If;
        mf = w;
      } else {
        mf += 4;
      }
      skip_empty(If, mf);
    }
  };
#pragma unroll
  for (int q = 0; q < TC4_PF; ++q) fetch(buf[q]);
  lds_barrier();  // X[J][J] is in LDS
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  int Ip = J - 1, mp = w;   // process position
  bool newest_seen = false;  // this step's barrier B passed
  // the end of a wave's products of step I: barrier B if it has not passed it yet, partial sum to LDS (waves 1..3), barrier A
  auto end_products = [&]() {
    if (!newest_seen) lds_barrier();  // B: the block of the previous step is in LDS (this wave did not need it)
    if (w > 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) part[(w - 1) * 256 + (kq + 4 * r) * 16 + li] = acc[r];
      acc = (v4d){0.0, 0.0, 0.0, 0.0};
    }
    lds_barrier();  // A: the partial sums of the step are in LDS
    newest_seen = false;
  };
  // steps without a product of this wave: their two barriers
  auto idle_steps = [&]() {
    while (Ip >= 0 && mp >= 0 && mp >= J - Ip) {
      if (w == 0) {
        end_products();
        mp = -1;
        return;
      }
      end_products();
      --Ip;
      mp = w;
    }
  };
  idle_steps();
  while (Ip >= 0) {
#pragma unroll
    for (int q = 0; q < TC4_PF; ++q) {
      if (Ip >= 0) {  // (wave-uniform; MFMAs, LDS and barriers only)
        if (mp >= 0) {
          const int n = J - Ip, K = J - mp;
          if (mp == n - 1) {  // the product on the block of the previous step
            lds_barrier();    // B
            newest_seen = true;
          }
          double bv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) bv[u] = xs[K * 256 + (4 * u + kq) * 16 + li];
#pragma unroll
          for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(buf[q][u], bv[u], acc, 0, 0, 0);
          mp += 4;
          if (mp >= n) {
            end_products();
            if (w == 0) {
              mp = -1;
            } else {
              --Ip;
              mp = w;
              idle_steps();
            }
          }
        } else {  // wave 0: S = sum of the partial sums;  X[I][J] = - W_I S  (register u of S is the B operand of step u)
          const int n = J - Ip;
#pragma unroll
          for (int pw = 1; pw < 4; ++pw) {
            if (pw < n) {  // (waves beyond the step's products wrote zeros: skip the read)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[r] += part[(pw - 1) * 256 + (kq + 4 * r) * 16 + li];
            }
          }
          v4d out = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int u = 0; u < 4; ++u) out = __builtin_amdgcn_mfma_f64_16x16x4f64(-buf[q][u], acc[u], out, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r) xs[Ip * 256 + (kq + 4 * r) * 16 + li] = col < N ? out[r] : 0.0;
          acc = (v4d){0.0, 0.0, 0.0, 0.0};
          --Ip;
          mp = 0;
          idle_steps();
        }
      }
      fetch(buf[q]);  // this register set: the item TC4_PF further on
    }
  }
  lds_barrier();  // the last block of the column is in LDS
  // the column, from LDS: blocks 0 .. J-1 (block J is already there), zeros below
  for (int idx = tid; idx < 16 * J * 16; idx += 256) {
    const int row = idx >> 4, c = 16 * J + (idx & 15);
    if (c < N) Ui[(size_t)row * ldi + c] = xs[idx];
  }
  for (int row = 16 * (J + 1) + (tid >> 4); row < N; row += 16)
    if (col < N) Ui[(size_t)row * ldi + col] = 0.0;
}

// Kinv = Uinv Uinv^T by 16x16 tiles on the matrix cores, one wave per tile (I <= J) of the upper triangle, mirrored into the lower:
//   Kinv[I][J] = sum_{K >= J} Uinv[I][K] Uinv[J][K]^T      (both operands read rows of Uinv: A[i][k] = Ui[16 I + i][16 K + k], B[k][j] = Ui[16 J + j][16 K + k])
__global__ __launch_bounds__(256) void kinv_tiles_kernel(int N, const double* __restrict__ Ui, int ldi, double* __restrict__ Kinv, int ldk,
                                                         size_t ui_stride, size_t k_stride) {
  Ui += (size_t)blockIdx.y * ui_stride;
  Kinv += (size_t)blockIdx.y * k_stride;
  const int NBK = (N + 15) >> 4, nt = NBK * (NBK + 1) / 2;
  const int lane = threadIdx.x & 63, kq = lane >> 4, li = lane & 15;
  const int t = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (t >= nt) return;
  int I = 0, rem = t;
  while (rem >= NBK - I) {
    rem -= NBK - I;
    ++I;
  }
  const int J = I + rem;
  const bool ra = 16 * I + li < N, rb = 16 * J + li < N;
  const double* pa = Ui + (size_t)(ra ? 16 * I + li : 0) * ldi + kq;
  const double* pb = Ui + (size_t)(rb ? 16 * J + li : 0) * ldi + kq;
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  for (int K = J; K < NBK; ++K) {
    double av[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = 16 * K + 4 * u + kq;
      av[u] = (ra && c < N) ? pa[16 * K + 4 * u] : 0.0;
      bv[u] = (rb && c < N) ? pb[16 * K + 4 * u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * I + kq + 4 * r, col = 16 * J + li;
    if (row < N && col < N) {
      Kinv[(size_t)row * ldk + col] = acc[r];
      if (I != J) Kinv[(size_t)col * ldk + row] = acc[r];
    }
  }
}

// Kinv[i][j] = sum_{m >= max(i,j)} Ui[i][m] Ui[j][m]
__global__ void kinv_from_uinv_kernel(int N, const double* __restrict__ Ui, int ldi, double* __restrict__ Kinv, int ldk, size_t ui_stride,
                                      size_t k_stride) {
  Ui += (size_t)blockIdx.z * ui_stride;
  Kinv += (size_t)blockIdx.z * k_stride;
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int i = blockIdx.y;
  if (i >= N || j >= N) return;
  int m0 = max(i, j);
  const double* a = Ui + (size_t)i * ldi;
  const double* b = Ui + (size_t)j * ldi;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int m = m0;
  for (; m + 3 < N; m += 4) {
    s0 = fma(a[m], b[m], s0);
    s1 = fma(a[m + 1], b[m + 1], s1);
    s2 = fma(a[m + 2], b[m + 2], s2);
    s3 = fma(a[m + 3], b[m + 3], s3);
  }
  for (; m < N; ++m) s0 = fma(a[m], b[m], s0);
  Kinv[(size_t)i * ldk + j] = (s0 + s1) + (s2 + s3);
}

// Ui = U^-1 of `batch` upper-triangular matrices of n rows (strides in doubles): the 16x16 diagonal blocks, then the block columns (one
// workgroup each, the column's finished blocks in LDS: [NBK + 3][256] doubles)
static int launch_block_inverse(int n, const double* U, int ldu, double* Ui, int ldi, int batch, size_t u_stride, size_t ui_stride, hipStream_t st) {
  const int NBK = (n + 15) >> 4;
  hipLaunchKernelGGL(tri_diag_inverse_kernel, dim3(NBK, batch), dim3(64), 0, st, n, U, ldu, Ui, ldi, u_stride, ui_stride);
  MCP_LAUNCH_CHECK();
  MCP_ENSURE_MAX_LDS(tri_inverse_cols4_kernel);
  hipLaunchKernelGGL(tri_inverse_cols4_kernel, dim3(NBK, batch), dim3(256), sizeof(double) * 256 * (size_t)(NBK + 3), st, n, U, ldu, Ui, ldi,
                     u_stride, ui_stride);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

// Kinv = Ui Ui^T of `batch` matrices: one wave per 16x16 tile of the upper triangle, four to a workgroup
static int launch_kinv_tiles(int N, const double* Ui, int ldi, double* Kinv, int ldk, int batch, size_t ui_stride, size_t k_stride, hipStream_t st) {
  const int NBK = (N + 15) >> 4, nt = NBK * (NBK + 1) / 2;
  hipLaunchKernelGGL(kinv_tiles_kernel, dim3((nt + 3) / 4, batch), dim3(256), 0, st, N, Ui, ldi, Kinv, ldk, ui_stride, k_stride);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

// U^-1 and K^-1 = U^-1 U^-T of `batch` matrices (strides in doubles): diagonal blocks, block columns, tiles -- three launches
int mcp::launch_inverse_mfma(int N, const double* U, int ldu, double* Ui, int ldi, double* Kinv, int ldk, int batch, size_t u_stride,
                             size_t ui_stride, size_t k_stride, hipStream_t st) {
  const int rc = launch_block_inverse(N, U, ldu, Ui, ldi, batch, u_stride, ui_stride, st);
  return rc != MCP_OK ? rc : launch_kinv_tiles(N, Ui, ldi, Kinv, ldk, batch, ui_stride, k_stride, st);
}

// ---------------------------------------------------------------------------------------
// Factorisation across workgroups (round 5; N >= CHB_MIN): right-looking by panels of CHB_NB rows.  Per panel k
//   1. U_kk = chol(A_kk)                     the one-workgroup left-looking kernel above on the diagonal block
//   2. W = U_kk^-1                           tri_diag_inverse + tri_inverse_cols4 on that block (8 block columns)
//   3. U_kj = W^T A_kj   (j > k, in place)   chol_panel_solve_kernel:  one wave per 16 columns, the whole 128-row column slab in registers
//   4. A_ij -= U_ki^T U_kj  (k < i <= j)     chol_trailing_update_kernel: one wave per 32 x 32 tile, 64 x 64 per workgroup, upper tiles only
// Every product is  C[m][n] = sum_k P[k][m] Q[k][n]  on v_mfma_f64_16x16x4_f64 (A operand lane (kq, li) = P[k0 + kq][m0 + li], B likewise from Q,
// result register r = C[m0 + kq + 4 r][n0 + li]), operands straight from L2.  The one-workgroup kernel (chain-bound: 8.2 k cycles per 16 rows,
// one CU) took 3.1 ms at N = 1000 and stopped at 1152 rows; the panels' chain is 8 block rows each and the O(N^3) part runs on the whole chip.
// Scratch: mcp_chol_factor takes no workspace, but the strictly-lower triangle of A is output-zero by contract -- W_k lives in block (k, 0) of it
// ((1, 0) for k = 0), the panels' logdet terms in its last row; chol_finish_kernel sums those and zeroes the triangle.
// ---------------------------------------------------------------------------------------
#define CHB_NB 128
#define CHB_MIN 600
__global__ __launch_bounds__(256) void chol_panel_solve_kernel(int R, const double* __restrict__ W, int ldw, double* __restrict__ B, int ldb) {
  const int lane = threadIdx.x & 63, kq = lane >> 4, li = lane & 15;
  const int col = ((int)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + li;
  const bool ok = col < R;
  double b[CHB_NB / 4];
#pragma unroll
  for (int s = 0; s < CHB_NB / 4; ++s) b[s] = ok ? B[(size_t)(4 * s + kq) * ldb + col] : 0.0;
  v4d out[CHB_NB / 16];
#pragma unroll
  for (int mt = 0; mt < CHB_NB / 16; ++mt) {
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    // (W is upper triangular: rows k > 16 mt + 15 of its columns [16 mt, 16 mt + 16) are zero -- and were never written)
#pragma unroll
    for (int s = 0; s < 4 * (mt + 1); ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(W[(size_t)(4 * s + kq) * ldw + 16 * mt + li], b[s], acc, 0, 0, 0);
    out[mt] = acc;
  }
  if (ok) {
#pragma unroll
    for (int mt = 0; mt < CHB_NB / 16; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) B[(size_t)(16 * mt + kq + 4 * r) * ldb + col] = out[mt][r];
  }
}

__global__ __launch_bounds__(256) void chol_trailing_update_kernel(int R, const double* __restrict__ Up, int ldu, double* __restrict__ C, int ldc) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (ti > tj) return;  // (the upper tiles only)
  const int lane = threadIdx.x & 63, kq = lane >> 4, li = lane & 15, w = threadIdx.x >> 6;
  const int m0 = 64 * ti + 32 * (w >> 1), n0 = 64 * tj + 32 * (w & 1);
  if (m0 >= R || n0 >= R) return;
  const int ma = min(m0 + li, R - 1), mb = min(m0 + 16 + li, R - 1), na = min(n0 + li, R - 1), nb = min(n0 + 16 + li, R - 1);  // (clamped: such columns are not stored)
  v4d acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = v4d{0.0, 0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < CHB_NB / 4; s0 += 8) {  // 8 k-steps per batch: 32 loads in flight, then 32 MFMAs
    double a0[8], a1[8], b0[8], b1[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double* row = Up + (size_t)(4 * (s0 + u) + kq) * ldu;
      a0[u] = row[ma];
      a1[u] = row[mb];
      b0[u] = row[na];
      b1[u] = row[nb];
    }
    asm volatile("" : "+v"(a0[0]), "+v"(a0[1]), "+v"(a0[2]), "+v"(a0[3]), "+v"(a0[4]), "+v"(a0[5]), "+v"(a0[6]), "+v"(a0[7]), "+v"(a1[0]), "+v"(a1[1]),
                 "+v"(a1[2]), "+v"(a1[3]), "+v"(a1[4]), "+v"(a1[5]), "+v"(a1[6]), "+v"(a1[7]));
    asm volatile("" : "+v"(b0[0]), "+v"(b0[1]), "+v"(b0[2]), "+v"(b0[3]), "+v"(b0[4]), "+v"(b0[5]), "+v"(b0[6]), "+v"(b0[7]), "+v"(b1[0]), "+v"(b1[1]),
                 "+v"(b1[2]), "+v"(b1[3]), "+v"(b1[4]), "+v"(b1[5]), "+v"(b1[6]), "+v"(b1[7]));
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b0[u], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b1[u], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b0[u], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b1[u], acc[1][1], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + 16 * i + kq + 4 * r, col = n0 + 16 * j + li;
        if (row < R && col < R) C[(size_t)row * ldc + col] -= acc[i][j][r];
      }
}

// logdet = sum of the panels' terms (parked in the last row of the lower triangle), then the strictly-lower triangle back to zero
__global__ void chol_finish_kernel(int N, double* __restrict__ A, int lda, int np, double* __restrict__ logdet) {
  __shared__ double tot;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < np; ++k) s += A[(size_t)(N - 1) * lda + k];
    tot = s;
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) *logdet = tot;
  __syncthreads();  // (every block has read the terms of the last row before any block zeroes it: the last row belongs to the LAST block)
  for (int row = blockIdx.x; row < N; row += gridDim.x) {
    if (row == N - 1 && gridDim.x > 1) continue;  // (left to the tail kernel)
    for (int c = threadIdx.x; c < row; c += blockDim.x) A[(size_t)row * lda + c] = 0.0;
  }
}
__global__ void chol_finish_tail_kernel(int N, double* __restrict__ A, int lda) {
  for (int c = threadIdx.x; c < N - 1; c += blockDim.x) A[(size_t)(N - 1) * lda + c] = 0.0;
}

static int launch_chol_blocked(int N, double* A, int lda, double* logdet, uint32_t* status, hipStream_t st) {
  const int NB = CHB_NB, np = (N + NB - 1) / NB;
  if (N < 2 * NB + 1 || np > NB) return MCP_ERR_LIMIT;
  for (int k = 0; k < np; ++k) {
    const int k0 = k * NB, nb = N - k0 < NB ? N - k0 : NB, R = N - k0 - nb;
    double* Akk = A + (size_t)k0 * lda + k0;
    double* ldk = A + (size_t)(N - 1) * lda + k;
    if (nb > 16) {
      const int rc = launch_chol_left(nb, Akk, lda, ldk, status, 1, 0, 0, st);
      if (rc != MCP_OK) return rc;
    } else {
      const size_t lds = sizeof(double) * ((size_t)CH_NB * (CH_NB + 1) + (size_t)CH_NB * nb);
      hipLaunchKernelGGL(chol_factor_kernel, dim3(1), dim3(CH_NT), lds, st, nb, Akk, lda, ldk, status);
      MCP_LAUNCH_CHECK();
    }
    if (R > 0) {  // (nb == NB here)
      double* W = A + (size_t)(k == 0 ? NB : k0) * lda;
      const int rc = launch_block_inverse(NB, Akk, lda, W, lda, 1, 0, 0, st);
      if (rc != MCP_OK) return rc;
      double* Akj = Akk + nb;
      hipLaunchKernelGGL(chol_panel_solve_kernel, dim3((R + 63) / 64), dim3(256), 0, st, R, W, lda, Akj, lda);
      MCP_LAUNCH_CHECK();
      const int T = (R + 63) / 64;
      hipLaunchKernelGGL(chol_trailing_update_kernel, dim3(T, T), dim3(256), 0, st, R, Akj, lda, Akk + (size_t)nb * lda + nb, lda);
      MCP_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(chol_finish_kernel, dim3(256), dim3(256), 0, st, N, A, lda, np, logdet);
  MCP_LAUNCH_CHECK();
  hipLaunchKernelGGL(chol_finish_tail_kernel, dim3(1), dim3(256), 0, st, N, A, lda);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

// ---------------------------------------------------------------------------------------
// U^-1 and K^-1 beyond the one-launch forms' 1152 rows (round 5): Y = U^-T by block forward substitution, every product in the transposed-
// left form the MFMA operands load coalesced from row-major storage,  C = +- P^T Q:
//   W_I = U_II^-1                                     all diagonal blocks at once (tri_diag_inverse + tri_inverse_cols4, batched), into Uinv
//   Y[I][I] = W_I^T;  T = U[0:I0, I]^T Y[0:I0, 0:I0]  (K = I0; Y lower triangular: rows above a column block are skipped)
//   Y[I][0:I0] = - W_I^T T                            (K = 128)
// Y is built in the Kinv buffer, T in the lower triangle of Uinv (zero at the end by contract); then Uinv = Y^T by tiles and
// Kinv = Uinv Uinv^T (kinv_tiles_kernel) over the whole matrix.  Replaces the round-1 column kernels there: N = 2048 94 -> 1.5 ms, 4096 659 -> 6.6 ms.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tn_gemm_kernel(int M, int Nn, int K, const double* __restrict__ P, int ldp, const double* __restrict__ Q,
                                                      int ldq, double* __restrict__ C, int ldc, double sign, int q_lower) {
  const int lane = threadIdx.x & 63, kq = lane >> 4, li = lane & 15, w = threadIdx.x >> 6;
  const int m0 = 64 * (int)blockIdx.y + 32 * (w >> 1), n0 = 64 * (int)blockIdx.x + 32 * (w & 1);
  if (m0 >= M || n0 >= Nn) return;
  const int ma = min(m0 + li, M - 1), mb = min(m0 + 16 + li, M - 1), na = min(n0 + li, Nn - 1), nb = min(n0 + 16 + li, Nn - 1);
  v4d acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = v4d{0.0, 0.0, 0.0, 0.0};
  for (int k0 = q_lower ? (n0 & ~31) : 0; k0 < K; k0 += 32) {  // (Q lower triangular: its rows above column n0 are zero)
    double a0[8], a1[8], b0[8], b1[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int kr = min(k0 + 4 * u + kq, K - 1);
      const double* pr = P + (size_t)kr * ldp;
      const double* qr = Q + (size_t)kr * ldq;
      a0[u] = pr[ma];
      a1[u] = pr[mb];
      b0[u] = qr[na];
      b1[u] = qr[nb];
    }
    asm volatile("" : "+v"(a0[0]), "+v"(a0[1]), "+v"(a0[2]), "+v"(a0[3]), "+v"(a0[4]), "+v"(a0[5]), "+v"(a0[6]), "+v"(a0[7]), "+v"(a1[0]), "+v"(a1[1]),
                 "+v"(a1[2]), "+v"(a1[3]), "+v"(a1[4]), "+v"(a1[5]), "+v"(a1[6]), "+v"(a1[7]));
    asm volatile("" : "+v"(b0[0]), "+v"(b0[1]), "+v"(b0[2]), "+v"(b0[3]), "+v"(b0[4]), "+v"(b0[5]), "+v"(b0[6]), "+v"(b0[7]), "+v"(b1[0]), "+v"(b1[1]),
                 "+v"(b1[2]), "+v"(b1[3]), "+v"(b1[4]), "+v"(b1[5]), "+v"(b1[6]), "+v"(b1[7]));
    if (k0 + 32 > K) {  // (the last, partial batch: the clamped rows count once)
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + 4 * u + kq >= K) a0[u] = a1[u] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b0[u], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b1[u], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b0[u], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b1[u], acc[1][1], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + 16 * i + kq + 4 * r, col = n0 + 16 * j + li;
        if (row < M && col < Nn) C[(size_t)row * ldc + col] = sign * acc[i][j][r];
      }
}
// Y[I][I] = W_I^T for every diagonal block (W_I: the diagonal blocks of Ui)
__global__ void diag_blocks_transpose_kernel(int N, const double* __restrict__ Ui, int ldi, double* __restrict__ Y, int ldy) {
  const int I0 = (int)blockIdx.x * CHB_NB, nb = min(CHB_NB, N - I0);
  for (int e = threadIdx.x; e < nb * nb; e += blockDim.x) {
    const int r = e / nb, c = e - r * nb;
    Y[(size_t)(I0 + r) * ldy + I0 + c] = Ui[(size_t)(I0 + c) * ldi + I0 + r];
  }
}
// Ui = Y^T outside the diagonal blocks (32 x 32 tiles through LDS), the strictly-lower blocks of Ui back to zero
__global__ __launch_bounds__(256) void uinv_from_y_kernel(int N, const double* __restrict__ Y, int ldy, double* __restrict__ Ui, int ldi) {
  __shared__ double tile[32][33];
  const int br = blockIdx.y, bc = blockIdx.x;  // tile (br, bc) of Y, br >= bc
  if (br < bc) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const bool same_block = (32 * br) / CHB_NB == (32 * bc) / CHB_NB;  // inside a diagonal block of 128: Ui holds W_I already
  if (same_block) return;
  for (int r = ty; r < 32; r += 8) {
    const int row = 32 * br + r, col = 32 * bc + tx;
    tile[r][tx] = (row < N && col < N) ? Y[(size_t)row * ldy + col] : 0.0;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int row = 32 * bc + r, col = 32 * br + tx;  // Ui[col of Y][row of Y]
    if (row < N && col < N) Ui[(size_t)row * ldi + col] = tile[tx][r];
    const int lr = 32 * br + r, lc = 32 * bc + tx;    // the mirrored (strictly-lower) tile: the scratch of T -> zero
    if (lr < N && lc < N) Ui[(size_t)lr * ldi + lc] = 0.0;
  }
}

static int launch_inverse_blocked(int N, const double* U, int ldu, double* Ui, int ldi, double* Kinv, int ldk, hipStream_t st) {
  const int NB = CHB_NB, np = (N + NB - 1) / NB, nfull = N / NB, nlast = N - nfull * NB;
  const size_t step_u = (size_t)NB * ldu + NB, step_i = (size_t)NB * ldi + NB;  // from one diagonal block to the next
  if (nfull > 0) {  // W_I of the full blocks, batched over I
    const int rc = launch_block_inverse(NB, U, ldu, Ui, ldi, nfull, step_u, step_i, st);
    if (rc != MCP_OK) return rc;
  }
  if (nlast > 0) {
    const int rc = launch_block_inverse(nlast, U + nfull * step_u, ldu, Ui + nfull * step_i, ldi, 1, 0, 0, st);
    if (rc != MCP_OK) return rc;
  }
  double* Y = Kinv;
  hipLaunchKernelGGL(diag_blocks_transpose_kernel, dim3(np), dim3(256), 0, st, N, Ui, ldi, Y, ldk);
  MCP_LAUNCH_CHECK();
  for (int I = 1; I < np; ++I) {
    const int I0 = I * NB, nb = N - I0 < NB ? N - I0 : NB;
    double* T = Ui + (size_t)I0 * ldi;  // rows I0.., columns 0..I0 of the lower triangle
    // T [nb x I0] = U[0:I0, I0:I0+nb]^T Y[0:I0, 0:I0]
    hipLaunchKernelGGL(tn_gemm_kernel, dim3((I0 + 63) / 64, (nb + 63) / 64), dim3(256), 0, st, nb, I0, I0, U + I0, ldu, Y, ldk, T, ldi, 1.0, 1);
    MCP_LAUNCH_CHECK();
    // Y[I][0:I0] = - W_I^T T
    hipLaunchKernelGGL(tn_gemm_kernel, dim3((I0 + 63) / 64, (nb + 63) / 64), dim3(256), 0, st, nb, I0, nb, Ui + (size_t)I0 * ldi + I0, ldi, T, ldi,
                       Y + (size_t)I0 * ldk, ldk, -1.0, 0);
    MCP_LAUNCH_CHECK();
  }
  const int nt32 = (N + 31) / 32;
  hipLaunchKernelGGL(uinv_from_y_kernel, dim3(nt32, nt32), dim3(256), 0, st, N, Y, ldk, Ui, ldi);
  MCP_LAUNCH_CHECK();
  return launch_kinv_tiles(N, Ui, ldi, Kinv, ldk, 1, 0, 0, st);
}

extern "C" int mcp_chol_factor(int N, double* A, int lda, double* logdet, uint32_t* status, void* stream) {
  if (!A || !logdet || !status || N <= 0 || lda < N) return MCP_ERR_ARG;
  if (N > 8192) return MCP_ERR_LIMIT;
  if (N >= CHB_MIN) return launch_chol_blocked(N, A, lda, logdet, status, (hipStream_t)stream);  // panels across the chip
  if (N > 16) return launch_chol_left(N, A, lda, logdet, status, 1, 0, 0, (hipStream_t)stream);
  size_t lds = sizeof(double) * ((size_t)CH_NB * (CH_NB + 1) + (size_t)CH_NB * N);
  MCP_ENSURE_MAX_LDS(chol_factor_kernel);
  hipLaunchKernelGGL(chol_factor_kernel, dim3(1), dim3(CH_NT), lds, (hipStream_t)stream, N, A, lda, logdet, status);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_chol_inverse(int N, const double* U, int ldu, double* Uinv, int ldi, double* Kinv, int ldk, void* stream) {
  if (!U || !Uinv || !Kinv || N <= 0 || ldu < N || ldi < N || ldk < N) return MCP_ERR_ARG;
  if (N > 16384) return MCP_ERR_LIMIT;
  if (N > 1152) return launch_inverse_blocked(N, U, ldu, Uinv, ldi, Kinv, ldk, (hipStream_t)stream);
  if (N > 16) return launch_inverse_mfma(N, U, ldu, Uinv, ldi, Kinv, ldk, 1, 0, 0, 0, (hipStream_t)stream);
  hipLaunchKernelGGL(tri_inverse_wave_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, N, U, ldu, Uinv, ldi);
  MCP_LAUNCH_CHECK();
  dim3 grid((N + 255) / 256, N);
  hipLaunchKernelGGL(kinv_from_uinv_kernel, grid, dim3(256), 0, (hipStream_t)stream, N, Uinv, ldi, Kinv, ldk, (size_t)0, (size_t)0);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

// out = A G A for a SYMMETRIC A (K^-1) and any G: S = G^T A, out = S^T A -- two products in the transposed-left form of tn_gemm_kernel
// (coalesced MFMA operands from row-major storage).  The chain rule through K^-1 of GP_prior.forward's autograd graph:
// d K^-1 = - K^-1 dK K^-1  (GP_prior.py:109-110 under autograd; _ForwardFunction.backward).
extern "C" int mcp_sym_sandwich(int N, const double* A, int lda, const double* G, int ldg, double* out, int ldo, double* scratch, void* stream) {
  if (!A || !G || !out || !scratch || N <= 0 || lda < N || ldg < N || ldo < N) return MCP_ERR_ARG;
  if (N > 16384) return MCP_ERR_LIMIT;
  if (out == A || out == G || scratch == A || scratch == G || scratch == out) return MCP_ERR_ARG;
  const dim3 grid((N + 63) / 64, (N + 63) / 64);
  hipLaunchKernelGGL(tn_gemm_kernel, grid, dim3(256), 0, (hipStream_t)stream, N, N, N, G, ldg, A, lda, scratch, N, 1.0, 0);
  MCP_LAUNCH_CHECK();
  hipLaunchKernelGGL(tn_gemm_kernel, grid, dim3(256), 0, (hipStream_t)stream, N, N, N, scratch, N, A, lda, out, ldo, 1.0, 0);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

