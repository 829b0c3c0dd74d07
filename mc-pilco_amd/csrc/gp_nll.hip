// Marginal-likelihood gradient and the batched training epoch for gfx950 (mcp_nll_workspace_bytes, mcp_nll_grad,
// mcp_nll_epoch_workspace_bytes, mcp_nll_epoch, and the epoch's plan query mcp_nll_epoch_plan).  Replaces the objective of
// GP_prior.fit_model and its autograd pass in the reference
// (gpr_lib/GP_prior/GP_prior.py:91-115,179-230; Gaussian_likelihood.py:15-24; Model_learning.train_gp_likelihood,
// model_learning/Model_learning.py:398-421): once per EPOCH of the hyper-parameter training.  The epoch factorises and inverts its G Gram
// matrices with gp_linalg.hip's one-workgroup launchers in their batched form (gp_launch.h).
#include <type_traits>

#include "../../include/mcpilco_hip_debug.h"
#include "gp_launch.h"
#include "mcp_device.h"

using namespace mcp;

// ---------------------------------------------------------------------------------------
// Marginal-likelihood gradient (GP_prior.fit_model's objective, Gaussian_likelihood.py:15-24):
//   L = 1/2 (r^T Kinv r + logdet K),   dL/dtheta = 1/2 sum_ij Wm_ij dK_ij/dtheta,   Wm = Kinv - alpha alpha^T.
// One workgroup per row i: (1) threads over j stage Wm_ij, Wm_ij*kse_ij and the two MPK_2 factor values in LDS,
// (2) one thread per hyper-parameter sums over j.  slab[i][p]; nll_colsum_kernel adds the rows in a fixed order.
// Parameter layout (NP = 4D+3): [0,D) log lengthscales | D log lambda | D+1 noise (1/2 tr Wm) | [D+2,2D+3) MPK_1 (D+1)
//                               | [2D+3,3D+3) MPK_2 factor 0 | [3D+3,4D+3) MPK_2 factor 1
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void nll_grad_row(const mcp_kernel& kn, int N, const double* __restrict__ X, const double* __restrict__ Kinv, int ldk,
                                             const double* __restrict__ alpha, double* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* wm = sm;          // [N] Wm_ij
  double* wk = sm + N;      // [N] Wm_ij * kse_ij
  double* fa = sm + 2 * N;  // [N] MPK_2 factor A_ij
  double* fb = sm + 3 * N;  // [N] MPK_2 factor B_ij
  const int i = blockIdx.x, tid = threadIdx.x, D = kn.D;
  const double* xi = X + (size_t)i * D;
  const double ai = alpha[i];
  for (int j = tid; j < N; j += 256) {
    const double* xj = X + (size_t)j * D;
    double dist = 0.0, A = 0.0, Bv = 0.0;
    for (int d = 0; d < D; ++d) {
      double r = (xi[d] - xj[d]) * kn.inv_ls[d];
      dist = fma(r, r, dist);
      if (kn.poly_deg >= 2) {
        double xx = xi[d] * xj[d];
        A = fma(kn.w20[d], xx, A);
        Bv = fma(kn.w21[d], xx, Bv);
      }
    }
    double w = Kinv[(size_t)i * ldk + j] - ai * alpha[j];
    wm[j] = w;
    wk[j] = w * kern_lambda(kn) * exp(-dist);
    fa[j] = A;
    fb[j] = Bv;
  }
  __syncthreads();
  // (2) the sums over j, one per hyper-parameter: the 256 threads as nseg segments of NPpad >= NP lanes, segment s taking j = s, s + nseg, ...
  // (one thread per parameter left 157 of the 256 idle at D = 24 and walked 400 dependent global loads each); partial sums meet in LDS
  // and are added in segment order
  const int NP = 4 * D + 3;
  double* red = sm + 4 * N;  // [256]
  int NPpad = 32;
  while (NPpad < NP) NPpad <<= 1;
  if (NPpad <= 256) {
    const int nseg = 256 / NPpad, p = tid % NPpad, seg = tid / NPpad;
    double s0 = 0.0, s1 = 0.0;
    auto over_j = [&](auto term) {  // two accumulators: consecutive loads do not wait for each other's FMA
      int j = seg;
      for (; j + nseg < N; j += 2 * nseg) {
        s0 += term(j);
        s1 += term(j + nseg);
      }
      if (j < N) s0 += term(j);
    };
    if (p < D) {  // d/d log l_p :  kse * 2 (dx/l)^2
      const double il2 = kn.inv_ls[p] * kn.inv_ls[p], xip = xi[p];
      over_j([&](int j) {
        const double dx = xip - X[(size_t)j * D + p];
        return wk[j] * (2.0 * dx * dx * il2);
      });
    } else if (p == D) {  // d/d log lambda
      over_j([&](int j) { return wk[j]; });
    } else if (p == D + 1) {  // 1/2 tr Wm (the caller multiplies by d sigma_n^2 / d sigma_n_log)
      s0 = seg == 0 ? wm[i] : 0.0;
    } else if (p < 2 * D + 3) {  // MPK_1, feature e (e == D: the offset feature)
      const int e = p - (D + 2);
      if (kn.poly_deg >= 1) {
        const double c = 2.0 * kn.w1[e] * (e < D ? xi[e] : 1.0);
        if (e < D)
          over_j([&](int j) { return wm[j] * (c * X[(size_t)j * D + e]); });
        else
          over_j([&](int j) { return wm[j] * c; });
      }
    } else if (p < 3 * D + 3) {  // MPK_2 factor 0 parameter e: 2 w20_e x_ie x_je * B_ij
      const int e = p - (2 * D + 3);
      if (kn.poly_deg >= 2) {
        const double c = 2.0 * kn.w20[e] * xi[e];
        over_j([&](int j) { return (wm[j] * fb[j]) * (c * X[(size_t)j * D + e]); });
      }
    } else if (p < NP) {  // MPK_2 factor 1 parameter e: 2 w21_e x_ie x_je * A_ij
      const int e = p - (3 * D + 3);
      if (kn.poly_deg >= 2) {
        const double c = 2.0 * kn.w21[e] * xi[e];
        over_j([&](int j) { return (wm[j] * fa[j]) * (c * X[(size_t)j * D + e]); });
      }
    }
    red[tid] = s0 + s1;
    __syncthreads();
    if (tid < NP) {
      double s = 0.0;
      for (int sg = 0; sg < nseg; ++sg) s += red[sg * NPpad + tid];
      slab[(size_t)i * NP + tid] = 0.5 * s;
    }
    return;
  }
  for (int p = tid; p < NP; p += 256) {  // (more than 256 hyper-parameters: D > 63 -- beyond MCP_MAX_GPDIM today)
    double s = 0.0;
    if (p < D) {
      const double il2 = kn.inv_ls[p] * kn.inv_ls[p];
      for (int j = 0; j < N; ++j) {
        double dx = xi[p] - X[(size_t)j * D + p];
        s = fma(wk[j], 2.0 * dx * dx * il2, s);
      }
    } else if (p == D) {
      for (int j = 0; j < N; ++j) s += wk[j];
    } else if (p == D + 1) {
      s = wm[i];
    } else if (p < 2 * D + 3) {
      const int e = p - (D + 2);
      if (kn.poly_deg >= 1) {
        const double we = 2.0 * kn.w1[e];
        const double pie = e < D ? xi[e] : 1.0;
        for (int j = 0; j < N; ++j) s = fma(wm[j], we * pie * (e < D ? X[(size_t)j * D + e] : 1.0), s);
      }
    } else if (p < 3 * D + 3) {
      const int e = p - (2 * D + 3);
      if (kn.poly_deg >= 2) {
        const double we = 2.0 * kn.w20[e] * xi[e];
        for (int j = 0; j < N; ++j) s = fma(wm[j] * fb[j], we * X[(size_t)j * D + e], s);
      }
    } else {
      const int e = p - (3 * D + 3);
      if (kn.poly_deg >= 2) {
        const double we = 2.0 * kn.w21[e] * xi[e];
        for (int j = 0; j < N; ++j) s = fma(wm[j] * fa[j], we * X[(size_t)j * D + e], s);
      }
    }
    slab[(size_t)i * NP + p] = 0.5 * s;
  }
}
__global__ __launch_bounds__(256) void nll_grad_kernel(mcp_kernel kn, int N, const double* __restrict__ X, const double* __restrict__ Kinv,
                                                       int ldk, const double* __restrict__ alpha, double* __restrict__ slab) {
  nll_grad_row(kn, N, X, Kinv, ldk, alpha, slab);
}

__global__ void nll_colsum_kernel(int rows, int cols, const double* __restrict__ slab, double* __restrict__ out) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int r = 0;
  for (; r + 3 < rows; r += 4) {
    s0 += slab[(size_t)r * cols + c];
    s1 += slab[(size_t)(r + 1) * cols + c];
    s2 += slab[(size_t)(r + 2) * cols + c];
    s3 += slab[(size_t)(r + 3) * cols + c];
  }
  for (; r < rows; ++r) s0 += slab[(size_t)r * cols + c];
  out[c] = (s0 + s1) + (s2 + s3);
}

extern "C" size_t mcp_nll_workspace_bytes(int N, int D) { return (N > 0 && D > 0) ? sizeof(double) * (size_t)N * (4 * D + 3) : 0; }

extern "C" int mcp_nll_grad(const mcp_kernel* kern, int N, const double* X, const double* Kinv, int ldk, const double* alpha, double* grad,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!kernel_ok(kern) || !X || !Kinv || !alpha || !grad || !workspace || N <= 0 || ldk < N) return MCP_ERR_ARG;
  if (N > 4096) return MCP_ERR_LIMIT;  // four [N] row buffers live in LDS
  if (workspace_bytes < mcp_nll_workspace_bytes(N, kern->D)) return MCP_ERR_WORKSPACE;
  MCP_ENSURE_MAX_LDS(nll_grad_kernel);
  const int NP = 4 * kern->D + 3;
  double* slab = (double*)workspace;
  hipLaunchKernelGGL(nll_grad_kernel, dim3(N), dim3(256), sizeof(double) * (4 * (size_t)N + 256), (hipStream_t)stream, *kern, N, X, Kinv, ldk, alpha,
                     slab);
  MCP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nll_colsum_kernel, dim3((NP + 127) / 128), dim3(128), 0, (hipStream_t)stream, N, NP, slab, grad);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

// ---------------------------------------------------------------------------------------
// One epoch of GP hyper-parameter training for the G GPs of a model at once (mcp_nll_epoch): what GP_prior.fit_model does per epoch
// through forward + Marginal_log_likelihood + autograd (gpr_lib/GP_prior/GP_prior.py:91-115,179-230; Gaussian_likelihood.py:15-24;
// Model_learning.train_gp_likelihood, model_learning/Model_learning.py:398-421), from the optimizer's RAW parameters to their gradients
// without a host round trip: the GPs are independent, so every stage is ONE launch whose grid carries the GP index.
// Workspace, per GP (doubles): K -> U [N N] | Uinv [N N] | Kinv [N N] | alpha [N] | r [N] | slab [N NP] | grad [NP] | inv_ls [D] |
// w1 [D+1] | w20 [D] | w21 [D] | scal [3] | logdet [1]; in front of all of them the G mcp_kernel descriptors the stages read.
// ---------------------------------------------------------------------------------------
struct NllBatch {
  mcp_nll_gp gp[MCP_MAX_GP];
};
struct NllWs {
  size_t kn, K, Ui, Kinv, alpha, r, slab, grad, invls, w1, w20, w21, scal, logdet, per_gp, total;  // offsets in doubles
};
static inline NllWs nll_ws_layout(int G, int N, int D) {
  NllWs w;
  const size_t NP = 4 * (size_t)D + 3, NN = (size_t)N * N;
  size_t o = 0;
  auto take = [&](size_t n) {
    size_t r = o;
    o += (n + 1) & ~(size_t)1;
    return r;
  };
  w.K = take(NN);
  w.Ui = take(NN);
  w.Kinv = take(NN);
  w.alpha = take(N);
  w.r = take(N);
  w.slab = take((size_t)N * NP);
  w.grad = take(NP);
  w.invls = take(D);
  w.w1 = take(D + 1);
  w.w20 = take(D);
  w.w21 = take(D);
  w.scal = take(4);
  w.logdet = take(2);
  w.per_gp = o;
  w.kn = 0;  // the descriptors come first
  const size_t knd = ((size_t)G * sizeof(mcp_kernel) + 15) / 16 * 2;
  w.total = knd + (size_t)G * w.per_gp;
  return w;
}
__device__ __forceinline__ double* nll_gp_base(double* ws, int G, size_t per_gp, int g) {
  const size_t knd = ((size_t)G * sizeof(mcp_kernel) + 15) / 16 * 2;
  return ws + knd + (size_t)g * per_gp;
}

// raw parameters -> the kernels' operands: 1 / l, lambda = exp(log_lambda), sigma_n^2 = exp(sigma_n_log)^2 + sigma_n_num^2, the MPK weights
// s^2 with s_d = (k - d) exp(par_d) (Sparse_GP.py:613-623: the reference's get_Sigma), and the mcp_kernel descriptor that points at them
__global__ void nll_prep_kernel(NllBatch b, int G, int N, int D, int deg, int ard, double* __restrict__ ws, NllWs L) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const mcp_nll_gp& gp = b.gp[g];
  double* base = nll_gp_base(ws, G, L.per_gp, g);
  double *invls = base + L.invls, *w1 = base + L.w1, *w20 = base + L.w20, *w21 = base + L.w21, *scal = base + L.scal;
  for (int d = tid; d < D; d += blockDim.x) {
    invls[d] = exp(-gp.log_ls[ard ? d : 0]);
    if (deg >= 2) {
      const double s0 = 2.0 * exp(gp.mpk2[d]), s1 = exp(gp.mpk2[D + d]);
      w20[d] = s0 * s0;
      w21[d] = s1 * s1;
    }
  }
  if (deg >= 1)
    for (int d = tid; d <= D; d += blockDim.x) {
      const double s = gp.mpk1 ? exp(gp.mpk1[d]) : 0.0;  // (a degree-2 term without a degree-1 term: zero weights)
      w1[d] = s * s;
    }
  if (tid == 0) {
    scal[0] = gp.log_lambda ? exp(gp.log_lambda[0]) : 0.0;
    const double sn = gp.sigma_n_log ? exp(gp.sigma_n_log[0]) : 0.0;
    scal[1] = sn * sn + gp.sigma_n_num2;
    scal[2] = gp.mean ? gp.mean[0] : 0.0;
    mcp_kernel kn;
    kn.D = D;
    kn.poly_deg = deg;
    kn.lambda = kn.sigma_n2 = kn.mean = 0.0;
    kn.inv_ls = invls;
    kn.w1 = deg >= 1 ? w1 : nullptr;
    kn.w20 = deg >= 2 ? w20 : nullptr;
    kn.w21 = deg >= 2 ? w21 : nullptr;
    kn.scal = scal;
    reinterpret_cast<mcp_kernel*>(ws)[g] = kn;
  }
}
// 16 rows x 256 columns of one GP's Gram matrix per workgroup.  The 256 inputs x_j of the columns (transposed: xj[d][j], lanes read
// consecutive addresses), the 16 inputs x_i of the rows and the kernel's weights are staged in LDS once, so a thread's D-long loops run
// on LDS instead of on strided global loads whose latency they could not hide (one thread per entry with both inputs in global memory:
// 124 us for the six 400 x 400, D = 24 matrices of the UR5 model).  The arithmetic is kern_eval's, operation for operation.
#define CB_ROWS 16
// (DEG: the polynomial degree as a template parameter -- as a run-time test inside the unrolled row loop it was a scalar branch behind every LDS
//  read, each waiting for its own operand: 41 us for what takes 11 without the loop)
template <int DEG>
__global__ __launch_bounds__(256) void cov_build_batch_kernel(const mcp_kernel* __restrict__ kns, int N, const double* __restrict__ X,
                                                              double* __restrict__ ws, int G, NllWs L) {
  extern __shared__ __attribute__((aligned(16))) double cb[];
  const int g = blockIdx.z, i0 = blockIdx.y * CB_ROWS, j0 = blockIdx.x * 256, tid = threadIdx.x;
  const mcp_kernel kn = kns[g];
  const int D = kn.D;
  constexpr int deg = DEG;
  double* xj = cb;                       // [D][257]
  double* xi = xj + 257 * D;             // [CB_ROWS][D]
  double* par = xi + CB_ROWS * D;        // inv_ls[D] | w1[D + 1] | w20[D] | w21[D]
  const int nj = min(256, N - j0), ni = min(CB_ROWS, N - i0);
  for (int base = tid; base < nj * D; base += 8 * 256) {  // (eight loads in flight per thread: four waves alone on a CU hide nothing else)
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = base + u * 256;
      v[u] = e < nj * D ? X[(size_t)j0 * D + e] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = base + u * 256;
      if (e < nj * D) {
        const int r = e / D, d = e - r * D;
        xj[d * 257 + r] = v[u];
      }
    }
  }
  for (int e = tid; e < ni * D; e += 256) xi[e] = X[(size_t)i0 * D + e];
  for (int d = tid; d < D; d += 256) {
    par[d] = kn.inv_ls[d];
    par[2 * D + 1 + d] = deg >= 2 ? kn.w20[d] : 0.0;
    par[3 * D + 1 + d] = deg >= 2 ? kn.w21[d] : 0.0;
  }
  for (int d = tid; d <= D; d += 256) par[D + d] = deg >= 1 ? kn.w1[d] : 0.0;
  __syncthreads();
  if (tid >= nj) return;
  const double *inv_ls = par, *w1 = par + D, *w20 = par + 2 * D + 1, *w21 = par + 3 * D + 1;
  double* Kg = nll_gp_base(ws, G, L.per_gp, g) + L.K;
  const double sn2 = kern_sigma_n2(kn), lam = kern_lambda(kn);
  // feature by feature, the CB_ROWS rows side by side: this column's x_jd and the weights are read once per feature instead of once per
  // (row, feature), and the rows' sums are CB_ROWS independent chains; every sum still runs over d in kern_eval's order
  double dist[CB_ROWS], p1[CB_ROWS], pa[CB_ROWS], pb[CB_ROWS];
#pragma unroll
  for (int r = 0; r < CB_ROWS; ++r) {
    dist[r] = 0.0;
    p1[r] = w1[D];
    pa[r] = pb[r] = 0.0;
  }
  for (int d = 0; d < D; ++d) {
    const double xjd = xj[d * 257 + tid], il = inv_ls[d], wd = w1[d], wa = w20[d], wb = w21[d];
#pragma unroll
    for (int r = 0; r < CB_ROWS; ++r) {
      const double ad = xi[(r < ni ? r : 0) * D + d];
      const double q = (ad - xjd) * il;
      dist[r] = fma(q, q, dist[r]);
      if (deg >= 1) p1[r] = fma(wd * ad, xjd, p1[r]);
      if (deg >= 2) {
        const double ab = ad * xjd;
        pa[r] = fma(wa, ab, pa[r]);
        pb[r] = fma(wb, ab, pb[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < CB_ROWS; ++r) {
    if (r < ni) {
      double k = lam * exp(-dist[r]);
      if (deg >= 1) {
        k += p1[r];
        if (deg >= 2) k = fma(pa[r], pb[r], k);
      }
      if (i0 + r == j0 + tid) k += sn2;
      Kg[(size_t)(i0 + r) * N + j0 + tid] = k;
    }
  }
}
static inline size_t cov_build_batch_lds(int D) { return sizeof(double) * ((size_t)257 * D + (size_t)CB_ROWS * D + 4 * (size_t)D + 2); }
// r = Y y_scale - mean;  alpha = Kinv r  (one wave per row)
__global__ void nll_alpha_batch_kernel(NllBatch b, int G, int N, double* __restrict__ ws, NllWs L) {
  const int g = blockIdx.y, row = blockIdx.x * (blockDim.x / MCP_WAVE) + (threadIdx.x / MCP_WAVE), lane = threadIdx.x % MCP_WAVE;
  if (row >= N) return;
  const mcp_nll_gp& gp = b.gp[g];
  double* base = nll_gp_base(ws, G, L.per_gp, g);
  const double* Kinv = base + L.Kinv;
  const double mean = base[L.scal + 2];
  double s = 0.0;
  for (int m = lane; m < N; m += MCP_WAVE) s = fma(Kinv[(size_t)row * N + m], gp.Y[m] * gp.y_scale - mean, s);
  s = wave_sum(s);
  if (lane == 0) {
    base[L.alpha + row] = s;
    base[L.r + row] = gp.Y[row] * gp.y_scale - mean;
  }
}
__global__ __launch_bounds__(256) void nll_grad_batch_kernel(const mcp_kernel* __restrict__ kns, int N, const double* __restrict__ X,
                                                             double* __restrict__ ws, int G, NllWs L) {
  const int g = blockIdx.y;
  double* base = nll_gp_base(ws, G, L.per_gp, g);
  nll_grad_row(kns[g], N, X, base + L.Kinv, N, base + L.alpha, base + L.slab);
}
// The same rows by a workgroup of 16 waves that takes `rows` consecutive rows i, with the inputs staged in LDS once, TRANSPOSED
// (xs[d][j], odd pitch: lanes j read consecutive addresses), and the kernel's weights beside them.
//   (1) thread j:  Wm_ij, Wm_ij kse_ij, A_ij, B_ij                          (the D-long loops run on LDS)
//   (2) wave w:    hyper-parameters p = w, w + 16, ...  -- one parameter at a time, the SAME for all lanes (no divergence between the
//                  parameter classes), lanes over j, one wave reduction per parameter; summed over the workgroup's rows in registers:
//                  slab[workgroup][p], added up by nll_finish_kernel in workgroup order.
// The row kernel above walks D- and N-long loops of global loads per thread (strided, or one element per iteration, with one thread per
// parameter and the classes diverging inside a wave): 128 us per epoch at the UR5 shape (six GPs, N = 400, D = 24), where the
// arithmetic is a few microseconds.
#define NG_NT 1024
#define NG_KMAX ((4 * MCP_MAX_GPDIM + 3 + NG_NT / 64 - 1) / (NG_NT / 64))  // parameters per wave
template <int DEG>  // (the polynomial degree at compile time: no scalar branch inside the feature loops)
__global__ __launch_bounds__(NG_NT) void nll_grad_rows_kernel(const mcp_kernel* __restrict__ kns, int N, const double* __restrict__ X,
                                                              double* __restrict__ ws, int G, NllWs L, int rows) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i0 = blockIdx.x * rows;
  const mcp_kernel kn = kns[g];
  const int D = kn.D, NP = 4 * D + 3, Np = N | 1;
  constexpr int deg = DEG;
  double* wm = sm;               // [N] Wm_ij
  double* wk = sm + N;           // [N] Wm_ij * kse_ij
  double* fa = sm + 2 * N;       // [N] Wm_ij * A_ij   (MPK_2 factors)
  double* fb = sm + 3 * N;       // [N] Wm_ij * B_ij
  double* par = sm + 4 * N;      // inv_ls[D] | w1[D + 1] | w20[D] | w21[D]
  double* xs = par + 4 * D + 2;  // [D][Np]
  const double* base = nll_gp_base(ws, G, L.per_gp, g);
  const double *Kinv = base + L.Kinv, *alpha = base + L.alpha;
  double* slab = nll_gp_base(ws, G, L.per_gp, g) + L.slab;
  for (int base = tid; base < N * D; base += 12 * NG_NT) {  // (twelve loads in flight per thread: the staging is a chain of round trips otherwise)
    double v[12];
#pragma unroll
    for (int u = 0; u < 12; ++u) {
      const int e = base + u * NG_NT;
      v[u] = e < N * D ? X[e] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 12; ++u) {
      const int e = base + u * NG_NT;
      if (e < N * D) {
        const int r = e / D, d = e - r * D;
        xs[d * Np + r] = v[u];
      }
    }
  }
  for (int d = tid; d < D; d += NG_NT) {
    par[d] = kn.inv_ls[d];
    par[2 * D + 1 + d] = deg >= 2 ? kn.w20[d] : 0.0;
    par[3 * D + 1 + d] = deg >= 2 ? kn.w21[d] : 0.0;
  }
  for (int d = tid; d <= D; d += NG_NT) par[D + d] = deg >= 1 ? kn.w1[d] : 0.0;
  const double lam = kern_lambda(kn);
  const double *inv_ls = par, *w1 = par + D, *w20 = par + 2 * D + 1, *w21 = par + 3 * D + 1;
  double tot[NG_KMAX];  // this wave's parameters, this lane's share, summed over the workgroup's rows
#pragma unroll
  for (int kx = 0; kx < NG_KMAX; ++kx) tot[kx] = 0.0;
  __syncthreads();
  for (int i = i0; i < min(i0 + rows, N); ++i) {
    const double ai = alpha[i];
    for (int j = tid; j < N; j += NG_NT) {
      double dist = 0.0, A = 0.0, Bv = 0.0;
#pragma unroll 6
      for (int d = 0; d < D; ++d) {
        const double xid = xs[d * Np + i], xjd = xs[d * Np + j];
        double r = (xid - xjd) * inv_ls[d];
        dist = fma(r, r, dist);
        if (deg >= 2) {
          double xx = xid * xjd;
          A = fma(w20[d], xx, A);
          Bv = fma(w21[d], xx, Bv);
        }
      }
      double w = Kinv[(size_t)i * N + j] - ai * alpha[j];
      wm[j] = w;
      wk[j] = w * lam * exp(-dist);
      fa[j] = w * A;
      fb[j] = w * Bv;
    }
    __syncthreads();
#pragma unroll
    for (int kx = 0; kx < NG_KMAX; ++kx) {
      const int p = wv + kx * (NG_NT / 64);  // (wave-uniform)
      if (p >= NP) break;
      double s = 0.0;
      if (p < D) {  // d/d log l_p :  kse * 2 (dx/l)^2
        const double il2 = inv_ls[p] * inv_ls[p], xip = xs[p * Np + i];
#pragma unroll 4
        for (int j = lane; j < N; j += 64) {
          const double dx = xip - xs[p * Np + j];
          s = fma(wk[j], 2.0 * dx * dx * il2, s);
        }
      } else if (p == D) {  // d/d log lambda
#pragma unroll 4
        for (int j = lane; j < N; j += 64) s += wk[j];
      } else if (p == D + 1) {  // 1/2 tr Wm (the caller multiplies by d sigma_n^2 / d sigma_n_log)
        s = lane == 0 ? wm[i] : 0.0;
      } else if (p < 2 * D + 3) {  // MPK_1, feature e (e == D: the offset feature)
        const int e = p - (D + 2);
        if (deg >= 1) {
          const double c = 2.0 * w1[e] * (e < D ? xs[e * Np + i] : 1.0);
          if (e < D)
#pragma unroll 4
          for (int j = lane; j < N; j += 64) s = fma(wm[j], c * xs[e * Np + j], s);
          else
#pragma unroll 4
          for (int j = lane; j < N; j += 64) s = fma(wm[j], c, s);
        }
      } else if (p < 3 * D + 3) {  // MPK_2 factor 0 parameter e: 2 w20_e x_ie x_je * B_ij
        const int e = p - (2 * D + 3);
        if (deg >= 2) {
          const double c = 2.0 * w20[e] * xs[e * Np + i];
#pragma unroll 4
          for (int j = lane; j < N; j += 64) s = fma(fb[j], c * xs[e * Np + j], s);
        }
      } else {  // MPK_2 factor 1 parameter e: 2 w21_e x_ie x_je * A_ij
        const int e = p - (3 * D + 3);
        if (deg >= 2) {
          const double c = 2.0 * w21[e] * xs[e * Np + i];
#pragma unroll 4
          for (int j = lane; j < N; j += 64) s = fma(fa[j], c * xs[e * Np + j], s);
        }
      }
      tot[kx] += s;  // per lane, rows in order; the lanes meet once, below (the sum does not depend on how many GPs share the launch)
    }
    __syncthreads();  // (wm .. fb are rewritten by the next row)
  }
#pragma unroll
  for (int kx = 0; kx < NG_KMAX; ++kx) {
    const int p = wv + kx * (NG_NT / 64);
    if (p < NP) {  // (wave-uniform)
      const double t = 0.5 * wave_sum(tot[kx]);
      if (lane == 0) slab[(size_t)blockIdx.x * NP + p] = t;
    }
  }
}
// rows per workgroup: a function of N alone, so that a GP's sums are the same whether it is trained alone or in a batch
static inline int nll_grad_rows_per_wg(int N) { return (N + 127) / 128; }
static inline size_t nll_grad_rows_lds(int N, int D) { return sizeof(double) * (4 * (size_t)N + 4 * (size_t)D + 2 + (size_t)D * (N | 1)); }
__global__ __launch_bounds__(256) void nll_finish_kernel(NllBatch b, int G, int N, int D, int deg, int ard, double* __restrict__ ws, NllWs L,
                                                         int slab_rows) {
  __shared__ double sh[4 * MCP_MAX_GPDIM + 3];
  __shared__ double red[4];
  const int g = blockIdx.x, tid = threadIdx.x, NP = 4 * D + 3;
  const mcp_nll_gp& gp = b.gp[g];
  double* base = nll_gp_base(ws, G, L.per_gp, g);
  const double* slab = base + L.slab;
  for (int c = tid; c < NP; c += 256) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int r = 0;
    for (; r + 3 < slab_rows; r += 4) {  // (slab: one row per row of K, or per workgroup of nll_grad_rows_kernel)
      s0 += slab[(size_t)r * NP + c];
      s1 += slab[(size_t)(r + 1) * NP + c];
      s2 += slab[(size_t)(r + 2) * NP + c];
      s3 += slab[(size_t)(r + 3) * NP + c];
    }
    for (; r < slab_rows; ++r) s0 += slab[(size_t)r * NP + c];
    sh[c] = (s0 + s1) + (s2 + s3);
  }
  // r . alpha and sum alpha
  double ra = 0.0, sa = 0.0;
  for (int j = tid; j < N; j += 256) {
    const double a = base[L.alpha + j];
    ra = fma(base[L.r + j], a, ra);
    sa += a;
  }
  ra = wave_sum(ra);
  sa = wave_sum(sa);
  if ((tid & 63) == 0) red[tid >> 6] = ra;
  __syncthreads();
  const double rdot = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = sa;
  __syncthreads();
  const double asum = ((red[0] + red[1]) + red[2]) + red[3];
  if (tid == 0 && gp.loss) gp.loss[0] = 0.5 * (rdot + base[L.logdet]);
  if (gp.g_log_ls) {
    if (ard) {
      for (int d = tid; d < D; d += 256) gp.g_log_ls[d] = sh[d];
    } else if (tid == 0) {
      double s = 0.0;
      for (int d = 0; d < D; ++d) s += sh[d];
      gp.g_log_ls[0] = s;
    }
  }
  if (tid == 0) {
    if (gp.g_log_lambda) gp.g_log_lambda[0] = sh[D];
    if (gp.g_sigma_n_log && gp.sigma_n_log) gp.g_sigma_n_log[0] = sh[D + 1] * 2.0 * exp(2.0 * gp.sigma_n_log[0]);
    if (gp.g_mean) gp.g_mean[0] = -asum;
  }
  if (gp.g_mpk1 && deg >= 1)
    for (int e = tid; e <= D; e += 256) gp.g_mpk1[e] = sh[D + 2 + e];
  if (gp.g_mpk2 && deg >= 2)
    for (int e = tid; e < 2 * D; e += 256) gp.g_mpk2[e] = sh[2 * D + 3 + e];
}

// f(std::integral_constant<int, DEG>()) with the polynomial degree (0 <= deg <= 2, checked by the caller) as a compile-time constant
template <class F>
static int with_degree(int deg, F&& f) {
  if (deg >= 2) return f(std::integral_constant<int, 2>());
  if (deg == 1) return f(std::integral_constant<int, 1>());
  return f(std::integral_constant<int, 0>());
}

extern "C" size_t mcp_nll_epoch_workspace_bytes(int G, int N, int D) {
  if (G <= 0 || G > MCP_MAX_GP || N <= 0 || D <= 0 || D > MCP_MAX_GPDIM) return 0;
  return sizeof(double) * nll_ws_layout(G, N, D).total;
}

// The epoch's plan for (G, N, D), on the host: the workspace map and the gradient form.  mcp_nll_epoch runs what this returns and
// mcp_nll_epoch_plan (include/mcpilco_hip_debug.h) reports it, so the plan returned is the plan run.
static int nll_epoch_plan(int G, int N, int D, NllWs* L, mcp_nll_plan* pl) {
  if (G <= 0 || N <= 0 || D <= 0) return MCP_ERR_ARG;
  if (G > MCP_MAX_GP || D > MCP_MAX_GPDIM || N > 1152 || N <= 16) return MCP_ERR_LIMIT;  // (the MFMA-blocked factorisations: 16 < N, row panel in LDS)
  *L = nll_ws_layout(G, N, D);
  pl->first_gp = (int64_t)(L->total - (size_t)G * L->per_gp);
  pl->per_gp = (int64_t)L->per_gp;
  pl->total = (int64_t)L->total;
  pl->K = (int64_t)L->K;
  pl->Uinv = (int64_t)L->Ui;
  pl->Kinv = (int64_t)L->Kinv;
  pl->alpha = (int64_t)L->alpha;
  pl->r = (int64_t)L->r;
  pl->slab = (int64_t)L->slab;
  pl->grad = (int64_t)L->grad;
  pl->inv_ls = (int64_t)L->invls;
  pl->w1 = (int64_t)L->w1;
  pl->w20 = (int64_t)L->w20;
  pl->w21 = (int64_t)L->w21;
  pl->scal = (int64_t)L->scal;
  pl->logdet = (int64_t)L->logdet;
  if (nll_grad_rows_lds(N, D) <= 150 * 1024) {
    pl->grad_form = MCP_NLL_GRAD_ROWS;
    pl->rows_per_wg = nll_grad_rows_per_wg(N);
    pl->slab_rows = (N + pl->rows_per_wg - 1) / pl->rows_per_wg;
    pl->lds_bytes = (int64_t)nll_grad_rows_lds(N, D);
  } else {
    pl->grad_form = MCP_NLL_GRAD_ROW_PER_WG;
    pl->rows_per_wg = 1;
    pl->slab_rows = N;
    pl->lds_bytes = (int64_t)(sizeof(double) * (4 * (size_t)N + 256));
  }
  return MCP_OK;
}

extern "C" int mcp_nll_epoch_plan(int G, int N, int D, mcp_nll_plan* plan) {
  if (!plan) return MCP_ERR_ARG;
  NllWs L;
  return nll_epoch_plan(G, N, D, &L, plan);
}

extern "C" int mcp_nll_epoch(int G, const mcp_nll_gp* gps, int N, int D, int poly_deg, int ard, const double* X, uint32_t* status,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!gps || !X || !status || !workspace) return MCP_ERR_ARG;
  NllWs L;
  mcp_nll_plan pl;
  {
    const int rc = nll_epoch_plan(G, N, D, &L, &pl);
    if (rc != MCP_OK) return rc;
  }
  if (poly_deg < 0 || poly_deg > 2) return MCP_ERR_ARG;
  if (workspace_bytes < sizeof(double) * L.total) return MCP_ERR_WORKSPACE;
  NllBatch b;
  for (int g = 0; g < MCP_MAX_GP; ++g) b.gp[g] = gps[g < G ? g : 0];
  for (int g = 0; g < G; ++g) {
    if (!gps[g].log_ls || !gps[g].log_lambda || !gps[g].Y) return MCP_ERR_ARG;
    if (poly_deg >= 2 && !gps[g].mpk2) return MCP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)workspace;
  const mcp_kernel* kns = (const mcp_kernel*)workspace;
  const size_t knd = ((size_t)G * sizeof(mcp_kernel) + 15) / 16 * 2;
  double* g0 = ws + knd;
  hipLaunchKernelGGL(nll_prep_kernel, dim3(G), dim3(64), 0, st, b, G, N, D, poly_deg, ard, ws, L);
  MCP_LAUNCH_CHECK();
  if (cov_build_batch_lds(D) > 150 * 1024) return MCP_ERR_LIMIT;
  {
    const dim3 cgrid((N + 255) / 256, (N + CB_ROWS - 1) / CB_ROWS, G);
    const int rc = with_degree(poly_deg, [&](auto deg_c) -> int {
      constexpr int DEG = decltype(deg_c)::value;
      MCP_ENSURE_MAX_LDS(cov_build_batch_kernel<DEG>);
      hipLaunchKernelGGL(cov_build_batch_kernel<DEG>, cgrid, dim3(256), cov_build_batch_lds(D), st, kns, N, X, ws, G, L);
      return MCP_OK;
    });
    if (rc != MCP_OK) return rc;
  }
  MCP_LAUNCH_CHECK();
  {
    const int rc = launch_chol_left(N, g0 + L.K, N, g0 + L.logdet, status, G, L.per_gp, L.per_gp, st);
    if (rc != MCP_OK) return rc;
  }
  {
    const int rc = launch_inverse_mfma(N, g0 + L.K, N, g0 + L.Ui, N, g0 + L.Kinv, N, G, L.per_gp, L.per_gp, L.per_gp, st);
    if (rc != MCP_OK) return rc;
  }
  hipLaunchKernelGGL(nll_alpha_batch_kernel, dim3((N + 3) / 4, G), dim3(256), 0, st, b, G, N, ws, L);
  MCP_LAUNCH_CHECK();
  const int slab_rows = (int)pl.slab_rows;
  if (pl.grad_form == MCP_NLL_GRAD_ROWS) {
    const int rows = (int)pl.rows_per_wg;
    const int rc = with_degree(poly_deg, [&](auto deg_c) -> int {
      constexpr int DEG = decltype(deg_c)::value;
      MCP_ENSURE_MAX_LDS(nll_grad_rows_kernel<DEG>);
      hipLaunchKernelGGL(nll_grad_rows_kernel<DEG>, dim3(slab_rows, G), dim3(NG_NT), (size_t)pl.lds_bytes, st, kns, N, X, ws, G, L, rows);
      return MCP_OK;
    });
    if (rc != MCP_OK) return rc;
  } else {
    MCP_ENSURE_MAX_LDS(nll_grad_batch_kernel);
    hipLaunchKernelGGL(nll_grad_batch_kernel, dim3(slab_rows, G), dim3(256), (size_t)pl.lds_bytes, st, kns, N, X, ws, G, L);
  }
  MCP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nll_finish_kernel, dim3(G), dim3(256), 0, st, b, G, N, D, poly_deg, ard, ws, L, slab_rows);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}
