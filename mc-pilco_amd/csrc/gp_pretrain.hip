// Gram matrices, alpha and the packed operands of a trained GP for gfx950 (mcp_cov_build, mcp_cov_diag, mcp_gp_alpha, mcp_gp_pack).
// Replaces the kernel classes' get_covariance of the reference (Stationary_GP.py:162-170, Sparse_GP.py:426-441,625-646,
// GP_prior.py:314-335) and the alpha of GP_prior.forward / get_alpha (gpr_lib/GP_prior/GP_prior.py:91-135).  These run once per GP per
// trial (Model_learning.pretrain_gp), so they are written for clarity and fp64 accuracy.  The factorisation and the inverses are in
// gp_linalg.hip, subset-of-data selection in gp_sod.hip, the marginal-likelihood gradient and the training epoch in gp_nll.hip; the
// launchers those sources share are declared in gp_launch.h.
#include "gp_launch.h"
#include "mcp_device.h"

using namespace mcp;

// ---------------------------------------------------------------------------------------
// covariance matrices
// ---------------------------------------------------------------------------------------
__global__ void cov_build_kernel(mcp_kernel kn, int N1, const double* __restrict__ X1, int N2, const double* __restrict__ X2,
                                 int add_noise, double* __restrict__ K, int ldk) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int i = blockIdx.y;
  if (i >= N1 || j >= N2) return;
  double k = kern_eval(kn, X1 + (size_t)i * kn.D, 1, X2 + (size_t)j * kn.D, 1);
  if (add_noise && i == j) k += kern_sigma_n2(kn);
  K[(size_t)i * ldk + j] = k;
}

__global__ void cov_diag_kernel(mcp_kernel kn, int N, const double* __restrict__ X, int add_noise, double* __restrict__ diag) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double k = kern_diag(kn, X + (size_t)i * kn.D, 1);
  diag[i] = add_noise ? k + kern_sigma_n2(kn) : k;
}

__global__ void gp_alpha_kernel(int N, const double* __restrict__ Kinv, int ldk, const double* __restrict__ Y, double mean,
                                double* __restrict__ alpha) {
  // one wave per row: lanes stride the columns, DPP reduction
  int row = blockIdx.x * (blockDim.x / MCP_WAVE) + (threadIdx.x / MCP_WAVE);
  int lane = threadIdx.x % MCP_WAVE;
  if (row >= N) return;
  double s = 0.0;
  for (int m = lane; m < N; m += MCP_WAVE) s = fma(Kinv[(size_t)row * ldk + m], Y[m] - mean, s);
  s = wave_sum(s);
  if (lane == 0) alpha[row] = s;
}

__global__ void gp_pack_kernel(int N, int D, const double* __restrict__ X, const double* __restrict__ alpha,
                               const double* __restrict__ Kinv, int ldk, int Npad, double* __restrict__ Xt_out,
                               double* __restrict__ X_out, double* __restrict__ alpha_out, double* __restrict__ Kinv_out,
                               double* __restrict__ aX_out) {
  size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t idx = gid; idx < (size_t)Npad * Npad; idx += stride) {
    int i = (int)(idx / Npad), j = (int)(idx % Npad);
    Kinv_out[idx] = (i < N && j < N) ? Kinv[(size_t)i * ldk + j] : 0.0;
  }
  for (size_t idx = gid; idx < (size_t)Npad * D; idx += stride) {
    int j = (int)(idx / D), d = (int)(idx % D);
    double v = j < N ? X[(size_t)j * D + d] : 0.0;
    X_out[idx] = v;
    Xt_out[(size_t)d * Npad + j] = v;
  }
  for (size_t idx = gid; idx < (size_t)Npad; idx += stride) alpha_out[idx] = idx < (size_t)N ? alpha[idx] : 0.0;
  if (gid < (size_t)D) {
    double s = 0.0;
    for (int j = 0; j < N; ++j) s = fma(alpha[j], X[(size_t)j * D + gid], s);
    aX_out[gid] = s;
  }
}

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
bool mcp::kernel_ok(const mcp_kernel* k) {
  return k && k->D > 0 && k->D <= MCP_MAX_GPDIM && k->poly_deg >= 0 && k->poly_deg <= 2 && k->inv_ls &&
         (k->poly_deg < 1 || k->w1) && (k->poly_deg < 2 || (k->w20 && k->w21));
}

int mcp::launch_cov_build(const mcp_kernel& kn, int N1, const double* X1, int N2, const double* X2, int add_noise, double* K, int ldk, hipStream_t st) {
  hipLaunchKernelGGL(cov_build_kernel, dim3((N2 + 255) / 256, N1), dim3(256), 0, st, kn, N1, X1, N2, X2, add_noise, K, ldk);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cov_build(const mcp_kernel* kern, int N1, const double* X1, int N2, const double* X2, int add_noise, double* K,
                             int ldk, void* stream) {
  if (!kernel_ok(kern) || !X1 || !X2 || !K || N1 <= 0 || N2 <= 0 || ldk < N2) return MCP_ERR_ARG;
  return launch_cov_build(*kern, N1, X1, N2, X2, add_noise, K, ldk, (hipStream_t)stream);
}

extern "C" int mcp_cov_diag(const mcp_kernel* kern, int N, const double* X, int add_noise, double* diag, void* stream) {
  if (!kernel_ok(kern) || !X || !diag || N <= 0) return MCP_ERR_ARG;
  hipLaunchKernelGGL(cov_diag_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, *kern, N, X, add_noise, diag);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_gp_alpha(int N, const double* Kinv, int ldk, const double* Y, double mean, double* alpha, void* stream) {
  if (!Kinv || !Y || !alpha || N <= 0 || ldk < N) return MCP_ERR_ARG;
  hipLaunchKernelGGL(gp_alpha_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, N, Kinv, ldk, Y, mean, alpha);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_gp_pack(int N, int D, const double* X, const double* alpha, const double* Kinv, int ldk, int Npad, double* Xt_out,
                           double* X_out, double* alpha_out, double* Kinv_out, double* aX_out, void* stream) {
  if (!X || !alpha || !Kinv || !Xt_out || !X_out || !alpha_out || !Kinv_out || !aX_out) return MCP_ERR_ARG;
  if (N <= 0 || D <= 0 || D > MCP_MAX_GPDIM || Npad < N || (Npad % 16) != 0 || ldk < N) return MCP_ERR_ARG;
  hipLaunchKernelGGL(gp_pack_kernel, dim3(256), dim3(256), 0, (hipStream_t)stream, N, D, X, alpha, Kinv, ldk, Npad, Xt_out, X_out,
                     alpha_out, Kinv_out, aX_out);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

