// Host-side launchers of the GP pretrain and training sources that are called from another translation unit than their own
// (gp_pretrain.hip, gp_linalg.hip, gp_sod.hip, gp_nll.hip).  Declarations only: a __global__ function stays in the one source that launches it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mcpilco_hip.h"

namespace mcp {

// gp_pretrain.hip: the descriptor check of every entry that takes an mcp_kernel; K[N1][N2] = k(X1, X2) (+ sigma_n^2 on the diagonal)
bool kernel_ok(const mcp_kernel* k);
int launch_cov_build(const mcp_kernel& kn, int N1, const double* X1, int N2, const double* X2, int add_noise, double* K, int ldk, hipStream_t st);

// gp_linalg.hip, 16 < N <= 1152, `batch` matrices in one launch (strides in doubles): A = U^T U in place by the left-looking kernel of one
// workgroup per matrix; U^-1 and K^-1 = U^-1 U^-T by diagonal blocks, block columns and tiles
int launch_chol_left(int N, double* A, int lda, double* logdet, uint32_t* status, int batch, size_t a_stride, size_t ld_stride, hipStream_t st);
int launch_inverse_mfma(int N, const double* U, int ldu, double* Ui, int ldi, double* Kinv, int ldk, int batch, size_t u_stride,
                        size_t ui_stride, size_t k_stride, hipStream_t st);

}  // namespace mcp
