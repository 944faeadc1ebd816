// Row-wise kernels of the column-contrastive loss (contrast_kernels.hip);
// the logits themselves live in the EPI_NCE_* GEMM epilogues.
#pragma once
#include <hip/hip_runtime.h>

#define NCE_EPS 1e-8f
#define NCE_MAX_PARTS 256

// x (M rows of D bf16, row stride ld elements) -> out[M] = 1/max(|x_i|, eps)
void launch_nce_rnorm(const void* x, long ld, float* out, long M, int D,
                      hipStream_t s);
// part[M][ntn] -> lse[M] = 1/T + log(sum_k part[i][k]) and the scalar
// loss[0] = mean_i (lse[i] - pos[i]); blockpart holds NCE_MAX_PARTS floats
void launch_nce_loss(const float* part, const float* pos, float* lse,
                     float* blockpart, float* loss, long M, int ntn,
                     float invt, hipStream_t s);
// g (rows x D bf16, dense): g_i = go * (sum_sl acc[sl][i] - coef_i * x_i),
// acc = nsl slices of (rows, D) f32 added in slice order (16-byte aligned),
// coef_i = (sum_k part[i][k]) * rnorm_i^2, 0 for rows whose norm was clamped
void launch_nce_grad_rows(void* g, const float* acc, int nsl, const void* x,
                          long ld, const float* part, int ntn,
                          const float* rnorm, const float* go, long rows,
                          int D, hipStream_t s);
