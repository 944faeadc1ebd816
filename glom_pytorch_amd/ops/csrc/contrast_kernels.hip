// Row-wise kernels of the column-contrastive loss on CDNA4 (gfx950); see
// glom_pytorch_amd/contrast.py for the specification and gemm_device.h
// (gemm_epilogue_nce) for the GEMM epilogues that produce the partials.
//   - k_nce_rnorm:     1 / max(|row|, 1e-8) of a strided (M, D) bf16 matrix
//                      (k_rnorm's sibling: other clamp, plain row indexing)
//   - k_nce_loss_part: per row, sum the column-tile partials in tile order,
//                      lse_i = 1/T + log(sum), and sum lse_i - pos_i over a
//                      block's chunk of rows
//   - k_nce_loss_fin:  fixed-order sum of the block partials / M
//   - k_nce_grad_rows: g_i = go * (G'B_i - r_i * rnorm_i^2 * x_i), with G'B
//                      summed from the split-K f32 slices in slice order
// Every reduction has one fixed order and one writer per slot: results are
// run-to-run bitwise reproducible, no atomics, no host synchronisation.

#include "common.h"
#include "contrast_kernels.h"

#define NTHREADS 256
#define WPB (NTHREADS / WAVE)

static inline long cdivl(long a, long b) { return (a + b - 1) / b; }

// one wave per row, 16-byte loads (D % 8 == 0, ld % 8 == 0, aligned base)
__global__ __launch_bounds__(NTHREADS) void k_nce_rnorm(
        const ushort_t* __restrict__ x, long ld, float* __restrict__ out,
        long M, int D) {
    long row = (long)blockIdx.x * WPB + threadIdx.x / WAVE;
    if (row >= M) return;
    int lane = threadIdx.x % WAVE;
    const ushort_t* xr = x + row * ld;
    float ss = 0.f;
    for (int q0 = lane * 8; q0 < D; q0 += WAVE * 8) {
        union { uint4v v; ushort_t u[8]; } t;
        t.v = *(const uint4v*)(xr + q0);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            float v = bf2f(t.u[e]);
            ss += v * v;
        }
    }
    ss = wave_reduce_sum(ss);
    if (lane == 0) out[row] = 1.0f / fmaxf(sqrtf(ss), NCE_EPS);
}

// sum of v over the block in a fixed order, valid in thread 0
__device__ __forceinline__ float block_sum_fixed(float v, float* sh) {
    v = wave_reduce_sum(v);
    if (threadIdx.x % WAVE == 0) sh[threadIdx.x / WAVE] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < WPB; w++) t += sh[w];
    return t;
}

// grid: nb blocks, block b owns rows [b*chunk, min(M, (b+1)*chunk))
__global__ __launch_bounds__(NTHREADS) void k_nce_loss_part(
        const float* __restrict__ part, const float* __restrict__ pos,
        float* __restrict__ lse, float* __restrict__ blockpart, long M,
        int ntn, float invt, long chunk) {
    __shared__ float sh[WPB];
    long r0 = (long)blockIdx.x * chunk;
    long r1 = min(M, r0 + chunk);
    float acc = 0.f;
    for (long i = r0 + threadIdx.x; i < r1; i += NTHREADS) {
        const float* pr = part + i * ntn;
        float z = 0.f;
        for (int k = 0; k < ntn; k++) z += pr[k];
        float l = invt + logf(z);
        lse[i] = l;
        acc += l - pos[i];
    }
    float t = block_sum_fixed(acc, sh);
    if (threadIdx.x == 0) blockpart[blockIdx.x] = t;
}

// one wave: lane l sums blockpart[l], [l+64], ... in order
__global__ __launch_bounds__(WAVE) void k_nce_loss_fin(
        const float* __restrict__ blockpart, float* __restrict__ loss,
        int nb, float invm) {
    float acc = 0.f;
    for (int b = threadIdx.x; b < nb; b += WAVE) acc += blockpart[b];
    acc = wave_reduce_sum(acc);
    if (threadIdx.x == 0) loss[0] = acc * invm;
}

// one wave per row; every lane adds the row's partials in the same order.
// acc: nsl slices of (rows, D) f32, the split-K partials of G' @ other.
__global__ __launch_bounds__(NTHREADS) void k_nce_grad_rows(
        ushort_t* __restrict__ g, const float* __restrict__ acc, int nsl,
        const ushort_t* __restrict__ x, long ld,
        const float* __restrict__ part, int ntn,
        const float* __restrict__ rnorm, const float* __restrict__ go,
        long rows, int D) {
    long row = (long)blockIdx.x * WPB + threadIdx.x / WAVE;
    if (row >= rows) return;
    int lane = threadIdx.x % WAVE;
    const float* pr = part + row * ntn;
    float r = 0.f;
    for (int k = 0; k < ntn; k++) r += pr[k];
    const float rn = rnorm[row];
    // a clamped norm is a constant: no normalisation term for that row
    const float coef = rn < 1.0f / NCE_EPS ? r * rn * rn : 0.f;
    const float gout = go[0];
    ushort_t* gr = g + row * D;
    const ushort_t* xr = x + row * ld;
    const float* ar = acc + row * D;
    const long slab = rows * D;
    for (int q0 = lane * 8; q0 < D; q0 += WAVE * 8) {
        float v[8] = {};
        for (int sl = 0; sl < nsl; sl++) {
            f32x4 lo = *(const f32x4*)(ar + sl * slab + q0);
            f32x4 hi = *(const f32x4*)(ar + sl * slab + q0 + 4);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                v[e] += lo[e];
                v[4 + e] += hi[e];
            }
        }
        union { uint4v v; ushort_t u[8]; } o, b;
        b.v = *(const uint4v*)(xr + q0);
#pragma unroll
        for (int e = 0; e < 8; e++)
            o.u[e] = f2bf(gout * (v[e] - coef * bf2f(b.u[e])));
        *(uint4v*)(gr + q0) = o.v;
    }
}

void launch_nce_rnorm(const void* x, long ld, float* out, long M, int D,
                      hipStream_t s) {
    hipLaunchKernelGGL(k_nce_rnorm, dim3(cdivl(M, WPB)), dim3(NTHREADS), 0, s,
                       (const ushort_t*)x, ld, out, M, D);
}

void launch_nce_loss(const float* part, const float* pos, float* lse,
                     float* blockpart, float* loss, long M, int ntn,
                     float invt, hipStream_t s) {
    long nb = cdivl(M, NTHREADS);
    if (nb > NCE_MAX_PARTS) nb = NCE_MAX_PARTS;
    long chunk = cdivl(M, nb);
    nb = cdivl(M, chunk);            // no empty blocks
    hipLaunchKernelGGL(k_nce_loss_part, dim3(nb), dim3(NTHREADS), 0, s, part,
                       pos, lse, blockpart, M, ntn, invt, chunk);
    hipLaunchKernelGGL(k_nce_loss_fin, dim3(1), dim3(WAVE), 0, s, blockpart,
                       loss, (int)nb, 1.0f / (float)M);
}

void launch_nce_grad_rows(void* g, const float* acc, int nsl, const void* x,
                          long ld, const float* part, int ntn,
                          const float* rnorm, const float* go, long rows,
                          int D, hipStream_t s) {
    hipLaunchKernelGGL(k_nce_grad_rows, dim3(cdivl(rows, WPB)),
                       dim3(NTHREADS), 0, s, (ushort_t*)g, acc, nsl,
                       (const ushort_t*)x, ld, part, ntn, rnorm, go, rows, D);
}
