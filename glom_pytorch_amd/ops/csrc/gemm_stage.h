// LDS staging helpers shared by the 128x128 repack kernels (gemm_fast.hip:
// gemm_tn_fast, gemm_nn_fast, gemm_tn_sk) and gemm_nn_sk.hip.
#pragma once
#include "common.h"
#include "lds_swizzle.h"

#ifndef FBK
#define FBK 64
#endif

// LDS bank swizzle: the 16B-granule index in a 128B row is XORed with
// swz_row<SWZ>(row) (lds_swizzle.h: the functions, the lane groups they
// are derived against and the compile-time bank check). SWZ is the image's
// per-kernel constant; the fragment reads of that image use the same one.

// Transpose-stage one operand tile: source rows = reduction slice
// [t0, t0+64) (row stride ld), cols = output-dim slice [c0, c0+128).
// 128 threads per operand; thread (mb, cb) loads an 8(m) x 8(c) block and
// writes 8 column-vectors of 8 bf16 via ds_write_b128 into the swizzled
// [col][m] image (row length 64 elements = 128 B).
template <int SWZ>
__device__ __forceinline__ void stage_repack(
        ushort_t* lds, const ushort_t* src, long ld, int t0, int c0,
        int kend, int tid128) {
    int cb = tid128 & 15;   // 16 col-blocks of 8
    int mb = tid128 >> 4;   // 8 m-blocks of 8
    union { uint4v v; ushort_t u[8]; } rowv[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        int m = t0 + mb * 8 + r;
        if (m < kend)
            rowv[r].v = *(const uint4v*)(src + (long)m * ld + c0 + cb * 8);
        else
            rowv[r].v = 0;
    }
#pragma unroll
    for (int e = 0; e < 8; e++) {
        union { uint4v v; ushort_t u[8]; } col;
#pragma unroll
        for (int r = 0; r < 8; r++) col.u[r] = rowv[r].u[e];
        int row = cb * 8 + e;                       // output-dim index
        int off = (mb * 8) ^ (swz_row<SWZ>(row) << 3);   // swizzled m offset
        *(uint4v*)&lds[row * FBK + off] = col.v;
    }
}

// plain swizzled copy of a 128 x 64 row-major tile (rows r0.., cols k0..)
template <int SWZ>
__device__ __forceinline__ void stage_copy128(
        ushort_t* lds, const ushort_t* src, long ld, int r0, int k0,
        int maxK, int tid128) {
    // 128 threads stage a 128x64 tile: thread t handles rows t, t+... no:
    // 1024 chunks of 8 elements / 128 threads = 8 chunks each
#pragma unroll
    for (int cc = 0; cc < 8; cc++) {
        int c = tid128 * 8 + cc;
        int row = c >> 3;
        int g = c & 7;
        int gk = k0 + g * 8;
        union { uint4v v; ushort_t u[8]; } t;
        if (gk + 7 < maxK)
            t.v = *(const uint4v*)(src + (long)(r0 + row) * ld + gk);
        else
            t.v = 0;
        int off = (g * 8) ^ (swz_row<SWZ>(row) << 3);
        *(uint4v*)&lds[row * FBK + off] = t.v;
    }
}

