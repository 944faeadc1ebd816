// Tuned full-tile GEMM kernels for the GLOM hot path (gfx950).
//
// gemm_nt_fast: 128x128x64 tiles, 4 waves x (64x64), double-buffered LDS
// filled by direct global->LDS DMA (`global_load_lds` width 16) with the
// T2 XOR swizzle applied on the per-lane SOURCE address and again on the
// ds_read_b128 fragment reads (linear lane-order LDS destination, as
// rule 21 requires). One barrier per K-tile; the barrier's implicit
// vmcnt(0) drains the in-flight DMA of the next tile.
//
// gemm_tn_fast: both operands have the reduction (token) index as the
// SOURCE row, so tiles are transpose-staged: each thread loads an 8x8
// block with 16B vector loads, repacks to column vectors in registers,
// and writes 8 x ds_write_b128 into the swizzled [out-dim][k] image —
// replacing the v1 per-element LDS scatter (8x fewer, 8x wider writes).
//
// gemm_tn_tr: the same TN tiles copied as stored by global_load_lds and
// transposed by ds_read_b64_tr_b16 on the way into the MFMA (K % 64 == 0;
// default for the split-K weight grads). See the comment above it.
//
// Preconditions (host-checked, fast_ok): M%128==0, N%128==0, K%64==0
// (TN: K%8==0 with row predicates), all row strides %8==0, no on-load
// transforms. Everything else falls back to the generic gemm_kernel.

#include <cstdlib>

#include "common.h"
#include "gemm.h"
#include "gemm_device.h"
#include "gemm_stage.h"

#define BM 128
#define BN 128
#define FBK 64
#define NTHREADS 256

// Fused colsum partial (GemmParams::colsum_out, layout [M/64][N]): the one
// writer of rows [row0, row0 + 64*nslots) x column `col` stores its sum in
// the span's first slot and zeroes the others. Plain stores, no atomics.
__device__ __forceinline__ void colsum_store(
        float* colp, long N, long row0, int nslots, long col, float v) {
    float* q = colp + (row0 >> 6) * N + col;
    q[0] = v;
    for (int k = 1; k < nslots; k++) q[(long)k * N] = 0.f;
}

// Sum of `v` over the 4 lanes {l, l^16, l^32, l^48} (the kq groups of the
// MFMA C layout), identical bits in all four.
__device__ __forceinline__ float kq_sum(float v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// Issue this wave's share of one operand tile (128 rows x 64 cols bf16 =
// 16 KB = 16 DMA chunks of 1 KB; 4 chunks per wave) into a LINEAR LDS
// image, pre-swizzling the source address so a swizzled ds_read_b128 is
// conflict-free (granule ^= swz_row(row), lds_swizzle.h).
__device__ __forceinline__ void stage_glds(
        ushort_t* lds, const ushort_t* src, long ld, int r0, int k0,
        int wid, int lane) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
        int chunk = wid * 4 + c;
        int row = chunk * 8 + (lane >> 3);
        int swz8 = ((lane & 7) ^ swz_row<SWZ_NT_FAST>(row)) * 8;
        const ushort_t* gaddr = src + (long)(r0 + row) * ld + k0 + swz8;
        ushort_t* laddr = lds + chunk * 512;  // wave-uniform chunk base
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)gaddr,
            (__attribute__((address_space(3))) unsigned int*)laddr, 16, 0, 0);
    }
}

// NCE: the column-contrastive epilogues (EPI_NCE_FWD / EPI_NCE_BWD) as a
// separate instantiation, so the plain kernel's code does not change.
template <bool NCE>
__global__ __launch_bounds__(NTHREADS) void gemm_nt_fast_kernel(GemmParams p) {
    // ONE shared array: a second __shared__ object makes hipcc emit
    // s_waitcnt vmcnt(0) before the first ds_read of every k-step of a
    // glds pipeline, draining the prefetch (guide §5 ".s-level traps" (a)).
    __shared__ ushort_t smem[4 * BM * FBK];
    ushort_t* As0 = smem;
    ushort_t* Bs0 = smem + 2 * BM * FBK;

    const int pid = blockIdx.z;
    // XCD-aware block remap (T1), column-major: each XCD die owns a
    // contiguous run of N-columns (all M-tiles of a few n-tiles), so the
    // shared B panel of a column stays resident in that XCD's private L2
    // while the M sweep streams A.
    int nwg = gridDim.x * gridDim.y;
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, off = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + off;
    }
    const int n0 = (bid / gridDim.y) * BN;   // column-major: n outer
    const int m0 = (bid % gridDim.y) * BM;

    const ushort_t* Ap;
    const ushort_t* Bp;
    long lda, ldb;
    resolve_ptr2(p.A, p.Atab, p.Atabld, pid, p.nInner, &Ap, &lda);
    resolve_ptr2(p.B, p.Btab, p.Btabld, pid, p.nInner, &Bp, &ldb);

    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int wm = (wid >> 1) * 64;
    const int wn = (wid & 1) * 64;
    const int lrow = lane & 15;
    const int kq = lane >> 4;

    f32x4 acc[4][4] = {};

    const int nk = p.K / FBK;
    int cur = 0;
    stage_glds(As0, Ap, lda, m0, 0, wid, lane);
    stage_glds(Bs0, Bp, ldb, n0, 0, wid, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int kt = 0; kt < nk; kt++) {
        if (kt + 1 < nk) {
            stage_glds(As0 + (cur ^ 1) * BM * FBK, Ap, lda, m0,
                       (kt + 1) * FBK, wid, lane);
            stage_glds(Bs0 + (cur ^ 1) * BN * FBK, Bp, ldb, n0,
                       (kt + 1) * FBK, wid, lane);
        }
        short8 af[2][4], bfr[2][4];
#pragma unroll
        for (int s = 0; s < 2; s++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int row = wm + i * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_NT_FAST>(row) << 3);
                af[s][i] = *(const short8*)&As0[cur * BM * FBK + row * FBK + off];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int row = wn + j * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_NT_FAST>(row) << 3);
                bfr[s][j] = *(const short8*)&Bs0[cur * BN * FBK + row * FBK + off];
            }
        }
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[s][i], bfr[s][j], acc[i][j], 0, 0, 0);
        __syncthreads();   // drains the in-flight DMA (vmcnt0) + buffer reuse
        cur ^= 1;
    }
    if (NCE) {
        gemm_epilogue_nce<true>(p, m0, n0, wm, wn, lrow, kq, acc,
                                (float*)smem);
        return;
    }
    gemm_epilogue_lds(p, pid, m0, n0, wm, wn, lrow, kq, acc, smem);
}

__global__ __launch_bounds__(NTHREADS) void gemm_tn_fast_kernel(GemmParams p) {
    __shared__ ushort_t smem[128 * EPI_LDS_ROW];   // >= As+Bs (2*8192)
    ushort_t* As = smem;
    ushort_t* Bs = smem + BM * FBK;

    int pid = blockIdx.z;
    int slice = 0, k_begin = 0, k_end = p.K;
    if (p.splitk > 1) {
        pid = blockIdx.z % p.nproblems;
        slice = blockIdx.z / p.nproblems;
        int per = ((p.K + FBK - 1) / FBK + p.splitk - 1) / p.splitk * FBK;
        k_begin = slice * per;
        k_end = min(p.K, k_begin + per);
    }
    // XCD-aware block remap (T1), column-major: each XCD die owns a
    // contiguous run of N-columns (all M-tiles of a few n-tiles), so the
    // shared B panel of a column stays resident in that XCD's private L2
    // while the M sweep streams A.
    int nwg = gridDim.x * gridDim.y;
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, off = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + off;
    }
    const int n0 = (bid / gridDim.y) * BN;   // column-major: n outer
    const int m0 = (bid % gridDim.y) * BM;

    const ushort_t* Ap;
    const ushort_t* Bp;
    long lda, ldb;
    resolve_ptr2(p.A, p.Atab, p.Atabld, pid, p.nInner, &Ap, &lda);
    resolve_ptr2(p.B, p.Btab, p.Btabld, pid, p.nInner, &Bp, &ldb);

    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int wm = (wid >> 1) * 64;
    const int wn = (wid & 1) * 64;
    const int lrow = lane & 15;
    const int kq = lane >> 4;

    f32x4 acc[4][4] = {};

    for (int k0 = k_begin; k0 < k_end; k0 += FBK) {
        if (threadIdx.x < 128)
            stage_repack<SWZ_TN_FAST>(As, Ap, lda, k0, m0, k_end, threadIdx.x);
        else
            stage_repack<SWZ_TN_FAST>(Bs, Bp, ldb, k0, n0, k_end,
                                      threadIdx.x - 128);
        __syncthreads();
        short8 af[2][4], bfr[2][4];
#pragma unroll
        for (int s = 0; s < 2; s++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int row = wm + i * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_TN_FAST>(row) << 3);
                af[s][i] = *(const short8*)&As[row * FBK + off];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int row = wn + j * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_TN_FAST>(row) << 3);
                bfr[s][j] = *(const short8*)&Bs[row * FBK + off];
            }
        }
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[s][i], bfr[s][j], acc[i][j], 0, 0, 0);
        __syncthreads();
    }

    if (p.splitk > 1) {
        float* ws = p.ws + ((long)slice * p.nproblems + pid) * p.M * p.N;
#pragma unroll
        for (int i16 = 0; i16 < 4; i16++)
#pragma unroll
            for (int j16 = 0; j16 < 4; j16++) {
                int j = n0 + wn + j16 * 16 + lrow;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    int i = m0 + wm + i16 * 16 + kq * 4 + r;
                    ws[(long)i * p.N + j] = acc[i16][j16][r];
                }
            }
        return;
    }
    __syncthreads();   // all waves done with As/Bs before epilogue staging
    gemm_epilogue_lds(p, pid, m0, n0, wm, wn, lrow, kq, acc, smem);
}

void launch_gemm_nt_fast(const GemmParams& p, hipStream_t stream) {
    dim3 grid(p.N / BN, p.M / BM, p.nproblems);
    if (p.epilogue == EPI_NCE_FWD || p.epilogue == EPI_NCE_BWD)
        hipLaunchKernelGGL(gemm_nt_fast_kernel<true>, grid, dim3(NTHREADS), 0,
                           stream, p);
    else
        hipLaunchKernelGGL(gemm_nt_fast_kernel<false>, grid, dim3(NTHREADS),
                           0, stream, p);
}

void launch_gemm_tn_fast(const GemmParams& p, hipStream_t stream) {
    int sk = p.splitk > 1 ? p.splitk : 1;
    dim3 grid(p.N / BN, p.M / BM, p.nproblems * sk);
    hipLaunchKernelGGL(gemm_tn_fast_kernel, grid, dim3(NTHREADS), 0, stream,
                       p);
}

// ---------------------------------------------------------------- //
// NN fast kernel (attention AV / dq): A row-major [M][K] staged as a
// plain swizzled copy; B row-major [K][N] transpose-staged with the
// 8x8 register repack. Single LDS buffer, two barriers per K-step.

__global__ __launch_bounds__(NTHREADS) void gemm_nn_fast_kernel(GemmParams p) {
    __shared__ ushort_t smem[128 * EPI_LDS_ROW];   // >= As+Bs (2*8192)
    ushort_t* As = smem;
    ushort_t* Bs = smem + BM * FBK;

    const int pid = blockIdx.z;
    int nwg = gridDim.x * gridDim.y;
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, off = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + off;
    }
    const int n0 = (bid / gridDim.y) * BN;
    const int m0 = (bid % gridDim.y) * BM;

    const ushort_t* Ap;
    const ushort_t* Bp;
    long lda, ldb;
    resolve_ptr2(p.A, p.Atab, p.Atabld, pid, p.nInner, &Ap, &lda);
    resolve_ptr2(p.B, p.Btab, p.Btabld, pid, p.nInner, &Bp, &ldb);

    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int wm = (wid >> 1) * 64;
    const int wn = (wid & 1) * 64;
    const int lrow = lane & 15;
    const int kq = lane >> 4;

    f32x4 acc[4][4] = {};

    for (int k0 = 0; k0 < p.K; k0 += FBK) {
        if (threadIdx.x < 128)
            stage_copy128<SWZ_NN_FAST>(As, Ap, lda, m0, k0, p.K, threadIdx.x);
        else
            stage_repack<SWZ_NN_FAST>(Bs, Bp, ldb, k0, n0, p.K,
                                      threadIdx.x - 128);
        __syncthreads();
        short8 af[2][4], bfr[2][4];
#pragma unroll
        for (int s = 0; s < 2; s++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int row = wm + i * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_NN_FAST>(row) << 3);
                af[s][i] = *(const short8*)&As[row * FBK + off];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int row = wn + j * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_NN_FAST>(row) << 3);
                bfr[s][j] = *(const short8*)&Bs[row * FBK + off];
            }
        }
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[s][i], bfr[s][j], acc[i][j], 0, 0, 0);
        __syncthreads();
    }
    __syncthreads();
    gemm_epilogue_lds(p, pid, m0, n0, wm, wn, lrow, kq, acc, smem);
}

void launch_gemm_nn_fast(const GemmParams& p, hipStream_t stream) {
    dim3 grid(p.N / BN, p.M / BM, p.nproblems);
    hipLaunchKernelGGL(gemm_nn_fast_kernel, grid, dim3(NTHREADS), 0, stream,
                       p);
}




// ---------------------------------------------------------------- //
// 128x256-tile NT kernels: 8 waves (512 threads), per-wave 64x64, BK=64
// glds stages. 2x the per-block work of the 128^2 kernel, so the per-block
// prologue/epilogue halves relative to the K=512 GLOM shapes that dominate
// the step.

#define NT3 512
#define BN3 256
// 256 cols + 16 pad (16B-aligned LDS epilogue rows). The fused AV product
// reads its P operand from these rows as MFMA fragments: with 34 granules
// per row, row r at kq sits on 16-byte slot (2r + kq) mod 16, and a read
// group (8 rows at kq, the other 8 at kq+1, never r and r+8 together) gets
// 16 distinct slots. The former pad of 8 (slot r + kq) was 2-way in every
// group. The price: the 2-byte fragment-order stores into these rows count
// more conflict cycles with 34 granules per row than with 33 (+3.1M per
// plain call at 16256x1024x512 G6, +0.8M on the fused forward against
// -1.57M for its P reads; profiles/README.md). No pad clears both.
#define EPI2_ROW 272
static_assert(lds_model::p_read_worst(EPI2_ROW) == 4,
              "P-operand fragment reads of the fused AV must not conflict");
static_assert(128 * EPI2_ROW + 2 * 256 * FBK <= 3 * (128 + 256) * FBK,
              "epilogue rows + the two V buffers must fit the nt4 arena");

// ------- 3-ring stages, counted vmcnt, raw barriers, LDS epilogue ------
__global__ __launch_bounds__(NT3) void gemm_nt_fast4_kernel(GemmParams p) {
    __shared__ ushort_t smem[3 * (128 + 256) * FBK];   // 144 KiB, 3-ring
    const int abuf = 128 * FBK, bbuf = 256 * FBK, stride = abuf + bbuf;

    const int pid = blockIdx.z;
    int nwg = gridDim.x * gridDim.y;
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, off = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + off;
    }
    const int n0 = (bid / gridDim.y) * BN3;
    const int m0 = (bid % gridDim.y) * BM;

    const ushort_t* Ap;
    const ushort_t* Bp;
    long lda, ldb;
    resolve_ptr2(p.A, p.Atab, p.Atabld, pid, p.nInner, &Ap, &lda);
    resolve_ptr2(p.B, p.Btab, p.Btabld, pid, p.nInner, &Bp, &ldb);

    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int wm = (wid >> 2) * 64;
    const int wn = (wid & 3) * 64;
    const int lrow = lane & 15;
    const int kq = lane >> 4;

    f32x4 acc[4][4] = {};

    // A: 16 chunks over 8 waves (2 each); B: 32 chunks (4 each)
    auto stage = [&](int buf, int k0) {
        ushort_t* Al = smem + buf * stride;
        ushort_t* Bl = Al + abuf;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            int chunk = wid * 2 + c;
            int row = chunk * 8 + (lane >> 3);
            int swz8 = ((lane & 7) ^ swz_row<SWZ_NT4>(row)) * 8;
            const ushort_t* g = Ap + (long)(m0 + row) * lda + k0 + swz8;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) unsigned int*)g,
                (__attribute__((address_space(3))) unsigned int*)
                    (Al + chunk * 512), 16, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            int chunk = wid * 4 + c;
            int row = chunk * 8 + (lane >> 3);
            int swz8 = ((lane & 7) ^ swz_row<SWZ_NT4>(row)) * 8;
            const ushort_t* g = Bp + (long)(n0 + row) * ldb + k0 + swz8;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) unsigned int*)g,
                (__attribute__((address_space(3))) unsigned int*)
                    (Bl + chunk * 512), 16, 0, 0);
        }
    };

    const int nk = p.K / FBK;
    // 3-deep ring with counted vmcnt (T3+T4): tile t computes while t+1 is
    // landed/landing and t+2 streams; ONE raw barrier + ONE counted wait
    // per K-tile — the vmcnt(0) drain of the 2-buffer loop never happens.
    stage(0, 0);
    if (nk > 1) stage(1, FBK);
    if (nk > 1)
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    for (int kt = 0; kt < nk; kt++) {
        if (kt + 2 < nk) stage((kt + 2) % 3, (kt + 2) * FBK);
        const ushort_t* Al = smem + (kt % 3) * stride;
        const ushort_t* Bl = Al + abuf;
        short8 af[2][4], bfr[2][4];
#pragma unroll
        for (int s = 0; s < 2; s++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int row = wm + i * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_NT4>(row) << 3);
                af[s][i] = *(const short8*)&Al[row * FBK + off];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int row = wn + j * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_NT4>(row) << 3);
                bfr[s][j] = *(const short8*)&Bl[row * FBK + off];
            }
        }
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[s][i], bfr[s][j], acc[i][j], 0, 0, 0);
        if (kt + 1 < nk) {
            if (kt + 2 < nk)
                asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    }
    __syncthreads();   // all waves done computing before epilogue staging

    // ---- epilogue: 128x256 tile via LDS, full-line stores ----
    ushort_t* Cp;
    long ldc;
    {
        const ushort_t* tmp;
        OpArg ca;
        ca.base = p.Cbase; ca.sin = p.Csin; ca.sout = p.Csout; ca.ld = p.Cld;
        ca.flags = p.Cflags;
        resolve_ptr2(ca, (const void* const*)p.Ctab, p.Ctabld, pid, p.nInner,
                     &tmp, &ldc);
        Cp = (ushort_t*)tmp;
    }
    const ushort_t* biasp = nullptr;
    if (p.has_bias)
        biasp = (const ushort_t*)p.bias_base
                + (long)(pid % p.nInner) * p.bias_sin
                + (long)(pid / p.nInner) * p.bias_sout;
    const float* csp = nullptr;
    if (p.has_colscale)
        csp = (const float*)p.colscale_base
              + (long)(pid % p.nInner) * p.cs_sin
              + (long)(pid / p.nInner) * p.cs_sout;
    const ushort_t* auxp = nullptr;
    if (p.epilogue == EPI_GELUGRAD)
        auxp = (const ushort_t*)p.aux_base
               + (long)(pid % p.nInner) * p.aux_sin
               + (long)(pid / p.nInner) * p.aux_sout;
    ushort_t* out2p = nullptr;
    if (p.epilogue == EPI_GELU_PAIR)
        out2p = (ushort_t*)p.out2 + (long)(pid % p.nInner) * p.out2_sin
                + (long)(pid / p.nInner) * p.out2_sout;

    float csv[4] = {1.f, 1.f, 1.f, 1.f};
    float bvv[4] = {0.f, 0.f, 0.f, 0.f};
    if (csp && p.epilogue != EPI_SMBWD) {
#pragma unroll
        for (int j16 = 0; j16 < 4; j16++)
            csv[j16] = csp[n0 + wn + j16 * 16 + lrow];
    }
    if (biasp) {
#pragma unroll
        for (int j16 = 0; j16 < 4; j16++)
            bvv[j16] = bf2f(biasp[n0 + wn + j16 * 16 + lrow]);
    }
#pragma unroll
    for (int i16 = 0; i16 < 4; i16++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            int li = wm + i16 * 16 + kq * 4 + r;           // 0..127
            long gi = m0 + li;
            float vv[4];
#pragma unroll
            for (int j16 = 0; j16 < 4; j16++)
                vv[j16] = acc[i16][j16][r] * p.alpha * csv[j16];
            if (auxp) {
                const ushort_t* auxrow = auxp + gi * p.aux_ld;
                ushort_t av[4];
#pragma unroll
                for (int j16 = 0; j16 < 4; j16++)
                    av[j16] = auxrow[n0 + wn + j16 * 16 + lrow];
                float gx[4], gy[4];
#pragma unroll
                for (int j16 = 0; j16 < 4; j16++) gx[j16] = bf2f(av[j16]);
                gelu_grad_vec<4>(gx, gy);
#pragma unroll
                for (int j16 = 0; j16 < 4; j16++) vv[j16] *= gy[j16];
            }
#pragma unroll
            for (int j16 = 0; j16 < 4; j16++) {
                int lj = wn + j16 * 16 + lrow;             // 0..255
                smem[li * EPI2_ROW + lj] = f2bf(vv[j16] + bvv[j16]);
            }
        }
    }
    __syncthreads();

    if (p.epilogue == EPI_SOFTMAX || p.epilogue == EPI_SMBWD) {
        // Full-row fusions: this tile holds complete rows (N == 256), so
        // the masked row softmax (fwd) / softmax backward (bwd) runs here
        // instead of a separate kernel + a global-memory round trip.
        // 4 consecutive threads (one quartet, same wave) own one row.
        int t = threadIdx.x;
        int li = t >> 2;
        int qt = (t & 3) * 64;
        long gi = m0 + li;
        const bool* mrow =
            p.nlmask ? (const bool*)p.nlmask + gi * p.N + n0 + qt : nullptr;
        ushort_t* srow = smem + li * EPI2_ROW + qt;
        const float SELF = bf2f(f2bf(-5e-4f));
        const float NEG = -3.3895314e38f;

        if (p.epilogue == EPI_SOFTMAX) {
            // pass 1: masks + quartet max
            float mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                union { uint4v v; ushort_t u[8]; } x;
                x.v = *(const uint4v*)(srow + c * 8);
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    int gj = n0 + qt + c * 8 + e;
                    float v = bf2f(x.u[e]);
                    if (p.self_mask && gj == gi) v = SELF;
                    if (mrow && mrow[c * 8 + e]) v = NEG;
                    x.u[e] = f2bf(v);
                    mx = fmaxf(mx, v);
                }
                *(uint4v*)(srow + c * 8) = x.v;   // masked values back
            }
            mx = fmaxf(mx, __shfl_xor(mx, 1));
            mx = fmaxf(mx, __shfl_xor(mx, 2));
            // pass 2: exp + quartet sum (store unnormalized bf16)
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                union { uint4v v; ushort_t u[8]; } x;
                x.v = *(const uint4v*)(srow + c * 8);
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    float ex = __expf(bf2f(x.u[e]) - mx);
                    sum += ex;
                    x.u[e] = f2bf(ex);
                }
                *(uint4v*)(srow + c * 8) = x.v;
            }
            sum += __shfl_xor(sum, 1);
            sum += __shfl_xor(sum, 2);
            float inv = 1.0f / sum;
            // pass 3: normalize; P goes to global AND stays in LDS for the
            // fused AV product below
            ushort_t* prow = Cp + gi * ldc + n0 + qt;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                union { uint4v v; ushort_t u[8]; } x;
                x.v = *(const uint4v*)(srow + c * 8);
#pragma unroll
                for (int e = 0; e < 8; e++)
                    x.u[e] = f2bf(bf2f(x.u[e]) * inv);
                *(uint4v*)(prow + c * 8) = x.v;
                *(uint4v*)(srow + c * 8) = x.v;
            }
            if (p.out2) {
                // ---- fused AV: O[i,:] = sum_j P[i,j] * V[j,:] ----
                // P: LDS [128][EPI2_ROW]; V: global rows via aux fields;
                // O: out2 fields; d passed in p.npatch. K = N = 256.
                __syncthreads();
                const ushort_t* Vp = (const ushort_t*)p.aux_base
                    + (long)(pid % p.nInner) * p.aux_sin
                    + (long)(pid / p.nInner) * p.aux_sout;
                const long ldv = p.aux_ld;
                ushort_t* Op = (ushort_t*)p.out2
                    + (long)(pid % p.nInner) * p.out2_sin
                    + (long)(pid / p.nInner) * p.out2_sout;
                const int dtot = p.npatch;
                // double-buffered transpose-staged V: stage s = (dc, jt)
                // loads the NEXT piece before this stage's MFMAs (VMEM in
                // flight under compute) and transpose-writes it into the
                // other buffer after them — one barrier per stage instead
                // of the single-buffered {stage, sync, mfma, sync} chain.
                ushort_t* Vt0 = smem + 128 * EPI2_ROW;  // [256][FBK] x2
                ushort_t* Vt1 = Vt0 + 256 * FBK;
                const int wrow = (wid >> 2) * 64;
                const int wcol64 = (wid & 3) * 64;
                const int nstage = ((dtot + 255) / 256) * 4;
                const int tt = threadIdx.x, cb = tt & 31, mb = tt >> 5;
                union Pc { uint4v v; ushort_t u[8]; };
                Pc rv[8];
                auto load_piece = [&](int st) {
                    if (tt < 256) {
                        int jt = st & 3, dc = (st >> 2) * 256;
#pragma unroll
                        for (int r = 0; r < 8; r++) {
                            int j = jt * 64 + mb * 8 + r;
                            int gc = dc + cb * 8;
                            if (gc + 7 < dtot)
                                rv[r].v = *(const uint4v*)(Vp
                                    + (long)j * ldv + gc);
                            else
                                rv[r].v = 0;
                        }
                    }
                };
                auto write_piece = [&](int st) {
                    if (tt < 256) {
                        ushort_t* Vt = (st & 1) ? Vt1 : Vt0;
#pragma unroll
                        for (int e = 0; e < 8; e++) {
                            Pc col;
#pragma unroll
                            for (int r = 0; r < 8; r++)
                                col.u[r] = rv[r].u[e];
                            int row = cb * 8 + e;
                            int off = (mb * 8) ^ (swz_row<SWZ_NT4_V>(row) << 3);
                            *(uint4v*)&Vt[row * FBK + off] = col.v;
                        }
                    }
                };
                f32x4 acc2[4][4] = {};
                load_piece(0);
                write_piece(0);
                __syncthreads();
                for (int st = 0; st < nstage; st++) {
                    if (st + 1 < nstage) load_piece(st + 1);
                    const ushort_t* Vt = (st & 1) ? Vt1 : Vt0;
                    const int jt = st & 3, dc = (st >> 2) * 256;
                    short8 paf[2][4], vbf[2][4];
#pragma unroll
                    for (int ss = 0; ss < 2; ss++) {
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            int row = wrow + i * 16 + lrow;
                            int koff = jt * 64 + ss * 32 + kq * 8;
                            paf[ss][i] = *(const short8*)&smem[
                                row * EPI2_ROW + koff];
                        }
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            int row = wcol64 + j * 16 + lrow;
                            int off = (ss * 32 + kq * 8)
                                      ^ (swz_row<SWZ_NT4_V>(row) << 3);
                            vbf[ss][j] = *(const short8*)&Vt[
                                row * FBK + off];
                        }
                    }
#pragma unroll
                    for (int ss = 0; ss < 2; ss++)
#pragma unroll
                        for (int i = 0; i < 4; i++)
#pragma unroll
                            for (int j = 0; j < 4; j++)
                                acc2[i][j] =
                                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                        paf[ss][i], vbf[ss][j],
                                        acc2[i][j], 0, 0, 0);
                    if (st + 1 < nstage) write_piece(st + 1);
                    if ((st & 3) == 3) {
                        // dc chunk complete: store O from registers
#pragma unroll
                        for (int i16 = 0; i16 < 4; i16++)
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                long oi = m0 + wrow + i16 * 16 + kq * 4 + r;
                                ushort_t* orow2 = Op + oi * p.out2_ld;
#pragma unroll
                                for (int j16 = 0; j16 < 4; j16++) {
                                    int oc = dc + wcol64 + j16 * 16 + lrow;
                                    if (oc < dtot)
                                        orow2[oc] = f2bf(acc2[i16][j16][r]);
                                    acc2[i16][j16][r] = 0.f;
                                }
                            }
                    }
                    __syncthreads();
                }
            }
        } else {
            // EPI_SMBWD: dS = alpha2 * P * (dP - sum(P*dP)), masked -> 0;
            // dSr = dS * rnorm[j]. P comes via aux, rnorm via colscale
            // pointers (phase 1 ran with alpha=1, no colscale).
            const ushort_t* Prow = (const ushort_t*)p.aux_base
                + (long)(pid % p.nInner) * p.aux_sin
                + (long)(pid / p.nInner) * p.aux_sout + gi * p.aux_ld
                + n0 + qt;
            const float* rn = (const float*)p.colscale_base
                + (long)(pid % p.nInner) * p.cs_sin
                + (long)(pid / p.nInner) * p.cs_sout + n0 + qt;
            float tsum = 0.f;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                union { uint4v v; ushort_t u[8]; } dp, pp;
                dp.v = *(const uint4v*)(srow + c * 8);
                pp.v = *(const uint4v*)(Prow + c * 8);
#pragma unroll
                for (int e = 0; e < 8; e++)
                    tsum += bf2f(pp.u[e]) * bf2f(dp.u[e]);
            }
            tsum += __shfl_xor(tsum, 1);
            tsum += __shfl_xor(tsum, 2);
            ushort_t* dsrow = Cp + gi * ldc + n0 + qt;
            ushort_t* dsr_row = (ushort_t*)p.out2
                + (long)(pid % p.nInner) * p.out2_sin
                + (long)(pid / p.nInner) * p.out2_sout + gi * p.out2_ld
                + n0 + qt;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                union { uint4v v; ushort_t u[8]; } dp, pp, o1, o2;
                dp.v = *(const uint4v*)(srow + c * 8);
                pp.v = *(const uint4v*)(Prow + c * 8);
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    int gj = n0 + qt + c * 8 + e;
                    float v = p.alpha2 * bf2f(pp.u[e])
                              * (bf2f(dp.u[e]) - tsum);
                    if (p.self_mask && gj == gi) v = 0.f;
                    if (mrow && mrow[c * 8 + e]) v = 0.f;
                    o1.u[e] = f2bf(v);
                    o2.u[e] = f2bf(v * rn[c * 8 + e]);
                }
                *(uint4v*)(dsrow + c * 8) = o1.v;
                *(uint4v*)(dsr_row + c * 8) = o2.v;
            }
        }
        return;
    }
    {
        int t = threadIdx.x;              // 512 threads: 128 rows x 4 qtrs
        int li = t >> 2;
        int qt = (t & 3) * 64;
        long gi = m0 + li;
        ushort_t* crow = Cp + gi * ldc + n0 + qt;
        ushort_t* orow = out2p ? out2p + gi * p.out2_ld + n0 + qt : nullptr;
        const ushort_t* srow = smem + li * EPI2_ROW + qt;
#pragma unroll
        for (int c = 0; c < 8; c++)
            *(uint4v*)(crow + c * 8) = *(const uint4v*)(srow + c * 8);
        if (orow) {
#pragma unroll
            for (int c = 0; c < 8; c++) {
                union { uint4v v; ushort_t u[8]; } x, g;
                x.v = *(const uint4v*)(srow + c * 8);
                if (p.epilogue == 10) {
                    g.v = x.v;
                } else if (p.epilogue == 12) {      // debug: poly, no trans
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        float xv = bf2f(x.u[e]);
                        g.u[e] = f2bf(xv * (0.5f + 0.1f * xv));
                    }
                } else {
                    float xin[8], yv[8];
#pragma unroll
                    for (int e = 0; e < 8; e++) xin[e] = bf2f(x.u[e]);
                    gelu_f_vec<8>(xin, yv);
#pragma unroll
                    for (int e = 0; e < 8; e++) g.u[e] = f2bf(yv[e]);
                }
                *(uint4v*)(orow + c * 8) = g.v;
            }
        }
    }
    if (p.colsum_out) {
        // fused bias-grad: this tile's column sums (C values still live in
        // the LDS staging image) stored as this row tile's f32 partial
        float* outp = p.colsum_out + (long)(pid % p.nInner) * p.colsum_sin;
        int c = threadIdx.x;
        if (c < BN3) {
            float ssum = 0.f;
            for (int r = 0; r < 128; r++)
                ssum += bf2f(smem[r * EPI2_ROW + c]);
            colsum_store(outp, p.N, m0, BM / 64, n0 + c, ssum);
        }
    }
}


void launch_gemm_nt_fast4(const GemmParams& p, hipStream_t stream) {
    dim3 grid(p.N / BN3, p.M / BM, p.nproblems);
    hipLaunchKernelGGL(gemm_nt_fast4_kernel, grid, dim3(NT3), 0, stream, p);
}


// ------- wide register epilogue (shared by nt5p and nt8p) -------
// The MFMA C fragment of a 16x64 wave slab puts, in lane (kq, lrow),
// register r of fragment j16 at row 4*kq+r, column j16*16+lrow: stored
// directly that is one 2-byte access per lane and value. These helpers
// re-lay out the ALREADY ROUNDED bf16 values (pure data movement, so every
// stored bit and the f32 column sums are untouched) into 16 contiguous
// bytes per lane:
//   1. quad transpose (2 DPP quad_perm + 4 v_perm per fragment): lane
//      lrow = 4c+q trades its 4 rows of one column for row 4*kq+q,
//      columns 4c..4c+3 (the transpose is its own inverse);
//   2. lane-xor-4 exchange across a fragment pair (2P, 2P+1) (row_shr:4 /
//      row_shl:4 with a bank mask, 2 DPP per dword): even c keeps fragment
//      2P and receives lane c+1's half of it, odd c the same for 2P+1.
// Lane (kq, 4c+q) then owns row 4*kq+q, slab columns
// (2P + (c&1))*16 + (c>>1)*8 .. +7: one 16-byte access per (lane, P), 8 per
// 128x256-tile output instead of 64. The reverse direction turns 16-byte
// loads of the aux operand back into the fragment layout.
struct WideEpi {
    unsigned selA, selB, sel0, sel1;   // per-lane v_perm selectors
    bool qhi;                          // lane's q has bit 1 set
    int row;                           // row within the 16-row slab
    int col0;                          // slab column of pair 0's 8 values
    __device__ __forceinline__ WideEpi(int lane) {
        const int q = lane & 3, c = (lane >> 2) & 3;
        qhi = q & 2;
        selA = (q & 1) ? 0x05040100u : 0x07060302u;
        selB = (q & 1) ? 0x07060302u : 0x05040100u;
        sel0 = q == 0 ? 0x01000504u : q == 1 ? 0x05040100u
             : q == 2 ? 0x03020706u : 0x07060302u;
        sel1 = q == 0 ? 0x03020706u : q == 1 ? 0x07060302u
             : q == 2 ? 0x01000504u : 0x05040100u;
        row = (lane >> 4) * 4 + q;
        col0 = (c & 1) * 16 + (c >> 1) * 8;
    }
    // 4x4 transpose of 16-bit values across a lane quad. In: p0 = regs
    // (0,1), p1 = regs (2,3) packed low|high. Out: d0 = (0,1), d1 = (2,3)
    // of the transposed matrix.
    __device__ __forceinline__ void quad_tr(unsigned p0, unsigned p1,
                                            unsigned& d0, unsigned& d1) const {
        unsigned send = qhi ? p0 : p1, keep = qhi ? p1 : p0;
        unsigned recv = __builtin_amdgcn_mov_dpp(send, 0x4E, 0xf, 0xf, true);
        unsigned send2 = __builtin_amdgcn_perm(recv, keep, selA);
        unsigned own2 = __builtin_amdgcn_perm(recv, keep, selB);
        unsigned rb = __builtin_amdgcn_mov_dpp(send2, 0xB1, 0xf, 0xf, true);
        d0 = __builtin_amdgcn_perm(own2, rb, sel0);
        d1 = __builtin_amdgcn_perm(own2, rb, sel1);
    }
    // fragment -> rows: v[r][j16] (bf16 bits) -> out[P], P = 0,1
    __device__ __forceinline__ void to_rows(const ushort_t v[4][4],
                                            uint4v out[2]) const {
        unsigned d0[4], d1[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            quad_tr(v[0][j] | ((unsigned)v[1][j] << 16),
                    v[2][j] | ((unsigned)v[3][j] << 16), d0[j], d1[j]);
#pragma unroll
        for (int P = 0; P < 2; P++) {
            const int e = 2 * P, o = 2 * P + 1;
            // low 8 bytes: own even fragment / lane-4's odd fragment;
            // high 8 bytes: lane+4's even fragment / own odd fragment
            out[P][0] = __builtin_amdgcn_update_dpp(d0[e], d0[o], 0x114,
                                                    0xf, 0xA, false);
            out[P][1] = __builtin_amdgcn_update_dpp(d1[e], d1[o], 0x114,
                                                    0xf, 0xA, false);
            out[P][2] = __builtin_amdgcn_update_dpp(d0[o], d0[e], 0x104,
                                                    0xf, 0x5, false);
            out[P][3] = __builtin_amdgcn_update_dpp(d1[o], d1[e], 0x104,
                                                    0xf, 0x5, false);
        }
    }
    // `p` = this lane's (row, col0) element of the slab in a row-major
    // bf16 matrix, 16-byte aligned: two 16-byte accesses per lane and slab
    __device__ __forceinline__ void store(ushort_t* p,
                                          const ushort_t v[4][4]) const {
        uint4v w[2];
        to_rows(v, w);
        *(uint4v*)p = w[0];
        *(uint4v*)(p + 32) = w[1];
    }
    __device__ __forceinline__ void load(const ushort_t* p,
                                         uint4v w[2]) const {
        w[0] = *(const uint4v*)p;
        w[1] = *(const uint4v*)(p + 32);
    }
    // rows -> fragment (inverse of to_rows)
    __device__ __forceinline__ void to_frag(const uint4v in[2],
                                            ushort_t v[4][4]) const {
#pragma unroll
        for (int P = 0; P < 2; P++) {
            unsigned de0 = __builtin_amdgcn_update_dpp(in[P][0], in[P][2],
                                                       0x114, 0xf, 0xA, false);
            unsigned de1 = __builtin_amdgcn_update_dpp(in[P][1], in[P][3],
                                                       0x114, 0xf, 0xA, false);
            unsigned do0 = __builtin_amdgcn_update_dpp(in[P][2], in[P][0],
                                                       0x104, 0xf, 0x5, false);
            unsigned do1 = __builtin_amdgcn_update_dpp(in[P][3], in[P][1],
                                                       0x104, 0xf, 0x5, false);
            unsigned p0, p1;
            quad_tr(de0, de1, p0, p1);
            v[0][2 * P] = (ushort_t)p0; v[1][2 * P] = (ushort_t)(p0 >> 16);
            v[2][2 * P] = (ushort_t)p1; v[3][2 * P] = (ushort_t)(p1 >> 16);
            quad_tr(do0, do1, p0, p1);
            v[0][2 * P + 1] = (ushort_t)p0;
            v[1][2 * P + 1] = (ushort_t)(p0 >> 16);
            v[2][2 * P + 1] = (ushort_t)p1;
            v[3][2 * P + 1] = (ushort_t)(p1 >> 16);
        }
    }
};


// ------- persistent continuous-ring NT variant (nt5p) -------
// Each block sweeps PERSIST consecutive 128-row M-tiles of ONE 256-col
// N-column. The 3-ring never drains at tile boundaries (the global step
// stream g = tile*nk + kt staggers straight across tiles), so the per-tile
// prologue cost — ~50% of a K=512 block in nt4 (profiles/README
// K-amortization) — is paid once per PERSIST tiles. The epilogue runs from
// registers (no LDS image — the ring owns the arena) in the shadow of the
// next tile's MFMAs: 2-byte fragment-order accesses, or, per the WIDE
// template bits, 16-byte ones after an in-register transpose (WideEpi).
// Supports alpha/bias/colscale, GELUGRAD, GELU_PAIR, GELU and the fused f32
// colsum (one partial store per wave half/column/tile); no softmax/table-C
// epilogues — the dispatcher routes those to nt4.
// WIDE (GemmParams::wide_epi): bit 0 = 16-byte C / out2 stores, bit 1 =
// 16-byte aux loads issued ahead of the tile-end MFMAs; 0 = the 2-byte
// fragment-order epilogue. All give identical bits.
template <int PERSIST, int WIDE>
__global__ __launch_bounds__(NT3) void gemm_nt_fast5p_kernel(GemmParams p) {
    __shared__ ushort_t smem[3 * (128 + 256) * FBK];   // 144 KiB, 3-ring
    const int abuf = 128 * FBK, bbuf = 256 * FBK, stride = abuf + bbuf;

    const int pid = blockIdx.z;
    int nwg = gridDim.x * gridDim.y;
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, off = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + off;
    }
    const int n0 = (bid / gridDim.y) * BN3;
    const int m0 = (bid % gridDim.y) * (BM * PERSIST);

    const ushort_t* Ap;
    const ushort_t* Bp;
    long lda, ldb;
    resolve_ptr2(p.A, p.Atab, p.Atabld, pid, p.nInner, &Ap, &lda);
    resolve_ptr2(p.B, p.Btab, p.Btabld, pid, p.nInner, &Bp, &ldb);

    ushort_t* Cp;
    long ldc;
    {
        const ushort_t* tmp;
        OpArg ca;
        ca.base = p.Cbase; ca.sin = p.Csin; ca.sout = p.Csout; ca.ld = p.Cld;
        ca.flags = p.Cflags;
        resolve_ptr2(ca, (const void* const*)p.Ctab, p.Ctabld, pid, p.nInner,
                     &tmp, &ldc);
        Cp = (ushort_t*)tmp;
    }
    const ushort_t* biasp = nullptr;
    if (p.has_bias)
        biasp = (const ushort_t*)p.bias_base
                + (long)(pid % p.nInner) * p.bias_sin
                + (long)(pid / p.nInner) * p.bias_sout;
    const float* csp = nullptr;
    if (p.has_colscale)
        csp = (const float*)p.colscale_base
              + (long)(pid % p.nInner) * p.cs_sin
              + (long)(pid / p.nInner) * p.cs_sout;
    const ushort_t* auxp = nullptr;
    if (p.epilogue == EPI_GELUGRAD)
        auxp = (const ushort_t*)p.aux_base
               + (long)(pid % p.nInner) * p.aux_sin
               + (long)(pid / p.nInner) * p.aux_sout;
    float* colp = nullptr;
    if (p.colsum_out)
        colp = p.colsum_out + (long)(pid % p.nInner) * p.colsum_sin;
    ushort_t* o2p = nullptr;   // EPI_GELU_PAIR: gelu(pre-act) output
    if (p.epilogue == EPI_GELU_PAIR && p.out2)
        o2p = (ushort_t*)p.out2 + (long)(pid % p.nInner) * p.out2_sin
              + (long)(pid / p.nInner) * p.out2_sout;
    // EPI_GELU: C itself gets gelu(bf16 pre-act), the pre-act is not kept
    const bool gelu_c = p.epilogue == EPI_GELU;

    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int wm = (wid >> 2) * 64;
    const int wn = (wid & 3) * 64;
    const int lrow = lane & 15;
    const int kq = lane >> 4;
    const WideEpi we(lane);

    float csv[4] = {1.f, 1.f, 1.f, 1.f};
    float bvv[4] = {0.f, 0.f, 0.f, 0.f};
    if (csp) {
#pragma unroll
        for (int j16 = 0; j16 < 4; j16++)
            csv[j16] = csp[n0 + wn + j16 * 16 + lrow];
    }
    if (biasp) {
#pragma unroll
        for (int j16 = 0; j16 < 4; j16++)
            bvv[j16] = bf2f(biasp[n0 + wn + j16 * 16 + lrow]);
    }

    f32x4 acc[4][4] = {};

    const int nk = p.K / FBK;
    const int TOT = PERSIST * nk;
    auto stage_g = [&](int buf, int g) {
        const int mt0 = m0 + (g / nk) * BM;
        const int k0 = (g % nk) * FBK;
        ushort_t* Al = smem + buf * stride;
        ushort_t* Bl = Al + abuf;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            int chunk = wid * 2 + c;
            int row = chunk * 8 + (lane >> 3);
            int swz8 = ((lane & 7) ^ swz_row<SWZ_NT5P>(row)) * 8;
            const ushort_t* g_ = Ap + (long)(mt0 + row) * lda + k0 + swz8;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) unsigned int*)g_,
                (__attribute__((address_space(3))) unsigned int*)
                    (Al + chunk * 512), 16, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            int chunk = wid * 4 + c;
            int row = chunk * 8 + (lane >> 3);
            int swz8 = ((lane & 7) ^ swz_row<SWZ_NT5P>(row)) * 8;
            const ushort_t* g_ = Bp + (long)(n0 + row) * ldb + k0 + swz8;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) unsigned int*)g_,
                (__attribute__((address_space(3))) unsigned int*)
                    (Bl + chunk * 512), 16, 0, 0);
        }
    };

    stage_g(0, 0);
    if (TOT > 1) stage_g(1, 1);
    if (TOT > 1)
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    for (int g = 0; g < TOT; g++) {
        const bool tile_end = (g % nk) == nk - 1;
        // vmcnt retires IN ISSUE ORDER, so at tile-end steps the next
        // stage's glds must be issued AFTER the epilogue stores: the
        // bottom vmcnt(6) then covers [g+1 glds, stores] and leaves g+2's
        // glds in flight. Stores retire once their data leaves the VGPRs
        // (no memory round trip), so that wait stays cheap.
        if (!tile_end && g + 2 < TOT) stage_g((g + 2) % 3, g + 2);
        // Wide epilogue, EPI_GELUGRAD: all 8 16-byte aux loads of this tile
        // go out here, ahead of the step's MFMAs, which hide their latency.
        // Issue order at a tile_end step is then [g+1 glds (previous
        // step), aux loads, C stores, g+2 glds]: the compiler's wait for
        // the aux data retires g+1's glds a little early (they were issued
        // a whole step ago), and the bottom vmcnt(6) still covers
        // everything up to the stores and leaves exactly g+2's 6 glds in
        // flight, as before.
        uint4v auxw[4][2];
        if ((WIDE & 2) && tile_end && auxp) {
            const ushort_t* abase =
                auxp + (m0 + (long)(g / nk) * BM + wm + we.row) * p.aux_ld
                + n0 + wn + we.col0;
#pragma unroll
            for (int i16 = 0; i16 < 4; i16++)
                we.load(abase + (long)(i16 * 16) * p.aux_ld, auxw[i16]);
        }
        const ushort_t* Al = smem + (g % 3) * stride;
        const ushort_t* Bl = Al + abuf;
        short8 af[2][4], bfr[2][4];
#pragma unroll
        for (int s = 0; s < 2; s++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int row = wm + i * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_NT5P>(row) << 3);
                af[s][i] = *(const short8*)&Al[row * FBK + off];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int row = wn + j * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_NT5P>(row) << 3);
                bfr[s][j] = *(const short8*)&Bl[row * FBK + off];
            }
        }
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[s][i], bfr[s][j], acc[i][j], 0, 0, 0);

        if (tile_end) {
            // tile done: drain it from registers while the ring streams the
            // next tile
            const long mt0 = m0 + (long)(g / nk) * BM;
            float colacc[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (WIDE) {
                // same arithmetic, same (i16, r) order into colacc as the
                // narrow path below; only the rounded bf16 values are
                // re-laid out (WideEpi) so each lane moves 16 bytes
#pragma unroll
                for (int i16 = 0; i16 < 4; i16++) {
                    ushort_t avv[4][4], cbv[4][4], obv[4][4];
                    if (auxp) {
                        if constexpr (WIDE & 2) {
                            we.to_frag(auxw[i16], avv);
                        } else {
                            const ushort_t* ap =
                                auxp + (mt0 + wm + i16 * 16 + kq * 4)
                                       * p.aux_ld + n0 + wn + lrow;
#pragma unroll
                            for (int r = 0; r < 4; r++)
#pragma unroll
                                for (int j16 = 0; j16 < 4; j16++)
                                    avv[r][j16] =
                                        ap[r * p.aux_ld + j16 * 16];
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        float vv[4];
#pragma unroll
                        for (int j16 = 0; j16 < 4; j16++)
                            vv[j16] = acc[i16][j16][r] * p.alpha * csv[j16];
                        if (auxp) {
                            float gx[4], gy[4];
#pragma unroll
                            for (int j16 = 0; j16 < 4; j16++)
                                gx[j16] = bf2f(avv[r][j16]);
                            gelu_grad_vec<4>(gx, gy);
#pragma unroll
                            for (int j16 = 0; j16 < 4; j16++)
                                vv[j16] *= gy[j16];
                        }
#pragma unroll
                        for (int j16 = 0; j16 < 4; j16++) {
                            ushort_t cb = f2bf(vv[j16] + bvv[j16]);
                            colacc[j16] += bf2f(cb);
                            cbv[r][j16] = cb;
                        }
                        if (o2p || gelu_c) {
                            float gx[4], gy[4];
#pragma unroll
                            for (int j16 = 0; j16 < 4; j16++)
                                gx[j16] = bf2f(cbv[r][j16]);
                            gelu_f_vec<4>(gx, gy);
#pragma unroll
                            for (int j16 = 0; j16 < 4; j16++)
                                obv[r][j16] = f2bf(gy[j16]);
                        }
                        acc[i16][0][r] = 0.f; acc[i16][1][r] = 0.f;
                        acc[i16][2][r] = 0.f; acc[i16][3][r] = 0.f;
                    }
                    if constexpr (WIDE & 1) {
                        const long gi = mt0 + wm + i16 * 16 + we.row;
                        const long cj = n0 + wn + we.col0;
                        if (!gelu_c) we.store(Cp + gi * ldc + cj, cbv);
                        if (o2p || gelu_c)
                            we.store(gelu_c ? Cp + gi * ldc + cj
                                            : o2p + gi * p.out2_ld + cj,
                                     obv);
                    } else {
                        // wide aux loads only: fragment-order stores
                        const long gi = mt0 + wm + i16 * 16 + kq * 4;
                        const long cj = n0 + wn + lrow;
#pragma unroll
                        for (int r = 0; r < 4; r++)
#pragma unroll
                            for (int j16 = 0; j16 < 4; j16++) {
                                if (!gelu_c)
                                    Cp[(gi + r) * ldc + cj + j16 * 16] =
                                        cbv[r][j16];
                                if (gelu_c)
                                    Cp[(gi + r) * ldc + cj + j16 * 16] =
                                        obv[r][j16];
                                else if (o2p)
                                    o2p[(gi + r) * p.out2_ld + cj
                                        + j16 * 16] = obv[r][j16];
                            }
                    }
                }
            } else {
#pragma unroll
            for (int i16 = 0; i16 < 4; i16++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    long gi = mt0 + wm + i16 * 16 + kq * 4 + r;
                    float vv[4];
#pragma unroll
                    for (int j16 = 0; j16 < 4; j16++)
                        vv[j16] = acc[i16][j16][r] * p.alpha * csv[j16];
                    if (auxp) {
                        const ushort_t* auxrow = auxp + gi * p.aux_ld;
                        ushort_t av[4];
#pragma unroll
                        for (int j16 = 0; j16 < 4; j16++)
                            av[j16] = auxrow[n0 + wn + j16 * 16 + lrow];
                        float gx[4], gy[4];
#pragma unroll
                        for (int j16 = 0; j16 < 4; j16++)
                            gx[j16] = bf2f(av[j16]);
                        gelu_grad_vec<4>(gx, gy);
#pragma unroll
                        for (int j16 = 0; j16 < 4; j16++) vv[j16] *= gy[j16];
                    }
                    ushort_t* crow = Cp + gi * ldc + n0 + wn + lrow;
                    ushort_t cbv[4];
#pragma unroll
                    for (int j16 = 0; j16 < 4; j16++) {
                        ushort_t cb = f2bf(vv[j16] + bvv[j16]);
                        // colsum over the bf16-ROUNDED stored values,
                        // matching the LDS-epilogue colsum bit for bit
                        // per summand (only the fixed add order differs)
                        colacc[j16] += bf2f(cb);
                        cbv[j16] = cb;
                        if (!gelu_c) crow[j16 * 16] = cb;
                    }
                    if (o2p || gelu_c) {
                        // gelu of the bf16-rounded pre-activation:
                        // bitwise the standalone k_gelu pass
                        float gx[4], gy[4];
#pragma unroll
                        for (int j16 = 0; j16 < 4; j16++)
                            gx[j16] = bf2f(cbv[j16]);
                        gelu_f_vec<4>(gx, gy);
                        ushort_t* orow = gelu_c
                            ? crow
                            : o2p + gi * p.out2_ld + n0 + wn + lrow;
#pragma unroll
                        for (int j16 = 0; j16 < 4; j16++)
                            orow[j16 * 16] = f2bf(gy[j16]);
                    }
                    acc[i16][0][r] = 0.f; acc[i16][1][r] = 0.f;
                    acc[i16][2][r] = 0.f; acc[i16][3][r] = 0.f;
                }
            }
            }
            if (colp) {
                // this wave's 64 rows: fold the 4 kq lane groups, one store
#pragma unroll
                for (int j16 = 0; j16 < 4; j16++) {
                    float cs = kq_sum(colacc[j16]);
                    if (kq == 0)
                        colsum_store(colp, p.N, mt0 + wm, 1,
                                     n0 + wn + j16 * 16 + lrow, cs);
                }
            }
            if (g + 2 < TOT) stage_g((g + 2) % 3, g + 2);
        }

        if (g + 1 < TOT) {
            if (g + 2 < TOT)
                asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    }
}

void launch_gemm_nt_fast5p(const GemmParams& p, hipStream_t stream) {
    // sweep depth: 4 by default (dispatcher guarantees M % 512 == 0);
    // GLOM_NT5P_P=8 selects the deeper sweep when M allows it
    static const int pref = []() {
        const char* e = getenv("GLOM_NT5P_P");
        return e ? atoi(e) : 0;
    }();
    const int P = (pref == 8 && p.M % (BM * 8) == 0) ? 8
                : (pref == 2) ? 2 : 4;
    dim3 grid(p.N / BN3, p.M / (BM * P), p.nproblems);
    // without an aux operand bit 1 means nothing; wide stores with narrow
    // aux loads (1) is not built: nothing measured in its favour
    const bool has_aux = p.epilogue == EPI_GELUGRAD;
    const int wide = !has_aux ? ((p.wide_epi & 1) ? 3 : 0)
                   : (p.wide_epi & 2) ? (p.wide_epi & 3) : 0;
#define NT5P_LAUNCH(PP)                                                     \
    do {                                                                    \
        if (wide == 3)                                                      \
            hipLaunchKernelGGL((gemm_nt_fast5p_kernel<PP, 3>), grid,        \
                               dim3(NT3), 0, stream, p);                    \
        else if (wide == 2)                                                 \
            hipLaunchKernelGGL((gemm_nt_fast5p_kernel<PP, 2>), grid,        \
                               dim3(NT3), 0, stream, p);                    \
        else                                                                \
            hipLaunchKernelGGL((gemm_nt_fast5p_kernel<PP, 0>), grid,        \
                               dim3(NT3), 0, stream, p);                    \
    } while (0)
    if (P == 8)
        NT5P_LAUNCH(8);
    else if (P == 2)
        NT5P_LAUNCH(2);
    else
        NT5P_LAUNCH(4);
#undef NT5P_LAUNCH
}



// --------------------------------------------------------------------- //
// gemm_nt_fast8p: 256x256x64 tile, 8 waves (2M x 4N, 128x64 per wave),
// guide §5 "256² 8-phase template" schedule: the K-step is split into 4
// phases of {ds_read subtile || 2 global_load_lds -> barrier ->
// setprio(1) 16xMFMA setprio(0) -> counted per-wave vmcnt -> barrier}.
// 2 full-tile LDS buffers (128 KiB, 1 block/CU); each wave stages ONLY
// the data it will itself read (its B quarter + the A mfrag-pair of its
// wn slot), ordered B-first, so the counted waits leave later-needed
// halves in flight across phase barriers (T3+T4) and the phase split
// gives setprio something to arbitrate (T5).
//
// Per-wave wait schedule (steady state; derivation in-line):
//   end of phase 0: wave wn==1 waits vmcnt(2)   (its A(t) share)
//   end of phase 1: wave wn==2 waits vmcnt(4)
//   end of phase 2: wave wn==3 waits vmcnt(6)
//   end of phase 3: wave wn==0 waits vmcnt(0), others vmcnt(4)
// When the next tile is not staged (last K-tile) the protecting counts
// drop to 0/0/0/0 (nothing newer in the queue to leave in flight).

#define BM8 256
#define BN8 256
#define NT8 512

template <bool WIDE>
__global__ __launch_bounds__(NT8) void gemm_nt_fast8p_kernel(GemmParams p) {
    __shared__ ushort_t smem[2 * (BM8 + BN8) * FBK];   // 128 KiB
    const int abuf = BM8 * FBK, stride = (BM8 + BN8) * FBK;

    const int pid = blockIdx.z;
    int nwg = gridDim.x * gridDim.y;
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, off = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + off;
    }
    const int n0 = (bid / gridDim.y) * BN8;   // column-major: n outer
    const int m0 = (bid % gridDim.y) * BM8;

    const ushort_t* Ap;
    const ushort_t* Bp;
    long lda, ldb;
    resolve_ptr2(p.A, p.Atab, p.Atabld, pid, p.nInner, &Ap, &lda);
    resolve_ptr2(p.B, p.Btab, p.Btabld, pid, p.nInner, &Bp, &ldb);

    ushort_t* Cp;
    long ldc;
    {
        const ushort_t* tmp;
        OpArg ca;
        ca.base = p.Cbase; ca.sin = p.Csin; ca.sout = p.Csout; ca.ld = p.Cld;
        ca.flags = p.Cflags;
        resolve_ptr2(ca, (const void* const*)p.Ctab, p.Ctabld, pid, p.nInner,
                     &tmp, &ldc);
        Cp = (ushort_t*)tmp;
    }
    const ushort_t* biasp = nullptr;
    if (p.has_bias)
        biasp = (const ushort_t*)p.bias_base
                + (long)(pid % p.nInner) * p.bias_sin
                + (long)(pid / p.nInner) * p.bias_sout;
    const float* csp = nullptr;
    if (p.has_colscale)
        csp = (const float*)p.colscale_base
              + (long)(pid % p.nInner) * p.cs_sin
              + (long)(pid / p.nInner) * p.cs_sout;
    const ushort_t* auxp = nullptr;
    if (p.epilogue == EPI_GELUGRAD)
        auxp = (const ushort_t*)p.aux_base
               + (long)(pid % p.nInner) * p.aux_sin
               + (long)(pid / p.nInner) * p.aux_sout;
    float* colp = nullptr;
    if (p.colsum_out)
        colp = p.colsum_out + (long)(pid % p.nInner) * p.colsum_sin;

    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int whalf = wid >> 2;          // A half (0: rows 0-127, 1: 128-255)
    const int wq = wid & 3;              // B quarter / A stage slot
    const int wm = whalf * 128;
    const int wn = wq * 64;
    const int lrow = lane & 15;
    const int kq = lane >> 4;

    float csv[4] = {1.f, 1.f, 1.f, 1.f};
    float bvv[4] = {0.f, 0.f, 0.f, 0.f};
    if (csp) {
#pragma unroll
        for (int j16 = 0; j16 < 4; j16++)
            csv[j16] = csp[n0 + wn + j16 * 16 + lrow];
    }
    if (biasp) {
#pragma unroll
        for (int j16 = 0; j16 < 4; j16++)
            bvv[j16] = bf2f(biasp[n0 + wn + j16 * 16 + lrow]);
    }

    f32x4 acc[8][4] = {};

    // Stage 2 chunks (16 rows, 2 glds/thread) of this wave's OWN data.
    // part 0/1: B quarter rows [wq*64 + whalf*32 + 16*part)
    // part 2/3: A mfrag-pair rows [whalf*128 + wq*32 + 16*(part-2))
    auto stage2 = [&](int buf, int k0, int part) {
        ushort_t* img;
        int row0;
        if (part < 2) {
            img = smem + buf * stride + abuf;            // B image
            row0 = wq * 64 + whalf * 32 + part * 16;
        } else {
            img = smem + buf * stride;                    // A image
            row0 = whalf * 128 + wq * 32 + (part - 2) * 16;
        }
        const ushort_t* src = (part < 2 ? Bp : Ap);
        const long ld = (part < 2 ? ldb : lda);
        const int g0 = (part < 2 ? n0 : m0);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            int row = row0 + c * 8 + (lane >> 3);
            int swz8 = ((lane & 7) ^ swz_row<SWZ_NT8P>(row)) * 8;
            const ushort_t* g = src + (long)(g0 + row) * ld + k0 + swz8;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) unsigned int*)g,
                (__attribute__((address_space(3))) unsigned int*)
                    (img + (row >> 3) * 512), 16, 0, 0);
        }
    };

    const int nk = p.K / FBK;
    // prologue: stage tile 0 fully, drain, enter the loop (tile t's
    // phases stage tile t+1 into the buffer freed at the end of t-1)
#pragma unroll
    for (int part = 0; part < 4; part++) stage2(0, 0, part);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    for (int t = 0; t < nk; t++) {
        const ushort_t* Al = smem + (t & 1) * stride;
        const ushort_t* Bl = Al + abuf;
        const bool more = (t + 1) < nk;   // staging tile t+1 this pass
        short8 bfrag[2][4];
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int row = wn + j * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_NT8P>(row) << 3);
                bfrag[s][j] = *(const short8*)&Bl[row * FBK + off];
            }
#pragma unroll
        for (int ph = 0; ph < 4; ph++) {
            short8 af[2][2];
#pragma unroll
            for (int s = 0; s < 2; s++)
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    int row = wm + (2 * ph + i) * 16 + lrow;
                    int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_NT8P>(row) << 3);
                    af[s][i] = *(const short8*)&Al[row * FBK + off];
                }
            if (more) stage2((t + 1) & 1, (t + 1) * FBK, ph);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int s = 0; s < 2; s++)
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        acc[2 * ph + i][j] =
                            __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                af[s][i], bfrag[s][j], acc[2 * ph + i][j],
                                0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            // per-wave counted wait protecting the NEXT phase's ds_reads
            if (ph < 3) {
                if (__builtin_amdgcn_readfirstlane(wq) == ph + 1) {
                    if (!more)
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    else if (ph == 0)
                        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                    else if (ph == 1)
                        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else
                        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                }
            } else if (t + 1 < nk) {
                // tile boundary: everyone needs B(t+1); wn==0 also its
                // A(t+1) mfrag 0-1 share (the last 4 it issued)
                if (__builtin_amdgcn_readfirstlane(wq) == 0)
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else
                    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
        }
    }

    // ------------- register epilogue (mirrors nt5p, 8 mfrags) ----------
    float colacc[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (WIDE) {
        // nt5p's wide epilogue; the accumulators fill the register file
        // here, so aux is fetched one 16-row slab ahead, not a tile ahead
        const WideEpi we(lane);
        const long gi0 = (long)m0 + wm + we.row;
        const long cj = n0 + wn + we.col0;
        uint4v auxw[2][2];
        if (auxp) we.load(auxp + gi0 * p.aux_ld + cj, auxw[0]);
#pragma unroll
        for (int i16 = 0; i16 < 8; i16++) {
            ushort_t avv[4][4], cbv[4][4];
            if (auxp) {
                if (i16 + 1 < 8)
                    we.load(auxp + (gi0 + (i16 + 1) * 16) * p.aux_ld + cj,
                            auxw[(i16 + 1) & 1]);
                we.to_frag(auxw[i16 & 1], avv);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float vv[4];
#pragma unroll
                for (int j16 = 0; j16 < 4; j16++)
                    vv[j16] = acc[i16][j16][r] * p.alpha * csv[j16];
                if (auxp) {
                    float gx[4], gy[4];
#pragma unroll
                    for (int j16 = 0; j16 < 4; j16++)
                        gx[j16] = bf2f(avv[r][j16]);
                    gelu_grad_vec<4>(gx, gy);
#pragma unroll
                    for (int j16 = 0; j16 < 4; j16++) vv[j16] *= gy[j16];
                }
#pragma unroll
                for (int j16 = 0; j16 < 4; j16++) {
                    ushort_t cb = f2bf(vv[j16] + bvv[j16]);
                    colacc[j16] += bf2f(cb);
                    cbv[r][j16] = cb;
                }
            }
            we.store(Cp + (gi0 + i16 * 16) * ldc + cj, cbv);
        }
    } else {
#pragma unroll
    for (int i16 = 0; i16 < 8; i16++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            long gi = m0 + wm + i16 * 16 + kq * 4 + r;
            float vv[4];
#pragma unroll
            for (int j16 = 0; j16 < 4; j16++)
                vv[j16] = acc[i16][j16][r] * p.alpha * csv[j16];
            if (auxp) {
                const ushort_t* auxrow = auxp + gi * p.aux_ld;
                float gx[4], gy[4];
#pragma unroll
                for (int j16 = 0; j16 < 4; j16++)
                    gx[j16] = bf2f(auxrow[n0 + wn + j16 * 16 + lrow]);
                gelu_grad_vec<4>(gx, gy);
#pragma unroll
                for (int j16 = 0; j16 < 4; j16++) vv[j16] *= gy[j16];
            }
            ushort_t* crow = Cp + gi * ldc + n0 + wn + lrow;
#pragma unroll
            for (int j16 = 0; j16 < 4; j16++) {
                ushort_t cb = f2bf(vv[j16] + bvv[j16]);
                colacc[j16] += bf2f(cb);
                crow[j16 * 16] = cb;
            }
        }
    }
    }
    if (colp) {
        // this wave's 128 rows: fold the 4 kq lane groups, one store
#pragma unroll
        for (int j16 = 0; j16 < 4; j16++) {
            float cs = kq_sum(colacc[j16]);
            if (kq == 0)
                colsum_store(colp, p.N, (long)m0 + wm, 2,
                             n0 + wn + j16 * 16 + lrow, cs);
        }
    }
}

void launch_gemm_nt_fast8p(const GemmParams& p, hipStream_t stream) {
    dim3 grid(p.N / BN8, p.M / BM8, p.nproblems);
    if (p.wide_epi)
        hipLaunchKernelGGL(gemm_nt_fast8p_kernel<true>, grid, dim3(NT8), 0,
                           stream, p);
    else
        hipLaunchKernelGGL(gemm_nt_fast8p_kernel<false>, grid, dim3(NT8), 0,
                           stream, p);
}

// ------- split-K-only TN variant (32 KiB arena, 4 blocks/CU) -------
__global__ __launch_bounds__(NTHREADS) void gemm_tn_sk_kernel(GemmParams p) {
    __shared__ ushort_t smem[2 * BM * FBK];   // 32 KiB: 4 blocks/CU
    ushort_t* As = smem;
    ushort_t* Bs = smem + BM * FBK;

    int pid = blockIdx.z;
    int slice = 0, k_begin = 0, k_end = p.K;
    if (p.splitk > 1) {
        pid = blockIdx.z % p.nproblems;
        slice = blockIdx.z / p.nproblems;
        int per = ((p.K + FBK - 1) / FBK + p.splitk - 1) / p.splitk * FBK;
        k_begin = slice * per;
        k_end = min(p.K, k_begin + per);
    }
    // XCD-aware block remap (T1), column-major: each XCD die owns a
    // contiguous run of N-columns (all M-tiles of a few n-tiles), so the
    // shared B panel of a column stays resident in that XCD's private L2
    // while the M sweep streams A.
    int nwg = gridDim.x * gridDim.y;
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, off = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + off;
    }
    const int n0 = (bid / gridDim.y) * BN;   // column-major: n outer
    const int m0 = (bid % gridDim.y) * BM;

    const ushort_t* Ap;
    const ushort_t* Bp;
    long lda, ldb;
    resolve_ptr2(p.A, p.Atab, p.Atabld, pid, p.nInner, &Ap, &lda);
    resolve_ptr2(p.B, p.Btab, p.Btabld, pid, p.nInner, &Bp, &ldb);

    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int wm = (wid >> 1) * 64;
    const int wn = (wid & 1) * 64;
    const int lrow = lane & 15;
    const int kq = lane >> 4;

    f32x4 acc[4][4] = {};

    for (int k0 = k_begin; k0 < k_end; k0 += FBK) {
        if (threadIdx.x < 128)
            stage_repack<SWZ_TN_SK>(As, Ap, lda, k0, m0, k_end, threadIdx.x);
        else
            stage_repack<SWZ_TN_SK>(Bs, Bp, ldb, k0, n0, k_end,
                                    threadIdx.x - 128);
        __syncthreads();
        short8 af[2][4], bfr[2][4];
#pragma unroll
        for (int s = 0; s < 2; s++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int row = wm + i * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_TN_SK>(row) << 3);
                af[s][i] = *(const short8*)&As[row * FBK + off];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int row = wn + j * 16 + lrow;
                int off = (s * 32 + kq * 8) ^ (swz_row<SWZ_TN_SK>(row) << 3);
                bfr[s][j] = *(const short8*)&Bs[row * FBK + off];
            }
        }
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[s][i], bfr[s][j], acc[i][j], 0, 0, 0);
        __syncthreads();
    }

    if (p.splitk > 1) {
        float* ws = p.ws + ((long)slice * p.nproblems + pid) * p.M * p.N;
#pragma unroll
        for (int i16 = 0; i16 < 4; i16++)
#pragma unroll
            for (int j16 = 0; j16 < 4; j16++) {
                int j = n0 + wn + j16 * 16 + lrow;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    int i = m0 + wm + i16 * 16 + kq * 4 + r;
                    ws[(long)i * p.N + j] = acc[i16][j16][r];
                }
            }
        return;
    }
    // non-split-K falls back to the generic-epilogue variant (dispatch
    // guarantees splitk > 1 here)
}




void launch_gemm_tn_sk(const GemmParams& p, hipStream_t stream) {
    dim3 grid(p.N / BN, p.M / BM, p.nproblems * p.splitk);
    hipLaunchKernelGGL(gemm_tn_sk_kernel, grid, dim3(NTHREADS), 0, stream, p);
}

// ---------------------------------------------------------------- //
// TN kernel with direct-to-LDS staging and transposed LDS reads.
//
// Both TN operands are stored [k][out-dim]. The tiles are copied AS STORED
// ([BK k-rows][128 out-dim columns], 256-byte rows) by global_load_lds
// width 16 — no VGPR round trip, no register repack — and the transpose
// the MFMA needs (8 consecutive k per lane) happens in the LDS read path:
// ds_read_b64_tr_b16 hands lane i of a 16-lane group column i of a
// 4-row x 16-column block, so two of them (rows kq*8+0..3, kq*8+4..7) give
// exactly the short8 the repack kernels read with one ds_read_b128. Same
// MFMA, same k -> lane-group map, ascending k: results are bit-identical
// to gemm_tn_fast / gemm_tn_sk.
//
// LDS image (guide T10 layout (b)): 16-byte chunk ch of row r sits at
// byte 256*r + 16*(ch ^ tr_swz(r)), tr_swz(r) = ((r&3)<<2) | ((r>>2)&3).
// The DMA destination is linear, so the XOR goes on the per-lane SOURCE
// chunk (as in stage_glds). Bank check (bank = (addr/4) % 64, conflicts
// count per 32-lane half, 8 bytes = 2 banks per lane): a 256-byte row is
// exactly 64 banks, so the bank pair of a lane is 2*pos + (p&1) with
// pos = (c0 + (p>>1)) ^ tr_swz(row). A half holds lane groups kq and kq+1,
// i.e. rows r0+q and r0+8+q (q = 0..3) of one 16-column block: q toggles
// pos bits 2-3, p>>1 bit 0, the +8 rows bit 1 -> 16 distinct chunks x 2
// halves of a chunk = 32 distinct bank pairs, conflict-free.

typedef short short4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int tr_swz(int row) {
    return ((row & 3) << 2) | ((row >> 2) & 3);
}

// This wave's share of one [BK][128] operand tile: BK/4 DMA chunks of
// 4 rows (1 KB), BK/16 per wave. Lane l of a chunk lands at linear byte
// 16*l, i.e. row l>>4, chunk position l&15, and fetches the source chunk
// that the image keeps at that position.
template <int BK>
__device__ __forceinline__ void stage_glds_km(
        ushort_t* lds, const ushort_t* src, long ld, int k0, int c0,
        int wid, int lane) {
#pragma unroll
    for (int c = 0; c < BK / 16; c++) {
        int chunk = wid * (BK / 16) + c;
        int row = chunk * 4 + (lane >> 4);
        int ch = (lane & 15) ^ tr_swz(row);
        const ushort_t* gaddr = src + (long)(k0 + row) * ld + c0 + ch * 8;
        ushort_t* laddr = lds + chunk * 512;  // wave-uniform chunk base
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)gaddr,
            (__attribute__((address_space(3))) unsigned int*)laddr, 16, 0, 0);
    }
}

// Byte offset, inside a [BK][128] image, of this lane's address for the
// transposed read of rows r0+q (r0 % 4 == 0, q = 0..3) x columns
// [col0, col0+16): lane 4q+p of each 16-lane group addresses row q,
// columns 4p..4p+3 of the block.
__device__ __forceinline__ unsigned tr_off(int r0, int col0, int lane) {
    const int q = (lane >> 2) & 3, p = lane & 3;
    const int ch = (col0 >> 3) + (p >> 1);
    const int r = r0 + q;
    return (unsigned)(r * 256 + ((ch ^ tr_swz(r)) << 4) + ((p & 1) << 3));
}

// The transposed read is inline asm: through the builtin hipcc cannot
// tell the read from the in-flight global_load_lds destinations and puts
// s_waitcnt vmcnt(0) in front of the first read of every k-step, which
// drains the prefetch. The compiler therefore does NOT count these reads
// in lgkmcnt: every consumer sits behind tr_wait<N>() + tr_pin().
// Needs EXEC all ones: wave-uniform control flow only.
template <int OFF>
__device__ __forceinline__ short4v tr_read(unsigned addr) {
    short4v v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
                 : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
template <int N>
__device__ __forceinline__ void tr_wait() {
    asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(N) : "memory");
}
// makes every later use of `v` depend on a point after the wait
__device__ __forceinline__ void tr_pin(short4v& v) {
    asm volatile("" : "+v"(v));
}

// the 8 reads of one operand's four fragments for one MFMA k-group
template <int OFF>
__device__ __forceinline__ void tr_read4(
        short4v (&f)[4][2], const unsigned (&off)[4][2], unsigned sb) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        f[i][0] = tr_read<OFF>(off[i][0] + sb);
        f[i][1] = tr_read<OFF>(off[i][1] + sb);
    }
}
__device__ __forceinline__ void tr_pin4(short4v (&f)[4][2]) {
#pragma unroll
    for (int i = 0; i < 4; i++) { tr_pin(f[i][0]); tr_pin(f[i][1]); }
}

// BK: k-rows per stage (64 or 32); NST: stages in the ring (2: the
// nt_fast loop, one barrier + vmcnt(0) per step; 3: counted vmcnt, the
// stage after next streams during this step's MFMAs); SPLIT: split-K only
// (f32 slab epilogue, arena = the ring alone).
template <int BK, int NST, bool SPLIT>
__global__ __launch_bounds__(NTHREADS) void gemm_tn_tr_kernel(GemmParams p) {
    constexpr int OPER = BK * 128;           // elements per operand stage
    constexpr int STAGE = 2 * OPER;
    constexpr int RING = NST * STAGE;
    constexpr int ARENA =
        (SPLIT || RING >= 128 * EPI_LDS_ROW) ? RING : 128 * EPI_LDS_ROW;
    constexpr int NL = 2 * (BK / 16);        // DMA loads per wave per stage
    static_assert(NST == 2 || NST == 3, "ring depth");
    static_assert(NL == 4 || NL == 8, "vmcnt immediates below");
    __shared__ ushort_t smem[ARENA];         // ONE arena (see nt_fast)

    int pid = blockIdx.z;
    int slice = 0, k_begin = 0, k_end = p.K;
    if (p.splitk > 1) {
        pid = blockIdx.z % p.nproblems;
        slice = blockIdx.z / p.nproblems;
        int per = ((p.K + FBK - 1) / FBK + p.splitk - 1) / p.splitk * FBK;
        k_begin = slice * per;
        k_end = min(p.K, k_begin + per);
    }
    int nwg = gridDim.x * gridDim.y;
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, off = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + off;
    }
    const int n0 = (bid / gridDim.y) * BN;   // column-major: n outer
    const int m0 = (bid % gridDim.y) * BM;

    const ushort_t* Ap;
    const ushort_t* Bp;
    long lda, ldb;
    resolve_ptr2(p.A, p.Atab, p.Atabld, pid, p.nInner, &Ap, &lda);
    resolve_ptr2(p.B, p.Btab, p.Btabld, pid, p.nInner, &Bp, &ldb);

    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int wm = (wid >> 1) * 64;
    const int wn = (wid & 1) * 64;
    const int lrow = lane & 15;
    const int kq = lane >> 4;

    f32x4 acc[4][4] = {};

    // K % 64 == 0 (host-checked) and `per` a multiple of 64: every slice
    // is a whole number of stages; an empty slice (k_begin >= k_end) runs
    // no stage at all and stores its zero accumulators
    const int nk = k_end > k_begin ? (k_end - k_begin) / BK : 0;

    auto stage = [&](int buf, int kt) {
        ushort_t* Al = smem + buf * STAGE;
        stage_glds_km<BK>(Al, Ap, lda, k_begin + kt * BK, m0, wid, lane);
        stage_glds_km<BK>(Al + OPER, Bp, ldb, k_begin + kt * BK, n0, wid,
                          lane);
    };

    if (nk > 0) {
        stage(0, 0);
        if (NST == 3 && nk > 1) {
            stage(1, 1);
            if (NL == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else         asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
    }

    // per-lane LDS byte addresses of the fragment reads in stage 0:
    // [i][h] = rows kq*8 + 4h .. +3 of the 16 columns of fragment i; the
    // second MFMA k-group of a BK=64 stage is 32 rows = 8192 bytes on
    // (tr_swz is unchanged by +32 rows), the B tile OPER*2 bytes on
    const unsigned lds0 = (unsigned)(unsigned long)
        (__attribute__((address_space(3))) ushort_t*)smem;
    unsigned aoff[4][2], boff[4][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            aoff[i][h] = lds0 + tr_off(kq * 8 + 4 * h, wm + i * 16, lane);
            boff[i][h] = lds0 + tr_off(kq * 8 + 4 * h, wn + i * 16, lane);
        }
    auto cat = [](short4v lo, short4v hi) -> short8 {
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };

    for (int kt = 0; kt < nk; kt++) {
        if (kt + NST - 1 < nk) stage((kt + NST - 1) % NST, kt + NST - 1);
        const unsigned sb = (unsigned)((kt % NST) * STAGE * 2);
        short4v a0[4][2], b0[4][2];
        tr_read4<0>(a0, aoff, sb);
        tr_read4<OPER * 2>(b0, boff, sb);
        if constexpr (BK == 64) {
            // second k-group: A issued before the first group is waited
            // for, B right after, both in flight under the first MFMAs
            short4v a1[4][2], b1[4][2];
            tr_read4<8192>(a1, aoff, sb);
            tr_wait<8>();
            tr_pin4(a0); tr_pin4(b0);
            tr_read4<OPER * 2 + 8192>(b1, boff, sb);
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        cat(a0[i][0], a0[i][1]), cat(b0[j][0], b0[j][1]),
                        acc[i][j], 0, 0, 0);
            tr_wait<0>();
            tr_pin4(a1); tr_pin4(b1);
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        cat(a1[i][0], a1[i][1]), cat(b1[j][0], b1[j][1]),
                        acc[i][j], 0, 0, 0);
        } else {
            tr_wait<0>();
            tr_pin4(a0); tr_pin4(b0);
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        cat(a0[i][0], a0[i][1]), cat(b0[j][0], b0[j][1]),
                        acc[i][j], 0, 0, 0);
        }
        if (NST == 2) {
            // drains the in-flight DMA of the next stage + buffer reuse
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        } else if (kt + 1 < nk) {
            // stage kt+1 landed; stage kt+2 (issued above) may still fly:
            // raw barrier, __syncthreads would drain it with vmcnt(0)
            if (kt + 2 < nk) {
                if (NL == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                else         asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
        }
    }

    if (SPLIT || p.splitk > 1) {
        float* ws = p.ws + ((long)slice * p.nproblems + pid) * p.M * p.N;
#pragma unroll
        for (int i16 = 0; i16 < 4; i16++)
#pragma unroll
            for (int j16 = 0; j16 < 4; j16++) {
                int j = n0 + wn + j16 * 16 + lrow;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    int i = m0 + wm + i16 * 16 + kq * 4 + r;
                    ws[(long)i * p.N + j] = acc[i16][j16][r];
                }
            }
        return;
    }
    if constexpr (!SPLIT) {
        __syncthreads();   // all waves done with the ring before staging C
        gemm_epilogue_lds(p, pid, m0, n0, wm, wn, lrow, kq, acc, smem);
    }
}

// variant: 1 = BK 64 x 2 buffers (64 KiB, 2 blocks/CU), 2 = BK 32 x 3-ring
// (48 KiB, 3 blocks/CU), 3 = BK 32 x 2 buffers (32 KiB, 4 blocks/CU).
// Non-split calls need the C staging arena and always take variant 1.
void launch_gemm_tn_tr(const GemmParams& p, int variant, hipStream_t stream) {
    int sk = p.splitk > 1 ? p.splitk : 1;
    dim3 grid(p.N / BN, p.M / BM, p.nproblems * sk);
    dim3 blk(NTHREADS);
    if (sk == 1)
        hipLaunchKernelGGL((gemm_tn_tr_kernel<64, 2, false>), grid, blk, 0,
                           stream, p);
    else if (variant == 2)
        hipLaunchKernelGGL((gemm_tn_tr_kernel<32, 3, true>), grid, blk, 0,
                           stream, p);
    else if (variant == 3)
        hipLaunchKernelGGL((gemm_tn_tr_kernel<32, 2, true>), grid, blk, 0,
                           stream, p);
    else
        hipLaunchKernelGGL((gemm_tn_tr_kernel<64, 2, true>), grid, blk, 0,
                           stream, p);
}


// ---------------------------------------------------------------- //
// Measured-and-rejected variants (see git history + profiles/README.md):
//  - 256^2 2-phase and phase-pipelined kernels (1 block/CU sync stalls
//    beat the intensity gain: 670-774us vs 463us for the up shape)
//  - 128^2 3-ring (96 KiB LDS halves occupancy: down 292->357us)
//  - 128x256 TN (68 KiB arena halves tn_fast's 4 blocks/CU: dW1 +37%)
//  - 256^2 BK=32 3-ring (paired-row LDS; slower on K=512 and buggy)
//  - reg-pipelined TN 2-buf (issue-early/write-late, 64 KiB, 1 barrier
//    per step): loses to tn_fast/tn_sk on every dW shape (486->477,
//    560->542, 730->703, 775->756 TF; bench 962->943) — 4 blocks/CU
//    cross-block overlap hides the repack latency better than in-kernel
//    pipelining at 2 blocks/CU
//  - 128^2 persistent 3-ring (nt5p idea at BN=128, 96 KiB, 1 block/CU):
//    4-wave/64x64 cut hit 260 VGPRs (1 wave/SIMD) and halved throughput;
//    the 8-wave/64x32 cut (91 VGPRs) still lost on every target shape
//    (down 622->464 TF, dP 457->407; bench 949->908) — at 128-wide
//    tiles, 2 blocks/CU of the plain 2-buf kernel beats any 1-block/CU
//    in-ring overlap. The wide-tile nt5p wins come from intensity AND
//    persistence together, not persistence alone
//  - 16-byte register-epilogue STORES (WideEpi) where they did not pay
//    (scripts/wide_epi_ab.py, 10 interleaved rounds, TF median [min,max]):
//    nt5p EPI_GELU_PAIR 473.2 [409.5,478.5] -> 474.5 [459.6,477.5] (a
//    second session 477.4 -> 469.5), nt5p plain C 627.6 [622.9,630.0] ->
//    617.2 [609.8,618.4]; nt8p down-proj 792.4 -> 792.1, nt8p square
//    833.6 -> 835.1. 8x fewer store instructions bought nothing on these,
//    so the K=512 tail is not store-issue-bound; the code stays
//    selectable (set_wide_epilogue_mode(2), set_wide_epilogue_nt8p) and
//    off. What did pay: dH 390.3 -> 456.6 with early 16-byte aux loads
//    AND wide stores (442.6 with the loads alone), EPI_GELU 529.2 -> 542.8
//  - nt8p for the K=512 dH with the same wide aux path: 355.6 -> 461.1 TF,
//    level with nt5p's 463.4, not ahead: GLOM_NT8P_MINK stays 2048
//  - gemm_tn_tr split-K pipeline points that lost (scripts/tn_tr_ab.py,
//    TF median [min,max] of GEMM + finish; then the headline step, three
//    alternating runs, ms). Shipped: BK 64 x 2 buffers (64 KiB, 2
//    blocks/CU): dW1 626.5 [621.5,633.9], dW2 712.5 [704.4,721.1],
//    step 40.24 / 40.28 / 40.27 (old kernels 41.15 / 41.15 / 41.38).
//    BK 32 x 2 buffers (32 KiB, 4 blocks/CU): dW1 633.1 [631.2,634.7],
//    dW2 721.4 [716.8,725.7] - ahead or level alone, but the step is
//    40.47 / 40.46 / 40.47. BK 32 3-ring with counted vmcnt (48 KiB, 3
//    blocks/CU): dW1 604.7 [600.2,607.2], dW2 727.0 [706.7,738.8], step
//    41.34 / 41.40 / 41.43, slower than the old kernels. dW runs beside
//    the dH / dX streams; the step decides. Both stay selectable
//    (GLOM_TN_TR_VARIANT=3 / 2)
//  - gemm_tn_tr for the K=256 attention dv / dk-hat (non-split, 64 KiB
//    arena vs tn_fast's 34 KiB): level at op level (269.3 vs 269.5 TF),
//    step 40.5-40.8 vs 40.47 with them on tn_fast: K < 4096 non-split
//    calls keep gemm_tn_fast
//  - ds_read_b64_tr_b16 through the compiler builtin: correct, but hipcc
//    puts s_waitcnt vmcnt(0) before the first read of every k-step (it
//    cannot tell the read from the in-flight glds destinations), which
//    drains the prefetch; hence the inline asm + hand-placed lgkmcnt
//  - gemm_nt_fast3, the 2-buffer 128x256 kernel (96 KiB LDS, one barrier
//    per K-step): superseded by the 3-ring gemm_nt_fast4, MFMA-busy / SQ-busy
//    4.1 -> 6.2 (profiles/README.md, PMC tables); removed once nothing
//    launched it
// The shipping set: gemm_nt_fast (128^2 glds 2-buf), gemm_nt_fast4
// (128x256 8-wave, 3-ring), gemm_nt_fast5p (persistent
// continuous-ring, default for M%512==0 plain/GELUGRAD epilogues),
// gemm_tn_tr (glds + transposed reads; weight grads), gemm_tn_fast(+_sk)
// (K % 8 tails, short-K non-split), gemm_nn_fast.
