// Island-of-agreement analysis of GLOM level states on CDNA4 (gfx950):
//   - k_island_dots:   per-(p,n,l) row norm + raw dot products with the 2
//                      (4-connectivity) or 4 (8-connectivity) forward
//                      neighbours on the H x W patch grid
//   - k_island_finish: agreement = dot / (max(|a|,1e-8) * max(|b|,1e-8)),
//                      out-of-grid edges := 0
//   - k_island_labels: connected components of the kept-edge graph
//                      (agreement >= threshold), label = smallest linear
//                      cell index of the component
//   - k_island_sizes:  island size at each root cell + island count
// levels (*lead, N, L, D) bf16 is viewed as (P, N, L, D); agreement is
// (P, L, C, H, W) f32 with edge channels c=0 right, 1 down, 2 down-right,
// 3 down-left; labels/sizes are (P, L, H, W) i32, count (P, L) i32.
//
// Norms are computed ONCE per row, by the wave that owns the row, and
// the division is split into a post-pass (k_island_finish) over the
// agreement tensor. The alternatives were weighed and rejected: a norm
// PRE-pass re-reads the whole level tensor (1.3 GB at the headline
// trajectory shape) where the post-pass touches only rows*(C+1) floats
// (~1% of it); staging a tile of rows through LDS to share norms inside
// one block needs a halo of W+1 rows per tile and caps D; recomputing
// the neighbour norm inside each edge costs 2-4x the VALU work of the
// dots. The dots kernel is one wave per row as in k_rnorm, 16-byte loads
// strided over D. Each row is loaded 1+C times in all: once by its own
// wave and once by each wave that has it as a neighbour (the rows at
// +L*D and +(W-1..W+1)*L*D elements), which run a few blocks away. Where
// those repeat loads are served from (same-XCD L2, another XCD's L2 via
// the Infinity Cache, or HBM) has not been measured with counters; the
// end-to-end rate is in profiles/README.md ("Island analysis").
//
// The labelling kernel is one workgroup per (p,l) problem with the cell
// labels in LDS (N <= 1024). It alternates a HOOK pass (every kept edge
// whose endpoints have different roots hooks the larger root under the
// smaller with an LDS atomic min) with pointer jumping until a
// block-wide vote says the labels stopped moving, and repeats until a
// hook pass finds nothing to do. lab[x] <= x always holds and labels
// only decrease, so every chain is acyclic, the loop terminates, and
// the fixpoint (every cell labelled with the smallest index of its
// component) is independent of the order in which waves run: results
// are bitwise deterministic. No iteration count is assumed anywhere and
// nothing synchronises with the host.

#include "common.h"
#include "island_kernels.h"

#define NTHREADS 256
#define WPB (NTHREADS / WAVE)

// forward edge channel c of cell (h,w) stays inside the H x W grid
__device__ __forceinline__ bool edge_in_grid(int c, int h, int w, int H,
                                             int W) {
    switch (c) {
    case 0: return w + 1 < W;                 // right
    case 1: return h + 1 < H;                 // down
    case 2: return h + 1 < H && w + 1 < W;    // down-right
    default: return h + 1 < H && w >= 1;      // down-left
    }
}

// linear-index distance from a cell to its channel-c neighbour
__device__ __forceinline__ int edge_offset(int c, int W) {
    return c == 0 ? 1 : c == 1 ? W : c == 2 ? W + 1 : W - 1;
}

// levels (P,N,L,D) -> norm (P,L,N) f32 = ||row||_2, out (P,L,C,N) f32 raw
// dot products (0 for edges that leave the grid). One wave per row.
template <int C>
__global__ __launch_bounds__(NTHREADS) void k_island_dots(
        const ushort_t* __restrict__ levels, float* __restrict__ norm,
        float* __restrict__ out, long P, int H, int W, int L, int D) {
    const int N = H * W;
    long row = (long)blockIdx.x * WPB + threadIdx.x / WAVE;
    long total = P * N * L;
    if (row >= total) return;
    int lane = threadIdx.x % WAVE;
    int l = row % L;
    int n = (row / L) % N;
    long p = row / ((long)N * L);
    int h = n / W, w = n % W;
    const ushort_t* a = levels + row * D;

    // an edge that leaves the grid reads the own row again (an L1 hit, no
    // divergent load) and its result is discarded below
    bool ok[C];
    const ushort_t* nb[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        ok[c] = edge_in_grid(c, h, w, H, W);
        nb[c] = ok[c] ? a + (long)edge_offset(c, W) * L * D : a;
    }

    float ss = 0.f, dot[C];
#pragma unroll
    for (int c = 0; c < C; c++) dot[c] = 0.f;
    for (int q0 = lane * 8; q0 < D; q0 += WAVE * 8) {
        union { uint4v v; ushort_t u[8]; } t, u[C];
        t.v = *(const uint4v*)(a + q0);
#pragma unroll
        for (int c = 0; c < C; c++) u[c].v = *(const uint4v*)(nb[c] + q0);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            float v = bf2f(t.u[e]);
            ss += v * v;
#pragma unroll
            for (int c = 0; c < C; c++) dot[c] += v * bf2f(u[c].u[e]);
        }
    }
    ss = wave_reduce_sum(ss);
#pragma unroll
    for (int c = 0; c < C; c++) dot[c] = wave_reduce_sum(dot[c]);
    if (lane == 0) {
        long pl = p * L + l;
        norm[pl * N + n] = sqrtf(ss);
#pragma unroll
        for (int c = 0; c < C; c++)
            out[(pl * C + c) * N + n] = ok[c] ? dot[c] : 0.f;
    }
}

// in place over out (PL,C,N): raw dot -> cosine agreement
template <int C>
__global__ __launch_bounds__(NTHREADS) void k_island_finish(
        const float* __restrict__ norm, float* __restrict__ out, long PL,
        int H, int W) {
    const int N = H * W;
    long idx = (long)blockIdx.x * NTHREADS + threadIdx.x;
    if (idx >= PL * C * N) return;
    int n = idx % N;
    int c = (idx / N) % C;
    long pl = idx / ((long)N * C);
    float v = 0.f;
    if (edge_in_grid(c, n / W, n % W, H, W)) {
        float na = norm[pl * N + n];
        float nb = norm[pl * N + n + edge_offset(c, W)];
        v = out[idx] / (fmaxf(na, 1e-8f) * fmaxf(nb, 1e-8f));
    }
    out[idx] = v;
}

// follow lab[] to the root (lab[r] == r); chains strictly decrease
__device__ __forceinline__ int island_root(volatile int* lab, int i) {
    int r = lab[i];
    for (;;) {
        int p = lab[r];
        if (p == r) return r;
        r = p;
    }
}

// agreement (PL,C,N) f32 -> labels (PL,N) i32; one workgroup per problem
__global__ __launch_bounds__(NTHREADS) void k_island_labels(
        const float* __restrict__ agreement, int* __restrict__ labels,
        int H, int W, int C, float threshold) {
    __shared__ int lab[ISLAND_MAX_CELLS];
    __shared__ unsigned char kept[ISLAND_MAX_CELLS];
    const int N = H * W;
    const int tid = threadIdx.x;
    const float* agr = agreement + (long)blockIdx.x * C * N;

    for (int i = tid; i < N; i += NTHREADS) {
        int h = i / W, w = i % W;
        unsigned m = 0;
        for (int c = 0; c < C; c++)
            if (edge_in_grid(c, h, w, H, W) && agr[c * N + i] >= threshold)
                m |= 1u << c;
        kept[i] = (unsigned char)m;
        lab[i] = i;
    }
    __syncthreads();

    volatile int* vl = lab;
    for (;;) {
        // hook: join the two trees of every kept edge that still spans two
        int hooked = 0;
        for (int i = tid; i < N; i += NTHREADS) {
            unsigned m = kept[i];
            for (int c = 0; c < C; c++) {
                if (!((m >> c) & 1u)) continue;
                int ri = island_root(vl, i);
                int rj = island_root(vl, i + edge_offset(c, W));
                if (ri != rj) {
                    atomicMin(&lab[max(ri, rj)], min(ri, rj));
                    hooked = 1;
                }
            }
        }
        if (!__syncthreads_or(hooked)) break;
        // pointer jumping until every cell points at its root
        for (;;) {
            int moved = 0;
            for (int i = tid; i < N; i += NTHREADS) {
                int r = vl[i];
                int rr = vl[r];
                if (rr != r) {
                    vl[i] = rr;
                    moved = 1;
                }
            }
            if (!__syncthreads_or(moved)) break;
        }
    }

    int* o = labels + (long)blockIdx.x * N;
    for (int i = tid; i < N; i += NTHREADS) o[i] = lab[i];
}

// labels (PL,N) i32 -> sizes (PL,N) i32 (island size at its root cell, 0
// elsewhere) and count (PL) i32 (number of roots); either may be null.
// Integer LDS atomics: the result does not depend on their order.
__global__ __launch_bounds__(NTHREADS) void k_island_sizes(
        const int* __restrict__ labels, int* __restrict__ sizes,
        int* __restrict__ count, int N) {
    __shared__ int cnt[ISLAND_MAX_CELLS];
    __shared__ int roots;
    const int tid = threadIdx.x;
    const int* lb = labels + (long)blockIdx.x * N;
    for (int i = tid; i < N; i += NTHREADS) cnt[i] = 0;
    if (tid == 0) roots = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < N; i += NTHREADS) {
        int r = lb[i];
        if ((unsigned)r < (unsigned)N) atomicAdd(&cnt[r], 1);
        mine += (r == i);
    }
    if (mine) atomicAdd(&roots, mine);
    __syncthreads();
    if (sizes)
        for (int i = tid; i < N; i += NTHREADS)
            sizes[(long)blockIdx.x * N + i] = cnt[i];
    if (count && tid == 0) count[blockIdx.x] = roots;
}

// ---------------- host launchers ----------------

static inline long cdiv(long a, long b) { return (a + b - 1) / b; }

void launch_island_dots(const void* levels, float* norm, float* out, long P,
                        int H, int W, int L, int D, int C, hipStream_t s) {
    long rows = P * H * W * L;
    if (rows == 0) return;
    dim3 grid(cdiv(rows, WPB)), block(NTHREADS);
    if (C == 2)
        hipLaunchKernelGGL(k_island_dots<2>, grid, block, 0, s,
                           (const ushort_t*)levels, norm, out, P, H, W, L, D);
    else
        hipLaunchKernelGGL(k_island_dots<4>, grid, block, 0, s,
                           (const ushort_t*)levels, norm, out, P, H, W, L, D);
}

void launch_island_finish(const float* norm, float* out, long PL, int H,
                          int W, int C, hipStream_t s) {
    long total = PL * C * H * W;
    if (total == 0) return;
    dim3 grid(cdiv(total, NTHREADS)), block(NTHREADS);
    if (C == 2)
        hipLaunchKernelGGL(k_island_finish<2>, grid, block, 0, s, norm, out,
                           PL, H, W);
    else
        hipLaunchKernelGGL(k_island_finish<4>, grid, block, 0, s, norm, out,
                           PL, H, W);
}

void launch_island_labels(const float* agreement, int* labels, long PL,
                          int H, int W, int C, float threshold,
                          hipStream_t s) {
    if (PL == 0 || H * W == 0) return;
    hipLaunchKernelGGL(k_island_labels, dim3(PL), dim3(NTHREADS), 0, s,
                       agreement, labels, H, W, C, threshold);
}

void launch_island_sizes(const int* labels, int* sizes, int* count, long PL,
                         int N, hipStream_t s) {
    if (PL == 0) return;
    hipLaunchKernelGGL(k_island_sizes, dim3(PL), dim3(NTHREADS), 0, s,
                       labels, sizes, count, N);
}
