// Row-wise / elementwise CDNA4 kernels for the GLOM hot loop (gfx950):
//   - k_rnorm:        per-(b,n,l) inverse L2 norm of the level rows
//                     (fuses F.normalize of reference glom_pytorch.py:58)
//   - k_softmax_fwd:  masked row softmax over consensus scores
//                     (reference glom_pytorch.py:62-71: -5e-4 diagonal fill
//                     and -max non-local fill happen BEFORE the softmax)
//   - k_softmax_bwd:  row softmax backward + mask-zeroing + k-norm column
//                     scaling (emits both dS and dS*rnorm[j])
//   - k_knorm_combine: backward of k = x / max(||x||, eps) plus the final
//                     sum dlevels = dv + dq + dk of the attention backward
//   - k_mix_fwd/bwd:  level mixing (prev + bu + pad(td) + cons) / c_l with
//                     c = [4,..,4,3] (reference glom_pytorch.py:128-144)
// All inputs/outputs bf16; accumulation in f32. One wave owns one row for
// the row-wise kernels (scalar per-lane loads are coalesced across lanes).

#include "common.h"
#include "aux_kernels.h"

#define NTHREADS 256
#define WPB (NTHREADS / WAVE)

// levels (B,N,L,d) -> rnorm (B,L,N) f32, rnorm = 1 / max(||row||_2, 1e-12)
__global__ __launch_bounds__(NTHREADS) void k_rnorm(
        const ushort_t* __restrict__ levels, float* __restrict__ out,
        int B, int N, int L, int d) {
    long row = (long)blockIdx.x * WPB + threadIdx.x / WAVE;
    long total = (long)B * N * L;
    if (row >= total) return;
    int lane = threadIdx.x % WAVE;
    int l = row % L;
    long n = (row / L) % N;
    long b = row / ((long)N * L);
    const ushort_t* x = levels + row * d;
    float ss = 0.f;
    if (d % 8 == 0) {
        for (int q0 = lane * 8; q0 < d; q0 += WAVE * 8) {
            union { uint4v v; ushort_t u[8]; } t;
            t.v = *(const uint4v*)(x + q0);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float v = bf2f(t.u[e]);
                ss += v * v;
            }
        }
    } else {
        for (int q = lane; q < d; q += WAVE) {
            float v = bf2f(x[q]);
            ss += v * v;
        }
    }
    ss = wave_reduce_sum(ss);
    if (lane == 0)
        out[(b * L + l) * N + n] = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
}

// scores/P: (P, N, N) bf16; one wave per row i of problem p.
__global__ __launch_bounds__(NTHREADS) void k_softmax_fwd(
        const ushort_t* __restrict__ scores, ushort_t* __restrict__ probs,
        const bool* __restrict__ nonlocal_mask, int nprob, int N,
        int self_mask) {
    long row = (long)blockIdx.x * WPB + threadIdx.x / WAVE;
    if (row >= (long)nprob * N) return;
    int lane = threadIdx.x % WAVE;
    int i = row % N;
    const ushort_t* s = scores + row * N;
    ushort_t* o = probs + row * N;
    const bool* m = nonlocal_mask ? nonlocal_mask + (long)i * N : nullptr;
    const float SELF = bf2f(f2bf(-5e-4f));
    const float NEG = -3.3895314e38f;  // -finfo(bf16).max

    if (N % 8 == 0) {
        // vectorized: each lane owns contiguous 8-element chunks; the row
        // (< 1024 values at the stretch config) is re-read from L1/L2
        float mx = -INFINITY, sum = 0.f;
#pragma unroll 1
        for (int j0 = lane * 8; j0 < N; j0 += WAVE * 8) {
            union { uint4v v; ushort_t u[8]; } t;
            t.v = *(const uint4v*)(s + j0);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float v = bf2f(t.u[e]);
                if (self_mask && j0 + e == i) v = SELF;
                if (m && m[j0 + e]) v = NEG;
                mx = fmaxf(mx, v);
            }
        }
        mx = wave_reduce_max(mx);
        mx = __shfl(mx, 0, WAVE);
#pragma unroll 1
        for (int j0 = lane * 8; j0 < N; j0 += WAVE * 8) {
            union { uint4v v; ushort_t u[8]; } t, ov;
            t.v = *(const uint4v*)(s + j0);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float v = bf2f(t.u[e]);
                if (self_mask && j0 + e == i) v = SELF;
                if (m && m[j0 + e]) v = NEG;
                float ex = __expf(v - mx);
                sum += ex;
                ov.u[e] = f2bf(ex);
            }
            *(uint4v*)(o + j0) = ov.v;   // unnormalized, rescaled below
        }
        sum = wave_reduce_sum(sum);
        sum = __shfl(sum, 0, WAVE);
        float inv = 1.0f / sum;
#pragma unroll 1
        for (int j0 = lane * 8; j0 < N; j0 += WAVE * 8) {
            union { uint4v v; ushort_t u[8]; } t;
            t.v = *(const uint4v*)(o + j0);
#pragma unroll
            for (int e = 0; e < 8; e++) t.u[e] = f2bf(bf2f(t.u[e]) * inv);
            *(uint4v*)(o + j0) = t.v;
        }
        return;
    }
    float mx = -INFINITY;
    for (int j = lane; j < N; j += WAVE) {
        float v = bf2f(s[j]);
        if (self_mask && j == i) v = SELF;
        if (m && m[j]) v = NEG;
        mx = fmaxf(mx, v);
    }
    mx = wave_reduce_max(mx);
    mx = __shfl(mx, 0, WAVE);
    float sum = 0.f;
    for (int j = lane; j < N; j += WAVE) {
        float v = bf2f(s[j]);
        if (self_mask && j == i) v = SELF;
        if (m && m[j]) v = NEG;
        sum += expf(v - mx);
    }
    sum = wave_reduce_sum(sum);
    sum = __shfl(sum, 0, WAVE);
    float inv = 1.0f / sum;
    for (int j = lane; j < N; j += WAVE) {
        float v = bf2f(s[j]);
        if (self_mask && j == i) v = SELF;
        if (m && m[j]) v = NEG;
        o[j] = f2bf(expf(v - mx) * inv);
    }
}

// dS[i,j] = alpha * P[i,j] * (dP[i,j] - sum_k P[i,k] dP[i,k]), masked -> 0;
// dSr[i,j] = dS[i,j] * rnorm[p,j].
__global__ __launch_bounds__(NTHREADS) void k_softmax_bwd(
        const ushort_t* __restrict__ P, const ushort_t* __restrict__ dP,
        const float* __restrict__ rnorm, ushort_t* __restrict__ dS,
        ushort_t* __restrict__ dSr, const bool* __restrict__ nonlocal_mask,
        int nprob, int N, int self_mask, float alpha, int L, int l_lo) {
    // nprob counts the live problems: levels [l_lo, L) of every batch
    // entry; the buffers keep all L levels per entry (problem b * L + l)
    long row = (long)blockIdx.x * WPB + threadIdx.x / WAVE;
    if (row >= (long)nprob * N) return;
    int lane = threadIdx.x % WAVE;
    int i = row % N;
    long p = row / N;
    p = (p / (L - l_lo)) * L + l_lo + p % (L - l_lo);
    row = p * N + i;
    const ushort_t* pr = P + row * N;
    const ushort_t* dpr = dP + row * N;
    const float* rn = rnorm + p * N;
    const bool* m = nonlocal_mask ? nonlocal_mask + (long)i * N : nullptr;

    float t = 0.f;
    if (N % 8 == 0) {
#pragma unroll 1
        for (int j0 = lane * 8; j0 < N; j0 += WAVE * 8) {
            union { uint4v v; ushort_t u[8]; } a, bb;
            a.v = *(const uint4v*)(pr + j0);
            bb.v = *(const uint4v*)(dpr + j0);
#pragma unroll
            for (int e = 0; e < 8; e++) t += bf2f(a.u[e]) * bf2f(bb.u[e]);
        }
        t = wave_reduce_sum(t);
        t = __shfl(t, 0, WAVE);
#pragma unroll 1
        for (int j0 = lane * 8; j0 < N; j0 += WAVE * 8) {
            union { uint4v v; ushort_t u[8]; } a, bb, o1, o2;
            a.v = *(const uint4v*)(pr + j0);
            bb.v = *(const uint4v*)(dpr + j0);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float v = alpha * bf2f(a.u[e]) * (bf2f(bb.u[e]) - t);
                if (self_mask && j0 + e == i) v = 0.f;
                if (m && m[j0 + e]) v = 0.f;
                o1.u[e] = f2bf(v);
                o2.u[e] = f2bf(v * rn[j0 + e]);
            }
            *(uint4v*)(dS + row * N + j0) = o1.v;
            *(uint4v*)(dSr + row * N + j0) = o2.v;
        }
        return;
    }
    for (int j = lane; j < N; j += WAVE) t += bf2f(pr[j]) * bf2f(dpr[j]);
    t = wave_reduce_sum(t);
    t = __shfl(t, 0, WAVE);
    for (int j = lane; j < N; j += WAVE) {
        float v = alpha * bf2f(pr[j]) * (bf2f(dpr[j]) - t);
        if (self_mask && j == i) v = 0.f;
        if (m && m[j]) v = 0.f;
        dS[row * N + j] = f2bf(v);
        dSr[row * N + j] = f2bf(v * rn[j]);
    }
}

// Backward of k = x * r, r = 1/max(||x||, eps), fused with the attention
// gradient sum: out(B,N,L,d) = dv + dq + r*(dkhat - x*r^2*(dkhat . x))
// (when the norm clamps at eps, the projection term vanishes).
// dkhat layout (B,L,N,d); dv,dq,out (B,N,L,d); rnorm (B,L,N).
__global__ __launch_bounds__(NTHREADS) void k_knorm_combine(
        const ushort_t* __restrict__ dkhat, const ushort_t* __restrict__ lev,
        const float* __restrict__ rnorm, const ushort_t* __restrict__ dv,
        const ushort_t* __restrict__ dq, ushort_t* __restrict__ out,
        int B, int N, int L, int d, int l_lo) {
    // one wave per live row: levels [l_lo, L) of every (b, n)
    long row = (long)blockIdx.x * WPB + threadIdx.x / WAVE;
    const int Ll = L - l_lo;
    long total = (long)B * N * Ll;
    if (row >= total) return;
    int lane = threadIdx.x % WAVE;
    int l = l_lo + row % Ll;
    long n = (row / Ll) % N;
    long b = row / ((long)N * Ll);
    row = (b * N + n) * L + l;
    const ushort_t* dkh = dkhat + ((b * L + l) * N + n) * (long)d;
    const ushort_t* x = lev + row * d;
    float r = rnorm[(b * L + l) * N + n];
    bool clamped = r >= 0.999e12f;

    const bool vec = (d % 8 == 0);
    float dot = 0.f;
    if (!clamped) {
        if (vec) {
            for (int q0 = lane * 8; q0 < d; q0 += WAVE * 8) {
                union { uint4v v; ushort_t u[8]; } a, b;
                a.v = *(const uint4v*)(dkh + q0);
                b.v = *(const uint4v*)(x + q0);
#pragma unroll
                for (int e = 0; e < 8; e++)
                    dot += bf2f(a.u[e]) * bf2f(b.u[e]);
            }
        } else {
            for (int q = lane; q < d; q += WAVE)
                dot += bf2f(dkh[q]) * bf2f(x[q]);
        }
        dot = wave_reduce_sum(dot);
        dot = __shfl(dot, 0, WAVE);
    }
    float c = clamped ? 0.f : r * r * dot;
    if (vec) {
        for (int q0 = lane * 8; q0 < d; q0 += WAVE * 8) {
            union { uint4v v; ushort_t u[8]; } a, b, dvv, dqv, o;
            a.v = *(const uint4v*)(dkh + q0);
            b.v = *(const uint4v*)(x + q0);
            dvv.v = *(const uint4v*)(dv + row * d + q0);
            dqv.v = *(const uint4v*)(dq + row * d + q0);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float dk = r * (bf2f(a.u[e]) - bf2f(b.u[e]) * c);
                o.u[e] = f2bf(dk + bf2f(dvv.u[e]) + bf2f(dqv.u[e]));
            }
            *(uint4v*)(out + row * d + q0) = o.v;
        }
    } else {
        for (int q = lane; q < d; q += WAVE) {
            float dk = r * (bf2f(dkh[q]) - bf2f(x[q]) * c);
            out[row * d + q] =
                f2bf(dk + bf2f(dv[row * d + q]) + bf2f(dq[row * d + q]));
        }
    }
}

// out = (prev + bu + td_padded + cons) / c_l, elementwise over (B,N,L,d);
// td has L-1 level slots, the top slot contributes zero.
// bu0 (optional): level 0 of the bottom-up contribution comes from
// bu0 + bn * bu0_ld instead of bu's slice 0, which is then never read (the
// token MLP is loop-invariant, docs/ARCHITECTURE.md "Loop invariants").
// NEXT: also write, from the bf16-rounded values being stored, what the
// next iteration's k_add_pos and k_rnorm would compute from `out`:
//   td_next[b,n,l-1,:] = out[b,n,l,:] + pos[n,:]        (l >= 1)
//   rn_next[b,l,n]     = 1 / max(||out[b,n,l,:]||, 1e-12)
// Only for d == WAVE * 8 (512): one wave then holds exactly one row with
// lane -> q0 = lane * 8, which is k_rnorm's map, so the eight sequential
// adds and the wave_reduce_sum below repeat its summation order bit for
// bit. Other d keep the standalone kernels (the host never asks for NEXT).
template <bool NEXT>
__global__ __launch_bounds__(NTHREADS) void k_mix_fwd(
        const ushort_t* __restrict__ prev, const ushort_t* __restrict__ bu,
        const ushort_t* __restrict__ td, const ushort_t* __restrict__ cons,
        ushort_t* __restrict__ out, long total, int L, int d,
        const ushort_t* __restrict__ bu0, long bu0_ld,
        const ushort_t* __restrict__ pos, ushort_t* __restrict__ td_next,
        float* __restrict__ rn_next, int N) {
    long idx = ((long)blockIdx.x * NTHREADS + threadIdx.x) * 8;
    if (idx >= total) return;
    int q = idx % d;
    int l = (idx / d) % L;
    long bn = idx / ((long)d * L);
    union { uint4v v; ushort_t u[8]; } a, b, c4, t, o;
    a.v = *(const uint4v*)(prev + idx);
    b.v = *(const uint4v*)((bu0 && l == 0) ? bu0 + bn * bu0_ld + q
                                           : bu + idx);
    c4.v = *(const uint4v*)(cons + idx);
    bool has_td = l < L - 1;
    if (has_td) t.v = *(const uint4v*)(td + (bn * (L - 1) + l) * (long)d + q);
    float c = has_td ? 4.0f : 3.0f;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        float v = bf2f(a.u[e]) + bf2f(b.u[e]) + bf2f(c4.u[e]);
        if (has_td) v += bf2f(t.u[e]);
        o.u[e] = f2bf(v / c);
    }
    *(uint4v*)(out + idx) = o.v;
    if (NEXT) {
        // d == WAVE * 8: the wave is whole (total is a multiple of d) and
        // l, bn are wave-uniform
        long n = bn % N;
        long bb = bn / N;
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            float v = bf2f(o.u[e]);
            ss += v * v;
        }
        ss = wave_reduce_sum(ss);
        if (threadIdx.x % WAVE == 0)
            rn_next[(bb * L + l) * N + n] = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
        if (l >= 1) {
            union { uint4v v; ushort_t u[8]; } p;
            p.v = *(const uint4v*)(pos + n * (long)d + q);
#pragma unroll
            for (int e = 0; e < 8; e++)
                p.u[e] = f2bf(bf2f(o.u[e]) + bf2f(p.u[e]));
            *(uint4v*)(td_next + (bn * (L - 1) + l - 1) * (long)d + q) = p.v;
        }
    }
}

// dmix = dout / c_l (shared by prev/bu/cons); dtd = dout[..., :L-1, :] / 4
__global__ __launch_bounds__(NTHREADS) void k_mix_bwd(
        const ushort_t* __restrict__ dout, ushort_t* __restrict__ dmix,
        ushort_t* __restrict__ dtd, long total, int L, int d) {
    long idx = ((long)blockIdx.x * NTHREADS + threadIdx.x) * 8;
    if (idx >= total) return;
    int q = idx % d;
    int l = (idx / d) % L;
    long bn = idx / ((long)d * L);
    union { uint4v v; ushort_t u[8]; } g, o;
    g.v = *(const uint4v*)(dout + idx);
    bool has_td = l < L - 1;
    float c = has_td ? 4.0f : 3.0f;
#pragma unroll
    for (int e = 0; e < 8; e++) o.u[e] = f2bf(bf2f(g.u[e]) / c);
    *(uint4v*)(dmix + idx) = o.v;
    if (has_td) *(uint4v*)(dtd + (bn * (L - 1) + l) * (long)d + q) = o.v;
}

// k_mix_bwd for the levels [lo, L) only, and without the compact dtd copy:
// the top-down backward reads dmix itself with row stride L*d (backward
// merge, docs/ARCHITECTURE.md). Levels below lo of dmix are not written.
__global__ __launch_bounds__(NTHREADS) void k_mix_bwd_lo(
        const ushort_t* __restrict__ dout, ushort_t* __restrict__ dmix,
        long live, int L, int d, int lo) {
    long i8 = ((long)blockIdx.x * NTHREADS + threadIdx.x) * 8;
    if (i8 >= live) return;
    const long w = (long)(L - lo) * d;      // live span of one (b,n) row
    long bn = i8 / w;
    long r = i8 % w;
    int l = lo + (int)(r / d);
    long idx = bn * (long)L * d + (long)lo * d + r;
    union { uint4v v; ushort_t u[8]; } g, o;
    g.v = *(const uint4v*)(dout + idx);
    float c = (l < L - 1) ? 4.0f : 3.0f;
#pragma unroll
    for (int e = 0; e < 8; e++) o.u[e] = f2bf(bf2f(g.u[e]) / c);
    *(uint4v*)(dmix + idx) = o.v;
}

// Backward merge: the four levels-gradient contributions of one iteration,
// each defined on a range of level slices only (MergeRanges), summed with
// k_add4's expression and operand order; a contribution outside its range
// is not loaded and enters the sum as +0.0f, which is what the zero-filled
// slices of the unmerged path held. Levels below r.dead get +0 without any
// load. POSZ: an exact -0 result is stored as +0, as the autograd add of
// the all-zero trajectory slice made it (bf16(x + 0) == x otherwise).
// NEXT: also dmix_next = bf16(out / c_l) from the value being stored,
// k_mix_bwd's expression, for levels >= r.dead (the previous iteration's
// dmix; nothing reads it below that).
template <bool NEXT>
__global__ __launch_bounds__(NTHREADS) void k_grad_merge(
        const ushort_t* __restrict__ a, const ushort_t* __restrict__ b,
        const ushort_t* __restrict__ c, const ushort_t* __restrict__ dd,
        ushort_t* __restrict__ out, ushort_t* __restrict__ dmix_next,
        long total, int L, int d, MergeRanges r, int posz) {
    long idx = ((long)blockIdx.x * NTHREADS + threadIdx.x) * 8;
    if (idx >= total) return;
    int l = (idx / d) % L;
    union { uint4v v; ushort_t u[8]; } va, vb, vc, vd, o;
    const uint4v z = {0, 0, 0, 0};
    if (l < r.dead) {
        *(uint4v*)(out + idx) = z;
        return;
    }
    va.v = (l >= r.a_lo && l < r.a_hi) ? *(const uint4v*)(a + idx) : z;
    vb.v = (l >= r.b_lo && l < r.b_hi) ? *(const uint4v*)(b + idx) : z;
    vc.v = (l >= r.c_lo && l < r.c_hi) ? *(const uint4v*)(c + idx) : z;
    vd.v = (l >= r.d_lo && l < r.d_hi) ? *(const uint4v*)(dd + idx) : z;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        ushort_t v = f2bf(bf2f(va.u[e]) + bf2f(vb.u[e]) + bf2f(vc.u[e])
                          + bf2f(vd.u[e]));
        if (posz && v == 0x8000) v = 0;
        o.u[e] = v;
    }
    *(uint4v*)(out + idx) = o.v;
    if (NEXT) {
        float cl = (l < L - 1) ? 4.0f : 3.0f;
#pragma unroll
        for (int e = 0; e < 8; e++) o.u[e] = f2bf(bf2f(o.u[e]) / cl);
        *(uint4v*)(dmix_next + idx) = o.v;
    }
}

// td_in[b,n,g,:] = levels[b,n,g+1,:] + pos[n,:]  for g in 0..L-2
// (the top-down input of reference glom_pytorch.py:136, materialized once
// per iteration so the GEMM can stream it with plain 16B loads)
__global__ __launch_bounds__(NTHREADS) void k_add_pos(
        const ushort_t* __restrict__ levels, const ushort_t* __restrict__ pos,
        ushort_t* __restrict__ out, long total, int N, int L, int d) {
    long i8 = ((long)blockIdx.x * NTHREADS + threadIdx.x) * 8;
    if (i8 >= total) return;
    int G = L - 1;
    int q = i8 % d;
    int g = (i8 / d) % G;
    long bn = i8 / ((long)d * G);
    long n = bn % N;
    const ushort_t* lv = levels + (bn * L + g + 1) * (long)d + q;
    const ushort_t* pp = pos + n * (long)d + q;
    union { uint4v v; ushort_t u[8]; } a, b;
    a.v = *(const uint4v*)lv;
    b.v = *(const uint4v*)pp;
#pragma unroll
    for (int e = 0; e < 8; e++) a.u[e] = f2bf(bf2f(a.u[e]) + bf2f(b.u[e]));
    *(uint4v*)(out + i8) = a.v;
}

// ---------------- host launchers ----------------

static inline long cdiv(long a, long b) { return (a + b - 1) / b; }

void launch_add_pos(const void* levels, const void* pos, void* out,
                    long total, int N, int L, int d, hipStream_t s) {
    hipLaunchKernelGGL(k_add_pos, dim3(cdiv(total / 8, NTHREADS)),
                       dim3(NTHREADS), 0, s, (const ushort_t*)levels,
                       (const ushort_t*)pos, (ushort_t*)out, total, N, L, d);
}

void launch_rnorm(const void* levels, float* out, int B, int N, int L, int d,
                  hipStream_t s) {
    long rows = (long)B * N * L;
    hipLaunchKernelGGL(k_rnorm, dim3(cdiv(rows, WPB)), dim3(NTHREADS), 0, s,
                       (const ushort_t*)levels, out, B, N, L, d);
}

void launch_softmax_fwd(const void* scores, void* probs, const bool* mask,
                        int nprob, int N, int self_mask, hipStream_t s) {
    long rows = (long)nprob * N;
    hipLaunchKernelGGL(k_softmax_fwd, dim3(cdiv(rows, WPB)), dim3(NTHREADS),
                       0, s, (const ushort_t*)scores, (ushort_t*)probs, mask,
                       nprob, N, self_mask);
}

void launch_softmax_bwd(const void* P, const void* dP, const float* rnorm,
                        void* dS, void* dSr, const bool* mask, int nprob,
                        int N, int self_mask, float alpha, hipStream_t s,
                        int L, int l_lo) {
    long rows = (long)nprob * N;
    hipLaunchKernelGGL(k_softmax_bwd, dim3(cdiv(rows, WPB)), dim3(NTHREADS),
                       0, s, (const ushort_t*)P, (const ushort_t*)dP, rnorm,
                       (ushort_t*)dS, (ushort_t*)dSr, mask, nprob, N,
                       self_mask, alpha, L, l_lo);
}

void launch_knorm_combine(const void* dkhat, const void* lev,
                          const float* rnorm, const void* dv, const void* dq,
                          void* out, int B, int N, int L, int d,
                          hipStream_t s, int l_lo) {
    long rows = (long)B * N * (L - l_lo);
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_knorm_combine, dim3(cdiv(rows, WPB)), dim3(NTHREADS),
                       0, s, (const ushort_t*)dkhat, (const ushort_t*)lev,
                       rnorm, (const ushort_t*)dv, (const ushort_t*)dq,
                       (ushort_t*)out, B, N, L, d, l_lo);
}

void launch_mix_fwd(const void* prev, const void* bu, const void* td,
                    const void* cons, void* out, long total, int L, int d,
                    hipStream_t s, const void* bu0, long bu0_ld,
                    const void* pos, void* td_next, float* rn_next, int N) {
    dim3 grid(cdiv(total / 8, NTHREADS)), block(NTHREADS);
    if (td_next)
        hipLaunchKernelGGL(k_mix_fwd<true>, grid, block, 0, s,
                           (const ushort_t*)prev, (const ushort_t*)bu,
                           (const ushort_t*)td, (const ushort_t*)cons,
                           (ushort_t*)out, total, L, d, (const ushort_t*)bu0,
                           bu0_ld, (const ushort_t*)pos, (ushort_t*)td_next,
                           rn_next, N);
    else
        hipLaunchKernelGGL(k_mix_fwd<false>, grid, block, 0, s,
                           (const ushort_t*)prev, (const ushort_t*)bu,
                           (const ushort_t*)td, (const ushort_t*)cons,
                           (ushort_t*)out, total, L, d, (const ushort_t*)bu0,
                           bu0_ld, (const ushort_t*)nullptr,
                           (ushort_t*)nullptr, (float*)nullptr, N);
}

bool mix_fwd_can_emit_next(int L, int d) { return d == WAVE * 8 && L >= 2; }

void launch_mix_bwd(const void* dout, void* dmix, void* dtd, long total,
                    int L, int d, hipStream_t s) {
    hipLaunchKernelGGL(k_mix_bwd, dim3(cdiv(total / 8, NTHREADS)), dim3(NTHREADS),
                       0, s, (const ushort_t*)dout, (ushort_t*)dmix,
                       (ushort_t*)dtd, total, L, d);
}

void launch_mix_bwd_lo(const void* dout, void* dmix, long BN, int L, int d,
                       int lo, hipStream_t s) {
    const long live = BN * (long)(L - lo) * d;
    if (live <= 0) return;
    hipLaunchKernelGGL(k_mix_bwd_lo, dim3(cdiv(live / 8, NTHREADS)),
                       dim3(NTHREADS), 0, s, (const ushort_t*)dout,
                       (ushort_t*)dmix, live, L, d, lo);
}

void launch_grad_merge(const void* a, const void* b, const void* c,
                       const void* dd, void* out, void* dmix_next,
                       long total, int L, int d, const MergeRanges& r,
                       bool posz, hipStream_t s) {
    if (total <= 0) return;
    dim3 grid(cdiv(total / 8, NTHREADS)), block(NTHREADS);
    if (dmix_next)
        hipLaunchKernelGGL(k_grad_merge<true>, grid, block, 0, s,
                           (const ushort_t*)a, (const ushort_t*)b,
                           (const ushort_t*)c, (const ushort_t*)dd,
                           (ushort_t*)out, (ushort_t*)dmix_next, total, L, d,
                           r, posz ? 1 : 0);
    else
        hipLaunchKernelGGL(k_grad_merge<false>, grid, block, 0, s,
                           (const ushort_t*)a, (const ushort_t*)b,
                           (const ushort_t*)c, (const ushort_t*)dd,
                           (ushort_t*)out, (ushort_t*)nullptr, total, L, d,
                           r, posz ? 1 : 0);
}

// out = a + b + c + d, elementwise bf16 (the four levels-gradient
// contributions of one GLOM iteration summed in one pass)
__global__ __launch_bounds__(NTHREADS) void k_add4(
        const ushort_t* __restrict__ a, const ushort_t* __restrict__ b,
        const ushort_t* __restrict__ c, const ushort_t* __restrict__ d,
        ushort_t* __restrict__ out, long total) {
    long i8 = ((long)blockIdx.x * NTHREADS + threadIdx.x) * 8;
    if (i8 >= total) return;
    union { uint4v v; ushort_t u[8]; } va, vb, vc, vd, o;
    va.v = *(const uint4v*)(a + i8);
    vb.v = *(const uint4v*)(b + i8);
    vc.v = *(const uint4v*)(c + i8);
    vd.v = *(const uint4v*)(d + i8);
#pragma unroll
    for (int e = 0; e < 8; e++)
        o.u[e] = f2bf(bf2f(va.u[e]) + bf2f(vb.u[e]) + bf2f(vc.u[e])
                      + bf2f(vd.u[e]));
    *(uint4v*)(out + i8) = o.v;
}

void launch_add4(const void* a, const void* b, const void* c, const void* d,
                 void* out, long total, hipStream_t s) {
    hipLaunchKernelGGL(k_add4, dim3(cdiv(total / 8, NTHREADS)),
                       dim3(NTHREADS), 0, s, (const ushort_t*)a,
                       (const ushort_t*)b, (const ushort_t*)c,
                       (const ushort_t*)d, (ushort_t*)out, total);
}

// out = gelu(in), elementwise bf16 (the up-projection's activation pass;
// running this as its own bandwidth-bound kernel beats computing it in the
// GEMM epilogue, which runs at 1 block/CU with nothing to overlap)
__global__ __launch_bounds__(NTHREADS) void k_gelu(
        const ushort_t* __restrict__ in, ushort_t* __restrict__ out,
        long total) {
    long i8 = ((long)blockIdx.x * NTHREADS + threadIdx.x) * 8;
    if (i8 >= total) return;
    union { uint4v v; ushort_t u[8]; } x, o;
    x.v = *(const uint4v*)(in + i8);
    float xin[8], yv[8];
#pragma unroll
    for (int e = 0; e < 8; e++) xin[e] = bf2f(x.u[e]);
    gelu_f_vec<8>(xin, yv);
#pragma unroll
    for (int e = 0; e < 8; e++) o.u[e] = f2bf(yv[e]);
    *(uint4v*)(out + i8) = o.v;
}

void launch_gelu(const void* in, void* out, long total, hipStream_t s) {
    hipLaunchKernelGGL(k_gelu, dim3(cdiv(total / 8, NTHREADS)),
                       dim3(NTHREADS), 0, s, (const ushort_t*)in,
                       (ushort_t*)out, total);
}
