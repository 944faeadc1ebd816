#pragma once
#include <hip/hip_runtime.h>

void launch_add_pos(const void* levels, const void* pos, void* out,
                    long total, int N, int L, int d, hipStream_t s);
void launch_rnorm(const void* levels, float* out, int B, int N, int L, int d,
                  hipStream_t s);
void launch_softmax_fwd(const void* scores, void* probs, const bool* mask,
                        int nprob, int N, int self_mask, hipStream_t s);
// nprob live problems: levels [l_lo, L) of each batch entry, addressed in
// buffers that keep all L levels (defaults: every problem, as laid out)
void launch_softmax_bwd(const void* P, const void* dP, const float* rnorm,
                        void* dS, void* dSr, const bool* mask, int nprob,
                        int N, int self_mask, float alpha, hipStream_t s,
                        int L = 1, int l_lo = 0);
// rows of levels [l_lo, L) only; the other rows of `out` are not written
void launch_knorm_combine(const void* dkhat, const void* lev,
                          const float* rnorm, const void* dv, const void* dq,
                          void* out, int B, int N, int L, int d,
                          hipStream_t s, int l_lo = 0);
// bu0 (optional, row stride bu0_ld elements): level 0 of `bu` is read from
// there. td_next / rn_next (optional, both or neither; need pos, N and
// mix_fwd_can_emit_next): k_add_pos / k_rnorm of `out`, written by the mix
void launch_mix_fwd(const void* prev, const void* bu, const void* td,
                    const void* cons, void* out, long total, int L, int d,
                    hipStream_t s, const void* bu0 = nullptr,
                    long bu0_ld = 0, const void* pos = nullptr,
                    void* td_next = nullptr, float* rn_next = nullptr,
                    int N = 1);
bool mix_fwd_can_emit_next(int L, int d);
void launch_mix_bwd(const void* dout, void* dmix, void* dtd, long total,
                    int L, int d, hipStream_t s);
// dmix = dout / c_l for levels [lo, L) only; no dtd (d % 8 == 0)
void launch_mix_bwd_lo(const void* dout, void* dmix, long BN, int L, int d,
                       int lo, hipStream_t s);
// Level ranges [x_lo, x_hi) in which the four summands of k_grad_merge are
// defined; levels below `dead` are written as +0 without a load.
struct MergeRanges {
    int a_lo, a_hi, b_lo, b_hi, c_lo, c_hi, d_lo, d_hi, dead;
};
// out = bf16(a + b + c + dd) over (B,N,L,d), out-of-range summands +0;
// dmix_next (optional) = bf16(out / c_l) for levels >= r.dead; posz stores
// an exact -0 sum as +0 (d % 8 == 0, total = B*N*L*d)
void launch_grad_merge(const void* a, const void* b, const void* c,
                       const void* dd, void* out, void* dmix_next,
                       long total, int L, int d, const MergeRanges& r,
                       bool posz, hipStream_t s);
void launch_add4(const void* a, const void* b, const void* c, const void* d,
                 void* out, long total, hipStream_t s);
void launch_gelu(const void* in, void* out, long total, hipStream_t s);
