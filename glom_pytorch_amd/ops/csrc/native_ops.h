// Native-mandate kernels: patch embedding data movement, deterministic
// column-sum / positional-embedding gradient reductions, slice zero-fill,
// and the fused AdamW optimizer update. See native_ops.hip.
#pragma once
#include <hip/hip_runtime.h>

void launch_patchify(const void* img, void* X, int B, int C, int H, int W,
                     int P, int Kp, hipStream_t s);
void launch_unpatchify(const void* dX, void* dImg, int B, int C, int H,
                       int W, int P, int Kp, hipStream_t s);
void launch_pad_cols(const void* src, void* dst, long rows, int Kin, int Kp,
                     hipStream_t s);
void launch_slice_cols(const void* src, void* dst, long rows, int Kp,
                       int Kin, hipStream_t s);
// in (P, M, C) bf16 -> out (P, C) bf16, f32 accumulation, deterministic
// two-stage reduction through the caller-provided f32 partials buffer of
// shape (P, RB, C) where RB = colsum_rb(M).
int colsum_rb(long M);
void launch_colsum(const void* in, float* partials, void* out, int nprob,
                   long M, long C, hipStream_t s);
// second stage alone: partials (P, RB, C) f32 -> out (P, C) bf16, summed in
// fixed order (for partials written by a GEMM's fused-colsum epilogue).
void launch_colsum_fin(const float* partials, void* out, int nprob, long C,
                       int RB, hipStream_t s);
// in (M, C) bf16 with row stride ld: out (C,) = column sums of the columns
// [c_lo, C) in launch_colsum's order and bits, +0 below c_lo; out2
// (optional) = a copy of out[:C2]. partials: (colsum_rb(M), C) f32.
void launch_colsum_cone(const void* in, float* partials, void* out,
                        void* out2, long M, long C, long C2, long ld,
                        long c_lo, hipStream_t s);
// dLevels (B,N,L,d) -> dPos (N,d) = sum over b and l in [l0,L), l0 < L.
// partials: caller-provided (BCH, N, d) f32 workspace (BCH batch chunks);
// pass nullptr/0 for the scalar single-stage fallback.
void launch_dpos(const void* dlev, void* out, float* partials, int BCH,
                 int B, int N, int L, int d, hipStream_t s, int l0 = 1);
// zero the single level slice out[:, :, l0, :] of a (B,N,L,d) tensor
void launch_zero_slice(void* out, long BN, int L, int d, int l0,
                       hipStream_t s);
// zero the level slices out[:, :, l0 : l0 + nl, :]; nl <= 0 launches nothing
void launch_zero_slices(void* out, long BN, int L, int d, int l0, int nl,
                        hipStream_t s);

// ---------------- fused AdamW ----------------
#define OPT_MAX_T 24

struct OptTable {
    int nt;
    const unsigned short* g[OPT_MAX_T];   // bf16 grads
    float* mw[OPT_MAX_T];                 // fp32 master weights
    float* m1[OPT_MAX_T];                 // exp_avg
    float* m2[OPT_MAX_T];                 // exp_avg_sq
    unsigned short* pw[OPT_MAX_T];        // bf16 params (written back)
    long cum[OPT_MAX_T + 1];              // prefix numel offsets
};

#define OPT_NPART 1024

// deterministic global grad L2 norm: partials (OPT_NPART f32) -> norm[0];
// the finalize kernel also increments step_dev[0] by 1 (single block).
void launch_grad_norm(const OptTable& t, float* partials, float* norm,
                      float* step_dev, hipStream_t s);
// AdamW update (torch.optim.AdamW semantics incl. decoupled weight decay
// and bias correction), with the global-norm gradient clip fused:
// scale = min(1, max_norm / (norm + 1e-6)) applied to every grad read.
void launch_adamw(const OptTable& t, float lr, float b1, float b2, float eps,
                  float wd, float max_norm, const float* norm,
                  const float* step_dev, hipStream_t s);

// ---- scheduled variant: lr lives in device memory ----
// fp32 hyperparameter block owned by the optimizer (OPT_H_SIZE floats)
#define OPT_H_BASE_LR 0
#define OPT_H_KIND 1        // 0 constant, 1 linear decay, 2 cosine decay
#define OPT_H_WARMUP 2
#define OPT_H_TOTAL 3
#define OPT_H_MIN_RATIO 4
#define OPT_H_LR_T 5        // output: this step's lr, written by finalize
#define OPT_H_SIZE 8

// per-tensor hyperparameters, indexed like OptTable
struct OptGroups {
    float lr_scale[OPT_MAX_T];
    float wd[OPT_MAX_T];
};

// launch_grad_norm whose finalize kernel also evaluates the schedule at the
// incremented step count and writes hyper[OPT_H_LR_T] = base_lr * f(step).
void launch_grad_norm_sched(const OptTable& t, float* partials, float* norm,
                            float* step_dev, float* hyper, hipStream_t s);
// launch_adamw with lr = hyper[OPT_H_LR_T] * lr_scale[ti] and wd[ti] per
// tensor; same arithmetic, bit-identical for lr_scale == 1 and equal lr.
void launch_adamw_sched(const OptTable& t, const OptGroups& h, float b1,
                        float b2, float eps, float max_norm,
                        const float* norm, const float* step_dev,
                        const float* hyper, hipStream_t s);
