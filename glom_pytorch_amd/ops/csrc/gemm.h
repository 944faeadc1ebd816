// Shared host/device parameter block for the generic GLOM GEMM.
#pragma once

#include <hip/hip_runtime.h>

enum GemmLayout { LAYOUT_NT = 0, LAYOUT_NN = 1, LAYOUT_TN = 2 };
enum OpFlags { OP_GELU = 1, OP_POS = 2, OP_TABLE = 4 };
enum GemmEpilogue {
    EPI_NONE = 0,
    EPI_GELUGRAD = 1,
    EPI_GELU_PAIR = 2,
    // full-row fusions (tile spans the whole row, nt_fast4 only):
    EPI_SOFTMAX = 3,   // consensus scores -> masked row softmax -> P
    EPI_SMBWD = 4,     // dP -> row softmax backward -> dS (C), dSr (out2)
    // C = gelu(bf16(acc*alpha + bias)): EPI_GELU_PAIR's out2 without the
    // pre-activation (forward-only steps; nt5p only, see run_gemm)
    EPI_GELU = 5,
    // column-contrastive (InfoNCE) loss over cosine logits; the logits are
    // never stored (contrast.py, gemm_epilogue_nce). Hosts: the generic
    // kernel and gemm_nt_fast only, see run_gemm.
    EPI_NCE_FWD = 6,   // part[i][tile] = sum_j exp(s_ij - 1/T), pos[i] = s_ii
    EPI_NCE_BWD = 7,   // C = G' (bf16), part[i][tile] = sum_j g_ij * s_ij
};

#define GEMM_MAX_TABLE 16

// Per-operand addressing: strided mode resolves problem p's base pointer as
//   base + (p % nInner) * sin + (p / nInner) * sout      (element strides)
// or, when OP_TABLE is set, from the explicit pointer table (<=16 problems).
struct OpArg {
    const void* base;
    long sin, sout;
    long ld;     // leading (row) stride in elements
    int flags;   // OP_GELU | OP_POS | OP_TABLE
};

struct GemmParams {
    int M, N, K;
    int layout;          // GemmLayout
    int nproblems, nInner;
    int npatch;          // pos-emb row period for OP_POS
    int epilogue;        // GemmEpilogue
    float alpha;

    OpArg A, B;

    void* Cbase; long Csin, Csout, Cld; int Cflags;

    const void* bias_base; long bias_sin, bias_sout; int has_bias;
    const void* colscale_base; long cs_sin, cs_sout; int has_colscale;
    const void* aux_base; long aux_sin, aux_sout, aux_ld;

    const void* pos; long pos_ld;

    // optional fused column sum of C over the row axis (bias gradient):
    // the 256-wide NT kernels store per-row-span partial column sums into
    // colsum_out[p][M/64][N] (f32, no atomics: every (64-row slot, column)
    // has exactly one writer; a writer spanning several slots zeroes the
    // rest) during the epilogue, saving a full re-read of C. The caller
    // reduces the slots in fixed order (launch_colsum_fin), so the result
    // is run-to-run bitwise reproducible. colsum_sin = (M/64)*N.
    float* colsum_out; long colsum_sin;

    // attention-fusion extras (EPI_SOFTMAX / EPI_SMBWD)
    const void* nlmask;     // optional (N,N) bool non-local mask
    int self_mask;          // fill diagonal with -5e-4 before softmax
    float alpha2;           // d^-0.5 applied inside EPI_SMBWD

    // split-K (reduction split): when > 1, the kernel writes per-slice f32
    // partials into ws[slice][problem][M][N] and gemm_finish sums them into
    // C (only EPI_NONE, no bias/colscale). Used for the weight-grad GEMMs
    // whose natural grids underfill the 256 CUs (K = B*N tokens is huge).
    int splitk; float* ws;

    // EPI_GELU_PAIR: C gets the pre-activation (acc*alpha + bias), out2
    // gets gelu(pre-activation). Used by the FF up-projection so the
    // down-projection streams plain activations.
    void* out2; long out2_sin, out2_sout, out2_ld;

    // host-verified: every A/B row stride is a multiple of 8 elements and
    // tiles are full -> the glds/repack fast kernels may run
    int fast_ok;

    // host-verified: C / out2 / aux bases are 16-byte aligned and their row
    // strides multiples of 8 elements -> the register epilogues of nt5p
    // and nt8p may use 16-byte accesses (set by run_gemm): bit 0 = C/out2
    // stores, bit 1 = aux loads
    int wide_epi;

    const void* Atab[GEMM_MAX_TABLE]; long Atabld[GEMM_MAX_TABLE];
    const void* Btab[GEMM_MAX_TABLE]; long Btabld[GEMM_MAX_TABLE];
    void* Ctab[GEMM_MAX_TABLE]; long Ctabld[GEMM_MAX_TABLE];
};

// EPI_NCE_FWD / EPI_NCE_BWD arguments (single plain problem). GEMM row i is
// logit row row0 + i, GEMM column j is logit column j;
// s = acc * rrow[row] * rcol[col] * invt. A pair is allowed iff row == col,
// or all, or row / group != col / group. part[i][ceil(N/128)] gets one f32
// per (GEMM row, 128-column tile) from exactly one writer. BWD reads the
// saved log-sum-exp by row, or by column when lse_col is set (the
// operand-swapped dB pass), and scales g by invm = 1 / (logit rows).
// They travel in GemmParams fields that these epilogues do not otherwise
// use (no bias, column scale, aux, out2 or fused colsum), so the parameter
// block keeps its size and the other kernels their code:
//   rrow = bias_base   rcol = colscale_base   lse = aux_base
//   part = colsum_out  pos = out2             row0 = bias_sin
//   invt = alpha       invm = alpha2          group = npatch
//   self_mask: bit 0 = all, bit 1 = lse_col
struct NceArgs {
    const float* rrow; const float* rcol; const float* lse;
    float* part; float* pos;
    float invt, invm;
    int group, all, lse_col, row0, ntn;
};

static inline void nce_set(GemmParams& p, const NceArgs& a) {
    p.bias_base = a.rrow; p.colscale_base = a.rcol; p.aux_base = a.lse;
    p.colsum_out = a.part; p.out2 = a.pos; p.bias_sin = a.row0;
    p.alpha = a.invt; p.alpha2 = a.invm; p.npatch = a.group;
    p.self_mask = (a.all ? 1 : 0) | (a.lse_col ? 2 : 0);
    p.has_bias = p.has_colscale = 0;
}

__host__ __device__ static inline NceArgs nce_get(const GemmParams& p) {
    NceArgs a;
    a.rrow = (const float*)p.bias_base;
    a.rcol = (const float*)p.colscale_base;
    a.lse = (const float*)p.aux_base;
    a.part = p.colsum_out; a.pos = (float*)p.out2;
    a.invt = p.alpha; a.invm = p.alpha2;
    a.group = p.npatch; a.all = p.self_mask & 1;
    a.lse_col = (p.self_mask >> 1) & 1;
    a.row0 = (int)p.bias_sin; a.ntn = (p.N + 127) / 128;
    return a;
}

void launch_gemm(const GemmParams& p, hipStream_t stream);
// wide: re-blocked 16-byte kernel where C allows it (same bits)
void launch_gemm_finish(const GemmParams& p, hipStream_t stream,
                        bool wide = true);
void launch_gemm_nt_fast(const GemmParams& p, hipStream_t stream);
void launch_gemm_tn_fast(const GemmParams& p, hipStream_t stream);
void launch_gemm_nn_fast(const GemmParams& p, hipStream_t stream);
// split-K NN (gemm_nn_sk.hip): f32 partials into p.ws[slice][problem][M][N]
void launch_gemm_nn_sk(const GemmParams& p, hipStream_t stream);
void launch_gemm_nt_fast4(const GemmParams& p, hipStream_t stream);
void launch_gemm_nt_fast5p(const GemmParams& p, hipStream_t stream);
void launch_gemm_nt_fast8p(const GemmParams& p, hipStream_t stream);
void launch_gemm_tn_sk(const GemmParams& p, hipStream_t stream);
// direct-to-LDS + transposed-read TN kernel; variant: see gemm_fast.hip
void launch_gemm_tn_tr(const GemmParams& p, int variant, hipStream_t stream);
