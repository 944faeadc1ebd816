// Torch bindings: compose the generic MFMA GEMM + row-wise kernels into the
// five GLOM hot-path ops (grouped FF fwd/bwd, consensus attention fwd/bwd,
// level mix fwd/bwd). Layout contracts follow SURVEY.md §2.2/§2.3; the
// grouped-conv weights (G*mult*d, d, 1)/(G*d, mult*d, 1) are consumed
// directly as G packed GEMM operands.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "gemm.h"
#include "aux_kernels.h"
#include "native_ops.h"
#include "island_kernels.h"
#include "parse_kernels.h"
#include "contrast_kernels.h"

namespace {

// Untracked alias of `base` (shares storage, keeps it alive, but has its
// own TensorImpl/version counter). Used for trajectory-slab slices: a
// custom Function may return such an alias even though later steps write
// other slices of the same slab — a torch view would trip the
// view+inplace guard.
torch::Tensor alias_slab_slice(const torch::Tensor& slab, int64_t idx,
                               c10::IntArrayRef sizes) {
    int64_t n = 1;
    for (auto s : sizes) n *= s;
    void* ptr = (char*)slab.data_ptr() + idx * n * slab.element_size();
    auto keep = slab;   // captured by the deleter -> storage stays alive
    return torch::from_blob(
        ptr, sizes, [keep](void*) mutable {}, slab.options());
}

#define CHECK_IN(x)                                                        \
    TORCH_CHECK(x.is_cuda(), #x " must be on GPU");                        \
    TORCH_CHECK(x.is_contiguous(), #x " must be contiguous");              \
    TORCH_CHECK(x.scalar_type() == at::kBFloat16, #x " must be bf16")

hipStream_t cur_stream() {
    return c10::hip::getCurrentHIPStream().stream();
}

// nt8p dispatch mode: default ON for K>=2048 shapes (GLOM_NT8P=0 opts
// out; set_nt8p() for within-process A/B, guide §5.4 rule 24). History:
// +15% on the down-projection microbench but -1% end-to-end under the
// pre-overlap stream mix; with the forward-tail/backward overlap the
// balance flipped and nt8p measures +1.8% e2e (1437 -> 1463 img/s,
// same box) — see profiles/README.md round-2 notes.
int g_nt8p_mode = []() {
    const char* e = getenv("GLOM_NT8P");
    return (e && e[0] == '0') ? 0 : 1;
}();

void set_nt8p(bool on) { g_nt8p_mode = on ? 1 : 0; }

// TN kernel with direct-to-LDS staging and transposed LDS reads
// (gemm_tn_tr): bit-identical to gemm_tn_fast / gemm_tn_sk, so this is a
// pure speed switch.
//   0 = never (GLOM_TN_TR=0): the repack kernels, as before
//   1 = where it measured faster (default; tn_tr_auto below)
//   2 = every eligible TN call
// set_tn_tr(bool) picks 2 / 0 and set_tn_tr_mode(int) any of them, for
// within-process A/B (scripts/tn_tr_ab.py) and the tests. The variant is
// the split-K pipeline point (1: BK 64 x 2 buffers, 2: BK 32 x 3-ring,
// 3: BK 32 x 2 buffers; GLOM_TN_TR_VARIANT / set_tn_tr_variant).
int g_tn_tr = []() {
    const char* e = getenv("GLOM_TN_TR");
    return (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 1;
}();
int g_tn_tr_variant = []() {
    const char* e = getenv("GLOM_TN_TR_VARIANT");
    return (e && e[0] >= '1' && e[0] <= '3') ? e[0] - '0' : 1;
}();
void set_tn_tr(bool on) { g_tn_tr = on ? 2 : 0; }
void set_tn_tr_mode(int64_t m) {
    TORCH_CHECK(m >= 0 && m <= 2, "tn_tr mode is 0..2");
    g_tn_tr = (int)m;
}
int64_t get_tn_tr_mode() { return g_tn_tr; }
void set_tn_tr_variant(int64_t v) {
    TORCH_CHECK(v >= 1 && v <= 3, "tn_tr variant is 1..3");
    g_tn_tr_variant = (int)v;
}
int64_t get_tn_tr_variant() { return g_tn_tr_variant; }
// Default policy, from the op-level A/B (profiles/tn_tr_ab.txt): every
// split-K call and the non-split ones measured at K = 4096 and 8192 win
// (min above the repack kernels' max); at K = 1024 and the K = 256
// attention dv / dk-hat the two are level, and with those on the new
// kernel the headline step measured slower (its 64 KiB arena against
// tn_fast's 34 KiB), so short-K non-split calls keep gemm_tn_fast
static bool tn_tr_auto(const GemmParams& p) {
    return p.splitk > 1 || p.K >= 4096;
}
// Re-blocked split-K finish (gemm_finish4, 16-byte slab loads): same bits
// as the scalar kernel. GLOM_FINISH_WIDE=0 / set_finish_wide(false) revert.
int g_finish_wide = []() {
    const char* e = getenv("GLOM_FINISH_WIDE");
    return (e && e[0] == '0') ? 0 : 1;
}();
void set_finish_wide(bool on) { g_finish_wide = on ? 1 : 0; }

// GELU placement: 0 = standalone bandwidth pass after the up-projection
// (round-1 measurement); 1 = EPI_GELU_PAIR fused into the up-projection
// epilogue (nt5p register epilogue writes both Hpre and gelu(Hpre),
// saving the standalone pass's full re-read of Hpre).
// Default ON: bitwise-identical to the standalone pass and measured
// 0.74 -> 0.71 ms on the headline ff-forward (saves the standalone
// pass's full Hpre re-read); e2e within noise. GLOM_GELU_PAIR=0 reverts.
int g_gelu_pair = []() {
    const char* e = getenv("GLOM_GELU_PAIR");
    return (e && e[0] == '0') ? 0 : 1;
}();
void set_gelu_pair(bool on) { g_gelu_pair = on ? 1 : 0; }

// Register-epilogue width of the nt5p kernel: the rounded bf16 values can
// be transposed in registers and moved as 16-byte accesses instead of the
// 2-byte fragment-order ones; bitwise identical results either way.
//   0 = narrow everywhere (GLOM_WIDE_EPI=0)
//   1 = per epilogue, what measured faster (default; wide_epi_auto below)
//   2 = wide everywhere: stores and aux loads
//   3 = wide aux loads, narrow stores
// set_wide_epilogue(bool) picks 2 / 0 and set_wide_epilogue_mode(int) any
// of them, for within-process A/B (scripts/wide_epi_ab.py) and the tests.
int g_wide_epi = []() {
    const char* e = getenv("GLOM_WIDE_EPI");
    return (e && e[0] >= '0' && e[0] <= '3') ? e[0] - '0' : 1;
}();
// nt8p has its own switch: its tail is a smaller share of a K >= 2048
// tile, so it is judged (and defaulted) separately (GLOM_WIDE_EPI_NT8P)
int g_wide_epi_nt8p = []() {
    const char* e = getenv("GLOM_WIDE_EPI_NT8P");
    return (e && e[0] == '1') ? 1 : 0;
}();
void set_wide_epilogue(bool on) { g_wide_epi = on ? 2 : 0; }
void set_wide_epilogue_mode(int64_t m) {
    TORCH_CHECK(m >= 0 && m <= 3, "wide epilogue mode is 0..3");
    g_wide_epi = (int)m;
}
int64_t get_wide_epilogue_mode() { return g_wide_epi; }
// Default policy, from the op-level A/B at the headline shapes
// (profiles/wide_epilogue_ab.txt): dH gains from the early 16-byte aux
// loads, the single-output EPI_GELU a little from wide stores; with two
// output streams (EPI_GELU_PAIR) the wide stores measured no gain, with a
// plain C ~2% slower than the 2-byte ones, so both stay off.
static int wide_epi_auto(int epilogue) {
    return epilogue == EPI_GELUGRAD ? 3 : epilogue == EPI_GELU ? 1 : 0;
}
// GemmParams::wide_epi bits (1 = stores, 2 = aux loads) for nt5p
static int nt5p_wide_bits(int epilogue) {
    switch (g_wide_epi) {
    case 0: return 0;
    case 2: return 3;
    case 3: return 2;
    default: return wide_epi_auto(epilogue);
    }
}
void set_wide_epilogue_nt8p(bool on) { g_wide_epi_nt8p = on ? 1 : 0; }

// 16-byte accesses need 16-byte-aligned bases and row / problem strides
// that are multiples of 8 bf16 elements
static bool wide_epi_ok(const GemmParams& p) {
    auto al = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    bool ok = al(p.Cbase) && p.Cld % 8 == 0 && p.Csin % 8 == 0
              && p.Csout % 8 == 0;
    if (p.epilogue == EPI_GELU_PAIR)
        ok = ok && al(p.out2) && p.out2_ld % 8 == 0 && p.out2_sin % 8 == 0
             && p.out2_sout % 8 == 0;
    if (p.epilogue == EPI_GELUGRAD)
        ok = ok && al(p.aux_base) && p.aux_ld % 8 == 0 && p.aux_sin % 8 == 0
             && p.aux_sout % 8 == 0;
    return ok;
}

// persistent continuous-ring variant (default ON; opt out with
// GLOM_NT5P=0): one block sweeps 4 M-tiles of a column, register
// epilogue in the shadow of the next tile's MFMAs, fused colsum kept
static bool nt5p_enabled() {
    static const bool on = []() {
        const char* e = getenv("GLOM_NT5P");
        return !e || e[0] != '0';
    }();
    return on;
}
static long nt5p_min_grid() {
    static const long g = []() {
        const char* e = getenv("GLOM_NT5P_MING");
        return e ? atol(e) : 96;
    }();
    return g;
}
// Will run_gemm route this up-projection (bf16 NT, contiguous operands,
// plain C) to nt5p? Mirrors run_gemm's conditions for that shape family;
// run_gemm itself rejects EPI_GELU if the two ever disagree.
static bool nt5p_takes_up_proj(int64_t M, int64_t N, int64_t K, int64_t G) {
    return nt5p_enabled() && M % 512 == 0 && N % 256 == 0 && N >= 1024
           && K % 64 == 0 && K >= 64
           && (N / 256) * (M / 512) * G >= nt5p_min_grid();
}

void check_launch() {
    hipError_t e = hipGetLastError();
    TORCH_CHECK(e == hipSuccess, "HIP launch failed: ", hipGetErrorString(e));
}

// launches of the column-contrastive epilogues by hosting kernel, for the
// tests: {gemm_nt_fast, generic}
int64_t g_nce_launches[2] = {0, 0};
std::vector<int64_t> nce_launch_counts() {
    return {g_nce_launches[0], g_nce_launches[1]};
}
// A/B switch (scripts/contrast_bench.py): false sends the EPI_NCE_* GEMMs
// to the generic kernel even where gemm_nt_fast is eligible. Both hosts run
// the same epilogue code. Measured at M = 16384, D = 512: the fast host is
// 1.6x faster forward, 1.3x forward+backward (profiles/contrast_bench.txt).
int g_nce_fast = []() {
    const char* e = getenv("GLOM_NCE_FAST");
    return (e && e[0] == '0') ? 0 : 1;
}();
void set_nce_fast(bool on) { g_nce_fast = on ? 1 : 0; }

// Epilogue preconditions, checked here or by the callers named:
//   EPI_NONE / bias / colscale  every kernel
//   EPI_GELUGRAD, EPI_GELU_PAIR every kernel; aux / out2 set
//   EPI_SOFTMAX, EPI_SMBWD      nt_fast4 only, launched directly by the
//                               consensus ops (N == 256, d % 64 == 0)
//   EPI_GELU                    nt5p only (ask nt5p_takes_up_proj() first)
//   EPI_NCE_FWD, EPI_NCE_BWD    NT, one problem, no table / bias / colscale,
//                               arguments via nce_set(); generic kernel for any shape,
//                               gemm_nt_fast for full tiles (M, N % 128,
//                               K % 64, rows % 8 elements, 16-byte bases; BWD
//                               also C 16-byte aligned with Cld % 8); never
//                               the 256-wide kernels
// Central dispatcher: picks the tuned full-tile kernels (glds NT / repack
// TN) when the host-verified preconditions hold, applies split-K when the
// natural grid underfills the 256 CUs (the weight-grad TN GEMMs: tiny
// output, K = B*N tokens; partial f32 slabs summed by gemm_finish), and
// otherwise falls back to the generic predicated kernel.
// `lds_ok` asserts every A/B row stride (incl. table entries) is %8 == 0.
// `gate_problems` (0 = p.nproblems): the problem count the grid gates
// (split-K factor, nt5p and nt8p minimum grids) are judged by. Callers that
// launch only the live tail of a grouped problem (level cone, see
// grouped_ff_bwd) pass the full group count, so every live group is served
// by the kernel and split-K factor the full call gives it: same bits. It
// stays on the host; the kernels see only the live problems.
void run_gemm(GemmParams& p, hipStream_t s, const torch::TensorOptions& opts,
              bool lds_ok, long gate_problems = 0) {
    const long gate_np = gate_problems > 0 ? gate_problems : p.nproblems;
    const bool no_xform = !(p.A.flags & (OP_GELU | OP_POS))
                          && !(p.B.flags & (OP_GELU | OP_POS));
    const bool nce_generic = !g_nce_fast && (p.epilogue == EPI_NCE_FWD
                                             || p.epilogue == EPI_NCE_BWD);
    const bool nt_fast = p.layout == LAYOUT_NT && lds_ok && no_xform
                         && p.M % 128 == 0 && p.N % 128 == 0
                         && p.K % 64 == 0 && p.K >= 64 && !nce_generic;
    const bool tn_fast = p.layout == LAYOUT_TN && lds_ok && no_xform
                         && p.M % 128 == 0 && p.N % 128 == 0 && p.K % 8 == 0;
    const bool nn_fast = p.layout == LAYOUT_NN && lds_ok && no_xform
                         && p.M % 128 == 0 && p.N % 128 == 0 && p.K % 8 == 0;

    p.splitk = 1;
    p.ws = nullptr;
    torch::Tensor ws;
    long blocks = ((p.N + 127) / 128) * ((p.M + 127) / 128) * gate_np;
    if (p.layout == LAYOUT_TN && p.epilogue == EPI_NONE && !p.has_bias
        && !p.has_colscale && blocks < 1024 && p.K >= 4096) {
        long sk = std::min<long>(16, std::max<long>(1, 2048 / blocks));
        sk = std::min<long>(sk, p.K / 64);
        if (sk > 1) {
            ws = torch::empty({sk * p.nproblems * (long)p.M * p.N},
                              opts.dtype(at::kFloat));
            p.splitk = (int)sk;
            p.ws = ws.data_ptr<float>();
        }
    }
    const bool nce = p.epilogue == EPI_NCE_FWD || p.epilogue == EPI_NCE_BWD;
    if (nce) {
        auto al = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
        TORCH_CHECK(p.layout == LAYOUT_NT && p.nproblems == 1
                    && !((p.A.flags | p.B.flags | p.Cflags) & OP_TABLE)
                    && !p.has_bias && !p.has_colscale,
                    "EPI_NCE_* needs one plain NT problem");
        const NceArgs q = nce_get(p);
        TORCH_CHECK(q.rrow && q.rcol && q.part && q.group > 0,
                    "EPI_NCE_* parameters not set (nce_set)");
        TORCH_CHECK(p.epilogue == EPI_NCE_FWD ? q.pos != nullptr
                                              : (q.lse && p.Cbase),
                    "EPI_NCE_* outputs not set");
        TORCH_CHECK(!nt_fast
                    || (al(p.A.base) && al(p.B.base)
                        && (p.epilogue == EPI_NCE_FWD
                            || (al(p.Cbase) && p.Cld % 8 == 0))),
                    "EPI_NCE_* full-tile path needs 16-byte aligned operands");
    }
    const bool nt3 = nt_fast && p.N % 256 == 0 && p.N >= 1024 && !nce;
    const bool nt5p_on = nt5p_enabled();
    // N >= 1024 only: at N=512 (2 column panels) the persistent sweep
    // measured SLOWER than the 128^2 kernel on the down-projection
    // (637 -> 573 TF), so that shape keeps nt_fast
    // >= 96 (was 256): at the small-batch inference shapes (video B=8:
    // 192-block grids) the persistent sweep beats nt3 by ~20% (3172 ->
    // 3812 frames/s); training grids are >= 768 and unaffected.
    const bool nt5p = nt5p_on && nt3 && p.M % 512 == 0
                      && (long)(p.N / 256) * (p.M / 512) * gate_np
                         >= nt5p_min_grid()
                      && !(p.Cflags & OP_TABLE)
                      && (p.epilogue == EPI_NONE
                          || p.epilogue == EPI_GELUGRAD
                          || p.epilogue == EPI_GELU_PAIR
                          || p.epilogue == EPI_GELU);
    // only nt5p's register epilogue implements EPI_GELU; callers ask
    // nt5p_takes_up_proj() first and keep EPI_GELU_PAIR / the standalone
    // gelu pass otherwise
    TORCH_CHECK(p.epilogue != EPI_GELU || nt5p,
                "EPI_GELU needs an nt5p-eligible shape");
    static const bool disp_dbg = []() {
        const char* e = getenv("GLOM_DISPATCH_DEBUG");
        return e && e[0] == '1';
    }();
    // 8-phase 256^2 schedule (guide §5 template): per-phase interleave of
    // ds_read / glds / MFMA with counted per-wave vmcnt. GLOM_NT8P=0
    // opts out; set_nt8p() lets microbenches A/B within one process.
    const bool nt8p_on = g_nt8p_mode == 1;
    // measured (profiles/README.md): the 256^2 8-phase tile wins at
    // K >= 2048 (down-projection 685 -> 789 TF, square parity+), while
    // the K=512 up-projection family stays on nt5p's persistent ring
    // (8-phase loses its prologue amortization at 8 K-steps/tile)
    static const long nt8p_mink = []() {
        const char* e = getenv("GLOM_NT8P_MINK");
        return e ? atol(e) : 2048;
    }();
    const bool nt8p = nt8p_on && p.layout == LAYOUT_NT && lds_ok && no_xform
                      && p.M % 256 == 0 && p.N % 256 == 0 && p.K % 64 == 0
                      && p.K >= nt8p_mink
                      && !(p.Cflags & OP_TABLE)
                      && (p.epilogue == EPI_NONE
                          || p.epilogue == EPI_GELUGRAD)
                      && (long)(p.N / 256) * (p.M / 256) * gate_np >= 256;
    // whole K-steps only: K % 64 == 0 makes every split-K slice (`per` is
    // a multiple of 64) a whole number of stages; K % 8 tails stay on the
    // repack kernels. 16-byte DMA sources need 16-byte-aligned bases.
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    bool tn_al = al16(p.A.base) && al16(p.B.base);
    if (p.A.flags & OP_TABLE)
        for (int g = 0; g < p.nproblems; g++) tn_al = tn_al && al16(p.Atab[g]);
    if (p.B.flags & OP_TABLE)
        for (int g = 0; g < p.nproblems; g++) tn_al = tn_al && al16(p.Btab[g]);
    const bool tn_tr = (g_tn_tr == 2 || (g_tn_tr == 1 && tn_tr_auto(p)))
                       && tn_fast && p.K % 64 == 0 && p.K >= 64
                       && tn_al && p.A.sin % 8 == 0 && p.A.sout % 8 == 0
                       && p.B.sin % 8 == 0 && p.B.sout % 8 == 0;
    p.wide_epi = !wide_epi_ok(p) ? 0
                 : nt8p ? g_wide_epi_nt8p : nt5p_wide_bits(p.epilogue);
    if (disp_dbg)
        fprintf(stderr,
                "[dispatch] L%d M%ld N%ld K%ld epi%d nt3=%d nt5p=%d on=%d "
                "nt8p=%d ctabflag=%d m512=%d tn_tr=%d sk=%d finw=%d "
                "kern=%s\n",
                p.layout, (long)p.M, (long)p.N, (long)p.K, p.epilogue,
                (int)nt3, (int)nt5p, (int)nt5p_on, (int)nt8p,
                (int)(p.Cflags & OP_TABLE), (int)(p.M % 512 == 0),
                tn_tr ? (p.splitk > 1 ? g_tn_tr_variant : 1) : 0,
                p.splitk, g_finish_wide,
                nt8p ? "nt8p" : nt5p ? "nt5p" : nt3 ? "nt4"
                : nt_fast ? "nt_fast" : tn_tr ? "tn_tr"
                : tn_fast ? (p.splitk > 1 ? "tn_sk" : "tn_fast")
                : nn_fast ? "nn_fast" : "generic");
    if (nt8p)
        launch_gemm_nt_fast8p(p, s);
    else if (nt5p)
        launch_gemm_nt_fast5p(p, s);
    else if (nt3)
        launch_gemm_nt_fast4(p, s);   // 3-ring counted-vmcnt variant
    else if (nt_fast) {
        launch_gemm_nt_fast(p, s);
        if (nce) g_nce_launches[0]++;
    }
    else if (tn_tr)
        launch_gemm_tn_tr(p, g_tn_tr_variant, s);
    else if (tn_fast && p.splitk > 1)
        launch_gemm_tn_sk(p, s);     // 32KB arena: 4 blocks/CU for the
    else if (tn_fast)                // weight-grad split-K launches
        launch_gemm_tn_fast(p, s);
    else if (nn_fast)
        launch_gemm_nn_fast(p, s);
    else {
        launch_gemm(p, s);
        if (nce) g_nce_launches[1]++;
    }
    check_launch();
    if (p.splitk > 1) {
        launch_gemm_finish(p, s, g_finish_wide == 1);
        check_launch();
    }
}

GemmParams base_params(int64_t M, int64_t N, int64_t K, int layout,
                       int64_t nproblems, int64_t nInner, float alpha) {
    GemmParams p;
    std::memset(&p, 0, sizeof(p));
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    p.layout = layout;
    p.nproblems = (int)nproblems;
    p.nInner = (int)nInner;
    p.alpha = alpha;
    p.epilogue = EPI_NONE;
    return p;
}

// ------------------------------------------------------------------ //
// Level cone (docs/ARCHITECTURE.md "Level cone"): the backward ops take the
// first live group / level (`g_lo`, `l_lo`, default 0 = everything). The
// caller promises that the incoming gradient is exactly zero below it, so
// the GEMMs run on the live tail only (bases and tables offset, nproblems
// shrunk, gates judged by the full count) and what the dead groups would
// have produced, zeros, is filled in. Shapes never change.

// element `off` of a bf16 tensor
void* u16_at(const torch::Tensor& t, int64_t off) {
    return (void*)((uint16_t*)t.data_ptr() + off);
}

void zero_fill(void* ptr, int64_t bytes, hipStream_t s) {
    if (bytes <= 0) return;
    hipError_t e = hipMemsetAsync(ptr, 0, (size_t)bytes, s);
    TORCH_CHECK(e == hipSuccess, "zero fill failed: ", hipGetErrorString(e));
}

// Level slices of the FF data gradient dLevels (B,N,L,d) that no live
// group's dX writes. Bottom-up group g >= 1 writes slice g-1 (group 0
// writes dTokens), top-down group g writes slice g+1.
void zero_unwritten_dx(void* dLevels, int64_t BN, int64_t L, int64_t d,
                       int64_t mode, int64_t g_lo, hipStream_t s) {
    if (mode == 0) {
        // written: [max(g_lo, 1) - 1, L - 1); the top slice never is
        launch_zero_slices(dLevels, BN, (int)L, (int)d, 0,
                           (int)std::max<int64_t>(g_lo, 1) - 1, s);
        check_launch();
        launch_zero_slice(dLevels, BN, (int)L, (int)d, (int)L - 1, s);
        check_launch();
    } else {
        launch_zero_slices(dLevels, BN, (int)L, (int)d, 0,
                           (int)std::min<int64_t>(g_lo + 1, L), s);
        check_launch();
    }
}

// ------------------------------------------------------------------ //
// grouped feed-forward (bottom-up: mode 0, top-down: mode 1)
// reference glom_pytorch.py:23-36 (GroupedFeedForward) applied at :134/:136

// Pointer table of a bottom-up operand: group 0 is `tokens` (B,N,d; row
// stride d), group g >= 1 is level slice g-1 of `levels` (B,N,L,d; row
// stride L*d). Groups [first, G) go to entries 0 .. G-first-1.
template <class Ptr>
void token_level_table(Ptr* tab, long* ld, void* tokens,
                       const torch::Tensor& levels, int64_t first, int64_t G,
                       int64_t L, int64_t d) {
    for (int64_t g = first; g < G; g++) {
        tab[g - first] = g == 0 ? tokens : u16_at(levels, (g - 1) * d);
        ld[g - first] = g == 0 ? d : L * d;
    }
}

// The top-down input td_in = levels[..., 1:, :] + pos, (B,N,L-1,d): `ready`
// where the forward saved it or the previous iteration's level mix wrote
// it, else materialized here once, so that the GEMMs stream it with plain
// 16B loads / glds.
torch::Tensor td_input(const torch::Tensor& levels,
                       const c10::optional<torch::Tensor>& pos_opt,
                       const c10::optional<torch::Tensor>& ready,
                       hipStream_t s) {
    const int64_t B = levels.size(0), N = levels.size(1),
                  L = levels.size(2), d = levels.size(3);
    if (ready.has_value() && ready->numel() > 0) {
        const torch::Tensor& td_in = *ready;
        CHECK_IN(td_in);
        TORCH_CHECK(td_in.dim() == 4 && td_in.size(0) == B
                    && td_in.size(1) == N && td_in.size(2) == L - 1
                    && td_in.size(3) == d, "td_in must be (B,N,L-1,d)");
        return td_in;
    }
    TORCH_CHECK(pos_opt.has_value(), "top-down needs pos");
    const torch::Tensor& pos = *pos_opt;
    CHECK_IN(pos);
    auto td_in = torch::empty({B, N, L - 1, d}, levels.options());
    launch_add_pos(levels.data_ptr(), pos.data_ptr(), td_in.data_ptr(),
                   td_in.numel(), (int)N, (int)L, (int)d, s);
    check_launch();
    return td_in;
}

std::vector<torch::Tensor> grouped_ff_fwd(
        c10::optional<torch::Tensor> tokens_opt, torch::Tensor levels,
        c10::optional<torch::Tensor> pos_opt, torch::Tensor w1,
        torch::Tensor b1, torch::Tensor w2, torch::Tensor b2, int64_t mode,
        bool save_for_bwd = true, bool group0_done = false,
        c10::optional<torch::Tensor> td_in_ready = c10::nullopt) {
    CHECK_IN(levels); CHECK_IN(w1); CHECK_IN(b1); CHECK_IN(w2); CHECK_IN(b2);
    const int64_t B = levels.size(0), N = levels.size(1),
                  L = levels.size(2), d = levels.size(3);
    const int64_t G = (mode == 0) ? L : L - 1;
    TORCH_CHECK(G <= GEMM_MAX_TABLE, "levels > 16 unsupported by table mode");
    // group0_done (bottom-up only): group 0 reads `tokens`, not `levels`,
    // so within one forward its results repeat bit for bit; the caller kept
    // them from an earlier call and nothing will read this call's. Both
    // GEMMs then run groups [1, G) (bases and tables offset by one group,
    // gates judged by the full G, as the level cone does in the backward):
    // Y[:, :, 0], Hpre[0] and Hact[0] are left unwritten.
    TORCH_CHECK(!group0_done || (mode == 0 && G >= 2),
                "group0_done needs the bottom-up mode and levels >= 2");
    const int64_t g0 = group0_done ? 1 : 0;
    const int64_t Ga = G - g0;
    const int64_t m4 = w1.size(0) / G;
    const int64_t M = B * N;
    TORCH_CHECK(d % 8 == 0 && m4 % 8 == 0, "dim and mult*dim must be /8");
    TORCH_CHECK(w1.size(0) == G * m4 && w1.size(1) == d);
    TORCH_CHECK(w2.size(0) == G * d && w2.size(1) == m4);

    auto opts = levels.options();
    const bool pair = g_gelu_pair
                      && (M % 512 == 0) && (m4 % 256 == 0)
                      && m4 >= 1024;   // nt5p-eligible shapes only
    // forward-only callers (save_for_bwd == false) never read the
    // pre-activation (only the backward's gelu' does): where nt5p serves
    // the up-projection it writes gelu(pre-act) alone (EPI_GELU) and Hpre
    // is neither allocated nor written
    const bool gelu_only = !save_for_bwd && pair
                           && nt5p_takes_up_proj(M, m4, d, G);
    auto Hpre = gelu_only ? torch::empty({0}, opts)
                          : torch::empty({G, M, m4}, opts);
    auto Hact = torch::empty({G, M, m4}, opts);
    auto Y = torch::empty({B, N, G, d}, opts);
    hipStream_t s = cur_stream();

    torch::Tensor td_in;
    if (mode == 1) {
        TORCH_CHECK(pos_opt.has_value(), "top-down needs pos");
        CHECK_IN((*pos_opt));
        td_in = td_input(levels, pos_opt, td_in_ready, s);
    }

    // up-projection: Hpre_g = x_g @ W1_g^T + b1_g ; Hact_g = gelu(Hpre_g)
    {
        GemmParams p = base_params(M, m4, d, LAYOUT_NT, Ga, Ga, 1.0f);
        if (mode == 0) {
            TORCH_CHECK(tokens_opt.has_value(), "bottom-up needs tokens");
            auto tokens = tokens_opt.value();
            CHECK_IN(tokens);
            TORCH_CHECK(tokens.numel() == M * d, "tokens must be (B,N,d)");
            p.A.flags = OP_TABLE;
            token_level_table(p.Atab, p.Atabld, tokens.data_ptr(), levels,
                              g0, G, L, d);
        } else {
            p.A.base = td_in.data_ptr();
            p.A.sin = d; p.A.ld = G * d;
        }
        p.B.base = u16_at(w1, g0 * m4 * d); p.B.sin = m4 * d; p.B.ld = d;
        p.Csin = M * m4; p.Cld = m4;
        p.bias_base = u16_at(b1, g0 * m4); p.bias_sin = m4; p.has_bias = 1;
        if (gelu_only) {
            p.epilogue = EPI_GELU;
            p.Cbase = u16_at(Hact, g0 * M * m4);
        } else {
            p.Cbase = u16_at(Hpre, g0 * M * m4);
            if (pair) {
                p.epilogue = EPI_GELU_PAIR;
                p.out2 = u16_at(Hact, g0 * M * m4);
                p.out2_sin = M * m4; p.out2_ld = m4;
            }
        }
        run_gemm(p, s, opts, true, G);
        if (!pair) {
            // activation as its own bandwidth-bound pass (round-1 default)
            launch_gelu(u16_at(Hpre, g0 * M * m4), u16_at(Hact, g0 * M * m4),
                        Ga * M * m4, s);
            check_launch();
        }
    }
    // down-projection: Y_g = Hact_g @ W2_g^T + b2_g
    {
        GemmParams p = base_params(M, d, m4, LAYOUT_NT, Ga, Ga, 1.0f);
        p.A.base = u16_at(Hact, g0 * M * m4); p.A.sin = M * m4; p.A.ld = m4;
        p.B.base = u16_at(w2, g0 * d * m4); p.B.sin = d * m4; p.B.ld = m4;
        p.Cbase = u16_at(Y, g0 * d); p.Csin = d; p.Cld = G * d;
        p.bias_base = u16_at(b2, g0 * d); p.bias_sin = d; p.has_bias = 1;
        run_gemm(p, s, opts, true, G);
    }
    if (mode != 1) td_in = torch::empty({0}, opts);
    if (!save_for_bwd) Hpre = torch::empty({0}, opts);
    // td_in returned so the backward reuses it (saves re-running
    // k_add_pos per iteration in the weight-grad GEMM)
    return {Y, Hpre, Hact, td_in};
}

// ------------------------------------------------------------------ //
// FF backward. Each stage exists once, below; grouped_ff_bwd runs them all
// on the current stream, and ff_bwd_dh / ff_bwd_dx / ff_bwd_dw run the same
// stages from three calls so that the python layer can fork them over
// streams. Every stage takes the first live group (level cone) from the
// shape and the row stride of dY where it reads dY.

// One grouped FF problem. B, N, L and mode are known only to callers that
// hold `levels` or its sizes (mode stays -1 otherwise); the dX and dW1
// stages, which address level slices, need them.
struct FFShape {
    int64_t B = 0, N = 0, L = 0, d = 0;
    int64_t G = 0, m4 = 0, M = 0;   // groups, hidden width, rows B*N
    int64_t mode = -1;
    int64_t g_lo = 0, Ga = 0;       // live groups [g_lo, G): Ga of them,
                                    // the first at g_lo * (group stride)
};

FFShape ff_shape(int64_t G, int64_t M, int64_t m4, int64_t d, int64_t g_lo,
                 int64_t B = 0, int64_t N = 0, int64_t L = 0,
                 int64_t mode = -1) {
    TORCH_CHECK(g_lo >= 0 && g_lo <= G, "g_lo out of range");
    TORCH_CHECK(mode < 0 || (G == (mode == 0 ? L : L - 1) && M == B * N),
                "FF operands do not match (B, N, L)");
    FFShape f;
    f.B = B; f.N = N; f.L = L; f.d = d;
    f.G = G; f.m4 = m4; f.M = M;
    f.mode = mode;
    f.g_lo = g_lo; f.Ga = G - g_lo;
    return f;
}

// Row stride of dY in elements: dy_ld, or G*d where it is 0. The top-down
// call of the merged backward passes dmix (B,N,L,d) itself with
// dy_ld = L*d: its first L-1 level slices are what the compact dtd copy
// held.
int64_t ff_dy_ld(const FFShape& f, const torch::Tensor& dY, int64_t dy_ld) {
    const int64_t ldY = dy_ld > 0 ? dy_ld : f.G * f.d;
    TORCH_CHECK(ldY >= f.G * f.d && (dy_ld == 0 || ldY % 8 == 0),
                "dy_ld must be a multiple of 8 and at least G * d");
    TORCH_CHECK(f.M == 0 || dY.numel() >= (f.M - 1) * ldY + f.G * f.d,
                "dY is smaller than (M, G*d) at row stride dy_ld");
    return ldY;
}

// The dX outputs. The scattered dX GEMM writes every level slice of dLevels
// except one (mode 0: the top slice, which only the top-down path feeds;
// mode 1: slice 0) and those of the dead groups; just these are zeroed
// instead of a full-tensor fill, and with no_fill not even these, for a
// consumer that knows the written range (grad_merge).
torch::Tensor ff_dlevels(const FFShape& f, bool no_fill,
                         const torch::TensorOptions& opts, hipStream_t s) {
    auto dLevels = torch::empty({f.B, f.N, f.L, f.d}, opts);
    if (!no_fill)
        zero_unwritten_dx(dLevels.data_ptr(), f.M, f.L, f.d, f.mode, f.g_lo,
                          s);
    return dLevels;
}

// dTokens (mode 0; zero when group 0 is dead), else an empty tensor
torch::Tensor ff_dtokens(const FFShape& f, const torch::TensorOptions& opts,
                         hipStream_t s) {
    if (f.mode != 0) return torch::empty({0}, opts);
    auto dTokens = torch::empty({f.B, f.N, f.d}, opts);
    if (f.g_lo > 0) zero_fill(dTokens.data_ptr(), f.M * f.d * 2, s);
    return dTokens;
}

// dHpre_g = (dY_g @ W2_g) * gelu'(Hpre_g) -- NT with W2^T. When the 128x256
// kernels serve it, the bias grad dB1 = colsum(dHpre) fuses into the
// epilogue (saves a full re-read of the 400MB dHpre): returns the
// per-64-row f32 partials for ff_db1, or an undefined tensor.
torch::Tensor ff_dh(const FFShape& f, const torch::Tensor& dY, int64_t ldY,
                    const torch::Tensor& w2t, const torch::Tensor& Hpre,
                    const torch::Tensor& dHpre, hipStream_t s) {
    const int64_t M = f.M, m4 = f.m4, d = f.d, g_lo = f.g_lo;
    auto opts = dHpre.options();
    const bool fused = (M % 128 == 0) && (m4 % 256 == 0) && (m4 >= 1024)
                       && (d % 64 == 0);
    torch::Tensor db1f;
    GemmParams p = base_params(M, m4, d, LAYOUT_NT, f.Ga, f.Ga, 1.0f);
    p.A.base = u16_at(dY, g_lo * d); p.A.sin = d; p.A.ld = ldY;
    p.B.base = u16_at(w2t, g_lo * m4 * d); p.B.sin = m4 * d; p.B.ld = d;
    p.Cbase = u16_at(dHpre, g_lo * M * m4); p.Csin = M * m4; p.Cld = m4;
    p.epilogue = EPI_GELUGRAD;
    p.aux_base = u16_at(Hpre, g_lo * M * m4);
    p.aux_sin = M * m4; p.aux_ld = m4;
    if (fused) {
        // fully written by the epilogue
        db1f = torch::empty({f.Ga, M / 64, m4}, opts.dtype(at::kFloat));
        p.colsum_out = db1f.data_ptr<float>();
        p.colsum_sin = (M / 64) * m4;
    }
    run_gemm(p, s, opts, true, f.G);
    return db1f;
}

// dB1 of the live groups: the fixed-order finish of ff_dh's partials, or
// the native deterministic column sum of dHpre
void ff_db1(const FFShape& f, const torch::Tensor& db1f,
            const torch::Tensor& dHpre, const torch::Tensor& dB1,
            hipStream_t s) {
    const int64_t M = f.M, m4 = f.m4;
    if (db1f.defined()) {
        launch_colsum_fin(db1f.data_ptr<float>(), u16_at(dB1, f.g_lo * m4),
                          (int)f.Ga, m4, (int)(M / 64), s);
    } else {
        auto ws = torch::empty({(long)f.Ga * colsum_rb(M) * m4},
                               dHpre.options().dtype(at::kFloat));
        launch_colsum(u16_at(dHpre, f.g_lo * M * m4), ws.data_ptr<float>(),
                      u16_at(dB1, f.g_lo * m4), (int)f.Ga, M, m4, s);
    }
    check_launch();
}

// dX_g = dHpre_g @ W1_g -- NT with W1^T, scattered into dTokens and the
// level slices of dLevels
void ff_dx(const FFShape& f, const torch::Tensor& dHpre,
           const torch::Tensor& w1t, const torch::Tensor& dTokens,
           const torch::Tensor& dLevels, hipStream_t s) {
    const int64_t M = f.M, m4 = f.m4, d = f.d, g_lo = f.g_lo;
    GemmParams p = base_params(M, d, m4, LAYOUT_NT, f.Ga, f.Ga, 1.0f);
    p.A.base = u16_at(dHpre, g_lo * M * m4); p.A.sin = M * m4; p.A.ld = m4;
    p.B.base = u16_at(w1t, g_lo * d * m4); p.B.sin = d * m4; p.B.ld = m4;
    if (f.mode == 0) {
        p.Cflags = OP_TABLE;
        token_level_table(p.Ctab, p.Ctabld, dTokens.data_ptr(), dLevels,
                          g_lo, f.G, f.L, d);
    } else {
        p.Cbase = u16_at(dLevels, (g_lo + 1) * d);
        p.Csin = d; p.Cld = f.L * d;
    }
    run_gemm(p, s, dHpre.options(), true, f.G);
}

// dW1_g[h, j] = sum_m dHpre_g[m, h] * x_g[m, j]; x is tokens / levels
// (mode 0) or td_in (mode 1)
void ff_dw1(const FFShape& f, const torch::Tensor& dHpre,
            const c10::optional<torch::Tensor>& tokens_opt,
            const torch::Tensor& levels, const torch::Tensor& td_in,
            const torch::Tensor& dW1, hipStream_t s) {
    const int64_t M = f.M, m4 = f.m4, d = f.d, g_lo = f.g_lo;
    GemmParams p = base_params(m4, d, M, LAYOUT_TN, f.Ga, f.Ga, 1.0f);
    p.A.base = u16_at(dHpre, g_lo * M * m4); p.A.sin = M * m4; p.A.ld = m4;
    if (f.mode == 0) {
        const torch::Tensor& tokens = tokens_opt.value();
        CHECK_IN(tokens);
        p.B.flags = OP_TABLE;
        token_level_table(p.Btab, p.Btabld, tokens.data_ptr(), levels, g_lo,
                          f.G, f.L, d);
    } else {
        p.B.base = u16_at(td_in, g_lo * d);
        p.B.sin = d; p.B.ld = f.G * d;
    }
    p.Cbase = u16_at(dW1, g_lo * m4 * d); p.Csin = m4 * d; p.Cld = d;
    run_gemm(p, s, levels.options(), true, f.G);
}

// dW2_g[o, h] = sum_m dY_g[m, o] * Hact_g[m, h]
void ff_dw2(const FFShape& f, const torch::Tensor& dY, int64_t ldY,
            const torch::Tensor& Hact, const torch::Tensor& dW2,
            hipStream_t s) {
    const int64_t M = f.M, m4 = f.m4, d = f.d, g_lo = f.g_lo;
    GemmParams p = base_params(d, m4, M, LAYOUT_TN, f.Ga, f.Ga, 1.0f);
    p.A.base = u16_at(dY, g_lo * d); p.A.sin = d; p.A.ld = ldY;
    p.B.base = u16_at(Hact, g_lo * M * m4); p.B.sin = M * m4; p.B.ld = m4;
    p.Cbase = u16_at(dW2, g_lo * d * m4); p.Csin = d * m4; p.Cld = m4;
    run_gemm(p, s, Hact.options(), true, f.G);
}

// dB2 = colsum over the M token rows of dY viewed as (M, G*d) at row stride
// ldY; the dead groups' columns of dY are zero and sum to zero. Skipped
// where the result came in ready (db2_cone).
void ff_db2(const FFShape& f, const torch::Tensor& dY, int64_t ldY,
            const torch::Tensor& dB2, bool ready, hipStream_t s) {
    const int64_t M = f.M, Gd = f.G * f.d;
    if (ready) return;
    if (f.Ga == 0) {
        zero_fill(dB2.data_ptr(), Gd * 2, s);
        return;
    }
    auto ws = torch::empty({(long)colsum_rb(M) * Gd},
                           dY.options().dtype(at::kFloat));
    if (ldY == Gd)
        launch_colsum(dY.data_ptr(), ws.data_ptr<float>(), dB2.data_ptr(), 1,
                      M, Gd, s);
    else    // same chains over the row-strided matrix
        launch_colsum_cone(dY.data_ptr(), ws.data_ptr<float>(),
                           dB2.data_ptr(), nullptr, M, Gd, 0, ldY, 0, s);
    check_launch();
}

// dB2_ready: the dB2 result, already computed (db2_cone). no_fill: see
// ff_dlevels. Launch order: fills, dH, dX, dW1, dW2, dB1 finish, dB2 sum.
std::vector<torch::Tensor> grouped_ff_bwd(
        torch::Tensor dY, c10::optional<torch::Tensor> tokens_opt,
        torch::Tensor levels, c10::optional<torch::Tensor> pos_opt,
        torch::Tensor w1, torch::Tensor w2, torch::Tensor Hpre,
        torch::Tensor Hact, int64_t mode,
        c10::optional<torch::Tensor> w1t_opt = c10::nullopt,
        c10::optional<torch::Tensor> w2t_opt = c10::nullopt,
        c10::optional<torch::Tensor> td_in_opt = c10::nullopt,
        int64_t g_lo = 0, int64_t dy_ld = 0,
        c10::optional<torch::Tensor> dB2_ready = c10::nullopt,
        bool no_fill = false) {
    CHECK_IN(dY); CHECK_IN(levels); CHECK_IN(w1); CHECK_IN(w2); CHECK_IN(Hpre);
    CHECK_IN(Hact);
    const int64_t B = levels.size(0), N = levels.size(1),
                  L = levels.size(2), d = levels.size(3);
    const int64_t G = (mode == 0) ? L : L - 1;
    const int64_t m4 = w1.size(0) / G;
    const FFShape f = ff_shape(G, B * N, m4, d, g_lo, B, N, L, mode);
    const int64_t ldY = ff_dy_ld(f, dY, dy_ld);
    auto opts = levels.options();
    hipStream_t s = cur_stream();

    const bool ready = dB2_ready.has_value();
    if (ready) {
        CHECK_IN((*dB2_ready));
        TORCH_CHECK(dB2_ready->numel() == G * d, "dB2_ready must be (G*d,)");
    }
    auto dLevels = ff_dlevels(f, no_fill, opts, s);
    auto dW1 = torch::empty({G * m4, d}, opts);
    auto dW2 = torch::empty({G * d, m4}, opts);
    auto dB1 = torch::empty({G * m4}, opts);
    auto dB2 = ready ? *dB2_ready : torch::empty({G * d}, opts);
    zero_fill(dW1.data_ptr(), g_lo * m4 * d * 2, s);
    zero_fill(dW2.data_ptr(), g_lo * d * m4 * 2, s);
    zero_fill(dB1.data_ptr(), g_lo * m4 * 2, s);
    auto dTokens = ff_dtokens(f, opts, s);
    if (f.Ga == 0) {   // nothing live: the fills are the whole result
        ff_db2(f, dY, ldY, dB2, ready, s);
        return {dTokens, dLevels, dW1, dB1, dW2, dB2};
    }
    TORCH_CHECK(Hpre.numel() == G * f.M * m4 && Hact.numel() == G * f.M * m4,
                "Hpre / Hact must be (G, M, m4)");
    auto dHpre = torch::empty({G, f.M, m4}, opts);

    // per-group weight transposes turn the NN data grads into NT GEMMs
    // (callers that run many iterations pass them in, computed once)
    auto w1t = w1t_opt.has_value()
        ? w1t_opt.value()
        : w1.view({G, m4, d}).transpose(1, 2).contiguous();   // (G,d,m4)
    auto w2t = w2t_opt.has_value()
        ? w2t_opt.value()
        : w2.view({G, d, m4}).transpose(1, 2).contiguous();   // (G,m4,d)
    torch::Tensor td_in;
    if (mode == 1) td_in = td_input(levels, pos_opt, td_in_opt, s);

    auto db1f = ff_dh(f, dY, ldY, w2t, Hpre, dHpre, s);
    ff_dx(f, dHpre, w1t, dTokens, dLevels, s);
    ff_dw1(f, dHpre, tokens_opt, levels, td_in, dW1, s);
    ff_dw2(f, dY, ldY, Hact, dW2, s);
    ff_db1(f, db1f, dHpre, dB1, s);
    ff_db2(f, dY, ldY, dB2, ready, s);
    return {dTokens, dLevels, dW1, dB1, dW2, dB2};
}

// The three calls take the first live group `g_lo` like grouped_ff_bwd:
// dHpre keeps its (G, M, m4) shape, its dead groups are neither written by
// ff_bwd_dh nor read by the two calls after it. ff_bwd_dh finishes dB1
// directly after its GEMM.
std::vector<torch::Tensor> ff_bwd_dh(torch::Tensor dY, torch::Tensor w2t,
                                     torch::Tensor Hpre, int64_t g_lo = 0) {
    CHECK_IN(dY); CHECK_IN(w2t); CHECK_IN(Hpre);
    TORCH_CHECK(Hpre.dim() == 3, "Hpre must be (G, M, m4)");
    const FFShape f = ff_shape(Hpre.size(0), Hpre.size(1), Hpre.size(2),
                               dY.size(3), g_lo);
    const int64_t ldY = ff_dy_ld(f, dY, 0);
    auto opts = dY.options();
    hipStream_t s = cur_stream();
    auto dHpre = torch::empty({f.G, f.M, f.m4}, opts);
    auto dB1 = torch::empty({f.G * f.m4}, opts);
    zero_fill(dB1.data_ptr(), g_lo * f.m4 * 2, s);
    if (f.Ga == 0) return {dHpre, dB1};
    auto db1f = ff_dh(f, dY, ldY, w2t, Hpre, dHpre, s);
    ff_db1(f, db1f, dHpre, dB1, s);
    return {dHpre, dB1};
}

std::vector<torch::Tensor> ff_bwd_dx(torch::Tensor dHpre, torch::Tensor w1t,
                                     c10::optional<torch::Tensor> tokens_opt,
                                     int64_t B, int64_t N, int64_t L,
                                     int64_t mode, int64_t g_lo = 0) {
    CHECK_IN(dHpre); CHECK_IN(w1t);
    const int64_t G = dHpre.size(0), M = dHpre.size(1), m4 = dHpre.size(2);
    const FFShape f = ff_shape(G, M, m4, w1t.numel() / (G * m4), g_lo, B, N,
                               L, mode);
    if (mode == 0) { CHECK_IN(tokens_opt.value()); }
    hipStream_t s = cur_stream();
    auto dLevels = ff_dlevels(f, false, dHpre.options(), s);
    auto dTokens = ff_dtokens(f, dHpre.options(), s);
    if (f.Ga > 0) ff_dx(f, dHpre, w1t, dTokens, dLevels, s);
    return {dTokens, dLevels};
}

// Launch order: dW1, dW2, dB2.
std::vector<torch::Tensor> ff_bwd_dw(
        torch::Tensor dY, torch::Tensor dHpre,
        c10::optional<torch::Tensor> tokens_opt, torch::Tensor levels,
        c10::optional<torch::Tensor> pos_opt, torch::Tensor Hact,
        int64_t mode,
        c10::optional<torch::Tensor> td_in_opt = c10::nullopt,
        int64_t g_lo = 0) {
    CHECK_IN(dY); CHECK_IN(dHpre); CHECK_IN(levels); CHECK_IN(Hact);
    const int64_t G = dHpre.size(0), M = dHpre.size(1), m4 = dHpre.size(2);
    const int64_t d = levels.size(3);
    const FFShape f = ff_shape(G, M, m4, d, g_lo, levels.size(0),
                               levels.size(1), levels.size(2), mode);
    const int64_t ldY = ff_dy_ld(f, dY, 0);
    auto opts = levels.options();
    hipStream_t s = cur_stream();
    auto dW1 = torch::empty({G * m4, d}, opts);
    auto dW2 = torch::empty({G * d, m4}, opts);
    auto dB2 = torch::empty({G * d}, opts);
    zero_fill(dW1.data_ptr(), g_lo * m4 * d * 2, s);
    zero_fill(dW2.data_ptr(), g_lo * d * m4 * 2, s);
    if (f.Ga > 0) {
        torch::Tensor td_in;
        if (mode == 1) td_in = td_input(levels, pos_opt, td_in_opt, s);
        ff_dw1(f, dHpre, tokens_opt, levels, td_in, dW1, s);
        ff_dw2(f, dY, ldY, Hact, dW2, s);
    }
    ff_db2(f, dY, ldY, dB2, false, s);
    return {dW1, dW2, dB2};
}


// ------------------------------------------------------------------ //
// consensus attention (reference glom_pytorch.py:38-73)

// One GEMM operand per (batch, level): the three bf16 buffer shapes of the
// consensus ops, entered at level l_lo (0 in the forward; nInner = L - l_lo)
struct LevelOp {
    void* base; long sin, sout, ld;
    operator OpArg() const { return OpArg{base, sin, sout, ld, 0}; }
};
// (B,N,L,d): level slices, rows L*d apart
LevelOp op_bnld(const torch::Tensor& t, int64_t l_lo = 0) {
    const long N = t.size(1), L = t.size(2), d = t.size(3);
    return {u16_at(t, l_lo * d), d, N * L * d, L * d};
}
// (B,L,N,N) and (B,L,N,d): one compact matrix per level
LevelOp op_bl(const torch::Tensor& t, int64_t l_lo = 0) {
    const long L = t.size(1), R = t.size(2), C = t.size(3);
    return {u16_at(t, l_lo * R * C), R * C, L * R * C, C};
}
void set_c(GemmParams& p, const LevelOp& o) {
    p.Cbase = o.base; p.Csin = o.sin; p.Csout = o.sout; p.Cld = o.ld;
}
void set_aux(GemmParams& p, const LevelOp& o) {
    p.aux_base = o.base; p.aux_sin = o.sin; p.aux_sout = o.sout;
    p.aux_ld = o.ld;
}
void set_out2(GemmParams& p, const LevelOp& o) {
    p.out2 = o.base; p.out2_sin = o.sin; p.out2_sout = o.sout;
    p.out2_ld = o.ld;
}

std::vector<torch::Tensor> consensus_fwd(
        torch::Tensor levels, bool attend_self,
        c10::optional<torch::Tensor> mask_opt,
        c10::optional<torch::Tensor> rnorm_ready = c10::nullopt) {
    CHECK_IN(levels);
    const int64_t B = levels.size(0), N = levels.size(1),
                  L = levels.size(2), d = levels.size(3);
    const int64_t P = B * L;
    auto opts = levels.options();
    hipStream_t s = cur_stream();
    const bool* mask = nullptr;
    if (mask_opt.has_value()) {
        auto m = mask_opt.value();
        TORCH_CHECK(m.is_cuda() && m.is_contiguous()
                    && m.scalar_type() == at::kBool);
        mask = m.data_ptr<bool>();
    }

    const bool lds_ok = (N % 8 == 0) && (d % 8 == 0);
    torch::Tensor rnorm;
    if (rnorm_ready.has_value()) {
        // the previous iteration's level mix already wrote it
        rnorm = rnorm_ready.value();
        TORCH_CHECK(rnorm.is_cuda() && rnorm.is_contiguous()
                    && rnorm.scalar_type() == at::kFloat
                    && rnorm.dim() == 3 && rnorm.size(0) == B
                    && rnorm.size(1) == L && rnorm.size(2) == N,
                    "rnorm must be f32 (B,L,N)");
    } else {
        rnorm = torch::empty({B, L, N}, opts.dtype(at::kFloat));
        launch_rnorm(levels.data_ptr(), rnorm.data_ptr<float>(),
                     (int)B, (int)N, (int)L, (int)d, s);
        check_launch();
    }

    auto probs = torch::empty({B, L, N, N}, opts);
    const bool fused_sm = (N == 256) && (d % 64 == 0) && lds_ok;
    const bool fuse_av = fused_sm && !getenv("GLOM_NO_FUSE_AV");
    torch::Tensor out_av;
    if (fuse_av) out_av = torch::empty({B, N, L, d}, opts);
    // scores[i,j] = (q_i . k_j) * rnorm_j * d^-0.5, then masked row softmax
    {
        GemmParams p = base_params(N, N, d, LAYOUT_NT, P, L,
                                   (float)std::pow((double)d, -0.5));
        p.A = op_bnld(levels);
        p.B = p.A;
        set_c(p, op_bl(probs));
        p.colscale_base = rnorm.data_ptr<float>();
        p.cs_sin = N; p.cs_sout = L * N; p.has_colscale = 1;
        if (fused_sm) {
            // nt_fast4's 256-wide tile spans whole rows: softmax fuses into
            // the epilogue
            p.epilogue = EPI_SOFTMAX;
            p.self_mask = attend_self ? 0 : 1;
            p.nlmask = mask;
            p.splitk = 1;
            if (fuse_av) {
                // AV product fused too: O computed from the LDS-resident P
                set_out2(p, op_bnld(out_av));
                set_aux(p, op_bnld(levels));
                p.npatch = (int)d;
            }
            launch_gemm_nt_fast4(p, s);
            check_launch();
        } else {
            run_gemm(p, s, opts, lds_ok);
            launch_softmax_fwd(probs.data_ptr(), probs.data_ptr(), mask,
                               (int)P, (int)N, attend_self ? 0 : 1, s);
            check_launch();
        }
    }
    // out[i,:] = sum_j P[i,j] * levels[j,:]
    if (fuse_av)
        return {out_av, probs, rnorm};
    auto out = torch::empty({B, N, L, d}, opts);
    {
        GemmParams p = base_params(N, d, N, LAYOUT_NN, P, L, 1.0f);
        p.A = op_bl(probs);
        p.B = op_bnld(levels);
        set_c(p, op_bnld(out));
        run_gemm(p, s, opts, lds_ok);
    }
    return {out, probs, rnorm};
}

// `l_lo` (level cone): dOut is zero in levels < l_lo, so is the result
// there; the GEMMs and the combine run on levels [l_lo, L) of every batch
// entry. Every per-level buffer keeps all L levels and is entered at level
// l_lo (base + l_lo * inner stride, nInner = L - l_lo).
torch::Tensor consensus_bwd(torch::Tensor dOut, torch::Tensor levels,
                            torch::Tensor probs, torch::Tensor rnorm,
                            bool attend_self,
                            c10::optional<torch::Tensor> mask_opt,
                            int64_t l_lo = 0, bool no_fill = false) {
    // no_fill: levels < l_lo of the result are left unwritten (see
    // grouped_ff_bwd)
    CHECK_IN(dOut); CHECK_IN(levels); CHECK_IN(probs);
    const int64_t B = levels.size(0), N = levels.size(1),
                  L = levels.size(2), d = levels.size(3);
    TORCH_CHECK(l_lo >= 0 && l_lo <= L, "l_lo out of range");
    TORCH_CHECK(dOut.sizes() == levels.sizes() && probs.dim() == 4
                && probs.size(1) == L && probs.size(2) == N
                && probs.size(3) == N,
                "dOut must be (B,N,L,d) like levels, probs (B,L,N,N)");
    const int64_t Ll = L - l_lo;
    const int64_t P = B * Ll;       // live problems
    const int64_t Pfull = B * L;    // what the dispatch gates are judged by
    const bool lds_ok = (N % 8 == 0) && (d % 8 == 0);
    auto opts = levels.options();
    hipStream_t s = cur_stream();
    const bool* mask = nullptr;
    if (mask_opt.has_value()) mask = mask_opt.value().data_ptr<bool>();

    auto dLevels = torch::empty({B, N, L, d}, opts);
    if (!no_fill) {
        launch_zero_slices(dLevels.data_ptr(), B * N, (int)L, (int)d, 0,
                           (int)l_lo, s);
        check_launch();
    }
    if (Ll == 0) return dLevels;
    TORCH_CHECK(l_lo == 0 || d % 8 == 0, "l_lo needs dim % 8 == 0");
    const float* rn = rnorm.data_ptr<float>();
    const float scale = (float)std::pow((double)d, -0.5);

    // dP[i,j] = dOut_i . v_j, then row softmax backward -> dS, dSr
    const bool fused_sm = (N == 256) && (d % 64 == 0) && lds_ok;
    auto dS = torch::empty({B, L, N, N}, opts);
    auto dSr = torch::empty({B, L, N, N}, opts);
    torch::Tensor dP;
    {
        GemmParams p = base_params(N, N, d, LAYOUT_NT, P, Ll, 1.0f);
        p.A = op_bnld(dOut, l_lo);
        p.B = op_bnld(levels, l_lo);
        if (fused_sm) {
            set_c(p, op_bl(dS, l_lo));
            p.epilogue = EPI_SMBWD;
            set_aux(p, op_bl(probs, l_lo));
            set_out2(p, op_bl(dSr, l_lo));
            p.colscale_base = rn + l_lo * N;
            p.cs_sin = N; p.cs_sout = L * N; p.has_colscale = 1;
            p.self_mask = attend_self ? 0 : 1;
            p.nlmask = mask;
            p.alpha2 = scale;
            p.splitk = 1;
            launch_gemm_nt_fast4(p, s);
            check_launch();
        } else {
            dP = torch::empty({B, L, N, N}, opts);
            set_c(p, op_bl(dP, l_lo));
            run_gemm(p, s, opts, lds_ok, Pfull);
            launch_softmax_bwd(probs.data_ptr(), dP.data_ptr(), rn,
                               dS.data_ptr(), dSr.data_ptr(), mask, (int)P,
                               (int)N, attend_self ? 0 : 1, scale, s, (int)L,
                               (int)l_lo);
            check_launch();
        }
    }

    // dv[j,:] = sum_i P[i,j] dOut[i,:]
    auto dv = torch::empty({B, N, L, d}, opts);
    {
        GemmParams p = base_params(N, d, N, LAYOUT_TN, P, Ll, 1.0f);
        p.A = op_bl(probs, l_lo);
        p.B = op_bnld(dOut, l_lo);
        set_c(p, op_bnld(dv, l_lo));
        run_gemm(p, s, opts, lds_ok, Pfull);
    }
    // dq[i,:] = sum_j dSr[i,j] levels[j,:]
    auto dq = torch::empty({B, N, L, d}, opts);
    {
        GemmParams p = base_params(N, d, N, LAYOUT_NN, P, Ll, 1.0f);
        p.A = op_bl(dSr, l_lo);
        p.B = op_bnld(levels, l_lo);
        set_c(p, op_bnld(dq, l_lo));
        run_gemm(p, s, opts, lds_ok, Pfull);
    }
    // dkhat[j,:] = sum_i dS[i,j] levels[i,:]   (layout (B,L,N,d))
    auto dkhat = torch::empty({B, L, N, d}, opts);
    {
        GemmParams p = base_params(N, d, N, LAYOUT_TN, P, Ll, 1.0f);
        p.A = op_bl(dS, l_lo);
        p.B = op_bnld(levels, l_lo);
        set_c(p, op_bl(dkhat, l_lo));
        run_gemm(p, s, opts, lds_ok, Pfull);
    }
    launch_knorm_combine(dkhat.data_ptr(), levels.data_ptr(), rn,
                         dv.data_ptr(), dq.data_ptr(), dLevels.data_ptr(),
                         (int)B, (int)N, (int)L, (int)d, s, (int)l_lo);
    check_launch();
    return dLevels;
}

// ------------------------------------------------------------------ //
// level mixing (reference glom_pytorch.py:128-144)

// When (slab, slab_idx) is given, the output is written straight into
// slab[slab_idx] and returned as an untracked alias — the return_all
// trajectory is then materialized in place, with no torch.stack copy
// (SURVEY.md §2.3 note on the trajectory slab).
//
// bu0 (optional): a (B,N,d) view, rows contiguous and evenly strided, that
// holds level 0 of the bottom-up contribution; slice 0 of `bu` is then not
// read. glom_forward passes iteration 0's Y[:, :, 0, :] (row stride L*d), so
// no compact copy is made and nothing is copied back into later Ys.
//
// pos (optional): also produce the next iteration's top-down input and row
// norms from the rounded output (see k_mix_fwd). Returns {out, td_next,
// rn_next}; the last two are empty where the mix kernel does not emit them
// (d != 512), and the consumers then run k_add_pos / k_rnorm as before.
std::vector<torch::Tensor> level_mix_fwd_next(
        torch::Tensor levels, torch::Tensor bu, torch::Tensor td,
        torch::Tensor cons, c10::optional<torch::Tensor> slab = c10::nullopt,
        int64_t slab_idx = 0, c10::optional<torch::Tensor> bu0 = c10::nullopt,
        c10::optional<torch::Tensor> pos = c10::nullopt) {
    CHECK_IN(levels); CHECK_IN(bu); CHECK_IN(td); CHECK_IN(cons);
    const int64_t B = levels.size(0), N = levels.size(1),
                  L = levels.size(2), d = levels.size(3);
    TORCH_CHECK(d % 8 == 0, "dim must be a multiple of 8");
    TORCH_CHECK(bu.numel() == levels.numel() && cons.numel() == levels.numel()
                && td.numel() == B * N * (L - 1) * d,
                "level mix operands do not match levels");
    const void* bu0_ptr = nullptr;
    int64_t bu0_ld = 0;
    if (bu0.has_value()) {
        const auto& t = bu0.value();
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16
                    && t.dim() == 3 && t.size(0) == B && t.size(1) == N
                    && t.size(2) == d && t.stride(2) == 1
                    && t.stride(1) >= d && t.stride(1) % 8 == 0
                    && t.stride(0) == N * t.stride(1)
                    && ((uintptr_t)t.data_ptr() & 15) == 0,
                    "bu0 must be an evenly strided (B,N,d) bf16 view");
        bu0_ptr = t.data_ptr();
        bu0_ld = t.stride(1);
    }
    const bool emit = pos.has_value() && mix_fwd_can_emit_next((int)L, (int)d);
    auto td_next = torch::empty({0}, levels.options());
    auto rn_next = torch::empty({0}, levels.options().dtype(at::kFloat));
    if (emit) {
        CHECK_IN(pos.value());
        TORCH_CHECK(pos->numel() == N * d, "pos must be (N,d)");
        td_next = torch::empty({B, N, L - 1, d}, levels.options());
        rn_next = torch::empty({B, L, N}, levels.options().dtype(at::kFloat));
    }
    torch::Tensor out;
    if (slab.has_value()) {
        TORCH_CHECK(slab->is_contiguous()
                    && slab->scalar_type() == at::kBFloat16
                    && slab->numel() >= (slab_idx + 1) * levels.numel(),
                    "bad trajectory slab");
        out = alias_slab_slice(slab.value(), slab_idx, levels.sizes());
    } else {
        out = torch::empty_like(levels);
    }
    launch_mix_fwd(levels.data_ptr(), bu.data_ptr(), td.data_ptr(),
                   cons.data_ptr(), out.data_ptr(), levels.numel(), (int)L,
                   (int)d, cur_stream(), bu0_ptr, bu0_ld,
                   emit ? pos->data_ptr() : nullptr,
                   emit ? td_next.data_ptr() : nullptr,
                   emit ? rn_next.data_ptr<float>() : nullptr, (int)N);
    check_launch();
    return {out, td_next, rn_next};
}

torch::Tensor level_mix_fwd(torch::Tensor levels, torch::Tensor bu,
                            torch::Tensor td, torch::Tensor cons,
                            c10::optional<torch::Tensor> slab = c10::nullopt,
                            int64_t slab_idx = 0,
                            c10::optional<torch::Tensor> bu0 = c10::nullopt) {
    return level_mix_fwd_next(levels, bu, td, cons, slab, slab_idx, bu0,
                              c10::nullopt)[0];
}

// want_dtd = false (backward merge): dmix for the levels >= lo only, the
// rest left unwritten, and no compact dtd (returned empty)
std::vector<torch::Tensor> level_mix_bwd(torch::Tensor dout, int64_t lo = 0,
                                         bool want_dtd = true) {
    CHECK_IN(dout);
    const int64_t B = dout.size(0), N = dout.size(1), L = dout.size(2),
                  d = dout.size(3);
    TORCH_CHECK(d % 8 == 0, "dim must be a multiple of 8");
    TORCH_CHECK(lo >= 0 && lo <= L && (want_dtd ? lo == 0 : true),
                "lo out of range (and needs want_dtd = false)");
    auto dmix = torch::empty_like(dout);
    if (!want_dtd) {
        launch_mix_bwd_lo(dout.data_ptr(), dmix.data_ptr(), B * N, (int)L,
                          (int)d, (int)lo, cur_stream());
        check_launch();
        return {dmix, torch::empty({0}, dout.options())};
    }
    auto dtd = torch::empty({B, N, L - 1, d}, dout.options());
    launch_mix_bwd(dout.data_ptr(), dmix.data_ptr(), dtd.data_ptr(),
                   dout.numel(), (int)L, (int)d, cur_stream());
    check_launch();
    return {dmix, dtd};
}



// ------------------------------------------------------------------ //
// One full GLOM iteration as a single op pair (reference
// glom_pytorch.py:131-145): forward chains bottom-up, top-down, consensus
// and the level mix in one extension call; backward additionally sums the
// four levels-gradient contributions in one fused pass instead of three
// autograd accumulations.

std::vector<torch::Tensor> glom_step_fwd(
        torch::Tensor tokens, torch::Tensor levels, torch::Tensor pos,
        torch::Tensor bw1, torch::Tensor bb1, torch::Tensor bw2,
        torch::Tensor bb2, torch::Tensor tw1, torch::Tensor tb1,
        torch::Tensor tw2, torch::Tensor tb2, bool attend_self,
        c10::optional<torch::Tensor> mask,
        c10::optional<torch::Tensor> slab = c10::nullopt,
        int64_t slab_idx = 0, bool save_for_bwd = true,
        c10::optional<torch::Tensor> bu0 = c10::nullopt,
        c10::optional<torch::Tensor> td_in_ready = c10::nullopt,
        c10::optional<torch::Tensor> rnorm_ready = c10::nullopt,
        bool emit_next = false) {
    // bu0: level 0 of the bottom-up output, kept from iteration 0 of this
    // forward; the token MLP (group 0) is then skipped here.
    // td_in_ready / rnorm_ready: written by the previous iteration's mix.
    // emit_next: this mix writes them for the next one; results 8 and 9
    // (empty where the mix does not emit, see level_mix_fwd_next)
    auto bu = grouped_ff_fwd(tokens, levels, c10::nullopt, bw1, bb1, bw2,
                             bb2, 0, save_for_bwd, bu0.has_value());
    auto td = grouped_ff_fwd(c10::nullopt, levels, pos, tw1, tb1, tw2,
                             tb2, 1, save_for_bwd, false, td_in_ready);
    auto at = consensus_fwd(levels, attend_self, mask, rnorm_ready);
    auto mx = level_mix_fwd_next(
        levels, bu[0], td[0], at[0], slab, slab_idx, bu0,
        emit_next ? c10::optional<torch::Tensor>(pos) : c10::nullopt);
    std::vector<torch::Tensor> r = {mx[0], bu[1], bu[2], td[1], td[2],
                                    at[1], at[2], td[3]};
    if (emit_next) { r.push_back(mx[1]); r.push_back(mx[2]); }
    return r;
}

std::vector<torch::Tensor> glom_step_bwd(
        torch::Tensor dnew, torch::Tensor tokens, torch::Tensor levels,
        torch::Tensor pos, torch::Tensor bw1, torch::Tensor bw2,
        torch::Tensor tw1, torch::Tensor tw2, torch::Tensor buHpre,
        torch::Tensor buHact, torch::Tensor tdHpre, torch::Tensor tdHact,
        torch::Tensor probs, torch::Tensor rnorm, bool attend_self,
        c10::optional<torch::Tensor> mask,
        c10::optional<torch::Tensor> bw1t, c10::optional<torch::Tensor> bw2t,
        c10::optional<torch::Tensor> tw1t,
        c10::optional<torch::Tensor> tw2t,
        c10::optional<torch::Tensor> td_in = c10::nullopt,
        int64_t lo = 0) {
    // lo (level cone): dnew is zero in levels < lo. dmix / dtd inherit the
    // zeros; bottom-up groups, top-down groups and consensus levels below
    // lo are skipped and their (zero) results filled in, so add4 and dpos
    // below read what the full computation would have produced
    const int64_t L = levels.size(2);
    TORCH_CHECK(lo >= 0 && lo < L, "lo out of range");
    auto mix = level_mix_bwd(dnew);        // {dmix, dtd}
    auto bu = grouped_ff_bwd(mix[0], tokens, levels, c10::nullopt, bw1,
                             bw2, buHpre, buHact, 0, bw1t, bw2t,
                             c10::nullopt, lo);
    auto td = grouped_ff_bwd(mix[1], c10::nullopt, levels, pos, tw1, tw2,
                             tdHpre, tdHact, 1, tw1t, tw2t, td_in,
                             std::min<int64_t>(lo, L - 1));
    auto dAttn = consensus_bwd(mix[0], levels, probs, rnorm, attend_self,
                               mask, lo);
    auto dLevels = torch::empty_like(levels);
    launch_add4(mix[0].data_ptr(), bu[1].data_ptr(), td[1].data_ptr(),
                dAttn.data_ptr(), dLevels.data_ptr(), levels.numel(),
                cur_stream());
    check_launch();
    // dPos[n,:] = sum over batch and levels 1..L-1 of the top-down input
    // grads (native deterministic reduction, reference glom_pytorch.py:136)
    const int64_t B = levels.size(0), N = levels.size(1),
                  d = levels.size(3);
    auto dPos = torch::empty({N, d}, levels.options());
    const int BCH = (int)std::min<int64_t>(B, 8);
    auto ws = torch::empty({BCH * N * d}, levels.options().dtype(at::kFloat));
    launch_dpos(td[1].data_ptr(), dPos.data_ptr(), ws.data_ptr<float>(),
                BCH, (int)B, (int)N, (int)L, (int)d, cur_stream());
    check_launch();
    return {bu[0], dLevels, dPos, bu[2], bu[3], bu[4], bu[5],
            td[2], td[3], td[4], td[5]};
}

// Synthetic single-GEMM microbenchmark for kernel tuning (used by
// scripts/gemmbench.py; not part of the model path).
double bench_gemm(int64_t M, int64_t N, int64_t K, int64_t layout,
                  int64_t nproblems, int64_t epilogue, int64_t reps) {
    auto opts = torch::TensorOptions().dtype(at::kBFloat16)
                    .device(at::kCUDA);
    torch::Tensor A, Bt;
    if (layout == LAYOUT_TN)
        A = torch::randn({nproblems, K, M}, opts) * 0.05;
    else
        A = torch::randn({nproblems, M, K}, opts) * 0.05;
    if (layout == LAYOUT_NT)
        Bt = torch::randn({nproblems, N, K}, opts) * 0.05;
    else
        Bt = torch::randn({nproblems, K, N}, opts) * 0.05;
    auto C = torch::empty({nproblems, M, N}, opts);
    auto bias = torch::randn({nproblems, N}, opts);
    auto aux = torch::randn({nproblems, M, N}, opts);
    auto out2 = torch::empty({nproblems, M, N}, opts);
    hipStream_t s = cur_stream();

    auto run = [&]() {
        GemmParams p = base_params(M, N, K, (int)layout, nproblems,
                                   nproblems, 1.0f);
        p.A.base = A.data_ptr();
        p.A.sin = A.size(1) * A.size(2); p.A.ld = A.size(2);
        p.B.base = Bt.data_ptr();
        p.B.sin = Bt.size(1) * Bt.size(2); p.B.ld = Bt.size(2);
        p.Cbase = C.data_ptr(); p.Csin = M * N; p.Cld = N;
        p.epilogue = (int)epilogue;
        if (epilogue == EPI_GELUGRAD) {
            p.aux_base = aux.data_ptr(); p.aux_sin = M * N; p.aux_ld = N;
        }
        if (epilogue == EPI_GELU_PAIR || epilogue == EPI_GELU
            || epilogue == 10 || epilogue == 12) {
            p.bias_base = bias.data_ptr(); p.bias_sin = N; p.has_bias = 1;
            p.out2 = out2.data_ptr(); p.out2_sin = M * N; p.out2_ld = N;
        }
        run_gemm(p, s, opts, true);
    };
    for (int i = 0; i < 3; i++) run();
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0, s);
    for (int64_t i = 0; i < reps; i++) run();
    hipEventRecord(e1, s);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    return ms / reps;
}

// Test-and-tuning-only: C[g] = A[g]^T B[g] for A (G,K,M), B (G,K,N) through
// run_gemm's TN dispatch (EPI_NONE), so a TN result for a chosen shape can
// be taken out of the extension.
torch::Tensor gemm_tn(torch::Tensor A, torch::Tensor B) {
    CHECK_IN(A); CHECK_IN(B);
    TORCH_CHECK(A.dim() == 3 && B.dim() == 3 && A.size(0) == B.size(0)
                && A.size(1) == B.size(1), "A (G,K,M), B (G,K,N)");
    const int64_t G = A.size(0), K = A.size(1), M = A.size(2),
                  N = B.size(2);
    TORCH_CHECK(M % 8 == 0 && N % 8 == 0, "M and N must be /8");
    auto C = torch::empty({G, M, N}, A.options());
    GemmParams p = base_params(M, N, K, LAYOUT_TN, G, G, 1.0f);
    p.A.base = A.data_ptr(); p.A.sin = K * M; p.A.ld = M;
    p.B.base = B.data_ptr(); p.B.sin = K * N; p.B.ld = N;
    p.Cbase = C.data_ptr(); p.Csin = M * N; p.Cld = N;
    run_gemm(p, cur_stream(), A.options(), true);
    return C;
}

// Test-only, as gemm_tn: C[g] = A[g] B[g]^T (+ bias[g] per column) for
// A (G,M,K), B (G,N,K), bias (G,N) through run_gemm's NT dispatch.
torch::Tensor gemm_nt(torch::Tensor A, torch::Tensor B,
                      c10::optional<torch::Tensor> bias_opt = c10::nullopt) {
    CHECK_IN(A); CHECK_IN(B);
    TORCH_CHECK(A.dim() == 3 && B.dim() == 3 && A.size(0) == B.size(0)
                && A.size(2) == B.size(2), "A (G,M,K), B (G,N,K)");
    const int64_t G = A.size(0), M = A.size(1), K = A.size(2),
                  N = B.size(1);
    TORCH_CHECK(K % 8 == 0 && N % 8 == 0, "K and N must be /8");
    auto C = torch::empty({G, M, N}, A.options());
    GemmParams p = base_params(M, N, K, LAYOUT_NT, G, G, 1.0f);
    p.A.base = A.data_ptr(); p.A.sin = M * K; p.A.ld = K;
    p.B.base = B.data_ptr(); p.B.sin = N * K; p.B.ld = K;
    p.Cbase = C.data_ptr(); p.Csin = M * N; p.Cld = N;
    if (bias_opt.has_value()) {
        auto bias = bias_opt.value();
        CHECK_IN(bias);
        TORCH_CHECK(bias.dim() == 2 && bias.size(0) == G
                    && bias.size(1) == N, "bias (G,N)");
        p.bias_base = bias.data_ptr(); p.bias_sin = N; p.has_bias = 1;
    }
    run_gemm(p, cur_stream(), A.options(), true);
    return C;
}

// Test-only, as gemm_tn: C[g] = A[g] B[g] for A (G,M,K), B (G,K,N) through
// run_gemm's NN dispatch.
torch::Tensor gemm_nn(torch::Tensor A, torch::Tensor B) {
    CHECK_IN(A); CHECK_IN(B);
    TORCH_CHECK(A.dim() == 3 && B.dim() == 3 && A.size(0) == B.size(0)
                && A.size(2) == B.size(1), "A (G,M,K), B (G,K,N)");
    const int64_t G = A.size(0), M = A.size(1), K = A.size(2),
                  N = B.size(2);
    TORCH_CHECK(K % 8 == 0 && N % 8 == 0, "K and N must be /8");
    auto C = torch::empty({G, M, N}, A.options());
    GemmParams p = base_params(M, N, K, LAYOUT_NN, G, G, 1.0f);
    p.A.base = A.data_ptr(); p.A.sin = M * K; p.A.ld = K;
    p.B.base = B.data_ptr(); p.B.sin = K * N; p.B.ld = N;
    p.Cbase = C.data_ptr(); p.Csin = M * N; p.Cld = N;
    run_gemm(p, cur_stream(), A.options(), true);
    return C;
}

// Test-only: the raw f32 partials (sk, G, M, N) of gemm_nn_sk for A (G,M,K),
// B (G,K,N); the caller sums the slices. The kernel's one production user
// (the contrastive backward) feeds it non-integer operands.
torch::Tensor gemm_nn_splitk(torch::Tensor A, torch::Tensor B, int64_t sk) {
    CHECK_IN(A); CHECK_IN(B);
    TORCH_CHECK(A.dim() == 3 && B.dim() == 3 && A.size(0) == B.size(0)
                && A.size(2) == B.size(1), "A (G,M,K), B (G,K,N)");
    const int64_t G = A.size(0), M = A.size(1), K = A.size(2),
                  N = B.size(2);
    TORCH_CHECK(M % 128 == 0 && N % 128 == 0 && K % 8 == 0 && sk >= 1
                && sk <= 16, "gemm_nn_sk needs full 128^2 tiles, K / 8");
    auto ws = torch::empty({sk, G, M, N}, A.options().dtype(at::kFloat));
    GemmParams p = base_params(M, N, K, LAYOUT_NN, G, G, 1.0f);
    p.A.base = A.data_ptr(); p.A.sin = M * K; p.A.ld = K;
    p.B.base = B.data_ptr(); p.B.sin = K * N; p.B.ld = N;
    p.splitk = (int)sk; p.ws = ws.data_ptr<float>();
    launch_gemm_nn_sk(p, cur_stream());
    check_launch();
    return ws;
}

void add4_into(torch::Tensor a, torch::Tensor b, torch::Tensor c,
               torch::Tensor d, torch::Tensor out) {
    CHECK_IN(a); CHECK_IN(b); CHECK_IN(c); CHECK_IN(d); CHECK_IN(out);
    launch_add4(a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(),
                out.data_ptr(), out.numel(), cur_stream());
    check_launch();
}


// Backward merge (docs/ARCHITECTURE.md): dLevels of a step whose first
// live level is `lo`, from the four contributions in the ranges where the
// no_fill ops wrote them:
//   dmix, dAttn [lo, L)   bottom-up [max(lo,1)-1, L-1)   top-down [lo+1, L)
// posz: store an exact -0 as +0 (what the autograd add of the all-zero
// trajectory slice did on forwards that return the trajectory). next: also
// return dmix of the previous iteration, bf16(dLevels / c_l), written for
// levels >= max(lo-1, 0) only (else an empty tensor).
std::vector<torch::Tensor> grad_merge(torch::Tensor dmix, torch::Tensor bu_dl,
                                      torch::Tensor td_dl,
                                      torch::Tensor dattn, int64_t lo,
                                      bool posz, bool next) {
    CHECK_IN(dmix); CHECK_IN(bu_dl); CHECK_IN(td_dl); CHECK_IN(dattn);
    TORCH_CHECK(dmix.dim() == 4, "grad_merge expects (B,N,L,d)");
    const int64_t L = dmix.size(2), d = dmix.size(3);
    TORCH_CHECK(d % 8 == 0, "dim must be a multiple of 8");
    TORCH_CHECK(lo >= 0 && lo <= L, "lo out of range");
    TORCH_CHECK(bu_dl.sizes() == dmix.sizes() && td_dl.sizes() == dmix.sizes()
                && dattn.sizes() == dmix.sizes(),
                "grad_merge: the four contributions must share one shape");
    MergeRanges r;
    r.a_lo = (int)lo; r.a_hi = (int)L;
    r.b_lo = (int)std::max<int64_t>(lo, 1) - 1; r.b_hi = (int)L - 1;
    r.c_lo = (int)lo + 1; r.c_hi = (int)L;
    r.d_lo = (int)lo; r.d_hi = (int)L;
    r.dead = (int)std::max<int64_t>(lo - 1, 0);
    auto out = torch::empty_like(dmix);
    auto nxt = next ? torch::empty_like(dmix)
                    : torch::empty({0}, dmix.options());
    launch_grad_merge(dmix.data_ptr(), bu_dl.data_ptr(), td_dl.data_ptr(),
                      dattn.data_ptr(), out.data_ptr(),
                      next ? nxt.data_ptr() : nullptr, out.numel(), (int)L,
                      (int)d, r, posz, cur_stream());
    check_launch();
    return {out, nxt};
}

// Both FF nets' dB2 of one step from dmix (B,N,L,d), first live level lo:
// the column sum over the B*N rows of the columns [lo*d, L*d), +0 below.
// Returns {(L*d,) bottom-up, ((L-1)*d,) top-down}; the second is the first
// without the top level (same summands, same order).
std::vector<torch::Tensor> db2_cone(torch::Tensor dmix, int64_t lo) {
    CHECK_IN(dmix);
    TORCH_CHECK(dmix.dim() == 4, "db2_cone expects (B,N,L,d)");
    const int64_t M = dmix.size(0) * dmix.size(1), L = dmix.size(2),
                  d = dmix.size(3);
    TORCH_CHECK(d % 8 == 0, "dim must be a multiple of 8");
    TORCH_CHECK(lo >= 0 && lo <= L && M > 0, "lo out of range");
    auto bu = torch::empty({L * d}, dmix.options());
    auto td = torch::empty({(L - 1) * d}, dmix.options());
    auto ws = torch::empty({(long)colsum_rb(M) * L * d},
                           dmix.options().dtype(at::kFloat));
    launch_colsum_cone(dmix.data_ptr(), ws.data_ptr<float>(), bu.data_ptr(),
                       L > 1 ? td.data_ptr() : nullptr, M, L * d,
                       (L - 1) * d, L * d, lo * d, cur_stream());
    check_launch();
    return {bu, td};
}

// ------------------------------------------------------------------ //
// patch embedding (reference glom_pytorch.py:94-97,114): patchify
// rearrange + Linear(p^2*3 -> dim), K-padded to a /64 boundary so the
// tuned NT kernel serves the GEMM (zero columns are exact no-ops).

static int64_t pad_k(int64_t k) { return (k + 63) / 64 * 64; }

std::vector<torch::Tensor> patch_embed_fwd(torch::Tensor img,
                                           torch::Tensor w, torch::Tensor b,
                                           int64_t P) {
    CHECK_IN(img); CHECK_IN(w); CHECK_IN(b);
    const int64_t B = img.size(0), C = img.size(1), H = img.size(2),
                  W = img.size(3);
    const int64_t S = W / P, N = (H / P) * S;
    const int64_t K0 = P * P * C, Kp = pad_k(K0), dout = w.size(0);
    TORCH_CHECK(w.size(1) == K0, "embed weight/patch mismatch");
    auto opts = img.options();
    hipStream_t s = cur_stream();

    auto X = torch::empty({B, N, Kp}, opts);
    launch_patchify(img.data_ptr(), X.data_ptr(), (int)B, (int)C, (int)H,
                    (int)W, (int)P, (int)Kp, s);
    check_launch();
    auto Wp = torch::empty({dout, Kp}, opts);
    launch_pad_cols(w.data_ptr(), Wp.data_ptr(), dout, (int)K0, (int)Kp, s);
    check_launch();

    auto tokens = torch::empty({B, N, dout}, opts);
    GemmParams p = base_params(B * N, dout, Kp, LAYOUT_NT, 1, 1, 1.0f);
    p.A.base = X.data_ptr(); p.A.sin = 0; p.A.ld = Kp;
    p.B.base = Wp.data_ptr(); p.B.sin = 0; p.B.ld = Kp;
    p.Cbase = tokens.data_ptr(); p.Csin = 0; p.Cld = dout;
    p.bias_base = b.data_ptr(); p.bias_sin = 0; p.has_bias = 1;
    run_gemm(p, s, opts, true);
    return {tokens, X};
}

std::vector<torch::Tensor> patch_embed_bwd(torch::Tensor dTokens,
                                           torch::Tensor X, torch::Tensor w,
                                           int64_t P, int64_t imgH,
                                           int64_t imgW, bool need_dimg) {
    CHECK_IN(dTokens); CHECK_IN(X); CHECK_IN(w);
    const int64_t B = dTokens.size(0), N = dTokens.size(1),
                  dout = dTokens.size(2);
    const int64_t Kp = X.size(2), K0 = w.size(1), C = K0 / (P * P);
    const int64_t M = B * N;
    auto opts = dTokens.options();
    hipStream_t s = cur_stream();

    // dWp[o, k] = sum_m dTokens[m, o] * X[m, k]   (TN, split-K eligible)
    auto dWp = torch::empty({dout, Kp}, opts);
    {
        GemmParams p = base_params(dout, Kp, M, LAYOUT_TN, 1, 1, 1.0f);
        p.A.base = dTokens.data_ptr(); p.A.sin = 0; p.A.ld = dout;
        p.B.base = X.data_ptr(); p.B.sin = 0; p.B.ld = Kp;
        p.Cbase = dWp.data_ptr(); p.Csin = 0; p.Cld = Kp;
        run_gemm(p, s, opts, true);
    }
    auto dW = torch::empty({dout, K0}, opts);
    launch_slice_cols(dWp.data_ptr(), dW.data_ptr(), dout, (int)Kp,
                      (int)K0, s);
    check_launch();

    auto dB = torch::empty({dout}, opts);
    {
        auto cws = torch::empty({(long)colsum_rb(M) * dout},
                                opts.dtype(at::kFloat));
        launch_colsum(dTokens.data_ptr(), cws.data_ptr<float>(),
                      dB.data_ptr(), 1, M, dout, s);
        check_launch();
    }

    torch::Tensor dImg = torch::empty({0}, opts);
    if (need_dimg) {
        auto Wp = torch::empty({dout, Kp}, opts);
        launch_pad_cols(w.data_ptr(), Wp.data_ptr(), dout, (int)K0,
                        (int)Kp, s);
        check_launch();
        // dX[m, k] = sum_o dTokens[m, o] * Wp[o, k]   (NN)
        auto dX = torch::empty({B, N, Kp}, opts);
        GemmParams p = base_params(M, Kp, dout, LAYOUT_NN, 1, 1, 1.0f);
        p.A.base = dTokens.data_ptr(); p.A.sin = 0; p.A.ld = dout;
        p.B.base = Wp.data_ptr(); p.B.sin = 0; p.B.ld = Kp;
        p.Cbase = dX.data_ptr(); p.Csin = 0; p.Cld = Kp;
        run_gemm(p, s, opts, true);
        dImg = torch::empty({B, C, imgH, imgW}, opts);
        launch_unpatchify(dX.data_ptr(), dImg.data_ptr(), (int)B, (int)C,
                          (int)imgH, (int)imgW, (int)P, (int)Kp, s);
        check_launch();
    }
    return {dW, dB, dImg};
}

// l0 (default 1): first level summed; the caller knows the slices below it
// to be exact zeros (or unwritten). l0 >= L: nothing live, dPos = 0.
torch::Tensor dpos(torch::Tensor dLevels, int64_t l0 = 1) {
    CHECK_IN(dLevels);
    const int64_t B = dLevels.size(0), N = dLevels.size(1),
                  L = dLevels.size(2), d = dLevels.size(3);
    TORCH_CHECK(l0 >= 1, "l0 must be at least 1");
    auto out = torch::empty({N, d}, dLevels.options());
    if (l0 >= L) {
        zero_fill(out.data_ptr(), N * d * 2, cur_stream());
        return out;
    }
    const int BCH = (int)std::min<int64_t>(B, 8);
    auto ws = torch::empty({BCH * N * d},
                           dLevels.options().dtype(at::kFloat));
    launch_dpos(dLevels.data_ptr(), out.data_ptr(),
                d % 8 == 0 ? ws.data_ptr<float>() : nullptr, BCH,
                (int)B, (int)N, (int)L, (int)d, cur_stream(), (int)l0);
    check_launch();
    return out;
}

// (M, C) bf16 -> (C,) bf16 column sum, f32 accumulation in fixed order
// (bias gradient of a plain Linear, e.g. the trainer's decoder)
torch::Tensor colsum(torch::Tensor x) {
    CHECK_IN(x);
    TORCH_CHECK(x.dim() == 2, "colsum expects (M, C)");
    const int64_t M = x.size(0), C = x.size(1);
    auto out = torch::empty({C}, x.options());
    auto ws = torch::empty({(long)colsum_rb(M) * C},
                           x.options().dtype(at::kFloat));
    launch_colsum(x.data_ptr(), ws.data_ptr<float>(), out.data_ptr(), 1, M,
                  C, cur_stream());
    check_launch();
    return out;
}

// ------------------------------------------------------------------ //
// fused AdamW: one kernel pass over all parameter tensors (bf16 grads ->
// fp32 m/v/master -> bf16 param write-back) with the deterministic
// global-norm grad clip fused. step_dev is a persistent device counter
// (incremented on-device so the op is hipGraph-replay-safe).

static OptTable opt_table(const std::vector<torch::Tensor>& grads,
                          const std::vector<torch::Tensor>& masters,
                          const std::vector<torch::Tensor>& m1s,
                          const std::vector<torch::Tensor>& m2s,
                          const std::vector<torch::Tensor>& params,
                          const torch::Tensor& partials,
                          const torch::Tensor& norm,
                          const torch::Tensor& step_dev) {
    const size_t nt = grads.size();
    TORCH_CHECK(nt > 0 && nt <= OPT_MAX_T, "fused_adamw: 1..", OPT_MAX_T,
                " tensors supported, got ", nt);
    TORCH_CHECK(masters.size() == nt && m1s.size() == nt
                && m2s.size() == nt && params.size() == nt);
    TORCH_CHECK(partials.numel() >= OPT_NPART
                && partials.scalar_type() == at::kFloat);
    TORCH_CHECK(norm.numel() >= 1 && norm.scalar_type() == at::kFloat);
    TORCH_CHECK(step_dev.numel() >= 1
                && step_dev.scalar_type() == at::kFloat);
    OptTable t;
    std::memset(&t, 0, sizeof(t));
    t.nt = (int)nt;
    long cum = 0;
    for (size_t i = 0; i < nt; i++) {
        CHECK_IN(grads[i]); CHECK_IN(params[i]);
        TORCH_CHECK(masters[i].is_contiguous()
                    && masters[i].scalar_type() == at::kFloat);
        TORCH_CHECK(m1s[i].is_contiguous() && m2s[i].is_contiguous());
        const long n = grads[i].numel();
        TORCH_CHECK(masters[i].numel() == n && m1s[i].numel() == n
                    && m2s[i].numel() == n && params[i].numel() == n);
        t.g[i] = (const unsigned short*)grads[i].data_ptr();
        t.mw[i] = masters[i].data_ptr<float>();
        t.m1[i] = m1s[i].data_ptr<float>();
        t.m2[i] = m2s[i].data_ptr<float>();
        t.pw[i] = (unsigned short*)params[i].data_ptr();
        t.cum[i] = cum;
        cum += n;
    }
    t.cum[nt] = cum;
    return t;
}

void fused_adamw(std::vector<torch::Tensor> grads,
                 std::vector<torch::Tensor> masters,
                 std::vector<torch::Tensor> m1s,
                 std::vector<torch::Tensor> m2s,
                 std::vector<torch::Tensor> params,
                 double lr, double b1, double b2, double eps, double wd,
                 double max_norm, torch::Tensor partials, torch::Tensor norm,
                 torch::Tensor step_dev) {
    OptTable t = opt_table(grads, masters, m1s, m2s, params, partials, norm,
                           step_dev);
    hipStream_t s = cur_stream();
    launch_grad_norm(t, partials.data_ptr<float>(), norm.data_ptr<float>(),
                     step_dev.data_ptr<float>(), s);
    check_launch();
    launch_adamw(t, (float)lr, (float)b1, (float)b2, (float)eps, (float)wd,
                 (float)max_norm, norm.data_ptr<float>(),
                 step_dev.data_ptr<float>(), s);
    check_launch();
}

// The scheduled variant: lr comes from the device hyperparameter block
// `hyper` (layout OPT_H_* in native_ops.h; the finalize kernel evaluates the
// schedule at the incremented step count and writes this step's lr there),
// and lr scale / weight decay are per tensor. Same three launches, no sync,
// no allocation.
void fused_adamw_sched(std::vector<torch::Tensor> grads,
                       std::vector<torch::Tensor> masters,
                       std::vector<torch::Tensor> m1s,
                       std::vector<torch::Tensor> m2s,
                       std::vector<torch::Tensor> params,
                       std::vector<double> lr_scales,
                       std::vector<double> wds, double b1, double b2,
                       double eps, double max_norm, torch::Tensor partials,
                       torch::Tensor norm, torch::Tensor step_dev,
                       torch::Tensor hyper) {
    OptTable t = opt_table(grads, masters, m1s, m2s, params, partials, norm,
                           step_dev);
    const size_t nt = grads.size();
    TORCH_CHECK(lr_scales.size() == nt && wds.size() == nt,
                "fused_adamw_sched: one lr_scale and weight_decay per tensor");
    TORCH_CHECK(hyper.is_cuda() && hyper.is_contiguous()
                && hyper.numel() >= OPT_H_SIZE
                && hyper.scalar_type() == at::kFloat
                && hyper.device() == step_dev.device(),
                "fused_adamw_sched: hyper must be ", OPT_H_SIZE,
                " contiguous fp32 values on the optimizer's device");
    OptGroups h;
    std::memset(&h, 0, sizeof(h));
    for (size_t i = 0; i < nt; i++) {
        h.lr_scale[i] = (float)lr_scales[i];
        h.wd[i] = (float)wds[i];
    }
    hipStream_t s = cur_stream();
    launch_grad_norm_sched(t, partials.data_ptr<float>(),
                           norm.data_ptr<float>(),
                           step_dev.data_ptr<float>(),
                           hyper.data_ptr<float>(), s);
    check_launch();
    launch_adamw_sched(t, h, (float)b1, (float)b2, (float)eps,
                       (float)max_norm, norm.data_ptr<float>(),
                       step_dev.data_ptr<float>(), hyper.data_ptr<float>(),
                       s);
    check_launch();
}

// ------------------------------------------------------------------ //
// island-of-agreement analysis (glom_pytorch_amd/islands.py): neighbour
// cosine agreement on the patch grid and connected-component labels.
// Inference-side analysis ops: no autograd, no host synchronisation.

// levels (*lead, N, L, D) bf16 -> agreement (*lead, L, C, H, W) f32
torch::Tensor island_agreement(torch::Tensor levels, int64_t H, int64_t W,
                               int64_t connectivity) {
    CHECK_IN(levels);
    TORCH_CHECK(levels.dim() >= 3, "levels must be (*lead, N, L, D)");
    TORCH_CHECK(connectivity == 4 || connectivity == 8,
                "connectivity must be 4 or 8");
    const int64_t nd = levels.dim();
    const int64_t N = levels.size(nd - 3), L = levels.size(nd - 2),
                  D = levels.size(nd - 1);
    TORCH_CHECK(H > 0 && W > 0 && H * W == N, "grid does not match N");
    TORCH_CHECK(D % 8 == 0, "dim must be a multiple of 8");
    const int64_t C = connectivity == 4 ? 2 : 4;
    TORCH_CHECK(N * L * C < (1LL << 30), "grid too large (32-bit indices)");
    const int64_t P = N * L * D ? levels.numel() / (N * L * D) : 0;
    // one wave per row, 4 per block; one thread per edge, 256 per block
    TORCH_CHECK((P * N * L + 3) / 4 <= INT32_MAX
                && (P * L * C * N + 255) / 256 <= INT32_MAX,
                "too many rows for one launch");
    std::vector<int64_t> shape(levels.sizes().begin(),
                               levels.sizes().end() - 3);
    shape.insert(shape.end(), {L, C, H, W});
    auto fopts = levels.options().dtype(at::kFloat);
    auto out = torch::empty(shape, fopts);
    auto norm = torch::empty({P * L, N}, fopts);
    hipStream_t s = cur_stream();
    launch_island_dots(levels.data_ptr(), norm.data_ptr<float>(),
                       out.data_ptr<float>(), P, (int)H, (int)W, (int)L,
                       (int)D, (int)C, s);
    check_launch();
    launch_island_finish(norm.data_ptr<float>(), out.data_ptr<float>(),
                         P * L, (int)H, (int)W, (int)C, s);
    check_launch();
    return out;
}

// agreement (*lead, L, C, H, W) f32 -> labels (*lead, L, H, W) i32
torch::Tensor island_labels(torch::Tensor agreement, double threshold) {
    TORCH_CHECK(agreement.is_cuda() && agreement.is_contiguous()
                && agreement.scalar_type() == at::kFloat,
                "agreement must be a contiguous f32 GPU tensor");
    TORCH_CHECK(agreement.dim() >= 4,
                "agreement must be (*lead, L, C, H, W)");
    const int64_t nd = agreement.dim();
    const int64_t C = agreement.size(nd - 3), H = agreement.size(nd - 2),
                  W = agreement.size(nd - 1);
    TORCH_CHECK(C == 2 || C == 4, "agreement must have 2 or 4 channels");
    TORCH_CHECK(H * W <= ISLAND_MAX_CELLS, "native labelling needs N <= ",
                ISLAND_MAX_CELLS);
    const int64_t cell = C * H * W;
    const int64_t PL = cell ? agreement.numel() / cell : 0;
    TORCH_CHECK(PL <= INT32_MAX, "too many (lead, level) problems");
    std::vector<int64_t> shape(agreement.sizes().begin(),
                               agreement.sizes().end() - 3);
    shape.insert(shape.end(), {H, W});
    auto labels = torch::empty(shape, agreement.options().dtype(at::kInt));
    launch_island_labels(agreement.data_ptr<float>(),
                         labels.data_ptr<int>(), PL, (int)H, (int)W, (int)C,
                         (float)threshold, cur_stream());
    check_launch();
    return labels;
}

// labels (*lead, H, W) i32 -> {sizes (*lead, H, W), count (*lead)} i32;
// an output that is not wanted is neither allocated nor written (empty)
std::vector<torch::Tensor> island_sizes(torch::Tensor labels,
                                        bool want_sizes, bool want_count) {
    TORCH_CHECK(labels.is_cuda() && labels.is_contiguous()
                && labels.scalar_type() == at::kInt,
                "labels must be a contiguous i32 GPU tensor");
    TORCH_CHECK(labels.dim() >= 2, "labels must be (*lead, H, W)");
    const int64_t nd = labels.dim();
    const int64_t N = labels.size(nd - 2) * labels.size(nd - 1);
    TORCH_CHECK(N <= ISLAND_MAX_CELLS, "native island sizes need N <= ",
                ISLAND_MAX_CELLS);
    TORCH_CHECK(N > 0, "empty grid");
    const int64_t PL = labels.numel() / N;
    TORCH_CHECK(PL <= INT32_MAX, "too many (lead, level) problems");
    std::vector<int64_t> cshape(labels.sizes().begin(),
                                labels.sizes().end() - 2);
    auto sizes = want_sizes ? torch::empty_like(labels)
                            : torch::empty({0}, labels.options());
    auto count = want_count ? torch::empty(cshape, labels.options())
                            : torch::empty({0}, labels.options());
    if (want_sizes || want_count) {
        launch_island_sizes(labels.data_ptr<int>(),
                            want_sizes ? sizes.data_ptr<int>() : nullptr,
                            want_count ? count.data_ptr<int>() : nullptr,
                            PL, (int)N, cur_stream());
        check_launch();
    }
    return {sizes, count};
}

// ------------------------------------------------------------------ //
// parse trees from island labels (glom_pytorch_amd/parse.py): parent links
// between the islands of adjacent levels and island mean vectors. Like the
// island ops: no autograd, no host synchronisation.

// labels (*lead, L, H, W) i32 -> {parents, overlap} (*lead, L, H, W) i32
std::vector<torch::Tensor> island_parents(torch::Tensor labels) {
    TORCH_CHECK(labels.is_cuda() && labels.is_contiguous()
                && labels.scalar_type() == at::kInt,
                "labels must be a contiguous i32 GPU tensor");
    TORCH_CHECK(labels.dim() >= 3, "labels must be (*lead, L, H, W)");
    const int64_t nd = labels.dim();
    const int64_t L = labels.size(nd - 3);
    const int64_t N = labels.size(nd - 2) * labels.size(nd - 1);
    TORCH_CHECK(N <= PARSE_MAX_CELLS, "native island parents need N <= ",
                PARSE_MAX_CELLS);
    TORCH_CHECK(N > 0 && L > 0, "empty grid");
    const int64_t PL = labels.numel() / N;
    TORCH_CHECK(PL <= INT32_MAX && L <= INT32_MAX,
                "too many (lead, level) problems");
    auto parents = torch::empty_like(labels);
    auto overlap = torch::empty_like(labels);
    launch_island_parents(labels.data_ptr<int>(), parents.data_ptr<int>(),
                          overlap.data_ptr<int>(), PL, (int)L, (int)N,
                          cur_stream());
    check_launch();
    return {parents, overlap};
}

// levels (*lead, N, L, D) bf16, labels (*lead, L, H, W) i32 with H*W == N
// -> means (*lead, N, L, D) f32 or bf16
torch::Tensor island_means(torch::Tensor levels, torch::Tensor labels,
                           bool broadcast, bool out_bf16) {
    CHECK_IN(levels);
    TORCH_CHECK(labels.is_cuda() && labels.is_contiguous()
                && labels.scalar_type() == at::kInt,
                "labels must be a contiguous i32 GPU tensor");
    TORCH_CHECK(labels.device() == levels.device(),
                "levels and labels must be on the same device");
    TORCH_CHECK(levels.dim() >= 3, "levels must be (*lead, N, L, D)");
    TORCH_CHECK(labels.dim() == levels.dim(),
                "labels must be (*lead, L, H, W) with the lead of levels");
    const int64_t nd = levels.dim();
    const int64_t N = levels.size(nd - 3), L = levels.size(nd - 2),
                  D = levels.size(nd - 1);
    for (int64_t i = 0; i < nd - 3; i++)
        TORCH_CHECK(labels.size(i) == levels.size(i),
                    "levels and labels must have equal lead dimensions");
    TORCH_CHECK(labels.size(nd - 3) == L
                && labels.size(nd - 2) * labels.size(nd - 1) == N,
                "labels do not match the N and L of levels");
    TORCH_CHECK(N > 0 && L > 0 && D > 0, "empty levels");
    TORCH_CHECK(N <= PARSE_MAX_CELLS, "native island means need N <= ",
                PARSE_MAX_CELLS);
    TORCH_CHECK(D % 8 == 0, "dim must be a multiple of 8");
    TORCH_CHECK((uintptr_t)levels.data_ptr() % 16 == 0,
                "levels must be 16-byte aligned");
    const int64_t P = levels.numel() / (N * L * D);
    TORCH_CHECK(P * L <= INT32_MAX && L * D <= INT32_MAX,
                "too many (lead, level) problems");
    auto out = torch::empty(
        levels.sizes(),
        levels.options().dtype(out_bf16 ? at::kBFloat16 : at::kFloat));
    launch_island_means(levels.data_ptr(), labels.data_ptr<int>(),
                        out.data_ptr(), P, (int)N, (int)L, (int)D, broadcast,
                        out_bf16, cur_stream());
    check_launch();
    return out;
}

// ------------------------------------------------------------------ //
// column-contrastive loss (glom_pytorch_amd/contrast.py). a, b: (M, D)
// bf16 with unit column stride and a row stride that is a multiple of 8
// elements (level slices of a trajectory qualify), M = B * group rows.
// The (M, M) logits are never stored: the forward keeps one f32 per
// (row, 128-column tile), the backward recomputes them in row blocks of at
// most 64 MiB of bf16 G'. No atomics, no host synchronisation.

static void check_nce_in(const torch::Tensor& x, const char* name) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16
                && x.dim() == 2, name, " must be a 2-D bf16 GPU tensor");
    TORCH_CHECK(x.stride(1) == 1 && x.stride(0) % 8 == 0
                && x.size(1) % 8 == 0
                && ((uintptr_t)x.data_ptr() & 15) == 0,
                name, " needs unit column stride, dim and row stride "
                "multiples of 8 and a 16-byte aligned base");
}

static float* fptr(const torch::Tensor& t) { return t.data_ptr<float>(); }

static NceArgs nce_common(int64_t group, double temperature, bool all,
                          int64_t M) {
    NceArgs q;
    std::memset(&q, 0, sizeof(q));
    q.invt = (float)(1.0 / temperature);
    q.invm = (float)(1.0 / (double)M);
    q.group = (int)group;
    q.all = all ? 1 : 0;
    return q;
}

// -> {loss () f32, lse (M) f32, ra (M) f32, rb (M) f32}
std::vector<torch::Tensor> nce_fwd(torch::Tensor a, torch::Tensor b,
                                   int64_t group, double temperature,
                                   bool all) {
    check_nce_in(a, "a"); check_nce_in(b, "b");
    TORCH_CHECK(a.sizes() == b.sizes(), "a and b must have equal shapes");
    const int64_t M = a.size(0), D = a.size(1);
    TORCH_CHECK(M > 0 && group > 0 && M % group == 0, "bad group size");
    TORCH_CHECK(temperature >= 0.03, "native path needs temperature >= 0.03");
    TORCH_CHECK(M <= (1LL << 30), "too many rows");
    auto fo = a.options().dtype(at::kFloat);
    hipStream_t s = cur_stream();
    const int64_t ntn = (M + 127) / 128;
    auto ra = torch::empty({M}, fo), rb = torch::empty({M}, fo);
    auto lse = torch::empty({M}, fo), pos = torch::empty({M}, fo);
    auto part = torch::empty({M, ntn}, fo);
    auto bpart = torch::empty({NCE_MAX_PARTS}, fo);
    auto loss = torch::empty({}, fo);
    launch_nce_rnorm(a.data_ptr(), a.stride(0), fptr(ra), M, (int)D, s);
    check_launch();
    launch_nce_rnorm(b.data_ptr(), b.stride(0), fptr(rb), M, (int)D, s);
    check_launch();
    GemmParams p = base_params(M, M, D, LAYOUT_NT, 1, 1, 1.0f);
    p.A.base = a.data_ptr(); p.A.ld = a.stride(0);
    p.B.base = b.data_ptr(); p.B.ld = b.stride(0);
    p.epilogue = EPI_NCE_FWD;
    NceArgs q = nce_common(group, temperature, all, M);
    q.rrow = fptr(ra); q.rcol = fptr(rb);
    q.part = fptr(part); q.pos = fptr(pos);
    nce_set(p, q);
    run_gemm(p, s, a.options(), true);
    launch_nce_loss(fptr(part), fptr(pos), fptr(lse), fptr(bpart),
                    fptr(loss), M, (int)ntn, q.invt, s);
    check_launch();
    return {loss, lse, ra, rb};
}

// One side's gradient: rows = the side being differentiated (x, norms rx),
// columns = the other side (y, ry). lse_by_col: lse belongs to the columns
// (the dB pass, where the GEMM computes the transposed logits).
static torch::Tensor nce_bwd_side(const torch::Tensor& go,
                                  const torch::Tensor& x,
                                  const torch::Tensor& y,
                                  const torch::Tensor& rx,
                                  const torch::Tensor& ry,
                                  const torch::Tensor& lse, bool lse_by_col,
                                  int64_t group, double temperature, bool all,
                                  hipStream_t s) {
    const int64_t M = x.size(0), D = x.size(1);
    const int64_t ntn = (M + 127) / 128;
    // row blocks: Rc * M * 2 bytes <= 64 MiB, whole 128-row tiles if possible
    int64_t Rc = (32LL << 20) / M;
    if (Rc >= 128) Rc -= Rc % 128;
    Rc = std::max<int64_t>(1, std::min(Rc, M));
    auto opts = x.options();
    auto ws = torch::empty({Rc, M}, opts);
    auto part = torch::empty({Rc, ntn}, opts.dtype(at::kFloat));
    auto dx = torch::empty({M, D}, opts);
    // The product G'_block @ y has a small output (Rc x D) and a long
    // reduction (M): it runs split-K, about two blocks per CU, into f32
    // slices that the row kernel below adds in slice order. At least two
    // slices, so the result is rounded to bf16 once, after the row term.
    const int64_t tiles = ((Rc + 127) / 128) * ((D + 127) / 128);
    const int64_t sk = std::max<int64_t>(
        2, std::min<int64_t>({16, (512 + tiles - 1) / tiles, (M + 63) / 64}));
    auto acc = torch::empty({sk, Rc, D}, opts.dtype(at::kFloat));
    for (int64_t r0 = 0; r0 < M; r0 += Rc) {
        const int64_t rows = std::min(Rc, M - r0);
        {
            GemmParams p = base_params(rows, M, D, LAYOUT_NT, 1, 1, 1.0f);
            p.A.base = (const uint16_t*)x.data_ptr() + r0 * x.stride(0);
            p.A.ld = x.stride(0);
            p.B.base = y.data_ptr(); p.B.ld = y.stride(0);
            p.Cbase = ws.data_ptr(); p.Cld = M;
            p.epilogue = EPI_NCE_BWD;
            NceArgs q = nce_common(group, temperature, all, M);
            q.rrow = fptr(rx); q.rcol = fptr(ry);
            q.lse = fptr(lse); q.lse_col = lse_by_col ? 1 : 0;
            q.part = fptr(part);
            q.row0 = (int)r0;
            nce_set(p, q);
            run_gemm(p, s, opts, true);
        }
        {   // acc[slice] = G'_block (rows x M) . y (M x D) over slice's k
            GemmParams p = base_params(rows, D, M, LAYOUT_NN, 1, 1, 1.0f);
            p.A.base = ws.data_ptr(); p.A.ld = M;
            p.B.base = y.data_ptr(); p.B.ld = y.stride(0);
            p.splitk = (int)sk; p.ws = fptr(acc);
            // same preconditions as run_gemm's nn_fast (y is aligned)
            if (rows % 128 == 0 && D % 128 == 0 && M % 8 == 0)
                launch_gemm_nn_sk(p, s);
            else
                launch_gemm(p, s);
            check_launch();
        }
        launch_nce_grad_rows((uint16_t*)dx.data_ptr() + r0 * D, fptr(acc),
                             (int)sk,
                             (const uint16_t*)x.data_ptr() + r0 * x.stride(0),
                             x.stride(0), fptr(part), (int)ntn,
                             fptr(rx) + r0, fptr(go), rows, (int)D, s);
        check_launch();
    }
    return dx;
}

// -> {dA (M, D) bf16, dB (M, D) bf16}; an unwanted one is empty
std::vector<torch::Tensor> nce_bwd(torch::Tensor go, torch::Tensor a,
                                   torch::Tensor b, torch::Tensor lse,
                                   torch::Tensor ra, torch::Tensor rb,
                                   int64_t group, double temperature,
                                   bool all, bool need_a, bool need_b) {
    check_nce_in(a, "a"); check_nce_in(b, "b");
    TORCH_CHECK(a.sizes() == b.sizes(), "a and b must have equal shapes");
    const int64_t M = a.size(0);
    TORCH_CHECK(M > 0 && group > 0 && M % group == 0, "bad group size");
    TORCH_CHECK(temperature >= 0.03, "native path needs temperature >= 0.03");
    auto isf = [&](const torch::Tensor& t, int64_t n) {
        return t.is_cuda() && t.is_contiguous()
               && t.scalar_type() == at::kFloat && t.numel() == n;
    };
    TORCH_CHECK(isf(go, 1) && isf(lse, M) && isf(ra, M) && isf(rb, M),
                "go / lse / ra / rb must be contiguous f32 GPU tensors");
    hipStream_t s = cur_stream();
    auto none = torch::empty({0}, a.options());
    auto dA = need_a ? nce_bwd_side(go, a, b, ra, rb, lse, false, group,
                                    temperature, all, s) : none;
    auto dB = need_b ? nce_bwd_side(go, b, a, rb, ra, lse, true, group,
                                    temperature, all, s) : none;
    return {dA, dB};
}

std::string build_info() {
    return "glom_pytorch_amd HIP extension (gfx950, bf16 MFMA 16x16x32)";
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("grouped_ff_fwd", &grouped_ff_fwd, "grouped FF forward",
          py::arg("tokens"), py::arg("levels"), py::arg("pos"),
          py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
          py::arg("mode"), py::arg("save_for_bwd") = true,
          py::arg("group0_done") = false,
          py::arg("td_in") = c10::nullopt);
    m.def("grouped_ff_bwd", &grouped_ff_bwd, "grouped FF backward",
          py::arg("dY"), py::arg("tokens"), py::arg("levels"),
          py::arg("pos"), py::arg("w1"), py::arg("w2"),
          py::arg("Hpre"), py::arg("Hact"), py::arg("mode"),
          py::arg("w1t") = c10::nullopt,
          py::arg("w2t") = c10::nullopt,
          py::arg("td_in") = c10::nullopt, py::arg("g_lo") = 0,
          py::arg("dy_ld") = 0, py::arg("dB2_ready") = c10::nullopt,
          py::arg("no_fill") = false);
    m.def("consensus_fwd", &consensus_fwd, "consensus attention forward",
          py::arg("levels"), py::arg("attend_self"), py::arg("mask"),
          py::arg("rnorm") = c10::nullopt);
    m.def("consensus_bwd", &consensus_bwd, "consensus attention backward",
          py::arg("dOut"), py::arg("levels"), py::arg("probs"),
          py::arg("rnorm"), py::arg("attend_self"), py::arg("mask"),
          py::arg("l_lo") = 0, py::arg("no_fill") = false);
    m.def("level_mix_fwd", &level_mix_fwd, "level mix forward",
          py::arg("levels"), py::arg("bu"), py::arg("td"), py::arg("cons"),
          py::arg("slab") = c10::nullopt, py::arg("slab_idx") = 0,
          py::arg("bu0") = c10::nullopt);
    m.def("level_mix_fwd_next", &level_mix_fwd_next,
          "level mix forward, also emitting the next td_in / rnorm",
          py::arg("levels"), py::arg("bu"), py::arg("td"), py::arg("cons"),
          py::arg("slab") = c10::nullopt, py::arg("slab_idx") = 0,
          py::arg("bu0") = c10::nullopt, py::arg("pos") = c10::nullopt);
    m.def("level_mix_bwd", &level_mix_bwd, "level mix backward",
          py::arg("dout"), py::arg("lo") = 0, py::arg("want_dtd") = true);
    m.def("grad_merge", &grad_merge,
          "cone-aware sum of the four levels-gradient contributions",
          py::arg("dmix"), py::arg("bu_dl"), py::arg("td_dl"),
          py::arg("dattn"), py::arg("lo"), py::arg("posz"),
          py::arg("next"));
    m.def("db2_cone", &db2_cone, "dB2 of both FF nets from dmix",
          py::arg("dmix"), py::arg("lo") = 0);
    m.def("glom_step_fwd", &glom_step_fwd, "full GLOM iteration forward",
          py::arg("tokens"), py::arg("levels"), py::arg("pos"),
          py::arg("bw1"), py::arg("bb1"), py::arg("bw2"), py::arg("bb2"),
          py::arg("tw1"), py::arg("tb1"), py::arg("tw2"), py::arg("tb2"),
          py::arg("attend_self"), py::arg("mask"),
          py::arg("slab") = c10::nullopt, py::arg("slab_idx") = 0,
          py::arg("save_for_bwd") = true, py::arg("bu0") = c10::nullopt,
          py::arg("td_in") = c10::nullopt, py::arg("rnorm") = c10::nullopt,
          py::arg("emit_next") = false);
    m.def("glom_step_bwd", &glom_step_bwd, "full GLOM iteration backward",
          py::arg("dnew"), py::arg("tokens"), py::arg("levels"),
          py::arg("pos"), py::arg("bw1"), py::arg("bw2"), py::arg("tw1"),
          py::arg("tw2"), py::arg("buHpre"), py::arg("buHact"),
          py::arg("tdHpre"), py::arg("tdHact"), py::arg("probs"),
          py::arg("rnorm"), py::arg("attend_self"), py::arg("mask"),
          py::arg("bw1t") = c10::nullopt, py::arg("bw2t") = c10::nullopt,
          py::arg("tw1t") = c10::nullopt, py::arg("tw2t") = c10::nullopt,
          py::arg("td_in") = c10::nullopt, py::arg("lo") = 0);
    m.def("patch_embed_fwd", &patch_embed_fwd,
          "patchify + embed GEMM (K1)");
    m.def("patch_embed_bwd", &patch_embed_bwd, "patch embed backward");
    m.def("dpos", &dpos, "positional embedding gradient reduction",
          py::arg("dLevels"), py::arg("l0") = 1);
    m.def("colsum", &colsum, "fixed-order column sum (M,C) -> (C,)");
    m.def("fused_adamw", &fused_adamw,
          "fused AdamW + global-norm grad clip (torch semantics)");
    m.def("fused_adamw_sched", &fused_adamw_sched,
          "fused AdamW with device-resident lr schedule and per-tensor "
          "lr scale / weight decay");
    m.def("add4_into", &add4_into, "fused 4-way elementwise sum");
    m.def("ff_bwd_dh", &ff_bwd_dh, py::arg("dY"), py::arg("w2t"),
          py::arg("Hpre"), py::arg("g_lo") = 0);
    m.def("ff_bwd_dx", &ff_bwd_dx, py::arg("dHpre"), py::arg("w1t"),
          py::arg("tokens"), py::arg("B"), py::arg("N"), py::arg("L"),
          py::arg("mode"), py::arg("g_lo") = 0);
    m.def("ff_bwd_dw", &ff_bwd_dw, py::arg("dY"), py::arg("dHpre"),
          py::arg("tokens"), py::arg("levels"), py::arg("pos"),
          py::arg("Hact"), py::arg("mode"),
          py::arg("td_in") = c10::nullopt, py::arg("g_lo") = 0);
    m.def("set_nt8p", &set_nt8p, "toggle the 8-phase NT kernel (A/B)");
    m.def("set_tn_tr", &set_tn_tr,
          "toggle the transposed-read TN kernel (A/B, same bits)");
    m.def("set_tn_tr_mode", &set_tn_tr_mode,
          "0 never, 1 default policy, 2 every eligible TN call");
    m.def("get_tn_tr_mode", &get_tn_tr_mode);
    m.def("get_tn_tr_variant", &get_tn_tr_variant);
    m.def("set_tn_tr_variant", &set_tn_tr_variant,
          "split-K pipeline point of the transposed-read TN kernel (1..3)");
    m.def("set_finish_wide", &set_finish_wide,
          "toggle the re-blocked split-K finish (A/B, same bits)");
    m.def("gemm_tn", &gemm_tn, "C = A^T B per group (tests / tuning only)");
    m.def("gemm_nt", &gemm_nt, "C = A B^T + bias per group (tests only)",
          py::arg("A"), py::arg("B"), py::arg("bias") = c10::nullopt);
    m.def("gemm_nn", &gemm_nn, "C = A B per group (tests only)");
    m.def("gemm_nn_splitk", &gemm_nn_splitk,
          "f32 split-K partials of A B per group (tests only)");
    m.def("set_wide_epilogue", &set_wide_epilogue,
          "toggle the 16-byte register epilogue of nt5p (A/B)");
    m.def("set_wide_epilogue_mode", &set_wide_epilogue_mode,
          "0 narrow, 1 per-epilogue default, 2 all wide, 3 wide aux only");
    m.def("get_wide_epilogue_mode", &get_wide_epilogue_mode);
    m.def("set_wide_epilogue_nt8p", &set_wide_epilogue_nt8p,
          "toggle the 16-byte register epilogue of nt8p (A/B)");
    m.def("set_gelu_pair", &set_gelu_pair,
          "toggle fused GELU-pair up-projection epilogue (A/B)");
    m.def("island_agreement", &island_agreement,
          "neighbour cosine agreement on the patch grid",
          py::arg("levels"), py::arg("H"), py::arg("W"),
          py::arg("connectivity"));
    m.def("island_labels", &island_labels,
          "connected components of the kept-edge graph (min-index labels)");
    m.def("island_sizes", &island_sizes,
          "island size at each root cell and/or island count",
          py::arg("labels"), py::arg("want_sizes") = true,
          py::arg("want_count") = true);
    m.def("island_parents", &island_parents,
          "parent label and overlap of every island one level up");
    m.def("island_means", &island_means,
          "mean level-state vector of every island",
          py::arg("levels"), py::arg("labels"), py::arg("broadcast"),
          py::arg("out_bf16"));
    m.def("nce_fwd", &nce_fwd,
          "column-contrastive loss forward: (M,D) bf16 a, b -> "
          "{loss, lse, ra, rb}");
    m.def("nce_bwd", &nce_bwd, "column-contrastive loss backward");
    m.def("set_nce_fast", &set_nce_fast,
          "A/B: host the EPI_NCE_* epilogues on gemm_nt_fast where eligible");
    m.def("nce_launch_counts", &nce_launch_counts,
          "EPI_NCE_* launches so far: {gemm_nt_fast, generic}");
    m.def("build_info", &build_info);
    m.def("bench_gemm", &bench_gemm, "raw GEMM microbench (tuning only)");
}
