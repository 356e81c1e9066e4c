// C ABI of libcpt_hip.so (see include/cpt_hip.h): argument checks, error strings, per-kernel HIP
// event timing and the whole-model forward built from the kernels in gemm/attention/rowops.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include <algorithm>

#include "kernels.h"

// the switches are named without their namespace below, as the rest of this file's state is
#define CPT_SWITCH_USING(key, name, dflt, lo, hi, desc) using cpt::name;
CPT_SWITCH_TABLE(CPT_SWITCH_USING)
#undef CPT_SWITCH_USING
static thread_local char g_err[512] = "";

namespace cpt {
// the one writer of the calling thread's cpt_last_error() string (the other translation units declare it themselves)
int abi_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int abi_check(int rc, const char* what) {
    if (rc != CPT_OK) return abi_fail(rc, "%s: rejected arguments (status %d)", what, rc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return abi_fail(CPT_ERR_HIP - (int)e, "%s: %s", what, hipGetErrorString(e));
    return CPT_OK;
}
}  // namespace cpt
using cpt::abi_fail;
using cpt::abi_check;

#define TRY(expr, what)                          \
    do {                                         \
        int rc__ = abi_check((expr), what);      \
        if (rc__ != CPT_OK) return rc__;         \
    } while (0)

namespace {

// ---- per-kernel event timing ---------------------------------------------------------------
struct Prof {
    bool on = false;
    struct Rec { int id; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e;
        hipEventCreate(&e);
        return e;
    }
    void recycle() {
        for (auto& r : recs) { pool.push_back(r.a); pool.push_back(r.b); }
        recs.clear();
    }
} g_prof;

struct Scope {
    int idx = -1;
    hipStream_t s;
    Scope(int id, hipStream_t st) : s(st) {
        if (!g_prof.on) return;
        Prof::Rec r{id, g_prof.get(), g_prof.get()};
        hipEventRecord(r.a, s);
        g_prof.recs.push_back(r);
        idx = (int)g_prof.recs.size() - 1;
    }
    ~Scope() {
        if (idx >= 0) hipEventRecord(g_prof.recs[idx].b, s);
    }
};

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- the plan of cpt_model_fwd: every mode the forward branches on, decided from the dimensions, the batch shape and the output flags alone ----
// (what depends on a pointer or on the model's contents -- the fused embedding + region-feature launch, the K-tile-major QKV weight, the decoder
// prefetch, the column list -- is decided at its launch site)
enum { TAIL_NONE = 0, TAIL_BF16, TAIL_X3, TAIL_F32 };
struct FwdPlan {
    int B, Lt, Li, L, M;        // M = B * L: the rows that exist
    int Me;                     // rows the encoder's launches cover (> M: a ragged batch padded up to the panel residual mode's next shape, see pad_rows)
    int Mw;                     // rows the workspace's encoder tensors are carved for (>= Me)
    int dt;                     // dtype of everything outside the GEMMs (bf16x3: fp32)
    bool lp, x3;                // bf16; the bf16x3 parity mode
    bool fold;                  // the LayerNorm-folded bf16 encoder (the model carries cpt_layer_fold), residual stream in the 3-byte form
    int mask3;                  // [B][L][L] attention mask
    int attn_form;              // QKV projection + attention in one kernel: 0 = two kernels, else the form (cpt_set_tuning key 6) this shape runs
    bool two_kernel;            // fold: QKV GEMM, then the stand-alone attention kernel may write the panel
    bool panel, panel_ffn, rpanel;      // fold: ctx / the FFN activation / the residual stream itself in the panel layout (panel_modes)
    bool x3a, x3f;              // bf16x3: split-operand attention; FFN-up writes the split copy the FFN-down reads
    bool pre_ln;                // fold: the encoder's output is left un-normalised (no output reads every row)
    bool img_split2;            // region projection with K split over two workgroups per tile
    int head_splits;            // MLM head on the [MASK] rows: K splits of the transform GEMM (0 = the plain GEMM + LayerNorm)
    bool want_mask;             // the tail's rows: [MASK] (else [CLS])
    int tail;                   // the last layer on the head's rows only (TAIL_*), with its K-split counts:
    int tail_s1, tail_s2;       //   attention output and FFN up; FFN down
};

// The panel modes of the folded bf16 encoder at Me rows; each of their shape conditions is written here and nowhere else.
// Panel mode (round 3): the attention kernel writes ctx and the FFN-up epilogue writes h as MFMA A fragments (gemm_prod.hip), the two
// LayerNorm producers read them straight into registers; same bits as the row-major kernels.  Needs the (sequence, three heads)
// attention form (or the stand-alone attention kernel), the two-pass FFN-up kernel and tile-aligned shapes; everything else keeps the row-major tensors.
struct PanelModes { bool panel, panel_ffn, rpanel; };
PanelModes panel_modes(const FwdPlan& p, const cpt_dims& d, int Me, bool fold) {
    const int H = d.hidden, I = d.inter;
    PanelModes r;
    r.panel = fold && g_panel && (p.attn_form == 3 || p.two_kernel) && cpt::ffn_up_2pass_preferred(Me, I, H) &&
              cpt::panel_eligible(Me, H, H) && cpt::panel_eligible(Me, H, I);
    // h (FFN-up -> FFN-down) in the panel layout.  Round 3 kept it row-major when the producers run several rounds of tiles (GQA shape, 1680 tiles:
    // the 8-wave panel producer lost to the row-major kernel there, 4.05 vs 3.84 ms per step); with round 4's 4-wave producer the panel form wins
    // there too (3.63 ms; cpt_set_tuning key 28 = 0 restores the row-major FFN activation for multi-round shapes)
    r.panel_ffn = r.panel && ((long)(Me / 128) * (H / 192) <= 256 || g_panel_ffn_multi);
    // Round 5, the full panel mode -- (sequence, three heads) QKV + attention, two-pass FFN-up with panel output, both LayerNorm producers on the
    // panel kernel: the residual stream itself travels in the panel layout [M / 32][H / 16][64][8] (hi as bf16, lo as bytes).  The LayerNorm
    // producers run a register-direct epilogue and the two consumers gather their A tiles out of it; the embedding and region LayerNorm launches
    // write their rows at their panel positions, the heads gather their rows out of it.
    r.rpanel = r.panel && r.panel_ffn && p.attn_form == 3 && g_rpanel && cpt::lncons4_enabled() < 2;
    return r;
}

// Round 5: ROW PADDING.  The full panel mode (the form the bench shape runs in) needs B * L to be a multiple of 128 and enough FFN-up tiles to fill the chip;
// a ragged batch -- the reference's batches are sum-of-proposals long (zeroshot/refcoco_cpt.py:213-218) -- fell back to the row-major kernels: 63 sequences
// took 1.80 ms where 64 take 1.63, 48 took 1.81.  Every encoder kernel between the embedding and the heads is ROW-WISE except the attention, which works per
// sequence: so the encoder's tensors are simply sized and launched for the next row count the panel mode accepts (at most 1.5x the real rows), the rows behind
// B * L belong to no sequence, are never initialised and never read by anything that is returned.  Same bits on the real rows (the panel mode is bit-identical
// to the row-major encoder).
int pad_rows(const FwdPlan& p, const cpt_dims& d) {
    const long M = p.M;
    if (!p.lp || panel_modes(p, d, (int)M, true).rpanel) return (int)M;
    for (long Mp = (M + 127) / 128 * 128; Mp <= M + M / 2; Mp += 128)
        if (panel_modes(p, d, (int)Mp, true).rpanel) {
            // ... unless the padded shape starts a nearly empty FURTHER round of tiles (70 x 120 rows -> 8448 rows = 264 producer tiles of 128 x 192 and 264 FFN-up
            // tiles of 384 x 256: a second round for 8 of them; measured 2.87 ms padded against 2.60 ms on the row-major kernels): a round behind the first must
            // be at least half full, for both tile shapes
            const long tp = Mp / 128 * (d.hidden / 192), tf = (Mp + 383) / 384 * (d.inter / 256);
            for (long t : {tp, tf}) {
                const long rounds = (t + 255) / 256;
                if (rounds >= 2 && t - 256 * (rounds - 1) < 128) return (int)M;
            }
            return (int)Mp;
        }
    return (int)M;
}

// has_fold: the model carries the LayerNorm-folded weights (cpt_model.fold).  The workspace is sized for a folded model (cpt_fwd_workspace_bytes
// passes true; Mw assumes it whatever has_fold says), the launches go by the model at hand: a bf16 model without the folded weights never pads
// its rows (Me = M <= Mw), so a workspace sized by the public function is large enough either way.
FwdPlan make_plan(const cpt_dims& d, int B, int Lt, int Li, int flags, bool has_fold) {
    FwdPlan p;
    const int L = Lt + Li, M = B * L, H = d.hidden, I = d.inter;
    p.B = B; p.Lt = Lt; p.Li = Li; p.L = L; p.M = M;
    // bf16x3 parity mode: everything outside the GEMMs runs as in fp32 mode (the GEMMs: ModeGemm below)
    p.x3 = d.dtype == CPT_BF16X3;
    p.dt = p.x3 ? CPT_F32 : d.dtype;
    p.lp = p.dt == CPT_BF16;
    p.fold = p.lp && has_fold;
    p.mask3 = (flags & CPT_ATTN_MASK_3D) ? 1 : 0;
    const bool fuse_attn = p.lp && g_fuse_attn && L <= 128 && H % 64 == 0 && !p.mask3;
    p.attn_form = !fuse_attn ? 0 : g_fuse_attn != 3 ? g_fuse_attn : cpt::qkv_attn3_eligible(L, d.heads, H) ? 3 : 1;
    p.two_kernel = p.lp && !fuse_attn && !p.mask3 && L <= 288;        // 128 < L <= 288 (the GQA shape): QKV GEMM, then the stand-alone attention kernel writes the panel (beyond 288: row-major ctx)
    p.Mw = pad_rows(p, d);
    p.Me = p.fold ? p.Mw : M;
    const PanelModes pm = panel_modes(p, d, p.Me, p.fold);
    p.panel = pm.panel; p.panel_ffn = pm.panel_ffn; p.rpanel = pm.rpanel;
    // bf16x3, round 3: the FFN-up's GELU epilogue writes h as the split copy the FFN-down reads.  The fp32 FFN activation is then
    // never materialised, and its region [M][I] fp32 holds the FFN-up's own split input [M][3H] bf16.  (The LayerNorm passes writing
    // the split inputs of QKV / FFN-up themselves was built too: the two stand-alone passes it saves cost what its strided 8-byte stores
    // add to the LayerNorm launches -- 5.78-5.94 vs 5.84 ms -- so they stay.)
    // round 4: the mode's attention on bf16 MFMA with split operands, writing ctx as the split copy the attention-output GEMM reads (key 27)
    p.x3a = p.x3 && g_x3_attn && !p.mask3 && cpt::attention_x3_supported(L) && H % 8 == 0;
    p.x3f = p.x3 && I % 8 == 0 && (size_t)I * 4 >= (size_t)3 * H * 2;
    const bool all_rows = (flags & (CPT_OUT_SEQ | CPT_OUT_ALL_LOGITS)) != 0;      // an output reads every row of the encoder's output
    p.pre_ln = p.fold && !all_rows;
    // bf16: K split over two workgroups per tile, the LayerNorm pass adds the two partial matrices (gemm_img_proj)
    p.img_split2 = p.lp && d.img_dim_pad >= 128 && d.img_dim_pad % 64 == 0 && (size_t)2 * B * Li <= (size_t)M;
    // bf16, [MASK] rows only: the transform GEMM splits K over workgroups (4 tiles of 12 K-tiles each would run on 4 CUs), the pass
    // behind it adds the partial matrices, applies GELU and the LayerNorm.  The split depends on H only: same bits for every batch.
    const int hs = cpt::head_transform_splits(H);
    p.head_splits = (p.lp && !(flags & CPT_OUT_ALL_LOGITS) && H % 64 == 0 && hs > 1 && (size_t)hs * B <= (size_t)M) ? hs : 0;
    // Round 5: the last layer on the head's rows only.  When nothing but the B [MASK] rows (MLM head) or nothing but the B [CLS] rows (pooler / relation
    // head) is read behind the encoder, the last layer's attention output, FFN and LayerNorms are row-wise work on rows nobody reads: they run on
    // those B rows (gather + previous LayerNorm, three K-split dense layers with their row passes) -- the reference computes every row and then indexes
    // (modeling_rec.py:143-146, modeling_vcr.py:120-124); same values on the rows that are read.  The layer's attention still sees every row (K / V).
    p.want_mask = (flags & CPT_OUT_MASK_LOGITS) != 0;
    const bool want_cls = (flags & (CPT_OUT_POOLED | CPT_OUT_REL)) != 0;
    const bool tail_ok = g_tail && d.layers >= 2 && !all_rows && p.want_mask != want_cls;
    const size_t HI = (size_t)(H > I ? H : I);
    p.tail = TAIL_NONE;
    p.tail_s1 = p.tail_s2 = 0;
    if (tail_ok && p.fold) {
        // (the split-K partial matrices live in the FFN activation's region, the rows' FFN activation in the pre region)
        const int s1 = cpt::rows_gemm_splits(H), s2 = cpt::rows_gemm_splits(I);
        if (H % 64 == 0 && I % 64 == 0 && std::max((size_t)s1 * B * HI, (size_t)s2 * B * H) * 4 <= (size_t)M * I * 2 && (size_t)B * I * 2 <= (size_t)M * H * 4) {
            p.tail = TAIL_BF16; p.tail_s1 = s1; p.tail_s2 = s2;
        }
    } else if (tail_ok && p.x3a && p.x3f) {
        // the same for the bf16x3 parity mode (split-operand attention + fused split copies): the K-split row GEMMs run on the split operands (K' = 3 K),
        // the row passes keep fp32 and re-split; same three-term products, same gelu as the mode's all-row launches
        const int s1 = cpt::rows_gemm_splits(3 * H), s2 = cpt::rows_gemm_splits(3 * I);
        if (H % 64 == 0 && I % 64 == 0 && s1 <= 24 && s2 <= 24 &&
            std::max((size_t)s1 * B * HI, (size_t)s2 * B * H) * 4 <= (size_t)M * I * 4 && (size_t)B * I * 6 <= (size_t)M * 3 * H * 4 &&
            (size_t)B * 3 * H * 2 <= (size_t)M * H * 4) {      // (the [B][3H] bf16 split copies of the gathered rows live in the ctx / pre regions of M * H * 4 bytes: L = 1 would overrun them)
            p.tail = TAIL_X3; p.tail_s1 = s1; p.tail_s2 = s2;
        }
    } else if (tail_ok && d.dtype == CPT_F32) {
        p.tail = TAIL_F32;      // the same launches as the mode's all-row form (cpt_gemm + layernorm_rows), on the B gathered rows
    }
    return p;
}

struct FwdLayout {
    size_t x_f32, x_lp, qkv, ctx, pre, a_f32, a_lp, ffn, imgp, rows, rows_f32, t1, t2, pooled_f32, pooled_lp, stats, loss, split, total;
};

FwdLayout fwd_layout(const cpt_dims& d, const FwdPlan& p, int flags) {
    const bool lp = p.lp;
    const size_t es = lp ? 2 : 4;
    const size_t B = p.B, Li = p.Li, H = d.hidden;
    const size_t hr = (flags & CPT_OUT_ALL_LOGITS) ? (size_t)p.M : B;   // rows through the MLM head
    const size_t M = p.Mw;                                              // encoder tensors: B * L rows, or rounded up to the next full-panel shape (pad_rows)
    FwdLayout w;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += al(bytes); return at; };
    w.x_f32 = take(M * H * 4);
    w.x_lp = lp ? take(M * H * 2) : w.x_f32;
    w.qkv = take(M * 3 * H * es);
    w.ctx = take(M * H * es);
    w.pre = take(M * H * 4);
    w.a_f32 = take(M * H * 4);
    w.a_lp = lp ? take(M * H * 2) : w.a_f32;
    w.ffn = take(M * (size_t)d.inter * es);
    w.imgp = take(B * Li * d.img_dim_pad * es);
    w.rows = take(hr * H * es);
    w.rows_f32 = take(B * H * 4);
    w.stats = take((size_t)d.layers * 2 * cpt::ln_stat_slots(H) * M * 2 * 4);
    w.t1 = take(hr * H * 4);
    w.t2 = lp ? take(hr * H * 2) : take(hr * H * 4);
    w.pooled_f32 = take(B * H * 4);
    w.pooled_lp = lp ? take(B * H * 2) : w.pooled_f32;
    w.loss = take(256);
    // bf16x3: the split copy [rows][3K] bf16 of whichever GEMM input is current (largest: the FFN-down input, M x 3I)
    w.split = 0;
    if (p.x3) {
        size_t mx = M * 3 * (size_t)(d.inter > d.hidden ? d.inter : d.hidden);
        const size_t im = B * Li * 3 * d.img_dim_pad;
        if (im > mx) mx = im;
        w.split = take(mx * 2);
    }
    w.total = o;
    return w;
}

}  // namespace

#ifdef CPT_ABLATION
// development build: the one definition of every switch of the table (switches.h), and the table as data
namespace cpt {
#define CPT_SWITCH_DEF(key, name, dflt, lo, hi, desc) int name = dflt;
CPT_SWITCH_TABLE(CPT_SWITCH_DEF)
#undef CPT_SWITCH_DEF
}  // namespace cpt
namespace {
struct SwitchRow { int key; int* var; int dflt, lo, hi; };
#define CPT_SWITCH_ROW(key, name, dflt, lo, hi, desc) {key, &cpt::name, dflt, lo, hi},
const SwitchRow g_switch_rows[] = { CPT_SWITCH_TABLE(CPT_SWITCH_ROW) };
#undef CPT_SWITCH_ROW
}  // namespace
#endif

extern "C" {

int cpt_version(void) { return CPT_ABI_VERSION; }
const char* cpt_last_error(void) { return g_err; }

int cpt_check_device(int dev) {
    hipDeviceProp_t p;
    hipError_t e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return abi_fail(CPT_ERR_HIP - (int)e, "hipGetDeviceProperties(%d): %s", dev, hipGetErrorString(e));
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return abi_fail(CPT_ERR_ARCH, "device %d is %s; libcpt_hip is built for gfx950 (MI355X) only", dev, p.gcnArchName);
    return CPT_OK;
}

int cpt_build_info(void) {
#ifdef CPT_ABLATION
    return 1;
#else
    return 0;
#endif
}

int cpt_set_tuning(int key, int value) {
#ifndef CPT_ABLATION
    // product build: every switch is a compile-time constant (switches.h) -- nothing to set, nothing global to restore
    (void)value;
    if (key == -1) return CPT_OK;
    return abi_fail(CPT_ERR_ARCH, "cpt_set_tuning(%d): the kernel-variant switches exist in the CPT_ABLATION build only (libcpt_hip_abl.so, CPT_AMD_ABLATION=1); "
                              "this library always runs its shipped configuration", key);
#else
    if (key == -1) {       // every key back to its default (tests restore the library with this after every test)
        for (const SwitchRow& r : g_switch_rows) *r.var = r.dflt;
        cpt::set_gemm_trace_filter(255, 0);
        return CPT_OK;
    }
    if (key == 8) { cpt::set_gemm_trace_filter(value & 255, value >> 8); return CPT_OK; }   // a diagnostic, not a switch: trace filter (epilogue id | K << 8); 255: all
    for (const SwitchRow& r : g_switch_rows) {
        if (r.key != key) continue;
        int v = value < r.lo ? r.lo : (value > r.hi ? r.hi : value);
        if (key == 24 && v != 0 && v != 4) v = 8;      // three legal values inside the range: everything else is the 8-wave shape
        *r.var = v;
        return CPT_OK;
    }
    return abi_fail(CPT_ERR_SHAPE, "cpt_set_tuning: unknown key %d", key);
#endif
}

int cpt_debug_gemm_trace(void* buf) {
    cpt::set_gemm_trace(buf);
    cpt::set_q3_trace(buf);
    return CPT_OK;
}

int cpt_prof_enable(int on) {
    hipDeviceSynchronize();
    g_prof.recycle();
    g_prof.on = on != 0;
    return CPT_OK;
}

int cpt_prof_read(int kernel_id, double* total_ms, int64_t* launches) {
    if (!total_ms || !launches) return abi_fail(CPT_ERR_NULL, "cpt_prof_read: null output");
    hipDeviceSynchronize();
    double t = 0;
    int64_t n = 0;
    for (auto& r : g_prof.recs) {
        if (r.id != kernel_id) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { t += ms; ++n; }
    }
    *total_ms = t;
    *launches = n;
    return CPT_OK;
}

int cpt_gemm(int dtype, int epi, const void* A, int lda, const void* W, int ldw, const float* bias,
             const float* resid, int ldr, void* out, int out_dtype, int ldo, int M, int N, int K,
             void* stream) {
    if (!A || !W || !out) return abi_fail(CPT_ERR_NULL, "cpt_gemm: null operand");
    Scope p(CPT_K_OP, (hipStream_t)stream);
    return abi_check(cpt::gemm(dtype, epi, A, lda, W, ldw, bias, resid, ldr, out, out_dtype, ldo, M, N, K, (hipStream_t)stream), "cpt_gemm");
}

int cpt_embed_ln(const int64_t* ids, const int64_t* tt, const int64_t* pos, const float* word,
                 const float* posw, const float* typew, const float* g, const float* bta, float eps,
                 float* out_f32, void* out_lp, int lp_dtype, int B, int Lt, int L, int H, int vocab,
                 int max_pos, int type_vocab, void* stream) {
    return abi_check(cpt::embed_ln(ids, tt, pos, word, posw, typew, g, bta, eps, out_f32, out_lp, lp_dtype, B, Lt, L, H, vocab, max_pos, type_vocab, (hipStream_t)stream), "cpt_embed_ln");
}

int cpt_layernorm_rows(const float* x, const float* g, const float* bta, float eps, float* out_f32,
                       void* out_lp, int lp_dtype, int R, int H, int grp, int grp_stride,
                       int grp_off, void* stream) {
    return abi_check(cpt::layernorm_rows(x, g, bta, eps, out_f32, out_lp, lp_dtype, R, H, grp, grp_stride, grp_off, (hipStream_t)stream), "cpt_layernorm_rows");
}

int cpt_attention(int dtype, const void* qkv, const int64_t* attn_mask, void* ctx, void* probs,
                  int B, int L, int heads, void* stream) {
    return abi_check(cpt::attention(dtype, qkv, attn_mask, ctx, probs, B, L, heads, (hipStream_t)stream), "cpt_attention");
}

int cpt_split3(const float* x, int ld, void* out, int R, int K, int weight_order, void* stream) {
    if (!x || !out) return abi_fail(CPT_ERR_NULL, "cpt_split3: null operand");
    return abi_check(cpt::split3(x, ld, out, R, K, weight_order, (hipStream_t)stream), "cpt_split3");
}

int cpt_pad_cast(const float* x, void* out, int dtype, int R, int K, int Kp, void* stream) {
    if (!x || !out) return abi_fail(CPT_ERR_NULL, "cpt_pad_cast: null operand");
    return abi_check(cpt::pad_cast(x, out, dtype, R, K, Kp, (hipStream_t)stream), "cpt_pad_cast");
}

int cpt_gemm_ln_cons(const void* A, int lda, const void* Wf, int ldw, const float* st_in, const float* colc, const float* cold,
                     float eps, int hidden, int gelu, void* out, int ldo, int M, int N, int K, void* stream) {
    return abi_check(cpt::gemm_ln_cons(A, lda, Wf, ldw, st_in, colc, cold, eps, hidden, gelu, out, ldo, M, N, K, (hipStream_t)stream), "cpt_gemm_ln_cons");
}

int cpt_gemm_ln_prod(const void* A, int lda, const void* W, int ldw, const float* bias, const float* resid, int ldr, const float* st_in,
                     const float* g_in, const float* b_in, float eps, int hidden, float* out_f32, void* out_lp, float* st_out, int ldo,
                     int M, int N, int K, void* stream) {
    return abi_check(cpt::gemm_ln_prod(A, lda, W, ldw, bias, resid, ldr, st_in, g_in, b_in, eps, hidden, out_f32, out_lp, st_out, ldo,
                                          M, N, K, (hipStream_t)stream), "cpt_gemm_ln_prod");
}

int cpt_gemm_ln_prod3(const void* A, int lda, const void* W, int ldw, const float* bias, const void* resid_hi, const void* resid_lo, int ldr,
                      const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, void* out_hi, void* out_lo,
                      float* st_out, int ldo, int M, int N, int K, void* stream) {
    return abi_check(cpt::gemm_ln_prod3(A, lda, W, ldw, bias, resid_hi, resid_lo, ldr, st_in, g_in, b_in, eps, hidden, out_hi, out_lo, st_out, ldo,
                                           M, N, K, (hipStream_t)stream), "cpt_gemm_ln_prod3");
}

int cpt_panel_pack(const void* src_bf16, int ld, void* dst_bf16, int M, int K, int to_panel, void* stream) {
    return abi_check(cpt::panel_pack(src_bf16, ld, dst_bf16, M, K, to_panel, (hipStream_t)stream), "cpt_panel_pack");
}
// ---- operator-level test entry points with a per-call kernel choice (cpt_hip_debug.h) ----
int cpt_gemm_tile(int tile, int dtype, int epi, const void* A, int lda, const void* W, int ldw, const float* bias,
                  const float* resid, int ldr, void* out, int out_dtype, int ldo, int M, int N, int K, void* stream) {
    cpt::OverrideScope sc(tile, -1);
    return cpt_gemm(dtype, epi, A, lda, W, ldw, bias, resid, ldr, out, out_dtype, ldo, M, N, K, stream);
}
int cpt_gemm_ln_cons_tile(int tile, const void* A_bf16, int lda, const void* Wf_bf16, int ldw, const float* st_in, const float* colc,
                          const float* cold, float eps, int hidden, int gelu, void* out_bf16, int ldo, int M, int N, int K, void* stream) {
    cpt::OverrideScope sc(tile, -1);
    return cpt_gemm_ln_cons(A_bf16, lda, Wf_bf16, ldw, st_in, colc, cold, eps, hidden, gelu, out_bf16, ldo, M, N, K, stream);
}
int cpt_gemm_ln_prod_tile(int tile, const void* A, int lda, const void* W, int ldw, const float* bias, const float* resid, int ldr, const float* st_in,
                          const float* g_in, const float* b_in, float eps, int hidden, float* out_f32, void* out_lp, float* st_out, int ldo,
                          int M, int N, int K, void* stream) {
    cpt::OverrideScope sc(tile, -1);
    return cpt_gemm_ln_prod(A, lda, W, ldw, bias, resid, ldr, st_in, g_in, b_in, eps, hidden, out_f32, out_lp, st_out, ldo, M, N, K, stream);
}
int cpt_gemm_ln_prod3_tile(int tile, const void* A, int lda, const void* W, int ldw, const float* bias, const void* resid_hi, const void* resid_lo, int ldr,
                           const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, void* out_hi, void* out_lo,
                           float* st_out, int ldo, int M, int N, int K, void* stream) {
    cpt::OverrideScope sc(tile, -1);
    return cpt_gemm_ln_prod3(A, lda, W, ldw, bias, resid_hi, resid_lo, ldr, st_in, g_in, b_in, eps, hidden, out_hi, out_lo, st_out, ldo, M, N, K, stream);
}
int cpt_gemm_ln_prod3_panel_waves(int waves, const void* A_panel, const void* W, int ldw, const float* bias, const void* resid_hi, const void* resid_lo, int ldr,
                                  const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, void* out_hi, void* out_lo,
                                  float* st_out, int ldo, int M, int N, int K, void* stream) {
    if (waves != 0 && waves != 4 && waves != 8) return abi_fail(CPT_ERR_SHAPE, "cpt_gemm_ln_prod3_panel_waves: waves %d (0, 4 or 8)", waves);
    cpt::OverrideScope sc(-1, waves);
    return cpt_gemm_ln_prod3_panel(A_panel, W, ldw, bias, resid_hi, resid_lo, ldr, st_in, g_in, b_in, eps, hidden, out_hi, out_lo, st_out, ldo, M, N, K, stream);
}

int cpt_panel_pack_bytes(const void* src_i8, int ld, void* dst_i8, int M, int K, int to_panel, void* stream) {
    return abi_check(cpt::panel_pack(src_i8, ld, dst_i8, M, K, to_panel, (hipStream_t)stream, 1), "cpt_panel_pack_bytes");
}
int cpt_gemm_ln_prod3_rpanel(const void* A_panel, const void* W, int ldw, const float* bias, const void* resid_hi_panel, const void* resid_lo_panel,
                             const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, void* out_hi_panel, void* out_lo_panel,
                             float* st_out, int M, int N, int K, int waves, void* stream) {
    if (waves != 0 && waves != 4 && waves != 8) return abi_fail(CPT_ERR_SHAPE, "cpt_gemm_ln_prod3_rpanel: waves %d (0 = by shape, 4 or 8)", waves);
    cpt::OverrideScope sc(-1, waves == 0 ? -1 : waves);
    if (!cpt::panel_eligible(M, N, K))
        return abi_fail(CPT_ERR_SHAPE, "cpt_gemm_ln_prod3_rpanel: needs M %% 128 == 0, N %% 192 == 0, K %% 256 == 0, K >= 512 (got M=%d N=%d K=%d)", M, N, K);
    return abi_check(cpt::gemm_ln_prod3_panel(A_panel, W, ldw, bias, resid_hi_panel, resid_lo_panel, N, st_in, g_in, b_in, eps, hidden, out_hi_panel, out_lo_panel,
                                                 st_out, N, M, N, K, (hipStream_t)stream, nullptr, 0, nullptr, 0, 1), "cpt_gemm_ln_prod3_rpanel");
}

int cpt_gemm_ln_prod3_panel(const void* A_panel, const void* W, int ldw, const float* bias, const void* resid_hi, const void* resid_lo, int ldr,
                            const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, void* out_hi, void* out_lo,
                            float* st_out, int ldo, int M, int N, int K, void* stream) {
    if (!cpt::panel_eligible(M, N, K))
        return abi_fail(CPT_ERR_SHAPE, "cpt_gemm_ln_prod3_panel: needs M %% 128 == 0, N %% 192 == 0, K %% 256 == 0, K >= 512 (got M=%d N=%d K=%d)", M, N, K);
    return abi_check(cpt::gemm_ln_prod3_panel(A_panel, W, ldw, bias, resid_hi, resid_lo, ldr, st_in, g_in, b_in, eps, hidden, out_hi, out_lo, st_out, ldo,
                                                 M, N, K, (hipStream_t)stream), "cpt_gemm_ln_prod3_panel");
}

int cpt_resid3_split(const float* x, void* hi_bf16, void* lo_i8, size_t n, void* stream) {
    return abi_check(cpt::r3_split(x, hi_bf16, lo_i8, n, (hipStream_t)stream), "cpt_resid3_split");
}

int cpt_resid3_merge(const void* hi_bf16, const void* lo_i8, const int64_t* pos, float* out, int R, int L, int H, int gather, void* stream) {
    return abi_check(cpt::r3_merge(hi_bf16, lo_i8, pos, out, R, L, H, gather, (hipStream_t)stream), "cpt_resid3_merge");
}

int cpt_gemm_nn(const void* A, int lda, const void* W, int ldw, const float* resid, int ldr, void* out, int out_dtype, int ldo, int M, int N, int K,
                int w_rows, void* partials, size_t partial_bytes, void* stream) {
    if (!cpt::gemm_nn_eligible(M, N, K, lda, ldw))
        return abi_fail(CPT_ERR_SHAPE, "cpt_gemm_nn: needs N %% 192 == 0 or N %% 128 == 0, K %% 64 == 0, lda/ldw %% 8 == 0 (got M=%d N=%d K=%d)", M, N, K);
    return abi_check(cpt::gemm_nn(A, lda, W, ldw, resid, ldr, out, out_dtype, ldo, M, N, K, (hipStream_t)stream, w_rows, partials, partial_bytes), "cpt_gemm_nn");
}

int cpt_gemm_tn(const void* A, int lda, const void* W, int ldw, float* out, int ldo, int M, int N, int K, int k_rows, void* partials,
                size_t partial_bytes, void* stream) {
    if (!cpt::gemm_tn_eligible(M, N, K, lda, ldw, ldo))
        return abi_fail(CPT_ERR_SHAPE, "cpt_gemm_tn: needs M %% 128 == 0, N %% 128 == 0 (or 192), K %% 64 == 0, lda/ldw %% 8 == 0, ldo == N (got M=%d N=%d K=%d)", M, N, K);
    return abi_check(cpt::gemm_tn(A, lda, W, ldw, out, ldo, M, N, K, partials, partial_bytes, (hipStream_t)stream, k_rows), "cpt_gemm_tn");
}

int cpt_fold_ln_weights(const float* W, const float* gamma, const float* beta, const float* bias, void* Wf_bf16,
                        float* colc, float* cold, int N, int K, void* stream) {
    return abi_check(cpt::fold_ln_weights(W, gamma, beta, bias, Wf_bf16, colc, cold, N, K, (hipStream_t)stream), "cpt_fold_ln_weights");
}

int cpt_retile_k32(const void* src_bf16, void* dst_bf16, int N, int K, void* stream) {
    return abi_check(cpt::retile_k32(src_bf16, dst_bf16, N, K, (hipStream_t)stream), "cpt_retile_k32");
}

int cpt_select_regions(const float* mask_logits, int V, const int64_t* color_ids, int C, const int32_t* query_first, int Q,
                       int64_t none_id, int divide_by_none, int64_t* out_idx, float* out_score, void* stream) {
    return abi_check(cpt::select_regions(mask_logits, V, color_ids, C, query_first, Q, none_id, divide_by_none, out_idx, out_score,
                                            (hipStream_t)stream), "cpt_select_regions");
}

int cpt_rec_choose(const float* scores, int S, int V, const int32_t* q_index, int Qb, int Q, const int32_t* seq_first, const int32_t* cols, int C,
                   const int32_t* cand_first, const double* rects, const double* gt, const uint8_t* has_gt, int none, int divide_by_none,
                   int32_t* idx, float* score, double* iou, uint8_t* correct, float* cand_score, int32_t* counts, void* stream) {
    if (!scores || !q_index || !seq_first || !cols || !cand_first || !rects || !gt || !has_gt || !idx || !score || !iou || !correct || !counts)
        return abi_fail(CPT_ERR_NULL, "cpt_rec_choose: null argument");
    if (S <= 0 || V <= 0 || Qb <= 0 || Q <= 0 || C <= 0 || none < 0 || none >= V)
        return abi_fail(CPT_ERR_SHAPE, "cpt_rec_choose: S %d V %d Qb %d Q %d C %d none %d", S, V, Qb, Q, C, none);
    return abi_check(cpt::rec_choose(scores, S, V, q_index, Qb, Q, seq_first, cols, C, cand_first, rects, gt, has_gt, none, divide_by_none, idx, score,
                                     iou, correct, cand_score, counts, (hipStream_t)stream), "cpt_rec_choose");
}

int cpt_argmax_columns(const float* logits, int V, const int64_t* ids, int n_ids, int R, int64_t* out_idx, float* out_val, void* stream) {
    return abi_check(cpt::argmax_columns(logits, V, ids, n_ids, R, out_idx, out_val, (hipStream_t)stream), "cpt_argmax_columns");
}

int cpt_gather_rows(const void* src, int dtype, const int64_t* pos, void* out, int B, int L, int H,
                    void* stream) {
    if (!src || !out) return abi_fail(CPT_ERR_NULL, "cpt_gather_rows: null operand");
    return abi_check(cpt::gather_rows(src, dtype, pos, out, B, L, H, (hipStream_t)stream), "cpt_gather_rows");
}

int cpt_ce_rows(const float* logits, const int64_t* labels, float* loss, float* dlogits, int R, int V,
                void* stream) {
    return abi_check(cpt::ce_rows(logits, labels, loss, dlogits, R, V, (hipStream_t)stream), "cpt_ce_rows");
}

size_t cpt_fwd_workspace_bytes(const cpt_dims* d, int B, int Lt, int Li, int flags) {
    if (!d || B <= 0 || Lt <= 0 || Li < 0) return 0;
    return fwd_layout(*d, make_plan(*d, B, Lt, Li, flags, true), flags).total;      // (true: sized for a folded model, see make_plan)
}

// ---- cpt_model_fwd: the stages -----------------------------------------------------------------------------------------------------
namespace {

// A GEMM of the forward's compute mode, out = A [Mr][K] x W [N][K]^T.  bf16x3: the fp32 input is split into the [rows][hi | hi | lo] bf16 copy
// (split: the workspace region that holds it) and the bf16 MFMA kernel runs over K' = 3K against the [N][hi | lo | hi] weights, fp32 out.
struct ModeGemm {
    bool x3;
    int dt;
    void* split;
    hipStream_t s;
    int operator()(int epi, const void* A, int lda, const void* W, int K, const float* bias, const float* resid, int ldr, void* out,
                   int out_dt, int ldo, int Mr, int N) const {
        if (!x3) return cpt::gemm(dt, epi, A, lda, W, K, bias, resid, ldr, out, out_dt, ldo, Mr, N, K, s);
        const int rc = cpt::split3((const float*)A, lda, split, Mr, K, 0, s);
        if (rc != CPT_OK) return rc;
        return cpt::gemm(CPT_BF16, epi, split, 3 * K, W, 3 * K, bias, resid, ldr, out, CPT_F32, ldo, Mr, N, 3 * K, s);
    }
};

// what every stage works on: the call's arguments, its plan and its tensors in the workspace
struct Fwd {
    const FwdPlan& p;
    const cpt_dims& d;
    const cpt_model* m; const cpt_batch* b; const cpt_outputs* o; int flags;      // the call's arguments
    bool cols;                  // decoder on a list of vocabulary columns (cpt_outputs.logit_cols)
    unsigned char* ws;
    const FwdLayout& w;
    hipStream_t s;
    ModeGemm gm;
    int B, Lt, Li, L, M, H, I;  // M = B * L, the rows that exist (the folded encoder is launched for p.Me)
    int dt; bool lp;            // = p.dt, p.lp
    float* x_f32; void* x_lp; void* qkv; void* ctx; float* pre; float* a_f32; void* a_lp; void* ffn;
    const float* tmpl; int n_slots;      // soft template (cpt_model_fwd_soft): text ids in (0, n_slots) read their word row from it; NULL: none
    // Folded bf16 encoder, 3-byte residual stream (common.h r3_encode): the pre-LayerNorm sums live as bf16 hi (x_lp / a_lp, the GEMM operands) +
    // int8 lo (the head of the x_f32 / a_f32 regions, which hold no fp32 tensor in this mode); the producers read and write
    // 3 + 3 bytes per element instead of 4 + 6, and the embedding kernels write their rows in that form directly.
    void* x_lo() const { return x_f32; }
    void* a_lo() const { return a_f32; }
    // bytes of the decoder's weight table that the first of the MLM head's row launches pulls into the Infinity Cache (cpt_set_tuning key 26)
    size_t dec_pf0() const { return ((size_t)d.vocab * H * 2 / 100 * (size_t)g_dec_pf_pct) & ~(size_t)1023; }

    // ---- the stages ----
    // fused QKV projection + attention in the plan's form; form 3 reads the K-tile-major weight copy (cpt_layer_fold.w_qkv_t) when the model carries one
    int qkv_attn(const void* W, const float* bias, const float* st_in, const float* colc, const float* cold, const void* W_tiled) const {
        if (p.attn_form == 3) {
            const bool tl = W_tiled != nullptr;
            return cpt::gemm_qkv_attn3(x_lp, H, tl ? W_tiled : W, H, bias, st_in, colc, cold, d.ln_eps, H, b->attn_mask, ctx, H, B, L, d.heads, H, s,
                                       tl ? 1 : 0, p.panel, p.rpanel);
        }
        if (p.panel || p.rpanel) return CPT_ERR_SHAPE;
        return cpt::gemm_qkv_attn(x_lp, H, W, H, bias, st_in, colc, cold, d.ln_eps, H, b->attn_mask, ctx, H, B, L, d.heads, H, p.attn_form, s);
    }

    // (a2-a4) text embeddings -> rows b*L + t, region projection -> rows b*L + Lt + i
    int embed() const {
        const bool fold = p.fold;
        // folded bf16 encoder: the same launch also converts the region features (rowops.hip embed_pad_kernel)
        const bool embed_pad = fold && Li > 0 && g_embed_pad && d.img_dim_pad % 8 == 0 && ((uintptr_t)b->img_feats % 8) == 0;
        if (embed_pad) {
            Scope sc(CPT_K_EMBED, s);
            TRY(cpt::embed_ln_pad_cast(b->input_ids, b->token_type, b->position_ids, m->word_emb, m->pos_emb, m->type_emb, m->emb_ln_g, m->emb_ln_b, d.ln_eps,
                                       x_lp, x_lo(), B, Lt, L, H, d.vocab, d.max_pos, d.type_vocab, b->img_feats, ws + w.imgp, B * Li, d.img_dim, d.img_dim_pad, s, p.rpanel,
                                       nullptr, nullptr, nullptr, nullptr, tmpl, n_slots), "embed_ln + pad_cast(img_feats)");
        } else {
            Scope sc(CPT_K_EMBED, s);
            TRY(cpt::embed_ln(b->input_ids, b->token_type, b->position_ids, m->word_emb, m->pos_emb, m->type_emb,
                              m->emb_ln_g, m->emb_ln_b, d.ln_eps, fold ? nullptr : x_f32, lp ? x_lp : nullptr, dt, B, Lt, L, H,
                              d.vocab, d.max_pos, d.type_vocab, s, fold ? x_lo() : nullptr, p.rpanel, nullptr, nullptr, nullptr, tmpl, n_slots), "embed_ln");
        }
        if (Li > 0) {
            Scope sc(CPT_K_IMG, s);
            void* imgp = ws + w.imgp;
            if (!embed_pad) TRY(cpt::pad_cast(b->img_feats, imgp, dt, B * Li, d.img_dim, d.img_dim_pad, s), "pad_cast(img_feats)");
            if (p.img_split2) TRY(cpt::gemm_img_proj(imgp, d.img_dim_pad, m->w_img, d.img_dim_pad, m->b_img, pre, H, B * Li, H, d.img_dim_pad, s), "gemm(img_embedding, split K)");
            else TRY(gm(CPT_EPI_NONE, imgp, d.img_dim_pad, m->w_img, d.img_dim_pad, m->b_img, nullptr, 0, pre, CPT_F32, H, B * Li, H), "gemm(img_embedding)");
            const bool iln = d.use_img_ln && m->img_ln_g;
            cpt::LnRowsExtra e;
            e.resid = p.img_split2 ? pre + (size_t)B * Li * H : nullptr; e.out_lo = fold ? x_lo() : nullptr; e.out_panel = p.rpanel;
            TRY(cpt::layernorm_rows_ex(pre, iln ? m->img_ln_g : nullptr, iln ? m->img_ln_b : nullptr, d.img_ln_eps, fold ? nullptr : x_f32,
                                       lp ? x_lp : nullptr, dt, B * Li, H, Li, L, Lt, 0, s, &e), "layernorm(img)");
        }
        return CPT_OK;
    }

    // the last layer of the folded bf16 encoder on the head's rows (plan: TAIL_BF16); leaves the rows' encoder output in w.rows
    int tail_bf16(const cpt_layer& y, const cpt_layer& yp) const {
        Scope sc(CPT_K_HEAD, s);
        float* part = (float*)ffn;                       // split-K partial matrices (the FFN activation's region: no launch of this layer writes it)
        float* resid = (float*)(ws + w.rows_f32);      // LayerNorm of the previous layer's output on the head rows
        void* ctx_rows = ws + w.t1;
        void* h_rows = pre;
        const int64_t* pos = p.want_mask ? b->mask_pos : nullptr;
        // the tail's row launches carry the first part of the decoder prefetch (MLM head, full vocabulary)
        const size_t pf = (p.want_mask && m->w_dec && !cols) ? dec_pf0() : 0;
        TRY(cpt::tail_rows(x_lp, x_lo(), pos, yp.ln2_g, yp.ln2_b, d.ln_eps, ctx, ctx_rows, resid, B, L, H, s, p.rpanel, p.panel,
                           pf ? m->w_dec : nullptr, pf / 2), "tail: gather head rows + previous LayerNorm");
        TRY(cpt::gemm_rows_split(ctx_rows, H, y.w_ao, H, y.b_ao, part, B, H, H, s), "tail: gemm(attn out, split K)");
        TRY(cpt::tail_finish(part, p.tail_s1, resid, y.ln1_g, y.ln1_b, d.ln_eps, a_f32, a_lp, B, H, s), "tail: partials + residual + layernorm(attn)");
        TRY(cpt::gemm_rows_split(a_lp, H, y.w_in, H, y.b_in, part, B, I, H, s), "tail: gemm(ffn up, split K)");
        TRY(cpt::gelu_parts(part, p.tail_s1, h_rows, (size_t)B * I, s, pf ? (const unsigned char*)m->w_dec + pf / 2 : nullptr, pf - pf / 2),
            "tail: partials + gelu");
        TRY(cpt::gemm_rows_split(h_rows, I, y.w_out, I, y.b_out, part, B, H, I, s), "tail: gemm(ffn down, split K)");
        TRY(cpt::tail_finish(part, p.tail_s2, a_f32, y.ln2_g, y.ln2_b, d.ln_eps, nullptr, ws + w.rows, B, H, s), "tail: partials + residual + layernorm(ffn)");
        return CPT_OK;
    }

    // (a5-a9) the folded bf16 encoder.  LayerNorm folded into the GEMMs around it: x and a hold PRE-LayerNorm sums (3-byte form), the
    // producer GEMMs accumulate their row sums, the consumer GEMMs normalise in their epilogue.
    int encoder_folded() const {
        const int Me = p.Me;      // (every launch of this stage is row-wise or per sequence: the padded rows are computed and never read)
        const bool panel = p.panel, rpanel = p.rpanel;
        const bool pfw = panel;           // spare workgroups prefetch the next launch's weights (common.h prefetch_region)
        float* stats = (float*)(ws + w.stats);         // [layers][2] tables of [Me][slots][2] partial row sums (no zeroing needed)
        const size_t tbl = (size_t)cpt::ln_stat_slots(H) * Me * 2;
        for (int l = 0; l < d.layers; ++l) {
            const cpt_layer& y = m->layers[l];
            const cpt_layer_fold& f = m->fold[l];
            float* st1 = stats + ((size_t)l * 2 + 0) * tbl;
            float* st2 = stats + ((size_t)l * 2 + 1) * tbl;
            const float* st2p = l > 0 ? stats + ((size_t)(l - 1) * 2 + 1) * tbl : nullptr;
            const cpt_layer* yp = l > 0 ? &m->layers[l - 1] : nullptr;
            if (p.attn_form) {
                Scope sc(CPT_K_GEMM_QKV, s);      // QKV projection + attention, one kernel; q/k/v never reach HBM
                if (l == 0) TRY(qkv_attn(y.w_qkv, y.b_qkv, nullptr, nullptr, nullptr, f.w_qkv_t), "gemm(qkv)+attention");
                else TRY(qkv_attn(f.w_qkv_f, nullptr, st2p, f.c_qkv, f.d_qkv, f.w_qkv_t), "gemm(qkv, folded LN)+attention");
            } else {
                { Scope sc(CPT_K_GEMM_QKV, s);
                  if (l == 0) TRY(cpt::gemm(dt, CPT_EPI_NONE, x_lp, H, y.w_qkv, H, y.b_qkv, nullptr, 0, qkv, dt, 3 * H, Me, 3 * H, H, s), "gemm(qkv)");
                  else TRY(cpt::gemm_ln_cons(x_lp, H, f.w_qkv_f, H, st2p, f.c_qkv, f.d_qkv, d.ln_eps, H, 0, qkv, 3 * H, Me, 3 * H, H, s), "gemm(qkv, folded LN)"); }
                { Scope sc(CPT_K_ATTN, s);
                  TRY(cpt::attention(dt, qkv, b->attn_mask, ctx, nullptr, B, L, d.heads, s, nullptr, p.mask3, panel), "attention"); }
            }
            if (p.tail == TAIL_BF16 && l + 1 == d.layers) return tail_bf16(y, *yp);      // (the plan asks for two layers at least)
            { Scope sc(CPT_K_GEMM_AO, s);
              if (panel) TRY(cpt::gemm_ln_prod3_panel(ctx, y.w_ao, H, y.b_ao, x_lp, x_lo(), H, st2p, yp ? yp->ln2_g : nullptr, yp ? yp->ln2_b : nullptr, d.ln_eps, H,
                                                      a_lp, a_lo(), st1, H, Me, H, H, s, pfw ? f.w_in_f : nullptr, (size_t)I * H * 2, nullptr, 0, rpanel), "gemm(attn out, LN producer, panel A)");
              else TRY(cpt::gemm_ln_prod3(ctx, H, y.w_ao, H, y.b_ao, x_lp, x_lo(), H, st2p, yp ? yp->ln2_g : nullptr, yp ? yp->ln2_b : nullptr, d.ln_eps, H,
                                          a_lp, a_lo(), st1, H, Me, H, H, s), "gemm(attn out, LN producer, 3-byte residual)"); }
            { Scope sc(CPT_K_GEMM_FFN1, s);
              TRY(cpt::gemm_ln_cons(a_lp, H, f.w_in_f, H, st1, f.c_in, f.d_in, d.ln_eps, H, 1, ffn, I, Me, I, H, s, p.panel_ffn, pfw ? y.w_out : nullptr, (size_t)H * I * 2, rpanel), "gemm(ffn up, folded LN)"); }
            { Scope sc(CPT_K_GEMM_FFN2, s);
              if (p.panel_ffn) {
                  // next layer's QKV weight (the copy its launch will read) and attention-output weight
                  const void* nq = nullptr; const void* na = nullptr;
                  size_t nqb = (size_t)3 * H * H * 2, nab = (size_t)H * H * 2;
                  if (pfw && l + 1 < d.layers) {
                      const cpt_layer_fold& fn = m->fold[l + 1];
                      nq = fn.w_qkv_t ? fn.w_qkv_t : fn.w_qkv_f;
                      na = m->layers[l + 1].w_ao;
                  } else if (pfw && (flags & CPT_OUT_MASK_LOGITS) && m->w_tr) {
                      // last layer: the MLM head's transform dense (the 47 MB tied decoder table is streamed by the head's first launch, which has the chip to itself)
                      nq = m->w_tr; nqb = (size_t)H * H * 2;
                      na = nullptr; nab = 0;
                  }
                  TRY(cpt::gemm_ln_prod3_panel(ffn, y.w_out, I, y.b_out, a_lp, a_lo(), H, st1, y.ln1_g, y.ln1_b, d.ln_eps, H, x_lp, x_lo(), st2, H, Me, H, I, s,
                                               nq, nqb, na, nab, rpanel), "gemm(ffn down, LN producer, panel A)");
              } else TRY(cpt::gemm_ln_prod3(ffn, I, y.w_out, I, y.b_out, a_lp, a_lo(), H, st1, y.ln1_g, y.ln1_b, d.ln_eps, H, x_lp, x_lo(), st2, H, Me, H, I, s),
                         "gemm(ffn down, LN producer, 3-byte residual)"); }
        }
        // x now holds the last pre-LayerNorm sum: materialise LayerNorm only where an output reads every row
        if (!p.pre_ln) {
            const cpt_layer& yl = m->layers[d.layers - 1];
            Scope sc(CPT_K_LN, s);
            TRY(cpt::r3_merge(x_lp, x_lo(), nullptr, pre, Me, L, H, 0, s, rpanel), "resid3_merge(all rows)");   // (x_lo() lives in the x_f32 region)
            TRY(cpt::layernorm_rows(pre, yl.ln2_g, yl.ln2_b, d.ln_eps, x_f32, x_lp, dt, Me, H, Me, 0, 0, s), "layernorm(final)");
        }
        return CPT_OK;
    }

    // the last layer of the fp32 encoder on the head's rows (plan: TAIL_F32)
    int tail_f32(const cpt_layer& y) const {
        Scope sc(CPT_K_HEAD, s);
        const int64_t* pos = p.want_mask ? b->mask_pos : nullptr;
        float* xr = (float*)(ws + w.rows_f32);
        void* ctx_r = qkv;                                 // (q | k | v of this layer are consumed)
        TRY(cpt::gather_rows(ctx, dt, pos, ctx_r, B, L, H, s), "tail: gather(ctx rows)");
        TRY(cpt::gather_rows(x_f32, CPT_F32, pos, xr, B, L, H, s), "tail: gather(residual rows)");
        TRY(gm(CPT_EPI_RESID, ctx_r, H, y.w_ao, H, y.b_ao, xr, H, pre, CPT_F32, H, B, H), "tail: gemm(attn out)");
        TRY(cpt::layernorm_rows(pre, y.ln1_g, y.ln1_b, d.ln_eps, a_f32, nullptr, dt, B, H, B, 0, 0, s), "tail: layernorm(attn)");
        TRY(gm(CPT_EPI_GELU, a_f32, H, y.w_in, H, y.b_in, nullptr, 0, ffn, dt, I, B, I), "tail: gemm(ffn up)");
        TRY(gm(CPT_EPI_RESID, ffn, I, y.w_out, I, y.b_out, a_f32, H, pre, CPT_F32, H, B, H), "tail: gemm(ffn down)");
        TRY(cpt::layernorm_rows(pre, y.ln2_g, y.ln2_b, d.ln_eps, (float*)(ws + w.rows), nullptr, dt, B, H, B, 0, 0, s), "tail: layernorm(ffn)");
        return CPT_OK;
    }

    // the last layer of the bf16x3 encoder on the head's rows (plan: TAIL_X3)
    int tail_x3(const cpt_layer& y) const {
        Scope sc(CPT_K_HEAD, s);
        const int64_t* pos = p.want_mask ? b->mask_pos : nullptr;
        float* part = (float*)ffn;                        // [S][B][N] split-K partial matrices
        float* xr = (float*)(ws + w.rows_f32);           // residual rows (the previous layer's output)
        void* ctx_r = ctx;                                 // [B][3H] split copy of the rows' attention context (the fp32 ctx region is idle in this mode)
        void* asplit_r = pre;                              // [B][3H]
        void* hsplit_r = qkv;                              // [B][3I] (q | k | v of this layer are consumed)
        TRY(cpt::gather_rows(gm.split, CPT_BF16, pos, ctx_r, B, L, 3 * H, s), "tail: gather(ctx rows, split copy)");
        TRY(cpt::gather_rows(x_f32, CPT_F32, pos, xr, B, L, H, s), "tail: gather(residual rows)");
        TRY(cpt::gemm_rows_split(ctx_r, 3 * H, y.w_ao, 3 * H, y.b_ao, part, B, H, 3 * H, s), "tail: gemm(attn out, split K, split operands)");
        TRY(cpt::tail_finish(part, p.tail_s1, xr, y.ln1_g, y.ln1_b, d.ln_eps, a_f32, nullptr, B, H, s), "tail: partials + residual + layernorm(attn)");
        TRY(cpt::split3(a_f32, H, asplit_r, B, H, 0, s), "tail: split3(ffn up input)");
        TRY(cpt::gemm_rows_split(asplit_r, 3 * H, y.w_in, 3 * H, y.b_in, part, B, I, 3 * H, s), "tail: gemm(ffn up, split K, split operands)");
        TRY(cpt::gelu_parts(part, p.tail_s1, hsplit_r, (size_t)B * I, s, nullptr, 0, I), "tail: partials + gelu -> split copy");
        TRY(cpt::gemm_rows_split(hsplit_r, 3 * I, y.w_out, 3 * I, y.b_out, part, B, H, 3 * I, s), "tail: gemm(ffn down, split K, split operands)");
        TRY(cpt::tail_finish(part, p.tail_s2, a_f32, y.ln2_g, y.ln2_b, d.ln_eps, (float*)(ws + w.rows), nullptr, B, H, s), "tail: partials + residual + layernorm(ffn)");
        return CPT_OK;
    }

    // (a5-a9) the encoder with its LayerNorms as passes of their own and an fp32 residual: fp32, bf16x3, and bf16 models without the folded weights
    int encoder_plain() const {
        void* const splitbuf = gm.split;
        void* const asplit = ffn;                                                                     // bf16x3 fused mode: see FwdPlan x3f
        for (int l = 0; l < d.layers; ++l) {
            const cpt_layer& y = m->layers[l];
            if (p.attn_form) {
                Scope sc(CPT_K_GEMM_QKV, s);
                TRY(qkv_attn(y.w_qkv, y.b_qkv, nullptr, nullptr, nullptr, nullptr), "gemm(qkv)+attention");
            } else {
                { Scope sc(CPT_K_GEMM_QKV, s);
                  TRY(gm(CPT_EPI_NONE, x_lp, H, y.w_qkv, H, y.b_qkv, nullptr, 0, qkv, dt, 3 * H, M, 3 * H), "gemm(qkv)"); }
                { Scope sc(CPT_K_ATTN, s);
                  if (p.x3a) TRY(cpt::attention_x3((const float*)qkv, b->attn_mask, nullptr, splitbuf, B, L, d.heads, s), "attention (split operands)");
                  else TRY(cpt::attention(dt, qkv, b->attn_mask, ctx, nullptr, B, L, d.heads, s, nullptr, p.mask3), "attention"); }
            }
            if (l + 1 == d.layers && p.tail == TAIL_F32) return tail_f32(y);
            if (l + 1 == d.layers && p.tail == TAIL_X3) return tail_x3(y);
            { Scope sc(CPT_K_GEMM_AO, s);
              if (p.x3a) TRY(cpt::gemm(CPT_BF16, CPT_EPI_RESID, splitbuf, 3 * H, y.w_ao, 3 * H, y.b_ao, x_f32, H, pre, CPT_F32, H, M, H, 3 * H, s), "gemm(attn out, split ctx)");
              else TRY(gm(CPT_EPI_RESID, ctx, H, y.w_ao, H, y.b_ao, x_f32, H, pre, CPT_F32, H, M, H), "gemm(attn out)"); }
            { Scope sc(CPT_K_LN, s);
              TRY(cpt::layernorm_rows(pre, y.ln1_g, y.ln1_b, d.ln_eps, a_f32, lp ? a_lp : nullptr, dt, M, H, M, 0, 0, s), "layernorm(attn)"); }
            if (p.x3f) {
                // the FFN-up's GELU epilogue writes h as the split copy the FFN-down reads; its own input split sits in the (then unused) fp32 h region
                { Scope sc(CPT_K_GEMM_FFN1, s);
                  TRY(cpt::split3((const float*)a_lp, H, asplit, M, H, 0, s), "split3(ffn up input)");
                  TRY(cpt::gemm_gelu_x3(asplit, 3 * H, y.w_in, 3 * H, y.b_in, splitbuf, M, I, 3 * H, s), "gemm(ffn up, split output)"); }
                { Scope sc(CPT_K_GEMM_FFN2, s);
                  TRY(cpt::gemm(CPT_BF16, CPT_EPI_RESID, splitbuf, 3 * I, y.w_out, 3 * I, y.b_out, a_f32, H, pre, CPT_F32, H, M, H, 3 * I, s), "gemm(ffn down)"); }
            } else {
                { Scope sc(CPT_K_GEMM_FFN1, s);
                  TRY(gm(CPT_EPI_GELU, a_lp, H, y.w_in, H, y.b_in, nullptr, 0, ffn, dt, I, M, I), "gemm(ffn up)"); }
                { Scope sc(CPT_K_GEMM_FFN2, s);
                  TRY(gm(CPT_EPI_RESID, ffn, I, y.w_out, I, y.b_out, a_f32, H, pre, CPT_F32, H, M, H), "gemm(ffn down)"); }
            }
            { Scope sc(CPT_K_LN, s);
              TRY(cpt::layernorm_rows(pre, y.ln2_g, y.ln2_b, d.ln_eps, x_f32, lp ? x_lp : nullptr, dt, M, H, M, 0, 0, s), "layernorm(ffn)"); }
        }
        return CPT_OK;
    }

    // sequence_output: the encoder's output, every real row, as fp32
    int seq_out() const {
        if (!o->seq) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd: seq output is NULL");
        hipError_t e = hipMemcpyAsync(o->seq, x_f32, (size_t)M * H * 4, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return abi_fail(CPT_ERR_HIP - (int)e, "copy sequence_output: %s", hipGetErrorString(e));
        return CPT_OK;
    }

    // The B rows a head reads -- [CLS] (pos == NULL) or [MASK] (pos = mask_pos) -- of the encoder's output, in the compute dtype, into w.rows:
    // the tail already wrote them / LayerNorm of the pre-LayerNorm rows / a plain gather.  pf: the part of the decoder table the [MASK] form prefetches.
    int head_rows(const int64_t* pos, const void* pf, size_t pf_bytes) const {
        void* rows = ws + w.rows;
        if (p.tail != TAIL_NONE) return CPT_OK;
        if (!p.pre_ln) {
            TRY(cpt::gather_rows(x_lp, dt, pos, rows, B, L, H, s), pos ? "gather([MASK])" : "gather([CLS])");
            return CPT_OK;
        }
        const cpt_layer& yl = m->layers[d.layers - 1];
        if (pos) {
            TRY(cpt::head_rows_ln3(x_lp, x_lo(), pos, yl.ln2_g, yl.ln2_b, d.ln_eps, rows, B, L, H, s, pf, pf_bytes, p.rpanel), "gather + merge + layernorm([MASK] rows)");
        } else {
            float* rf = (float*)(ws + w.rows_f32);
            TRY(cpt::r3_merge(x_lp, x_lo(), nullptr, rf, B, L, H, 1, s, p.rpanel), "resid3_merge([CLS] pre-LN)");
            TRY(cpt::layernorm_rows(rf, yl.ln2_g, yl.ln2_b, d.ln_eps, nullptr, rows, dt, B, H, B, 0, 0, s), "layernorm([CLS] rows)");
        }
        return CPT_OK;
    }

    // (a10) pooler, optional NSP-style relation head
    int pooler() const {
        Scope sc(CPT_K_HEAD, s);
        float* pooled = (flags & CPT_OUT_POOLED) ? o->pooled : (float*)(ws + w.pooled_f32);
        if (!pooled) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd: pooled output is NULL");
        if (int rc = head_rows(nullptr, nullptr, 0)) return rc;
        TRY(gm(CPT_EPI_TANH, ws + w.rows, H, m->w_pool, H, m->b_pool, nullptr, 0, pooled, CPT_F32, H, B, H), "gemm(pooler)");
        if (flags & CPT_OUT_REL) {
            if (!o->rel) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd: rel output is NULL");
            const void* pin = pooled;
            if (lp) {
                void* plp = ws + w.pooled_lp;
                TRY(cpt::layernorm_rows(pooled, nullptr, nullptr, 0.f, nullptr, plp, dt, B, H, B, 0, 0, s), "cast(pooled)");
                pin = plp;
            }
            TRY(gm(CPT_EPI_NONE, pin, H, m->w_rel, H, m->b_rel, nullptr, 0, o->rel, CPT_F32, d.n_rel, B, d.n_rel), "gemm(seq_relationship)");
        }
        return CPT_OK;
    }

    // (a11,a12) MLM head on the [MASK] rows (or every row), optional CE loss
    int mlm_head() const {
        Scope sc(CPT_K_HEAD, s);
        if (!o->logits) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd: logits output is NULL");
        const bool all = flags & CPT_OUT_ALL_LOGITS;
        const int R = all ? M : B;
        const void* rows = x_lp;
        // the decoder's weight table (47 MB at Oscar-base) is pulled into the Infinity Cache by spare workgroups of the head's two row launches:
        // g_dec_pf_pct percent by the first (gather + LayerNorm; with a tail: the tail's row launches), the rest by the reduce + GELU + LayerNorm launch
        const size_t dec_bytes = (size_t)d.vocab * H * 2;
        const size_t pf0 = cols ? dec_bytes : dec_pf0();      // (column list: no table prefetch -- pf0 = all: nothing left for the second launch either)
        if (!all) {
            if (int rc = head_rows(b->mask_pos, !cols ? m->w_dec : nullptr, cols ? 0 : pf0)) return rc;
            rows = ws + w.rows;
        }
        float* t1 = (float*)(ws + w.t1);
        void* t2 = ws + w.t2;
        const bool dec_pf_split = p.pre_ln && !all;
        if (p.head_splits) {
            TRY(cpt::gemm_head_transform(rows, H, m->w_tr, H, m->b_tr, pre, R, H, H, s), "gemm(head transform, split K)");
            TRY(cpt::head_finish(pre, p.head_splits, m->tr_ln_g, m->tr_ln_b, d.ln_eps, t2, R, H, s,
                                 dec_pf_split && pf0 < dec_bytes ? (const unsigned char*)m->w_dec + pf0 : nullptr, dec_bytes - pf0), "reduce + gelu + layernorm(head)");
        } else {
            TRY(gm(CPT_EPI_GELU, rows, H, m->w_tr, H, m->b_tr, nullptr, 0, t1, CPT_F32, H, R, H), "gemm(head transform)");
            TRY(cpt::layernorm_rows(t1, m->tr_ln_g, m->tr_ln_b, d.ln_eps, lp ? nullptr : (float*)t2, lp ? t2 : nullptr, dt, R, H, R, 0, 0, s), "layernorm(head)");
        }
        if (cols) TRY(cpt::decoder_cols(t2, p.x3 ? 2 : (lp ? 0 : 1), m->w_dec, m->b_dec, o->logit_cols, (int)o->n_logit_cols, o->logits, R, H, d.vocab, s), "decoder(column list)");
        else TRY(gm(CPT_EPI_NONE, t2, H, m->w_dec, H, m->b_dec, nullptr, 0, o->logits, CPT_F32, d.vocab, R, d.vocab), "gemm(decoder)");
        if (flags & CPT_OUT_LOSS) {
            hipError_t e = hipMemsetAsync(o->loss, 0, 2 * sizeof(float), s);
            if (e != hipSuccess) return abi_fail(CPT_ERR_HIP - (int)e, "zero loss: %s", hipGetErrorString(e));
            TRY(cpt::ce_rows(o->logits, b->labels, o->loss, nullptr, R, d.vocab, s), "ce_rows");
        }
        return CPT_OK;
    }
};

}  // namespace

// seq_in_ws (cpt_model_fwd_rows): with CPT_OUT_SEQ the encoder output stays in the workspace (x_f32 / x_lp of fwd_layout), o->seq is not used
static int model_fwd(const cpt_model* m, const cpt_batch* b, const cpt_outputs* o, int flags,
                     void* workspace, size_t workspace_bytes, void* stream, bool seq_in_ws, const cpt_soft_template* soft = nullptr) {
    if (!m || !b || !o || !workspace) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd: null argument");
    if (soft && soft->tmpl) {
        if (soft->n_slots < 2 || soft->n_slots > m->dims.vocab) return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd_soft: n_slots %d outside [2, vocabulary %d]", soft->n_slots, m->dims.vocab);
        if ((uintptr_t)soft->tmpl & 15) return abi_fail(CPT_ERR_ALIGN, "cpt_model_fwd_soft: tmpl must be 16-byte aligned");
    }
    const cpt_dims& d = m->dims;
    hipStream_t s = (hipStream_t)stream;
    const int B = b->B, Lt = b->Lt, Li = b->Li, L = Lt + Li, H = d.hidden;
    if (B <= 0 || Lt <= 0 || Li < 0) return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd: bad batch shape B=%d Lt=%d Li=%d", B, Lt, Li);
    if (d.heads <= 0 || H != d.heads * 64) return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd: hidden %d / heads %d: head_dim must be 64", H, d.heads);
    if (L > cpt::attention_max_len(1)) return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd: sequence length %d > %d not supported", L, cpt::attention_max_len(1));
    if (d.dtype == CPT_BF16X3_MASTERS)
        return abi_fail(CPT_ERR_DTYPE, "cpt_model_fwd: CPT_BF16X3_MASTERS (fp32 master weights) is the training step's tag; inference reads the split copies under CPT_BF16X3");
    if (d.dtype != CPT_F32 && d.dtype != CPT_BF16 && d.dtype != CPT_BF16X3) return abi_fail(CPT_ERR_DTYPE, "cpt_model_fwd: dtype %d", d.dtype);
    if (d.img_dim_pad < d.img_dim || d.img_dim_pad % 8) return abi_fail(CPT_ERR_ALIGN, "cpt_model_fwd: img_dim_pad %d must be >= img_dim and a multiple of 8", d.img_dim_pad);
    if (Li > 0 && !b->img_feats) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd: img_feats is NULL with Li=%d", Li);
    if ((flags & (CPT_OUT_MASK_LOGITS | CPT_OUT_ALL_LOGITS)) == (CPT_OUT_MASK_LOGITS | CPT_OUT_ALL_LOGITS))
        return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd: choose mask-row logits or all-row logits, not both");
    if ((flags & CPT_OUT_MASK_LOGITS) && !b->mask_pos) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd: mask_pos required for CPT_OUT_MASK_LOGITS");
    if ((flags & CPT_OUT_LOSS) && !(flags & (CPT_OUT_MASK_LOGITS | CPT_OUT_ALL_LOGITS)))
        return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd: CPT_OUT_LOSS needs a logits output");
    if ((flags & CPT_OUT_LOSS) && (!b->labels || !o->loss)) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd: labels/loss required for CPT_OUT_LOSS");
    if ((flags & CPT_OUT_REL) && (!m->w_rel || d.n_rel <= 0)) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd: model has no seq_relationship head");
    const bool cols = o->logit_cols != nullptr && o->n_logit_cols > 0;
    if (cols && (!(flags & CPT_OUT_MASK_LOGITS) || (flags & CPT_OUT_LOSS)))
        return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd: logit_cols goes with CPT_OUT_MASK_LOGITS and without CPT_OUT_LOSS");
    if (cols && o->n_logit_cols > d.vocab) return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd: n_logit_cols %lld > vocabulary %d", (long long)o->n_logit_cols, d.vocab);
    const FwdPlan p = make_plan(d, B, Lt, Li, flags, m->fold != nullptr);
    const FwdLayout w = fwd_layout(d, p, flags);
    if (workspace_bytes < w.total) return abi_fail(CPT_ERR_WORKSPACE, "cpt_model_fwd: workspace %zu < required %zu bytes", workspace_bytes, w.total);
    if ((uintptr_t)workspace & 255) return abi_fail(CPT_ERR_ALIGN, "cpt_model_fwd: workspace must be 256-byte aligned");

    unsigned char* ws = (unsigned char*)workspace;
    const Fwd c = {p, d, m, b, o, flags, cols, ws, w, s, ModeGemm{p.x3, p.dt, ws + w.split, s}, B, Lt, Li, L, p.M, H, d.inter, p.dt, p.lp,
                   (float*)(ws + w.x_f32), ws + w.x_lp, ws + w.qkv, ws + w.ctx, (float*)(ws + w.pre), (float*)(ws + w.a_f32), ws + w.a_lp, ws + w.ffn,
                   soft ? soft->tmpl : nullptr, (soft && soft->tmpl) ? soft->n_slots : 0};
    int rc = c.embed();
    if (rc == CPT_OK) rc = p.fold ? c.encoder_folded() : c.encoder_plain();
    if (rc == CPT_OK && (flags & CPT_OUT_SEQ) && !seq_in_ws) rc = c.seq_out();
    if (rc == CPT_OK && (flags & (CPT_OUT_POOLED | CPT_OUT_REL))) rc = c.pooler();
    if (rc == CPT_OK && (flags & (CPT_OUT_MASK_LOGITS | CPT_OUT_ALL_LOGITS))) rc = c.mlm_head();
    return rc;
}

int cpt_model_fwd(const cpt_model* m, const cpt_batch* b, const cpt_outputs* o, int flags,
                  void* workspace, size_t workspace_bytes, void* stream) {
    return model_fwd(m, b, o, flags, workspace, workspace_bytes, stream, false);
}

int cpt_model_fwd_soft(const cpt_model* m, const cpt_soft_template* st, const cpt_batch* b, const cpt_outputs* o, int flags,
                       void* workspace, size_t workspace_bytes, void* stream) {
    return model_fwd(m, b, o, flags, workspace, workspace_bytes, stream, false, st);
}

// ---- MLM head on a list of rows + full-vocabulary log-sum-exp (VG-CPT predicate scoring) -----------------------------------------
// The encoder runs as cpt_model_fwd with CPT_OUT_SEQ (the whole last layer; its output stays in the workspace), the head rows are gathered
// by (sequence, position), then transform + LayerNorm as the all-row head, then the mode's decoder GEMM over all V columns -- into `logits`
// itself without a column list, else into the workspace -- and one pass per row for the log-sum-exp (head_lse.hip row_lse).
namespace {
struct RowsLayout { size_t enc, x_lp, g, t1, t2, split, full, total; };
RowsLayout rows_layout(const cpt_dims& d, const FwdPlan& p, int R, int n_cols, int enc_flags) {
    const size_t H = d.hidden, V = d.vocab;
    const FwdLayout fl = fwd_layout(d, p, enc_flags);
    RowsLayout w;
    size_t o = al(fl.total);
    auto take = [&](size_t bytes) { size_t p = o; o += al(bytes); return p; };
    w.enc = 0;
    w.x_lp = fl.x_lp;       // the encoder output (LayerNorm'ed) in the compute dtype, row-major [B * L][H] (fp32 and bf16x3: the x_f32 region itself)
    w.g = take((size_t)R * H * 4);
    w.t1 = take((size_t)R * H * 4);
    w.t2 = take((size_t)R * H * 4);
    w.split = p.x3 ? take((size_t)R * 3 * H * 2) : 0;
    w.full = n_cols > 0 ? take((size_t)R * V * 4) : 0;
    w.total = o;
    return w;
}
}  // namespace

size_t cpt_fwd_rows_workspace_bytes(const cpt_dims* d, int B, int Lt, int Li, int n_rows, int n_cols) {
    if (!d || B <= 0 || Lt <= 0 || Li < 0 || n_rows <= 0 || n_cols < 0) return 0;
    // (a [B][L][L] mask never pads the encoder's rows: the 2-D layout is the larger one)
    const int f2 = CPT_OUT_SEQ, f3 = CPT_OUT_SEQ | CPT_ATTN_MASK_3D;
    return std::max(rows_layout(*d, make_plan(*d, B, Lt, Li, f2, true), n_rows, n_cols, f2).total,
                    rows_layout(*d, make_plan(*d, B, Lt, Li, f3, true), n_rows, n_cols, f3).total);
}

static int model_fwd_rows(const cpt_model* m, const cpt_soft_template* soft, const cpt_batch* b, const int64_t* cols, int n_cols, float* logits, float* row_lse,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || !b) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd_rows: null argument");
    const cpt_dims& d = m->dims;
    hipStream_t s = (hipStream_t)stream;
    const int B = b->B, Lt = b->Lt, Li = b->Li, L = Lt + Li, R = b->n_rows, H = d.hidden, V = d.vocab;
    if (B <= 0 || Lt <= 0 || Li < 0) return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd_rows: bad batch shape B=%d Lt=%d Li=%d", B, Lt, Li);
    if (d.dtype != CPT_F32 && d.dtype != CPT_BF16 && d.dtype != CPT_BF16X3) return abi_fail(CPT_ERR_DTYPE, "cpt_model_fwd_rows: dtype %d", d.dtype);
    if (R <= 0) return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd_rows: n_rows %d must be > 0", R);
    if (!logits) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd_rows: logits is NULL");
    if ((long)R > (long)B * L) return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd_rows: n_rows %d > B * L = %ld", R, (long)B * L);
    if (!b->row_seq || !b->mask_pos) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd_rows: row_seq and mask_pos are required");
    if (cols && (n_cols <= 0 || n_cols > V)) return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd_rows: n_cols %d outside (0, %d]", n_cols, V);
    if (!m->w_tr || !m->w_dec) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd_rows: model has no MLM head");
    if (!workspace) return abi_fail(CPT_ERR_NULL, "cpt_model_fwd_rows: null workspace");
    const int nc = cols ? n_cols : 0;
    const int eflags = CPT_OUT_SEQ | (b->mask_3d ? CPT_ATTN_MASK_3D : 0);
    const FwdPlan p = make_plan(d, B, Lt, Li, eflags, m->fold != nullptr);
    const RowsLayout w = rows_layout(d, p, R, nc, eflags);
    if (workspace_bytes < w.total) return abi_fail(CPT_ERR_WORKSPACE, "cpt_model_fwd_rows: workspace %zu < required %zu bytes", workspace_bytes, w.total);
    if ((uintptr_t)workspace & 255) return abi_fail(CPT_ERR_ALIGN, "cpt_model_fwd_rows: workspace must be 256-byte aligned");
    {   // the row list and the column list, checked on the host
        std::vector<int64_t> rs((size_t)R), mp((size_t)R), cl((size_t)(cols ? n_cols : 0));
        hipError_t e = hipMemcpyAsync(rs.data(), b->row_seq, (size_t)R * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(mp.data(), b->mask_pos, (size_t)R * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && cols) e = hipMemcpyAsync(cl.data(), cols, (size_t)n_cols * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return abi_fail(CPT_ERR_HIP - (int)e, "cpt_model_fwd_rows: read row list: %s", hipGetErrorString(e));
        for (int r = 0; r < R; ++r) {
            if (rs[r] < 0 || rs[r] >= B || (r > 0 && rs[r] < rs[r - 1]))
                return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd_rows: row_seq[%d] = %lld: must be ascending in [0, %d)", r, (long long)rs[r], B);
            if (mp[r] < 0 || mp[r] >= L)
                return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd_rows: mask_pos[%d] = %lld outside [0, %d)", r, (long long)mp[r], L);
        }
        for (size_t j = 0; j < cl.size(); ++j)
            if (cl[j] < 0 || cl[j] >= V)
                return abi_fail(CPT_ERR_SHAPE, "cpt_model_fwd_rows: cols[%zu] = %lld outside [0, %d)", j, (long long)cl[j], V);
    }
    unsigned char* ws = (unsigned char*)workspace;
    cpt_outputs o;
    memset(&o, 0, sizeof(o));
    int rc = model_fwd(m, b, &o, eflags, workspace, workspace_bytes, stream, true, soft);
    if (rc != CPT_OK) return rc;

    Scope sc(CPT_K_HEAD, s);
    const int dt = p.dt;
    const bool lp = p.lp;
    const ModeGemm gm = {p.x3, dt, ws + w.split, s};
    void* g = ws + w.g;
    float* t1 = (float*)(ws + w.t1);
    void* t2 = ws + w.t2;
    TRY(cpt::gather_rows(ws + w.x_lp, dt, b->mask_pos, g, R, L, H, s, b->row_seq, B), "gather(head rows)");
    TRY(gm(CPT_EPI_GELU, g, H, m->w_tr, H, m->b_tr, nullptr, 0, t1, CPT_F32, H, R, H), "gemm(head transform)");
    TRY(cpt::layernorm_rows(t1, m->tr_ln_g, m->tr_ln_b, d.ln_eps, lp ? nullptr : (float*)t2, lp ? t2 : nullptr, dt, R, H, R, 0, 0, s), "layernorm(head)");
    if (!cols) {
        TRY(gm(CPT_EPI_NONE, t2, H, m->w_dec, H, m->b_dec, nullptr, 0, logits, CPT_F32, V, R, V), "gemm(decoder)");
        if (row_lse) TRY(cpt::row_lse(logits, row_lse, R, V, s), "row log-sum-exp");
    } else {
        float* full = (float*)(ws + w.full);
        TRY(gm(CPT_EPI_NONE, t2, H, m->w_dec, H, m->b_dec, nullptr, 0, full, CPT_F32, V, R, V), "gemm(decoder)");
        if (row_lse) TRY(cpt::row_lse(full, row_lse, R, V, s), "row log-sum-exp");
        TRY(cpt::gather_cols(full, cols, logits, R, n_cols, V, s), "gather(column list)");
    }
    return CPT_OK;
}

int cpt_model_fwd_rows(const cpt_model* m, const cpt_batch* b, const int64_t* cols, int n_cols, float* logits, float* row_lse,
                       void* workspace, size_t workspace_bytes, void* stream) {
    return model_fwd_rows(m, nullptr, b, cols, n_cols, logits, row_lse, workspace, workspace_bytes, stream);
}

int cpt_model_fwd_rows_soft(const cpt_model* m, const cpt_soft_template* st, const cpt_batch* b, const int64_t* cols, int n_cols, float* logits,
                            float* row_lse, void* workspace, size_t workspace_bytes, void* stream) {
    return model_fwd_rows(m, st, b, cols, n_cols, logits, row_lse, workspace, workspace_bytes, stream);
}

int cpt_mean_logprob_scores(const float* logits, int n_cols, int n_rows, const float* row_lse, const int32_t* slot_row, int G, int K,
                            const int32_t* cand_cols, const int32_t* cand_len, int C, float* out, void* stream) {
    if (!logits || !row_lse || !slot_row || !cand_cols || !cand_len || !out) return abi_fail(CPT_ERR_NULL, "cpt_mean_logprob_scores: null argument");
    if (n_cols <= 0 || n_rows <= 0 || G <= 0 || K <= 0 || C <= 0)
        return abi_fail(CPT_ERR_SHAPE, "cpt_mean_logprob_scores: n_cols %d n_rows %d G %d K %d C %d", n_cols, n_rows, G, K, C);
    return abi_check(cpt::mean_logprob(logits, n_cols, n_rows, row_lse, slot_row, G, K, cand_cols, cand_len, C, out, (hipStream_t)stream),
                        "cpt_mean_logprob_scores");
}

size_t cpt_vg_recall_workspace_bytes(const int32_t* cand_off, int n_img) {
    if (!cand_off || n_img <= 0) return 0;
    long long big = 0;
    for (int i = 0; i < n_img; ++i) {
        const long long n = (long long)cand_off[i + 1] - cand_off[i];
        if (n > cpt::vg_recall_tile()) big += n;
    }
    return cpt::vg_recall_ws_bytes(big);
}

int cpt_vg_recall_ranks(const float* scores, int n_rows, int C, const int32_t* cand_off, const int32_t* cand, int n_cand, const int32_t* gt_off,
                        const int32_t* gt, int n_gt, int n_img, int32_t* out_rank, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cand_off || !gt_off || (n_rows > 0 && !scores) || (n_cand > 0 && !cand) || (n_gt > 0 && (!gt || !out_rank)))
        return abi_fail(CPT_ERR_NULL, "cpt_vg_recall_ranks: null argument");
    if (n_img <= 0 || C < 2 || n_rows < 0 || n_cand < 0 || n_gt < 0)
        return abi_fail(CPT_ERR_SHAPE, "cpt_vg_recall_ranks: n_img %d C %d n_rows %d n_cand %d n_gt %d", n_img, C, n_rows, n_cand, n_gt);
    return abi_check(cpt::vg_recall(scores, n_rows, C, cand_off, cand, n_cand, gt_off, gt, n_gt, n_img, out_rank, workspace, workspace_bytes,
                                       (hipStream_t)stream), "cpt_vg_recall_ranks");
}

}  // extern "C"

// ---- VCR Q->AR: the two relation heads on pooled rows, and the Q->AR choice (qar_head.hip) ----
extern "C" {

size_t cpt_rel2_workspace_bytes(int B) {
    if (B <= 0) return 0;
    return 256 + ((size_t)B * 4 + 255) / 256 * 256;      // [0, 256): the finish ticket; then B row losses
}

int cpt_rel2_scores(int dtype, const float* pooled, int B, int H, int n_rel, int B0, const void* w0, const float* b0, const void* w1, const float* b1,
                    const int64_t* labels, const int64_t* labels_host, float* rel, float* score, float* loss, float* loss_mean, float* dlogits,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!pooled || !rel) return abi_fail(CPT_ERR_NULL, "cpt_rel2_scores: null argument");
    if (B <= 0 || H <= 0 || n_rel < 1 || n_rel > 64) return abi_fail(CPT_ERR_SHAPE, "cpt_rel2_scores: B %d H %d n_rel %d (1 <= n_rel <= 64)", B, H, n_rel);
    if (B0 < 0 || B0 > B) return abi_fail(CPT_ERR_SHAPE, "cpt_rel2_scores: B0 %d outside [0, B = %d]", B0, B);
    if ((B0 > 0 && (!w0 || !b0)) || (B0 < B && (!w1 || !b1))) return abi_fail(CPT_ERR_NULL, "cpt_rel2_scores: a head with rows has no weights");
    if (score && n_rel < 2) return abi_fail(CPT_ERR_SHAPE, "cpt_rel2_scores: the choice score needs n_rel >= 2");
    if (dtype < CPT_F32 || dtype > CPT_BF16X3_MASTERS) return abi_fail(CPT_ERR_DTYPE, "cpt_rel2_scores: dtype %d", dtype);
    hipStream_t s = (hipStream_t)stream;
    float* rowloss = nullptr;
    unsigned* ticket = nullptr;
    float* dl = nullptr;
    if (labels) {
        if (!workspace || workspace_bytes < cpt_rel2_workspace_bytes(B)) return abi_fail(CPT_ERR_WORKSPACE, "cpt_rel2_scores: workspace %zu < %zu bytes", workspace_bytes, cpt_rel2_workspace_bytes(B));
        if (!dlogits) return abi_fail(CPT_ERR_NULL, "cpt_rel2_scores: labels need dlogits [B][n_rel] (the launch's per-row gradient)");
        if (int rc = cpt::rel2_check_labels(labels, labels_host, B, n_rel, "cpt_rel2_scores", s)) return rc;
        ticket = (unsigned*)workspace;
        rowloss = (float*)((char*)workspace + 256);
        dl = dlogits;
    }
    // (without labels the head pointers of an empty group are never read: pass the other head's so the kernel sees valid pointers)
    const void* w0_ = B0 > 0 ? w0 : w1; const float* b0_ = B0 > 0 ? b0 : b1;
    const void* w1_ = B0 < B ? w1 : w0; const float* b1_ = B0 < B ? b1 : b0;
    return abi_check(cpt::rel2_fwd(dtype == CPT_BF16, pooled, B, H, n_rel, B0, w0_, b0_, w1_, b1_, labels, rel, score, dl, rowloss, ticket, loss,
                                      loss_mean, s), "cpt_rel2_scores");
}

int cpt_vcr_qar_choose(const float* q_a, const float* qa_r, int n_q, int n_ans, int n_rats, const int64_t* ans_label, const int64_t* rat_label,
                       int64_t* preds, uint8_t* flags, int32_t* counts, void* stream) {
    if (!q_a || !qa_r || !ans_label || !rat_label || !preds || !flags) return abi_fail(CPT_ERR_NULL, "cpt_vcr_qar_choose: null argument");
    if (n_q <= 0 || n_ans <= 0 || n_rats <= 0) return abi_fail(CPT_ERR_SHAPE, "cpt_vcr_qar_choose: n_q %d n_ans %d n_rats %d", n_q, n_ans, n_rats);
    return abi_check(cpt::qar_choose(q_a, qa_r, n_q, n_ans, n_rats, ans_label, rat_label, preds, flags, counts, (hipStream_t)stream),
                        "cpt_vcr_qar_choose");
}

}  // extern "C"

// ---- GQA / VCR Q->A evaluation choices and global-norm clipping (choose.hip) ----
extern "C" {

int cpt_gqa_choose(const float* scores, int R, int C, const int32_t* piece_sid, const int32_t* gt_sid, int G, int64_t* pred, uint8_t* correct,
                   int32_t* counts, void* stream) {
    if (!scores || !piece_sid || !gt_sid || !pred || !correct) return abi_fail(CPT_ERR_NULL, "cpt_gqa_choose: null argument");
    if (R <= 0 || C <= 0 || G <= 0) return abi_fail(CPT_ERR_SHAPE, "cpt_gqa_choose: R %d C %d G %d", R, C, G);
    return abi_check(cpt::gqa_choose(scores, R, C, piece_sid, gt_sid, G, pred, correct, counts, (hipStream_t)stream), "cpt_gqa_choose");
}

int cpt_nsp_choose(const float* rel, int N, int n_rel, int interval, const int64_t* labels, float* scores, int64_t* pred, uint8_t* correct,
                   int32_t* counts, void* stream) {
    if (!rel || !labels || !scores || !pred || !correct) return abi_fail(CPT_ERR_NULL, "cpt_nsp_choose: null argument");
    if (N <= 0 || n_rel < 2 || interval <= 0) return abi_fail(CPT_ERR_SHAPE, "cpt_nsp_choose: N %d n_rel %d (>= 2) interval %d", N, n_rel, interval);
    if (N % interval) return abi_fail(CPT_ERR_SHAPE, "cpt_nsp_choose: %d sequences are no whole number of questions of %d choices", N, interval);
    return abi_check(cpt::nsp_choose(rel, N / interval, interval, n_rel, labels, scores, pred, correct, counts, (hipStream_t)stream), "cpt_nsp_choose");
}

size_t cpt_grad_clip_workspace_bytes(void) { return cpt::grad_clip_ws_bytes(); }

int cpt_grad_clip(float* g, size_t n, float max_norm, const double* sq_in, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!g || !out || !workspace) return abi_fail(CPT_ERR_NULL, "cpt_grad_clip: null argument");
    if (n == 0) return abi_fail(CPT_ERR_SHAPE, "cpt_grad_clip: empty buffer");
    if (((uintptr_t)g & 3) || ((uintptr_t)workspace & 3)) return abi_fail(CPT_ERR_SHAPE, "cpt_grad_clip: g and workspace must be 4-byte aligned");
    if (workspace_bytes < cpt::grad_clip_ws_bytes())
        return abi_fail(CPT_ERR_WORKSPACE, "cpt_grad_clip: workspace %zu < %zu bytes", workspace_bytes, cpt::grad_clip_ws_bytes());
    return abi_check(cpt::grad_clip(g, n, max_norm, sq_in, out, workspace, (hipStream_t)stream), "cpt_grad_clip");
}

int cpt_batch_extents(const int64_t* mask, int B, int Lt, int Li, const int64_t* mask_pos, int n_pos, int32_t* out, void* stream) {
    if (!mask || !out || (n_pos > 0 && !mask_pos)) return abi_fail(CPT_ERR_NULL, "cpt_batch_extents: null argument");
    if (B <= 0 || Lt <= 0 || Li < 0 || n_pos < 0) return abi_fail(CPT_ERR_SHAPE, "cpt_batch_extents: B %d Lt %d Li %d n_pos %d", B, Lt, Li, n_pos);
    return abi_check(cpt::batch_extents(mask, B, Lt, Li, mask_pos, n_pos, out, (hipStream_t)stream), "cpt_batch_extents");
}

int cpt_trim_batch(const int64_t* input_ids, const int64_t* token_type, const int64_t* position_ids, const int64_t* attn_mask, const float* img_feats,
                   int B, int Lt, int Li, int img_dim, int Lt_out, int Li_out, int64_t* input_ids_out, int64_t* token_type_out,
                   int64_t* position_ids_out, int64_t* attn_mask_out, float* img_feats_out, void* stream) {
    if (B <= 0 || Lt <= 0 || Li < 0 || Lt_out <= 0 || Lt_out > Lt || Li_out < 0 || Li_out > Li || (Li_out > 0 && img_dim <= 0))
        return abi_fail(CPT_ERR_SHAPE, "cpt_trim_batch: B %d, %d + %d -> %d + %d, img_dim %d", B, Lt, Li, Lt_out, Li_out, img_dim);
    if (!input_ids || !attn_mask || !input_ids_out || !attn_mask_out || (token_type && !token_type_out) || (position_ids && !position_ids_out) ||
        (Li_out > 0 && (!img_feats || !img_feats_out)))
        return abi_fail(CPT_ERR_NULL, "cpt_trim_batch: null argument");
    return abi_check(cpt::trim_batch(input_ids, token_type, position_ids, attn_mask, img_feats, B, Lt, Li, img_dim, Lt_out, Li_out, input_ids_out,
                                     token_type_out, position_ids_out, attn_mask_out, img_feats_out, (hipStream_t)stream), "cpt_trim_batch");
}

int cpt_train_extents(const int64_t* mask, int B, int Lt, int Li, const int64_t* label_grid, const int64_t* positions, int n_pos, int32_t* out,
                      void* stream) {
    if (!mask || !out || (n_pos > 0 && !positions)) return abi_fail(CPT_ERR_NULL, "cpt_train_extents: null argument");
    if (B <= 0 || Lt <= 0 || Li < 0 || n_pos < 0) return abi_fail(CPT_ERR_SHAPE, "cpt_train_extents: B %d Lt %d Li %d n_pos %d", B, Lt, Li, n_pos);
    return abi_check(cpt::train_extents(mask, B, Lt, Li, label_grid, positions, n_pos, out, (hipStream_t)stream), "cpt_train_extents");
}

int cpt_trim_batch_labels(const int64_t* input_ids, const int64_t* token_type, const int64_t* position_ids, const int64_t* attn_mask,
                          const float* img_feats, const int64_t* label_grid, int B, int Lt, int Li, int img_dim, int Lt_out, int Li_out,
                          int64_t* input_ids_out, int64_t* token_type_out, int64_t* position_ids_out, int64_t* attn_mask_out, float* img_feats_out,
                          int64_t* label_grid_out, void* stream) {
    if (B <= 0 || Lt <= 0 || Li < 0 || Lt_out <= 0 || Lt_out > Lt || Li_out < 0 || Li_out > Li || (Li_out > 0 && img_dim <= 0))
        return abi_fail(CPT_ERR_SHAPE, "cpt_trim_batch_labels: B %d, %d + %d -> %d + %d, img_dim %d", B, Lt, Li, Lt_out, Li_out, img_dim);
    if (!input_ids || !attn_mask || !input_ids_out || !attn_mask_out || (token_type && !token_type_out) || (position_ids && !position_ids_out) ||
        (Li_out > 0 && (!img_feats || !img_feats_out)) || !label_grid || !label_grid_out)
        return abi_fail(CPT_ERR_NULL, "cpt_trim_batch_labels: null argument");
    return abi_check(cpt::trim_batch(input_ids, token_type, position_ids, attn_mask, img_feats, B, Lt, Li, img_dim, Lt_out, Li_out, input_ids_out,
                                     token_type_out, position_ids_out, attn_mask_out, img_feats_out, (hipStream_t)stream, label_grid, label_grid_out),
                     "cpt_trim_batch_labels");
}

int cpt_gather_batch(const cpt_resident_store* store, const int32_t* seq_idx, int B, int Lt_out, int Li_out, int64_t* input_ids_out,
                     int64_t* token_type_out, int64_t* attn_mask_out, int64_t* mask_pos_out, float* img_feats_out, void* stream) {
    if (!store || !seq_idx || !input_ids_out || !token_type_out || !attn_mask_out || (Li_out > 0 && !img_feats_out))
        return abi_fail(CPT_ERR_NULL, "cpt_gather_batch: null argument");
    if (B <= 0 || Lt_out <= 0 || Lt_out > store->Lt || Li_out < 0 || Li_out > store->Li || store->n_seq <= 0 || (Li_out > 0 && store->img_dim <= 0))
        return abi_fail(CPT_ERR_SHAPE, "cpt_gather_batch: B %d, %d + %d -> %d + %d, img_dim %d, %d sequences", B, store->Lt, store->Li, Lt_out, Li_out,
                        store->img_dim, store->n_seq);
    return abi_check(cpt::gather_batch(store, seq_idx, B, Lt_out, Li_out, input_ids_out, token_type_out, attn_mask_out, mask_pos_out, img_feats_out,
                                       (hipStream_t)stream), "cpt_gather_batch");
}

int cpt_gather_batch_heads(const cpt_resident_store* store, const cpt_resident_heads* heads, const int32_t* seq_idx, const int32_t* row_first, int B, int R,
                           int Lt_out, int Li_out, int64_t* input_ids_out, int64_t* token_type_out, int64_t* attn_mask_out, int64_t* mask_pos_out,
                           float* img_feats_out, int64_t* head_rows_out, int64_t* head_labels_out, int64_t* label_grid_out, int64_t* seq_label_out,
                           void* stream) {
    if (!store || !heads || !seq_idx || !input_ids_out || !token_type_out || !attn_mask_out || (Li_out > 0 && !img_feats_out))
        return abi_fail(CPT_ERR_NULL, "cpt_gather_batch_heads: null argument");
    if (B <= 0 || R < 0 || Lt_out <= 0 || Lt_out > store->Lt || Li_out < 0 || Li_out > store->Li || store->n_seq <= 0 ||
        (Li_out > 0 && store->img_dim <= 0) || heads->n_heads < 0)
        return abi_fail(CPT_ERR_SHAPE, "cpt_gather_batch_heads: B %d, R %d, %d + %d -> %d + %d, img_dim %d, %d sequences, %d head entries", B, R, store->Lt,
                        store->Li, Lt_out, Li_out, store->img_dim, store->n_seq, heads->n_heads);
    if (((head_labels_out && R > 0) || label_grid_out) && !heads->head_label)
        return abi_fail(CPT_ERR_NULL, "cpt_gather_batch_heads: labels asked for of a set without head_label");
    if (seq_label_out && !heads->seq_label)
        return abi_fail(CPT_ERR_NULL, "cpt_gather_batch_heads: sequence labels asked for of a set without seq_label");
    return abi_check(cpt::gather_batch_heads(store, heads, seq_idx, row_first, B, R, Lt_out, Li_out, input_ids_out, token_type_out, attn_mask_out,
                                             mask_pos_out, img_feats_out, head_rows_out, head_labels_out, label_grid_out, seq_label_out,
                                             (hipStream_t)stream), "cpt_gather_batch_heads");
}

}  // extern "C"
