// Few-shot training step of the CPT hot path: forward with saved activations, explicit backward,
// fused AdamW.  Replaces autograd over /root/reference/Oscar/oscar/modeling/modeling_rec.py:137-152 +
// modeling_bert.py:199-279 as driven by Oscar/oscar/fewshot/refcoco_cpt.py:231-249.
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>

#include "kernels.h"

namespace cpt { int abi_fail(int code, const char* fmt, ...); int abi_check(int rc, const char* what); }
using cpt::abi_check;
using cpt::abi_fail;
// the switches of this file (switches.h has the table) are named without their namespace below
using cpt::g_wgrad_tn; using cpt::g_bias_fuse; using cpt::g_wgrad_pair; using cpt::g_fwd_split2; using cpt::g_ln_lean; using cpt::g_qkv_defer;

namespace {

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
inline int up64(int x) { return (x + 63) / 64 * 64; }

struct TrainLayout {
    size_t x_f32, a_f32, layer0, layer_stride;
    size_t o_xin, o_qkv, o_ctx, o_pre1, o_a, o_u, o_h, o_pre2, o_st1, o_st2, o_ast, o_kb1, o_kb2;     // offsets inside a layer block (st1 / st2, round 6: (mean, rstd) per row of the two LayerNorms, read by their backward)
    size_t xout, imgp, imgpre, rows, uh, t2, dlogits, loss;
    size_t dx, dpre, da, dpre_lp, dlp2, dctx, dbig, tA, tB, wT, gimg, dl_lp, dt2, duh, duh_lp, drows, dimg, dimg_lp, dmask, dmask_lp;
    size_t t_ctx, t_xres, t_pre1, t_a, t_af, t_u, t_h, t_pre2, t_st1, t_st2, t_kb1, t_kb2, t_dpre, t_dlpF, t_dlpA, t_dbig, t_da, t_dctx;      // round 6: the pruned last layer's compact [B][.] activations and gradients
    size_t qkvp, qkvp_bytes;      // round 6: partial matrices of the Q|K|V weight gradient's K-split launch, added up by spare workgroups of the NEXT layer's three-problem weight-gradient launch
    size_t lnp[2], lnp_bytes, csp; int csp_rows;      // round 6: partial column sums left for a later launch's column-sum job -- two alternating LayerNorm-backward tables, the FFN-up bias rows of the GELU-gradient GEMM
    size_t sA, sW, sA_bytes, sW_bytes;      // bf16x3: split copies of a GEMM's two fp32 operands ([rows][hi | hi | lo] and [rows][hi | lo | hi])
    size_t total, tA_bytes, tB_bytes;
    int Mp, Bp, Vp, Rp;
};

// Rh: rows the head runs on -- the labelled positions (cpt_batch.n_rows), or one per sequence
TrainLayout train_layout(const cpt_dims& d, int B, int Lt, int Li, int Rh) {
    const size_t es = d.dtype == CPT_BF16 ? 2 : 4;
    const size_t L = (size_t)Lt + Li, M = (size_t)B * L, H = d.hidden, I = d.inter, V = d.vocab, Dp = d.img_dim_pad;
    const size_t R = (size_t)B * Li;
    TrainLayout w;
    w.Mp = up64((int)M); w.Bp = up64(Rh); w.Vp = up64((int)V); w.Rp = up64((int)std::max<size_t>(R, 1));
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t p = o; o += al(bytes); return p; };
    w.x_f32 = take(M * H * 4);
    w.a_f32 = take(M * H * 4);
    {   // one block per layer
        size_t q = 0;
        auto sub = [&](size_t bytes) { size_t p = q; q += al(bytes); return p; };
        w.o_xin = sub(M * H * es); w.o_qkv = sub(M * 3 * H * es); w.o_ctx = sub(M * H * es); w.o_pre1 = sub(M * H * 4);
        w.o_a = sub(M * H * es); w.o_u = sub(M * I * es); w.o_h = sub(M * I * es); w.o_pre2 = sub(M * H * 4);
        w.o_st1 = sub(M * 2 * 4); w.o_st2 = sub(M * 2 * 4);
        w.o_kb1 = sub(M * 64 * 2); w.o_kb2 = sub(M * 64 * 2);      // keep bits of the two hidden dropouts (one 16-bit word per lane of the row pass), read back by the LayerNorm backward
        w.o_ast = sub((size_t)B * d.heads * L * 2 * 4);      // softmax statistics (row max, 1 / row sum) of every (sequence, head, query): the one-pass attention backward reads them
        w.layer_stride = q;
        w.layer0 = take(q * d.layers);
    }
    w.xout = take(M * H * es);
    w.imgp = take(R * Dp * es);
    w.imgpre = take(R * H * 4);
    w.rows = take((size_t)Rh * H * es);
    w.uh = take((size_t)Rh * H * 4);
    w.t2 = take((size_t)Rh * H * es);
    w.dlogits = take((size_t)Rh * V * 4);
    w.loss = take(256);
    // backward temporaries
    w.dx = take(M * H * 4);
    w.dpre = take(M * H * 4);
    w.da = take(M * H * 4);
    w.dpre_lp = take(M * H * es);
    w.dlp2 = take(M * H * es);        // round 3: the attention-side LayerNorm backward's low-precision output when the FFN-side one must outlive it (three-problem weight-gradient launch)
    w.dctx = take(M * H * es);
    w.dbig = take(M * std::max(3 * H, I) * es);
    const size_t cols = std::max<size_t>({(size_t)w.Mp, (size_t)w.Bp, (size_t)w.Rp});
    w.tA_bytes = std::max<size_t>({3 * H, I, V}) * cols * es;
    w.tA = take(w.tA_bytes);
    w.tB_bytes = std::max<size_t>({I, Dp, H}) * cols * es;      // also the scratch of ln_bwd's two-stage column sums
    w.tB = take(w.tB_bytes);
    w.wT = take(std::max<size_t>({3 * H * H, I * H, H * (size_t)w.Vp}) * es);
    w.gimg = take(H * Dp * 4);
    w.dl_lp = take((size_t)Rh * w.Vp * es);
    w.dt2 = take((size_t)Rh * H * 4);
    w.duh = take((size_t)Rh * H * 4);
    w.duh_lp = take((size_t)Rh * H * es);
    w.drows = take((size_t)Rh * H * 4);
    w.dimg = take(R * H * 4);
    w.dimg_lp = take(R * H * es);
    w.dmask = take(M * H * 4);        // dropout: masked gradient of a dense output (the unmasked one feeds the residual path)
    w.dmask_lp = take(M * H * es);
    w.lnp_bytes = (M / 4 + 2) * 3 * H * 4;      // (ln_bwd_part_rows(M) <= M / 4 + 1 rows of [3][H])
    w.lnp[0] = take(w.lnp_bytes); w.lnp[1] = take(w.lnp_bytes);
    w.csp_rows = (int)((M + 31) / 32);
    w.csp = take((size_t)w.csp_rows * I * 4);
    {
        // (gemm_tn splits K at most 256 / tiles ways, at most eight)
        const size_t tiles = (3 * H / 128) * (H % 192 == 0 ? H / 192 : std::max<size_t>(H / 128, 1));
        const size_t smax = (d.dtype == CPT_BF16 && tiles > 0) ? std::min<size_t>(8, 256 / std::max<size_t>(tiles, 1)) : 0;
        w.qkvp_bytes = smax > 1 ? smax * 3 * H * H * 4 : 0;
        w.qkvp = take(w.qkvp_bytes);
    }
    {
        const size_t Bq = (size_t)B;
        w.t_ctx = take(Bq * H * es); w.t_xres = take(Bq * H * 4); w.t_pre1 = take(Bq * H * 4); w.t_a = take(Bq * H * es); w.t_af = take(Bq * H * 4);
        w.t_u = take(Bq * I * es); w.t_h = take(Bq * I * es); w.t_pre2 = take(Bq * H * 4); w.t_st1 = take(Bq * 8); w.t_st2 = take(Bq * 8); w.t_kb1 = take(Bq * 128); w.t_kb2 = take(Bq * 128);
        w.t_dpre = take(Bq * H * 4); w.t_dlpF = take(Bq * H * es); w.t_dlpA = take(Bq * H * es); w.t_dbig = take(Bq * I * es); w.t_da = take(Bq * H * 4);
        w.t_dctx = take(Bq * H * es);
    }
    w.sA = w.sW = 0; w.sA_bytes = w.sW_bytes = 0;
    if (d.dtype == CPT_BF16X3_MASTERS) {
        // A operands: activations [M][<= max(3H, I)], transposed gradients [<= max(3H, I)][Mp], the head's [Rh][Vp] / [V][Bp], region rows [R][Dp] / [H][Rp]
        const size_t wide = std::max<size_t>(3 * H, I);
        const size_t a_el = std::max<size_t>({wide * (size_t)w.Mp, (size_t)w.Vp * (size_t)w.Bp, (size_t)w.Rp * Dp, H * (size_t)w.Rp});
        // W operands: weights [<= max(3H, I, V)][<= max(H, I)] and their transposes, transposed activations [<= max(I, Dp, H)][cols]
        const size_t w_el = std::max<size_t>({3 * H * H, I * H, H * (size_t)w.Vp, H * Dp, std::max<size_t>({I, Dp, H}) * cols});
        w.sA_bytes = 6 * a_el; w.sW_bytes = 6 * w_el;
        w.sA = take(w.sA_bytes); w.sW = take(w.sW_bytes);
    }
    w.total = o;
    return w;
}

// dgrad(..., gelu_u): the shape has no fused GELU-gradient epilogue -- the caller runs the unfused pair (dgrad, then gelu_bwd)
constexpr int NOT_FUSED = 1 << 20;

// One error style.  TRY(expr, what): expr is a bare status (a launcher's, gm's); a failure, or a launch error behind it, is reported under `what`.
// PASS(expr): the status is handed on as it is -- a helper that has reported already, or a bare one inside a helper whose caller reports it with TRY.
#define TRY(expr, what) do { if (int rc__ = abi_check((expr), what)) return rc__; } while (0)
#define PASS(expr) do { if (int rc__ = (expr)) return rc__; } while (0)

// bf16x3 training: ONE predicate decides whether a step's attention runs on the mode's split-operand MFMA kernels -- forward AND backward
// (the forward used to pick by a macro and the backward on its own, and the shape gate asked the fp32 kernel either way).
bool x3_attention_at(bool x3, int L, bool m3d) { return x3 && !m3d && cpt::attention_x3_supported(L) && cpt::attention_bwd_x3_supported(L, m3d); }

// Everything a training step decides from (model, batch, dropout, switches), each predicate written once.  cpt_train_fwd and cpt_train_bwd make the same
// plan from the same arguments: the backward reads the buffers the forward wrote under the same answers, which is why a switch must not change
// between the two calls (include/cpt_hip_debug.h -- the ablation build reads the live switches here, at call time; nothing is stamped into the workspace).
struct TrainPlan {
    int B, Lt, Li, L, M, H, I, V, Dp;      // sequences, text / region / total positions, rows B * L, hidden, intermediate, vocabulary, padded region feature size
    int R, Rh;           // region rows B * Li; head rows: the labelled positions of a label grid (cpt_batch.n_rows; forward and backward reject one on the NSP head), else one per sequence
    int Mp, Bp, Vp, Rp;  // M, Rh, V, max(R, 1) rounded up to a 64-row K-tile (TrainLayout)
    int dt;              // element type of activations and library GEMMs: dims.dtype, fp32 under bf16x3
    bool x3;             // CPT_BF16X3_MASTERS: fp32 everywhere, the GEMMs on bf16 split copies of their operands (TrainCtx::gm)
    bool nsp, rel2;      // NSP head (pooler + seq_relationship) instead of the MLM head; rel2: with the second relation head of VCR Q->AR
    bool ph, pa;         // hidden / attention dropout on
    bool m3d;            // attn_mask is [B][L][L]
    bool x3_attn;        // attention forward and backward on the split-operand kernels
    bool attn_stats;     // the attention forward stores its softmax statistics (o_ast) and the backward reads them and the context rows
    bool bf16_tn;        // bf16 step with the TN / NN / K-split GEMM forms (weight and data gradients without operand transposes)
    bool fwd_parts;      // attn-out / FFN-down leave K-split partial matrices to the row pass behind them (cpt_set_tuning key 22)
    bool lean;           // round 6: with hidden dropout every residual add sits in a row pass, which re-forms the LayerNorm output it adds from the pre-LayerNorm rows the backward keeps anyway
                         // (+ (mean, rstd), gain, shift): the LayerNorm launches then write no fp32 output (11.8 of 53-65 MB per launch at 3840 rows; at few rows the extra loads cost what that buys)
    bool emb_pad;        // the embedding launch carries the region features' pad + cast (bf16, 8-byte aligned img_feats)
    // The pruned last layer: the LAST encoder layer's attention output, FFN and both LayerNorms run on the head's rows only (one per sequence: the
    // [MASK] row, or [CLS] for the NSP head) in the training forward AND backward -- every other row of that layer's output is dead (the loss reads
    // B rows; modeling_rec.py:142-150) and so is its gradient.  bf16 step, no label grid, tile-aligned hidden sizes, 2-D mask, L >= 4, and a shape the
    // fused GELU-gradient GEMM takes on B rows.
    bool tail;
    bool fuse_db;        // bf16: the LayerNorm backward applies the dense output's dropout mask and sums the bias gradient's columns itself (no dropout_rows / colsum launches)
    bool bin_parts;      // the GELU-gradient GEMM leaves the FFN-up bias gradient as partial rows for a later column-sum job (bit 0 of key 18)
    bool qkv_bias;       // the attention backward sums the Q|K|V bias gradient itself (bit 1 of key 18)
    bool pair;           // two weight gradients over the same rows share a launch
    bool triple;         // round 3: FFN down | FFN up | attention output weight gradients in ONE launch where their tiles fit one round (hidden 768: 96 + 96 + 24)
    bool qkv_defer;      // round 6: the Q|K|V weight gradient's K-split partial matrices wait for the next layer's triple launch (key 37)
    TrainLayout w;
};

// the plan's terms of (dims, batch shape) alone -- shapes, element type, layout: all the workspace-size functions need; the mode bits are not set
TrainPlan plan_shapes(const cpt_dims& d, int B, int Lt, int Li, int n_rows) {
    TrainPlan p = {};
    p.B = B; p.Lt = Lt; p.Li = Li; p.L = Lt + Li; p.M = B * p.L; p.H = d.hidden; p.I = d.inter; p.V = d.vocab; p.Dp = d.img_dim_pad;
    p.R = B * Li; p.Rh = n_rows > 0 ? n_rows : B;
    p.w = train_layout(d, B, Lt, Li, p.Rh);
    p.Mp = p.w.Mp; p.Bp = p.w.Bp; p.Vp = p.w.Vp; p.Rp = p.w.Rp;
    p.x3 = d.dtype == CPT_BF16X3_MASTERS;
    p.dt = p.x3 ? CPT_F32 : d.dtype;
    return p;
}
TrainPlan make_train_plan(const cpt_model* m, const cpt_rel2* x, const cpt_batch* b, const cpt_dropout* drop) {
    const cpt_dims& d = m->dims;
    TrainPlan p = plan_shapes(d, b->B, b->Lt, b->Li, b->n_rows);
    const bool bf16 = p.dt == CPT_BF16;
    p.nsp = !m->w_tr && !m->w_dec; p.rel2 = x != nullptr;
    p.ph = drop && drop->p_hidden > 0.f; p.pa = drop && drop->p_attn > 0.f;
    p.m3d = b->mask_3d && b->attn_mask;
    p.x3_attn = x3_attention_at(p.x3, p.L, p.m3d);
    p.attn_stats = bf16 && !p.m3d;
    p.bf16_tn = g_wgrad_tn && bf16;
    p.fwd_parts = g_fwd_split2 && p.bf16_tn;
    p.lean = p.ph && g_ln_lean && p.M >= 2048;
    p.emb_pad = p.Li > 0 && bf16 && p.Dp % 8 == 0 && !((uintptr_t)b->img_feats & 7);
    p.tail = p.bf16_tn && b->n_rows == 0 && d.layers >= 1 && p.H % 192 == 0 && p.I % 192 == 0 && p.L >= 4 && !p.m3d && cpt::gemm_nn_eligible(p.B, p.I, p.H, p.H, p.I);
    p.fuse_db = bf16;
    p.bin_parts = (g_bias_fuse & 1) != 0; p.qkv_bias = (g_bias_fuse & 2) != 0;
    p.pair = p.bf16_tn && g_wgrad_pair;
    p.triple = p.bf16_tn && g_wgrad_pair >= 2 && cpt::gemm_tn_triple_eligible(p.H, p.I, p.I, p.H, p.H, p.H, p.Mp);
    p.qkv_defer = g_qkv_defer && p.triple;
    return p;
}

int check_common(const cpt_model* m, const cpt_batch* b, void* ws, size_t ws_bytes, const TrainPlan& p, const char* who) {
    const cpt_dims& d = m->dims;
    if (b->B <= 0 || b->Lt <= 0 || b->Li < 0) return abi_fail(CPT_ERR_SHAPE, "%s: bad batch shape", who);
    if (b->n_rows < 0 || (long)b->n_rows > (long)b->B * (b->Lt + b->Li) || (b->n_rows > 0 && !b->row_seq))
        return abi_fail(CPT_ERR_SHAPE, "%s: n_rows %d needs row_seq and at most B * L = %ld rows", who, b->n_rows, (long)b->B * (b->Lt + b->Li));
    if (d.heads <= 0 || d.hidden != d.heads * 64) return abi_fail(CPT_ERR_SHAPE, "%s: head_dim must be 64", who);
    if (d.dtype == CPT_BF16X3)
        return abi_fail(CPT_ERR_DTYPE, "%s: CPT_BF16X3 describes the standing split weight copies cpt_model_fwd reads; the training step takes the fp32 "
                        "master weights under CPT_BF16X3_MASTERS (ABI 6)", who);
    if (d.dtype != CPT_F32 && d.dtype != CPT_BF16 && d.dtype != CPT_BF16X3_MASTERS) return abi_fail(CPT_ERR_DTYPE, "%s: dtype %d", who, d.dtype);
    if (d.img_dim_pad < d.img_dim || d.img_dim_pad % 64) return abi_fail(CPT_ERR_ALIGN, "%s: img_dim_pad must be a multiple of 64 for training", who);
    if (d.hidden % 64 || d.inter % 64) return abi_fail(CPT_ERR_ALIGN, "%s: hidden/intermediate sizes must be multiples of 64", who);
    const bool nsp_ok = p.nsp && m->w_pool && m->w_rel && d.n_rel > 0;      // the plan's NSP head, complete (past these checks: the same answer as p.nsp)
    if (!b->labels || (!nsp_ok && !b->mask_pos)) return abi_fail(CPT_ERR_NULL, "%s: labels (and, for the MLM head, mask_pos) are required", who);
    if (b->Li > 0 && !b->img_feats) return abi_fail(CPT_ERR_NULL, "%s: img_feats is NULL", who);
    if (!nsp_ok && (!m->w_tr || !m->w_dec)) return abi_fail(CPT_ERR_NULL, "%s: model has neither the MLM head nor the NSP head (pooler + seq_relationship)", who);
    if (nsp_ok && d.n_rel > 64) return abi_fail(CPT_ERR_SHAPE, "%s: n_rel %d > 64", who, d.n_rel);
    if (ws_bytes < p.w.total) return abi_fail(CPT_ERR_WORKSPACE, "%s: workspace %zu < required %zu bytes", who, ws_bytes, p.w.total);
    if ((uintptr_t)ws & 255) return abi_fail(CPT_ERR_ALIGN, "%s: workspace must be 256-byte aligned", who);
    return CPT_OK;
}

// Dropout sites of the model (counter word 3 of the Philox stream, dropout.h): 0 = embeddings (text and region rows,
// after their LayerNorms); layer l: 1 + 3l attention probabilities, 2 + 3l BertSelfOutput, 3 + 3l BertOutput.
cpt::DropSpec drop_spec(const cpt_dropout* d, int site, bool attn) {
    cpt::DropSpec s = {};
    if (!d) return s;
    const double p = attn ? d->p_attn : d->p_hidden;
    if (!(p > 0.0)) return s;
    s.k0 = (uint32_t)d->seed; s.k1 = (uint32_t)(d->seed >> 32);
    s.step = (uint32_t)d->step; s.site = (uint32_t)site;
    const double full = attn ? 65536.0 : 4294967296.0;
    double t = p * full;
    if (t < 1.0) t = 1.0;
    if (t > full - 1.0) t = full - 1.0;
    s.thresh = (uint32_t)(t + 0.5);
    s.scale = (float)(1.0 / (1.0 - (double)s.thresh / full));      // exact effective rate: E[mask * scale] = 1
    return s;
}
int check_drop(const cpt_dropout* d, const char* who) {
    if (!d) return CPT_OK;
    if (!(d->p_hidden >= 0.f && d->p_hidden < 1.f) || !(d->p_attn >= 0.f && d->p_attn < 1.f))
        return abi_fail(CPT_ERR_SHAPE, "%s: dropout probabilities must be in [0, 1)", who);
    return CPT_OK;
}

// VCR Q->AR second head: B0, n_rel, head 1's weights and the label range ([-1, n_rel): from the host copy when given, else read back once)
int check_rel2(const cpt_model* m, const cpt_rel2* x, const cpt_batch* b, const char* who, void* stream, bool labels_too = true) {
    const int n_rel = m->dims.n_rel;
    if (!x->w_rel1 || !x->b_rel1 || !m->w_rel || !m->b_rel) return abi_fail(CPT_ERR_NULL, "%s: both relation heads (w_rel / b_rel, w_rel1 / b_rel1) are required", who);
    if (n_rel < 1 || n_rel > 64) return abi_fail(CPT_ERR_SHAPE, "%s: n_rel %d outside [1, 64]", who, n_rel);
    if (x->score && n_rel < 2) return abi_fail(CPT_ERR_SHAPE, "%s: the choice score needs n_rel >= 2", who);
    if (x->B0 < 0 || x->B0 > b->B) return abi_fail(CPT_ERR_SHAPE, "%s: B0 %d outside [0, B = %d]", who, x->B0, b->B);
    if (b->n_rows != 0) return abi_fail(CPT_ERR_SHAPE, "%s: label grids (n_rows) belong to the MLM head", who);
    if (!labels_too) return CPT_OK;
    if (!b->labels) return abi_fail(CPT_ERR_NULL, "%s: labels are required", who);
    return cpt::rel2_check_labels(b->labels, x->labels_host, b->B, n_rel, who, (hipStream_t)stream);
}

// queue a column-sum job behind the ones already waiting for a carrier launch; a full queue first goes out on a launch of its own, so no
// partial sum is ever dropped
int col_jobs_push(cpt::ColJobs& q, hipStream_t s, const float* src, int rows, int cols, int row_stride, int seg, float* d0, float* d1 = nullptr,
                  float* d2 = nullptr) {
    if (cpt::col_jobs_add(q, src, rows, cols, row_stride, seg, d0, d1, d2)) return CPT_OK;
    PASS(cpt::col_jobs_flush(q, s));
    q = cpt::ColJobs{};
    return cpt::col_jobs_add(q, src, rows, cols, row_stride, seg, d0, d1, d2) ? CPT_OK : CPT_ERR_SHAPE;
}

// What the stages of a step share: the plan (as base: its terms read as plain names below), the call's arguments and the GEMM helpers.
struct TrainCtx : TrainPlan {
    const cpt_model* m; const cpt_batch* b; cpt_dims d; unsigned char* ws; hipStream_t s; const cpt_dropout* drop;
    cpt_bucket_fn bucket_fn; void* user;

    void* at(size_t off) const { return ws + off; }
    float* f32(size_t off) const { return (float*)(ws + off); }
    void* LB(int l, size_t off) const { return ws + w.layer0 + (size_t)l * w.layer_stride + off; }      // offset `off` of layer l's block
    float* LBf(int l, size_t off) const { return (float*)LB(l, off); }
    cpt::DropSpec site(int site, bool attn = false) const { return drop_spec(drop, site, attn); }
    // buckets of data-parallel training (include/cpt_hip.h).  Forward: the host callback runs BEFORE the first launch that reads the bucket's parameters, so the caller can make `stream` wait for
    // its all-gather.  Backward: right AFTER the last launch that writes the bucket's gradients has been enqueued (the tied word-embedding table belongs to bucket 0: its lookup gradient comes last).
    void bucket(int i) const { if (bucket_fn) bucket_fn(user, i); }

    // One Linear-shaped product out[Mr][N] = A[Mr][K] . W[N][K]^T of the training step.  fp32 / bf16: the library GEMM of that type.  bf16x3 (the parity mode at
    // MFMA-bf16 rates, include/cpt_hip.h): both fp32 operands are split on the spot into [hi | hi | lo] / [hi | lo | hi] bf16 copies and the bf16 kernel runs
    // over K' = 3K -- a.w ~ hi.hi + hi.lo + lo.hi with fp32 accumulation; everything outside the GEMMs runs as in fp32 mode.  (The weights change every
    // step, so unlike inference there is no standing split copy of them.)  Returns a bare status.
    int gm(int epi, const void* A, int lda, const void* W, int ldw, const float* bias, const float* resid, int ldr, void* out, int out_dt, int ldo, int Mr, int N,
           int K) const {
        if (!x3) return cpt::gemm(dt, epi, A, lda, W, ldw, bias, resid, ldr, out, out_dt, ldo, Mr, N, K, s);
        if (out_dt != CPT_F32) return CPT_ERR_DTYPE;
        if ((size_t)Mr * K * 6 > w.sA_bytes || (size_t)N * K * 6 > w.sW_bytes) return CPT_ERR_WORKSPACE;
        if (int r3 = cpt::split3((const float*)A, lda, at(w.sA), Mr, K, 0, s)) return r3;
        if (int r3 = cpt::split3((const float*)W, ldw, at(w.sW), N, K, 1, s)) return r3;
        return cpt::gemm(CPT_BF16, epi, at(w.sA), 3 * K, at(w.sW), 3 * K, bias, resid, ldr, out, CPT_F32, ldo, Mr, N, 3 * K, s);
    }
    // out[Nout][Kout] (fp32 gradient of a Linear weight) = dY^T . X over `rows` rows
    int wgrad(const void* dY, int dY_dt, int ldy, int Nout, const void* X, int ldx, int Kout, int rows, int rows_p, float* out, int ldo, const char* what,
              cpt::ReduceJob* defer = nullptr) const {
        // bf16, tile-aligned shapes: the TN form of the GEMM reads dY and X as they are (transpose reads in LDS); tA serves as its split-K partial buffer.  Everything else (fp32 mode,
        // head-sized problems) goes through explicit transposes.  (rows_p = rows rounded up to a K-tile: the missing rows read as zero through the buffer bounds)
        if (bf16_tn && dY_dt == CPT_BF16 && cpt::gemm_tn_eligible(Nout, Kout, rows_p, ldy, ldx, ldo)) {
            // (defer: the partial matrices go to their own buffer -- tA is reused right away -- and are added up by a later launch's spare workgroups)
            if (defer && w.qkvp_bytes) TRY(cpt::gemm_tn(dY, ldy, X, ldx, out, ldo, Nout, Kout, rows_p, at(w.qkvp), w.qkvp_bytes, s, rows, defer), what);
            else TRY(cpt::gemm_tn(dY, ldy, X, ldx, out, ldo, Nout, Kout, rows_p, at(w.tA), w.tA_bytes, s, rows), what);
            return CPT_OK;
        }
        // bf16x3: the same TN kernel over row-stacked split copies of the two fp32 operands (contraction 3 rows_p: hi.hi + hi.lo + lo.hi)
        if (x3 && g_wgrad_tn && dY_dt == CPT_F32 && cpt::gemm_tn_eligible(Nout, Kout, 3 * rows_p, Nout, Kout, ldo) &&
            (size_t)6 * rows_p * Nout <= w.sA_bytes && (size_t)6 * rows_p * Kout <= w.sW_bytes) {
            TRY(cpt::split3_rows((const float*)dY, ldy, at(w.sA), rows, rows_p, Nout, 0, s), what);
            TRY(cpt::split3_rows((const float*)X, ldx, at(w.sW), rows, rows_p, Kout, 1, s), what);
            TRY(cpt::gemm_tn(at(w.sA), Nout, at(w.sW), Kout, out, ldo, Nout, Kout, 3 * rows_p, at(w.tA), w.tA_bytes, s, 3 * rows_p), what);
            return CPT_OK;
        }
        TRY(cpt::transpose_cast(dY, dY_dt, ldy, at(w.tA), dt, rows_p, rows, Nout, s), what);
        TRY(cpt::transpose_cast(X, dt, ldx, at(w.tB), dt, rows_p, rows, Kout, s), what);
        // (split-K with fp32 atomics was measured slower at B=32: 11.7-16.6 ms/step vs 10.4 -- see DESIGN.md)
        TRY(gm(CPT_EPI_NONE, at(w.tA), rows_p, at(w.tB), rows_p, nullptr, nullptr, 0, out, CPT_F32, ldo, Nout, Kout, rows_p), what);
        return CPT_OK;
    }
    // two dense weight gradients out[N][K] = dY[M][N]^T . X[M][K] over all M rows: one launch where the pair kernel takes the shapes (bf16, tile-aligned), else one by one
    struct WG { const void* dY; int N; const void* X; int K; float* out; const char* what; };
    int wgrad_pair(const WG& a, const WG& c, const char* what) const {
        if (pair) {
            const int r = cpt::gemm_tn_pair(a.dY, a.N, a.X, a.K, a.out, a.N, a.K, c.dY, c.N, c.X, c.K, c.out, c.N, c.K, Mp, M, at(w.tA), w.tA_bytes, s);
            if (r != CPT_ERR_SHAPE) return abi_check(r, what);
        }
        PASS(wgrad(a.dY, dt, a.N, a.N, a.X, a.K, a.K, M, Mp, a.out, a.K, a.what));
        return wgrad(c.dY, dt, c.N, c.N, c.X, c.K, c.K, M, Mp, c.out, c.K, c.what);
    }
    // out[rows][Kout] = dY[rows][Nout] . Wt[Nout][Kout]  (+ resid), Wt given as the Linear weight [Nout][Kout]; NOT_FUSED: see above.
    // colsum_rows > 0: gelu_colsum is a table of partial rows (gemm_nn); S_out: a K-split launch leaves its *S_out partial matrices in tA for the
    // LayerNorm backward behind it, which adds them and the residual itself (*S_out = 1: `out` is complete)
    int dgrad(const void* dY, int ldy, int Nout_p, const void* Wt, int ldw, int Nout, int Kout, int rows, const float* resid, void* out, int out_dt, const char* what,
              const void* gelu_u = nullptr, float* gelu_colsum = nullptr, int colsum_rows = 0, int* S_out = nullptr, int split2_bf16 = 0) const {
        if (S_out) *S_out = 1;
        // bf16, tile-aligned: the NN form reads the weight as stored (transpose reads in LDS)
        // (Nout < Nout_p: the K-tile padding columns of dY are zero and the weight rows beyond Nout read as zero)
        if (bf16_tn && cpt::gemm_nn_eligible(rows, Kout, Nout_p, ldy, ldw)) {
            TRY(cpt::gemm_nn(dY, ldy, Wt, ldw, resid, Kout, out, out_dt, Kout, rows, Kout, Nout_p, s, Nout, at(w.tA), w.tA_bytes, gelu_u, Kout, gelu_colsum, colsum_rows, S_out, split2_bf16), what);
            return CPT_OK;
        }
        if (gelu_u) return NOT_FUSED;
        // bf16x3: the same NN kernel on split operands -- dY as [rows][hi | hi | lo], the weight AS STORED split into three row blocks
        // (hi; lo; hi): contraction 3 Nout_p, no transposed weight copy
        if (x3 && g_wgrad_tn && out_dt == CPT_F32 && Nout_p % 4 == 0 && cpt::gemm_nn_eligible(rows, Kout, 3 * Nout_p, 3 * Nout_p, Kout) &&
            (size_t)6 * rows * Nout_p <= w.sA_bytes && (size_t)6 * Nout_p * Kout <= w.sW_bytes) {
            TRY(cpt::split3((const float*)dY, ldy, at(w.sA), rows, Nout_p, 0, s), what);
            TRY(cpt::split3_rows((const float*)Wt, ldw, at(w.sW), Nout, Nout_p, Kout, 1, s), what);
            TRY(cpt::gemm_nn(at(w.sA), 3 * Nout_p, at(w.sW), Kout, resid, Kout, out, CPT_F32, Kout, rows, Kout, 3 * Nout_p, s, 3 * Nout_p, at(w.tA), w.tA_bytes, nullptr, 0, nullptr), what);
            return CPT_OK;
        }
        TRY(cpt::transpose_cast(Wt, dt, ldw, at(w.wT), dt, Nout_p, Nout, Kout, s), what);
        TRY(gm(resid ? CPT_EPI_RESID : CPT_EPI_NONE, dY, ldy, at(w.wT), Nout_p, nullptr, resid, Kout, out, out_dt, Kout, rows, Kout, Nout_p), what);
        return CPT_OK;
    }
};

void set_ctx(TrainCtx& c, const TrainPlan& p, const cpt_model* m, const cpt_batch* b, void* workspace, void* stream, const cpt_dropout* drop, cpt_bucket_fn fn, void* user) {
    static_cast<TrainPlan&>(c) = p;
    c.m = m; c.b = b; c.d = m->dims; c.ws = (unsigned char*)workspace; c.s = (hipStream_t)stream; c.drop = drop; c.bucket_fn = fn; c.user = user;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------------
// One dense + (dropout) + residual + LayerNorm side of a layer: the attention output (BertSelfOutput) or the FFN down projection (BertOutput)
struct DenseLnNames { const char *gemm_parts, *ln_parts, *gemm, *ln_drop, *ln_plain; };      // what the launches of a side are called in error reports
struct DenseLn {
    const struct DenseLnNames* what;
    const void *A, *W; const float* bias; int K;
    const float *ln_g, *ln_b;
    const float *res, *res_st, *res_g, *res_b;      // residual rows; lean: the pre-LayerNorm rows of the LayerNorm in front with its (mean, rstd), gain and shift
    size_t pre, st, kb;      // layer-block offsets of the stored pre-LayerNorm sum, the row statistics and the dropout keep bits
    int site;                // dropout site (drop_spec)
    float* out_f32; void* out_lp;
};
const DenseLnNames WHAT_AO = {"gemm(attn out, K split)", "partials+dropout(attn out)+residual+layernorm", "gemm(attn out)", "dropout(attn out)+residual+layernorm", "layernorm(attn)"};
const DenseLnNames WHAT_FD = {"gemm(ffn down, K split)", "partials+dropout(ffn down)+residual+layernorm", "gemm(ffn down)", "dropout(ffn down)+residual+layernorm", "layernorm(ffn)"};

struct TrainFwd : TrainCtx {
    const cpt_rel2* x;      // the second relation head of VCR Q->AR (cpt_train_fwd_rel2), NULL for every other model
    const cpt_outputs* o;
    const float* tmpl; int n_slots;      // soft template (cpt_train_fwd_soft): text ids in (0, n_slots) read their word row from it; NULL for every other call
    unsigned* ce_ticket() const { return (unsigned*)at(w.loss + 16); }      // finish ticket of the cross-entropy launch at the end of the forward
    // the rows' {loss, 1} pairs of that launch, added up in row order by its last workgroup (2 Rh floats): dt2, [Rh][H] fp32, is a temporary of the
    // backward's head and idle during the forward.  The loss is then a function of the inputs alone: two runs, the same bits
    float* ce_row_loss() const { return f32(w.dt2); }

    int embed() const {
        bucket(0);
        // (round 6: the embedding launch also clears the loss accumulator and the finish ticket of the cross-entropy launch at the end of this forward -- no memset launch; with regions
        // in bf16 it carries the region features' pad + cast as well.  BertEmbeddings' dropout on the text rows and modeling_bert.py:266 on the region rows are applied by the launches
        // that write those rows -- the same site mask at the same element indices as the dropout pass over all rows they replace)
        float* x_f32 = f32(w.x_f32);
        const cpt::DropSpec edrop = site(0);
        if (emb_pad)
            TRY(cpt::embed_ln_pad_cast(b->input_ids, b->token_type, b->position_ids, m->word_emb, m->pos_emb, m->type_emb, m->emb_ln_g, m->emb_ln_b, d.ln_eps,
                                       LB(0, w.o_xin), nullptr, B, Lt, L, H, d.vocab, d.max_pos, d.type_vocab, b->img_feats, at(w.imgp), B * Li, d.img_dim, d.img_dim_pad, s, 0,
                                       x_f32, o->loss, ce_ticket(), ph ? &edrop : nullptr, tmpl, n_slots), "embed_ln + dropout + pad_cast(img_feats)");
        else
            TRY(cpt::embed_ln(b->input_ids, b->token_type, b->position_ids, m->word_emb, m->pos_emb, m->type_emb, m->emb_ln_g, m->emb_ln_b, d.ln_eps, x_f32,
                              LB(0, w.o_xin), dt, B, Lt, L, H, d.vocab, d.max_pos, d.type_vocab, s, nullptr, 0, o->loss, ce_ticket(), ph ? &edrop : nullptr, tmpl, n_slots), "embed_ln + dropout");
        if (Li <= 0) return CPT_OK;
        if (!emb_pad) TRY(cpt::pad_cast(b->img_feats, at(w.imgp), dt, B * Li, d.img_dim, d.img_dim_pad, s), "pad_cast(img_feats)");
        TRY(gm(CPT_EPI_NONE, at(w.imgp), d.img_dim_pad, m->w_img, d.img_dim_pad, m->b_img, nullptr, 0, f32(w.imgpre), CPT_F32, H, B * Li, H, d.img_dim_pad), "gemm(img_embedding)");
        const bool iln = d.use_img_ln && m->img_ln_g;       // use_img_layernorm = 0 (modeling_bert.py:263): the projection is used as is
        cpt::LnRowsExtra e;
        e.out_drop = ph ? &edrop : nullptr;
        TRY(cpt::layernorm_rows_ex(f32(w.imgpre), iln ? m->img_ln_g : nullptr, iln ? m->img_ln_b : nullptr, d.img_ln_eps, x_f32, LB(0, w.o_xin), dt, B * Li, H, Li, L, Lt, 0, s, &e),
            "layernorm(img) + dropout");
        return CPT_OK;
    }

    // Q|K|V projection and attention of layer l (all rows, also in front of the pruned last layer)
    int attention(int l) const {
        const cpt_layer& y = m->layers[l];
        bucket(1 + l);
        TRY(gm(CPT_EPI_NONE, LB(l, w.o_xin), H, y.w_qkv, H, y.b_qkv, nullptr, 0, LB(l, w.o_qkv), dt, 3 * H, M, 3 * H, H), "gemm(qkv)");
        const cpt::DropSpec da_spec = site(1 + 3 * l, true);
        if (x3_attn)      // bf16x3: the mode's split-operand MFMA attention (fp32 ctx out), same dropout stream
            TRY(cpt::attention_x3(LBf(l, w.o_qkv), b->attn_mask, LBf(l, w.o_ctx), nullptr, B, L, d.heads, s, pa ? &da_spec : nullptr), "attention (split operands)");
        else
            TRY(cpt::attention(dt, LB(l, w.o_qkv), b->attn_mask, LB(l, w.o_ctx), nullptr, B, L, d.heads, s, pa ? &da_spec : nullptr, m3d, 0,
                               attn_stats ? LBf(l, w.o_ast) : nullptr), "attention");
        return CPT_OK;
    }

    // The K-split / dropout / plain branch of a dense layer with fp32 output and the LayerNorm behind it, once for both sides.
    int dense_ln(int l, const DenseLn& q) const {
        float* pre = LBf(l, q.pre);
        const cpt::DropSpec sp = site(q.site);
        cpt::LnRowsExtra e;
        e.stat_out = LBf(l, q.st);
        // round 3: where the dense layer's K is split over workgroups (few rows; or 2048..6144 rows with a long K), its partial matrices go straight to the
        // row pass behind it, which adds them in split order -- no reduction launch in between (key 22).  (FFN-down at M = 3840: two 128 x 192 half-K
        // workgroups per tile, 240 workgroups at twice the arithmetic intensity of the 64 x 192 tiles; at 480 rows eight K slices per 64 x 192 tile)
        int S = 0;
        const int rp = fwd_parts ? cpt::gemm_nt_partials(q.A, q.K, q.W, q.K, q.bias, f32(w.tA), w.tA_bytes, M, H, q.K, s, &S) : CPT_ERR_SHAPE;
        const bool parts = rp != CPT_ERR_SHAPE;
        if (parts) {
            TRY(rp, q.what->gemm_parts);
            e.x_parts = S; e.x_stride = (size_t)M * H;
        } else {
            // (gemm_nt_split: K split over workgroups at small row counts)  Without dropout the residual add sits in the GEMM epilogue; with it, in the row pass
            const float* resid = ph ? nullptr : q.res;
            int rs = bf16_tn ? cpt::gemm_nt_split(q.A, q.K, q.W, q.K, q.bias, resid, H, pre, H, M, H, q.K, at(w.tA), w.tA_bytes, s) : CPT_ERR_SHAPE;
            if (rs == CPT_ERR_SHAPE) rs = gm(resid ? CPT_EPI_RESID : CPT_EPI_NONE, q.A, q.K, q.W, q.K, q.bias, resid, H, pre, CPT_F32, H, M, H, q.K);
            TRY(rs, q.what->gemm);
        }
        if (parts || ph) {      // dropout + residual + LayerNorm in one row pass (pre = dropout(dense) + residual is stored for the backward pass)
            e.resid = q.res; e.drop = ph ? &sp : nullptr; e.pre_out = pre; e.keep_out = (unsigned short*)LB(l, q.kb);
            e.resid_stat = q.res_st; e.resid_g = q.res_g; e.resid_b = q.res_b;
        }
        TRY(cpt::layernorm_rows_ex(parts ? f32(w.tA) : pre, q.ln_g, q.ln_b, d.ln_eps, q.out_f32, q.out_lp, dt, M, H, M, 0, 0, 0, s, &e), parts ? q.what->ln_parts : ph ? q.what->ln_drop : q.what->ln_plain);
        return CPT_OK;
    }

    int layer(int l) const {
        const cpt_layer& y = m->layers[l];
        PASS(attention(l));
        float* x_f32 = f32(w.x_f32); float* a_f32 = f32(w.a_f32);
        DenseLn ao = {}, fd = {};
        ao.what = &WHAT_AO; ao.A = LB(l, w.o_ctx); ao.W = y.w_ao; ao.bias = y.b_ao; ao.K = H; ao.ln_g = y.ln1_g; ao.ln_b = y.ln1_b;
        ao.pre = w.o_pre1; ao.st = w.o_st1; ao.kb = w.o_kb1; ao.site = 2 + 3 * l; ao.out_f32 = lean ? nullptr : a_f32; ao.out_lp = LB(l, w.o_a);
        ao.res = x_f32;
        if (lean && l > 0) {      // (layer 0 adds the embedding rows: a real buffer)
            ao.res = LBf(l - 1, w.o_pre2); ao.res_st = LBf(l - 1, w.o_st2); ao.res_g = m->layers[l - 1].ln2_g; ao.res_b = m->layers[l - 1].ln2_b;
        }
        PASS(dense_ln(l, ao));
        if (dt == CPT_BF16 && H % 64 == 0 && I % 8 == 0) {
            TRY(cpt::gemm_gelu2(LB(l, w.o_a), H, y.w_in, H, y.b_in, LB(l, w.o_u), LB(l, w.o_h), I, M, I, H, s), "gemm(ffn up)+gelu");
        } else {
            TRY(gm(CPT_EPI_NONE, LB(l, w.o_a), H, y.w_in, H, y.b_in, nullptr, 0, LB(l, w.o_u), dt, I, M, I, H), "gemm(ffn up)");
            TRY(cpt::gelu_fwd(LB(l, w.o_u), LB(l, w.o_h), dt, (size_t)M * I, s), "gelu");
        }
        fd.what = &WHAT_FD; fd.A = LB(l, w.o_h); fd.W = y.w_out; fd.bias = y.b_out; fd.K = I; fd.ln_g = y.ln2_g; fd.ln_b = y.ln2_b;
        fd.pre = w.o_pre2; fd.st = w.o_st2; fd.kb = w.o_kb2; fd.site = 3 + 3 * l; fd.out_lp = l + 1 < d.layers ? LB(l + 1, w.o_xin) : at(w.xout);
        fd.out_f32 = (lean && !(tail && l == d.layers - 2)) ? nullptr : x_f32;      // (x_f32 is still written where the pruned last layer gathers its residual rows from it)
        fd.res = a_f32;
        if (lean) { fd.res = LBf(l, w.o_pre1); fd.res_st = LBf(l, w.o_st1); fd.res_g = y.ln1_g; fd.res_b = y.ln1_b; }
        return dense_ln(l, fd);
    }

    // a dense layer of the pruned last layer: its *S K-split partial matrices (or the one complete matrix) at tA, for the row pass behind it
    int tail_dense(const void* A, int K, const void* W, const float* bias, int* S, const char* what) const {
        int r = cpt::gemm_nt_partials(A, K, W, K, bias, f32(w.tA), w.tA_bytes, B, H, K, s, S);
        if (r == CPT_ERR_SHAPE) { *S = 1; r = gm(CPT_EPI_NONE, A, K, W, K, bias, nullptr, 0, f32(w.tA), CPT_F32, H, B, H, K); }
        return abi_check(r, what);
    }
    // round 6: the rest of the last layer on the B head rows (row b = position pos[b] of sequence b)
    int layer_tail(int l) const {
        const cpt_layer& y = m->layers[l];
        PASS(attention(l));
        const cpt::RowMap rm = {nsp ? nullptr : b->mask_pos, L, 1};
        void* ctx_r = at(w.t_ctx); float* xres_r = f32(w.t_xres); void* a_r = at(w.t_a); float* af_r = f32(w.t_af);
        TRY(cpt::tail_gather2(LB(l, w.o_ctx), f32(w.x_f32), rm.pos, ctx_r, xres_r, B, L, H, s), "gather(head rows of ctx, residual)");
        const cpt::DropSpec sp1 = site(2 + 3 * l), sp2 = site(3 + 3 * l);
        float* part = f32(w.tA);
        cpt::LnRowsExtra e;
        e.x_stride = (size_t)B * H; e.drop_rows = &rm;
        PASS(tail_dense(ctx_r, H, y.w_ao, y.b_ao, &e.x_parts, "gemm(attn out, head rows)"));
        e.resid = xres_r; e.drop = ph ? &sp1 : nullptr; e.pre_out = f32(w.t_pre1); e.stat_out = f32(w.t_st1); e.keep_out = (unsigned short*)at(w.t_kb1);
        TRY(cpt::layernorm_rows_ex(part, y.ln1_g, y.ln1_b, d.ln_eps, af_r, a_r, dt, B, H, B, 0, 0, 0, s, &e), "dropout(attn out)+residual+layernorm (head rows)");
        TRY(cpt::gemm_gelu2(a_r, H, y.w_in, H, y.b_in, at(w.t_u), at(w.t_h), I, B, I, H, s), "gemm(ffn up)+gelu (head rows)");
        PASS(tail_dense(at(w.t_h), I, y.w_out, y.b_out, &e.x_parts, "gemm(ffn down, head rows)"));
        // ... whose LayerNorm output IS the head's input (no gather of [MASK] / [CLS] rows in the head stages)
        e.resid = af_r; e.drop = ph ? &sp2 : nullptr; e.pre_out = f32(w.t_pre2); e.stat_out = f32(w.t_st2); e.keep_out = (unsigned short*)at(w.t_kb2);
        TRY(cpt::layernorm_rows_ex(part, y.ln2_g, y.ln2_b, d.ln_eps, nullptr, at(w.rows), dt, B, H, B, 0, 0, 0, s, &e), "dropout(ffn down)+residual+layernorm (head rows)");
        return CPT_OK;
    }

    // NSPCPT: pooled = tanh([CLS] W_pool^T + b_pool) (kept in `uh`), rel = pooled W_rel^T + b_rel, CE over n_rel classes
    int head_nsp() const {
        float* uh = f32(w.uh);
        float* dlg = f32(w.dlogits);
        bucket(d.layers + 1);
        if (!tail) TRY(cpt::gather_rows(at(w.xout), dt, nullptr, at(w.rows), B, L, H, s), "gather([CLS])");
        TRY(gm(CPT_EPI_TANH, at(w.rows), H, m->w_pool, H, m->b_pool, nullptr, 0, uh, CPT_F32, H, B, H, H), "gemm(pooler)");
        if (rel2) {
            // VCR Q->AR: both heads and the grouped cross entropy in one launch on the fp32 pooled rows (row losses behind the B x n_rel
            // dlogits block of the workspace; the embedding launch cleared the finish ticket)
            TRY(cpt::rel2_fwd(dt == CPT_BF16, uh, B, H, d.n_rel, x->B0, m->w_rel, m->b_rel, x->w_rel1, x->b_rel1, b->labels, o->rel, x->score, dlg,
                              dlg + (size_t)B * d.n_rel, ce_ticket(), o->loss, o->loss_mean, s), "rel2_fwd(two heads + grouped cross entropy)");
            return CPT_OK;
        }
        const void* pin = uh;
        if (dt == CPT_BF16) {
            TRY(cpt::layernorm_rows(uh, nullptr, nullptr, 0.f, nullptr, at(w.t2), dt, B, H, B, 0, 0, s), "cast(pooled)");
            pin = at(w.t2);
        }
        TRY(gm(CPT_EPI_NONE, pin, H, m->w_rel, H, m->b_rel, nullptr, 0, o->rel, CPT_F32, d.n_rel, B, d.n_rel, H), "gemm(seq_relationship)");
        TRY(cpt::ce_rows(o->rel, b->labels, o->loss, dlg, B, d.n_rel, s, ce_ticket(), o->loss_mean, f32(w.loss), ce_row_loss()), "ce_rows(rel)");
        return CPT_OK;
    }

    // MLM head on the Rh head rows: the [MASK] position of every sequence, or the n_rows labelled positions of a label grid (row_seq, mask_pos)
    int head_mlm() const {
        void* t2 = at(w.t2);
        bucket(d.layers + 1);
        if (!tail) TRY(cpt::gather_rows(at(w.xout), dt, b->mask_pos, at(w.rows), Rh, L, H, s, b->n_rows > 0 ? b->row_seq : nullptr, B), "gather([MASK])");
        TRY(gm(CPT_EPI_NONE, at(w.rows), H, m->w_tr, H, m->b_tr, nullptr, 0, f32(w.uh), CPT_F32, H, Rh, H, H), "gemm(head transform)");
        TRY(cpt::layernorm_rows_ex(f32(w.uh), m->tr_ln_g, m->tr_ln_b, d.ln_eps, dt == CPT_F32 ? (float*)t2 : nullptr, dt == CPT_F32 ? nullptr : t2, dt, Rh, H, Rh, 0, 0, 1, s),
            "gelu+layernorm(head)");
        TRY(gm(CPT_EPI_NONE, t2, H, m->w_dec, H, m->b_dec, nullptr, 0, o->logits, CPT_F32, d.vocab, Rh, d.vocab, H), "gemm(decoder)");
        // (the launch's last workgroup leaves {sum, count} in the workspace for the backward and the mean in o->loss_mean: no memset, copy or divide launch)
        TRY(cpt::ce_rows(o->logits, b->labels, o->loss, f32(w.dlogits), Rh, d.vocab, s, ce_ticket(), o->loss_mean, f32(w.loss), ce_row_loss()), "ce_rows");
        return CPT_OK;
    }
};

int check_soft(const cpt_model* m, const cpt_soft_template* st, bool need_grad, const char* who) {
    if (!st || !st->tmpl) return abi_fail(CPT_ERR_NULL, "%s: the soft template (tmpl) is NULL", who);
    if (need_grad && !st->g_tmpl) return abi_fail(CPT_ERR_NULL, "%s: g_tmpl is NULL", who);
    if (st->n_slots < 2 || st->n_slots > m->dims.vocab) return abi_fail(CPT_ERR_SHAPE, "%s: n_slots %d outside [2, vocabulary %d]", who, st->n_slots, m->dims.vocab);
    if (((uintptr_t)st->tmpl & 15) || (need_grad && ((uintptr_t)st->g_tmpl & 15))) return abi_fail(CPT_ERR_ALIGN, "%s: the template tensors must be 16-byte aligned", who);
    if (!m->w_tr || !m->w_dec)
        return abi_fail(CPT_ERR_SHAPE, "%s: soft-template tuning runs on the MLM head; the NSP-CPT heads (pooler + relation heads) are not supported", who);
    return CPT_OK;
}

int train_fwd_impl(const cpt_model* m, const cpt_rel2* x, const cpt_batch* b, const cpt_outputs* o, void* workspace, size_t workspace_bytes, void* stream,
                   cpt_bucket_fn before_bucket, void* user, const cpt_dropout* drop, const cpt_soft_template* soft = nullptr) {
    if (!m || !b || !o || !workspace) return abi_fail(CPT_ERR_NULL, "cpt_train_fwd: null argument");
    PASS(check_drop(drop, "cpt_train_fwd"));
    const TrainPlan p = make_train_plan(m, x, b, drop);
    PASS(check_common(m, b, workspace, workspace_bytes, p, "cpt_train_fwd"));
    if (p.nsp && b->n_rows > 0) return abi_fail(CPT_ERR_SHAPE, "cpt_train_fwd: label grids (n_rows) belong to the MLM head, not the NSP head");
    if (!o->loss || (p.nsp ? !o->rel : !o->logits)) return abi_fail(CPT_ERR_NULL, "cpt_train_fwd: loss and logits (NSP head: rel) outputs are required");
    if (x) {
        PASS(check_rel2(m, x, b, "cpt_train_fwd_rel2", stream));
        if (!p.nsp) return abi_fail(CPT_ERR_NULL, "cpt_train_fwd_rel2: the model needs the pooler and head 0 (w_pool, w_rel) and no MLM head");
    }
    if (p.L > 288) return abi_fail(CPT_ERR_SHAPE, "cpt_train_fwd: sequence length %d > 288", p.L);
    if (!p.x3_attn && !cpt::attention_bwd_supported(p.dt, p.L, p.pa, p.m3d)) {      // reject here, not after the forward has run (the backward's attention kernel sets the limit)
        int lmax = p.L;
        while (lmax > 0 && !x3_attention_at(p.x3, lmax, p.m3d) && !cpt::attention_bwd_supported(p.dt, lmax, p.pa, p.m3d)) --lmax;
        return abi_fail(CPT_ERR_SHAPE, "cpt_train_fwd: no attention backward for dtype %d at sequence length %d%s (longest supported: %d)", p.dt, p.L,
                        p.pa ? " with attention dropout" : "", lmax);
    }
    TrainFwd f = {};
    set_ctx(f, p, m, b, workspace, stream, drop, before_bucket, user);
    f.x = x; f.o = o;
    if (soft) { f.tmpl = soft->tmpl; f.n_slots = soft->n_slots; }
    PASS(f.embed());
    for (int l = 0; l < m->dims.layers; ++l) PASS(p.tail && l == m->dims.layers - 1 ? f.layer_tail(l) : f.layer(l));
    return p.nsp ? f.head_nsp() : f.head_mlm();
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------------
struct BwdState {      // what one layer's backward leaves for the next launches
    cpt::ColJobs pend;             // round 6: column-sum jobs waiting for a carrier launch (kernels.h)
    // round 6: the Q|K|V weight gradient's K-split partial matrices of layer l + 1 wait for the three-problem weight-gradient launch of layer l, whose tiles
    // leave 40 of 256 CUs idle at hidden 768 (cpt_set_tuning key 37); the bucket of layer l + 1 is announced behind that launch
    cpt::ReduceJob qjob;
    int ready_after_triple;
    int lnp_turn;                  // which of the two LayerNorm-backward partial tables the next launch writes
    int dxS, dxB;                  // dxS > 1: the gradient entering the layer lies in tA as that many K-split partial matrices (+ residual dpre); dxB: they are bf16 (two of them, gemm_nn split2_bf16)
};
// One LayerNorm backward of a layer with the dropout mask and bias gradient of the dense output in front of it: FFN side (LN2) or attention side (LN1)
struct LnBwdNames { const char *fused, *col_jobs, *ln_bwd, *dropout, *colsum; };      // what the launches of a side are called in error reports
struct LnBwdSide {
    const struct LnBwdNames* what;
    const float* dy; int S, Sbf16;      // incoming gradient, or S > 1 partial matrices of it in tA (bf16 ones: Sbf16)
    size_t pre, st, kb;           // layer-block offsets (DenseLn)
    const float* g; float *dg, *db, *dbias;
    int site; void* out_lp;       // dropout site; fused form: where the (masked) low-precision gradient goes
};
const LnBwdNames WHAT_LN2 = {"ln_bwd(ffn)+dropout+bias", "column-sum jobs (ffn side)", "ln_bwd(ffn)", "dropout_bwd(ffn down)", "colsum(b_out)"};
const LnBwdNames WHAT_LN1 = {"ln_bwd(attn)+dropout+bias", "column-sum jobs (attention side)", "ln_bwd(attn)", "dropout_bwd(attn out)", "colsum(b_ao)"};

struct TrainBwd : TrainCtx {
    const cpt_rel2* x; const cpt_model_grads* g; float loss_scale; const float* loss_scale_dev;
    // layer freezing (cpt_train_bwd_from): stages < stage are frozen -- 0 = the full walk; stage - 1 is then the boundary layer, the lowest one with
    // a parameter gradient (stage = layers + 1: the head alone).  below: a frozen backward goes on under the boundary (soft template), so the data
    // gradient that leaves the trainable stages is kept; without it nothing reads that gradient and the launch that forms it is left out.
    int stage; bool below;
    bool tied_frozen() const { return stage > 0; }                              // the word table (stage 0) is the decoder's weight: no wgrad(decoder)
    bool head_dx() const { return stage <= d.layers || below; }                 // the head's data gradient into the encoder is read by something
    bool layer_dx(int l) const { return stage == 0 || l > stage - 1 || below; } // ... and so is layer l's into the rows below it
    // with hidden dropout the gradient that enters a dense layer is the masked one (dmask); the unmasked one (dpre) keeps feeding the residual path
    const float* dpre_f() const { return f32(ph ? w.dmask : w.dpre); }
    const void* dpre_in() const { return dt == CPT_BF16 ? at(ph ? w.dmask_lp : w.dpre_lp) : (const void*)dpre_f(); }

    int head_nsp() const {
        if (!g->w_pool || !g->b_pool || !g->w_rel || !g->b_rel) return abi_fail(CPT_ERR_NULL, "cpt_train_bwd: NSP head needs the w_pool / b_pool / w_rel / b_rel gradient tensors");
        const int NR = d.n_rel, NRp = 64;
        const float* pooled = f32(w.uh);
        float* dt2 = f32(w.dt2); float* duh = f32(w.duh);
        if (rel2) {
            // VCR Q->AR: dpooled and both heads' gradients in one launch (fixed-order sums, no float atomics); the pooler chain below is unchanged
            if (!x->g_w_rel1 || !x->g_b_rel1) return abi_fail(CPT_ERR_NULL, "cpt_train_bwd_rel2: head 1 needs the g_w_rel1 / g_b_rel1 gradient tensors");
            TRY(cpt::rel2_bwd(dt == CPT_BF16, pooled, B, H, NR, x->B0, m->w_rel, x->w_rel1, f32(w.dlogits), loss_scale, loss_scale_dev,
                              dt2, g->w_rel, g->b_rel, x->g_w_rel1, x->g_b_rel1, s), "rel2_bwd(two heads)");
        } else {
            const void* pin = dt == CPT_BF16 ? at(w.t2) : (const void*)pooled;
            TRY(cpt::scale_cast(f32(w.dlogits), f32(w.loss), loss_scale, loss_scale_dev, at(w.dl_lp), dt, B, NR, NRp, s, g->b_rel), "scale(drel) + colsum(cls.bias)");
            PASS(dgrad(at(w.dl_lp), NRp, NRp, m->w_rel, H, NR, H, B, nullptr, dt2, CPT_F32, "dgrad(seq_relationship)"));
            PASS(wgrad(at(w.dl_lp), dt, NRp, NR, pin, H, H, B, Bp, g->w_rel, H, "wgrad(seq_relationship)"));
        }
        TRY(cpt::tanh_bwd(dt2, pooled, duh, dt == CPT_BF16 ? at(w.duh_lp) : nullptr, dt, (size_t)B * H, s), "tanh_bwd(pooler)");
        const void* dpo = dt == CPT_BF16 ? at(w.duh_lp) : (const void*)duh;
        TRY(cpt::colsum(duh, CPT_F32, H, g->b_pool, B, H, s), "colsum(pooler bias)");
        PASS(wgrad(dpo, dt, H, H, at(w.rows), H, H, B, Bp, g->w_pool, H, "wgrad(pooler)"));
        if (!head_dx()) return CPT_OK;
        return dgrad(dpo, H, H, m->w_pool, H, H, H, B, nullptr, f32(w.drows), CPT_F32, "dgrad(pooler)");
    }

    int head_mlm() const {
        float* dt2 = f32(w.dt2); float* duh = f32(w.duh);
        TRY(cpt::scale_cast(f32(w.dlogits), f32(w.loss), loss_scale, loss_scale_dev, at(w.dl_lp), dt, Rh, V, Vp, s, g->b_dec), "scale(dlogits) + colsum(cls.bias)");
        PASS(dgrad(at(w.dl_lp), Vp, Vp, m->w_dec, H, V, H, Rh, nullptr, dt2, CPT_F32, "dgrad(decoder)"));
        if (!tied_frozen()) PASS(wgrad(at(w.dl_lp), dt, Vp, V, at(w.t2), H, H, Rh, Bp, g->word_emb, H, "wgrad(decoder)"));
        TRY(cpt::ln_bwd(dt2, f32(w.uh), m->tr_ln_g, d.ln_eps, duh, dt == CPT_BF16 ? at(w.duh_lp) : nullptr, dt, g->tr_ln_g,
                        g->tr_ln_b, Rh, H, Rh, 0, 0, 1, s, nullptr, 0, nullptr, g->b_tr), "ln_bwd(head) + transform bias sums");      // (round 6: the bias gradient = column sums of this launch's output, summed inside it)
        const void* duh_in = dt == CPT_BF16 ? at(w.duh_lp) : (const void*)duh;
        PASS(wgrad(duh_in, dt, H, H, at(w.rows), H, H, Rh, Bp, g->w_tr, H, "wgrad(head transform)"));
        if (!head_dx()) return CPT_OK;
        return dgrad(duh_in, H, H, m->w_tr, H, H, H, Rh, nullptr, f32(w.drows), CPT_F32, "dgrad(head transform)");
    }

    // The fused / unfused branch of a LayerNorm backward, once for both sides.  Fused (bf16): the launch also applies the dense output's dropout mask to the
    // gradient that goes on into the dense layer (written as bf16 only) and leaves its column sums (gain, shift, bias gradient) as partial rows, which
    // spare workgroups of the NEXT LayerNorm backward add up (st.pend), as this one adds the last one's; it reads the forward's row statistics and keep
    // bits, and the incoming gradient possibly as the K-split partial matrices of the data-gradient GEMM in front (+ its residual dpre -- the row this
    // launch overwrites with its own output only after reading it).
    int ln_bwd_side(int l, BwdState& st, const LnBwdSide& q) const {
        float* dpre = f32(w.dpre);
        if (!fuse_db) {
            TRY(cpt::ln_bwd(q.dy, LBf(l, q.pre), q.g, d.ln_eps, dpre, nullptr, dt, q.dg, q.db, M, H, M, 0, 0, 0, s, f32(w.tB), w.tB_bytes), q.what->ln_bwd);
            if (ph) TRY(cpt::dropout_rows(dpre, nullptr, f32(w.dmask), nullptr, dt, M, H, site(q.site), s), q.what->dropout);
            TRY(cpt::colsum(dpre_f(), CPT_F32, H, q.dbias, M, H, s), q.what->colsum);
            return CPT_OK;
        }
        const cpt::DropSpec sp = site(q.site);
        cpt::LnBwdExtra e = {};
        e.stats = LBf(l, q.st); e.jobs = &st.pend; e.defer_reduce = 1; e.keep_bits = (const unsigned short*)LB(l, q.kb);
        if (q.S > 1) { e.dy_parts = q.S; e.dy_stride = (size_t)M * H; e.dy_resid = dpre; e.dy_parts_bf16 = q.Sbf16; }
        float* part = f32(w.lnp[st.lnp_turn]);
        TRY(cpt::ln_bwd(q.S > 1 ? f32(w.tA) : q.dy, LBf(l, q.pre), q.g, d.ln_eps, dpre, q.out_lp, dt, q.dg, q.db, M, H, M, 0, 0, 0, s, part, w.lnp_bytes,
                        ph ? &sp : nullptr, q.dbias, &e), q.what->fused);
        st.pend = cpt::ColJobs{};
        TRY(col_jobs_push(st.pend, s, part, cpt::ln_bwd_part_rows(M), 3 * H, 3 * H, H, q.dg, q.db, q.dbias), q.what->col_jobs);
        st.lnp_turn ^= 1;
        return CPT_OK;
    }

    // Attention backward of layer l, the Q|K|V weight gradient (alone, or with the attention output's in a pair launch) and the data gradient into dx.
    int attention(int l, BwdState& st, bool qkv_alone) const {
        const cpt_layer& y = m->layers[l];
        const cpt_layer_grads& gy = g->layers[l];
        void* dbig = at(w.dbig);
        const cpt::DropSpec da_spec = site(1 + 3 * l, true);
        if (x3_attn)
            TRY(cpt::attention_bwd_x3(LBf(l, w.o_qkv), b->attn_mask, (const float*)at(w.dctx), (float*)dbig, B, L, d.heads, s, pa ? &da_spec : nullptr,
                                      qkv_bias ? gy.b_qkv : nullptr), "attention_bwd (split operands)");
        else
            TRY(cpt::attention_bwd(dt, LB(l, w.o_qkv), b->attn_mask, at(w.dctx), dbig, B, L, d.heads, s, pa ? &da_spec : nullptr, qkv_bias ? gy.b_qkv : nullptr, m3d,
                                   attn_stats ? LB(l, w.o_ctx) : nullptr, attn_stats ? LBf(l, w.o_ast) : nullptr), "attention_bwd+bias");
        if (!qkv_bias) TRY(cpt::colsum(dbig, dt, 3 * H, gy.b_qkv, M, 3 * H, s), "colsum(b_qkv)");
        if (qkv_alone)
            PASS(wgrad(dbig, dt, 3 * H, 3 * H, LB(l, w.o_xin), H, H, M, Mp, gy.w_qkv, H, "wgrad(qkv)", qkv_defer ? &st.qjob : nullptr));
        else
            PASS(wgrad_pair({dpre_in(), H, LB(l, w.o_ctx), H, gy.w_ao, "wgrad(attn out)"}, {dbig, 3 * H, LB(l, w.o_xin), H, gy.w_qkv, "wgrad(qkv)"}, "wgrad(attn out | qkv)"));
        // (layer 0's result feeds the embedding passes: complete; above that a K-split launch leaves its partial matrices to the next LayerNorm backward)
        st.dxS = 1; st.dxB = 0;
        if (layer_dx(l)) {      // (the boundary layer of a frozen prefix without a template under it: nothing reads this gradient)
            const int rc = dgrad(dbig, 3 * H, 3 * H, y.w_qkv, H, 3 * H, H, M, f32(w.dpre), f32(w.dx), CPT_F32, "dgrad(qkv)+residual", nullptr, nullptr, 0, (fuse_db && l > 0) ? &st.dxS : nullptr, 1);
            st.dxB = (st.dxS == 2 && M >= 2048) ? 1 : 0;
            PASS(rc);
        }
        if (!fuse_db) bucket(1 + l);
        return CPT_OK;
    }

    // What the full walk hands on to the next layer's launches, brought to an end at the boundary of a frozen prefix: the column-sum jobs that wait
    // for a carrier launch (the boundary layer's attention-side LayerNorm sums) go out on a launch of their own, and so do the K-split partial
    // matrices of its Q|K|V weight gradient; then the layer's bucket is complete.
    int flush_boundary(int l, BwdState& st) const {
        if (st.pend.n > 0) TRY(cpt::col_jobs_flush(st.pend, s), "column-sum jobs (boundary layer)");
        st.pend = cpt::ColJobs{};
        if (st.qjob.S > 1) TRY(cpt::reduce_job_flush(st.qjob, s), "partial sums of wgrad(qkv), boundary layer");
        st.qjob = cpt::ReduceJob{};
        // (defensive: layer() announces a bucket waiting behind its triple launch before it returns and layer_tail() never sets one, so nothing waits
        // here today; a later stage function that leaves one must not lose it at the boundary)
        if (st.ready_after_triple >= 0) { bucket(st.ready_after_triple); st.ready_after_triple = -1; }
        if (fuse_db) bucket(1 + l);      // (unfused: attention() has announced it)
        return CPT_OK;
    }

    // round 6: the pruned last layer -- BertOutput, BertIntermediate, BertSelfOutput backward on the B head rows; the weight gradients contract over
    // B rows (one K-tile), the data gradient re-enters the full tensors at the head rows (everything else is zero).  drows IS the gradient of
    // the layer's compact output.
    int layer_tail(int l, BwdState& st) const {
        const cpt_layer& y = m->layers[l];
        const cpt_layer_grads& gy = g->layers[l];
        const cpt::RowMap rm = {nsp ? nullptr : b->mask_pos, L, 1};
        const cpt::DropSpec sp2 = site(3 + 3 * l), sp1 = site(2 + 3 * l);
        float* dpre_r = f32(w.t_dpre); float* da_r = f32(w.t_da);
        void* dlpF = at(w.t_dlpF); void* dlpA = at(w.t_dlpA); void* dbig_r = at(w.t_dbig); void* dctx_r = at(w.t_dctx);
        cpt::LnBwdExtra e2 = {};
        e2.stats = f32(w.t_st2); e2.drop_rows = rm; e2.keep_bits = (const unsigned short*)at(w.t_kb2);
        TRY(cpt::ln_bwd(f32(w.drows), f32(w.t_pre2), y.ln2_g, d.ln_eps, dpre_r, dlpF, dt, gy.ln2_g, gy.ln2_b, B, H, B, 0, 0, 0, s, nullptr, 0,
                        ph ? &sp2 : nullptr, gy.b_out, &e2), "ln_bwd(ffn, head rows)");
        // (the plan's tail term holds the fused GELU-gradient GEMM's shape gate: no NOT_FUSED here)
        PASS(dgrad(dlpF, H, H, y.w_out, I, H, I, B, nullptr, dbig_r, dt, "dgrad(ffn down)+gelu_bwd+bias (head rows)", at(w.t_u), gy.b_in));
        int daS = 1;
        PASS(dgrad(dbig_r, I, I, y.w_in, H, I, H, B, dpre_r, da_r, CPT_F32, "dgrad(ffn up)+residual (head rows)", nullptr, nullptr, 0, &daS));
        cpt::LnBwdExtra e1 = {};
        e1.stats = f32(w.t_st1); e1.drop_rows = rm; e1.keep_bits = (const unsigned short*)at(w.t_kb1);
        if (daS > 1) { e1.dy_parts = daS; e1.dy_stride = (size_t)B * H; e1.dy_resid = dpre_r; }
        TRY(cpt::ln_bwd(daS > 1 ? f32(w.tA) : da_r, f32(w.t_pre1), y.ln1_g, d.ln_eps, dpre_r, dlpA, dt, gy.ln1_g, gy.ln1_b, B, H, B, 0, 0, 0, s,
                        nullptr, 0, ph ? &sp1 : nullptr, gy.b_ao, &e1), "ln_bwd(attn, head rows)");
        const int Kp = up64(B);
        const int r3 = cpt::gemm_tn_triple(dlpF, H, at(w.t_h), I, gy.w_out, H, I, dbig_r, I, at(w.t_a), H, gy.w_in, I, H, dlpA, H, at(w.t_ctx), H, gy.w_ao, H, H, Kp, B, s);
        if (r3 == CPT_ERR_SHAPE) {
            PASS(wgrad(dlpF, dt, H, H, at(w.t_h), I, I, B, Kp, gy.w_out, I, "wgrad(ffn down, head rows)"));
            PASS(wgrad(dbig_r, dt, I, I, at(w.t_a), H, H, B, Kp, gy.w_in, H, "wgrad(ffn up, head rows)"));
            PASS(wgrad(dlpA, dt, H, H, at(w.t_ctx), H, H, B, Kp, gy.w_ao, H, "wgrad(attn out, head rows)"));
        } else TRY(r3, "wgrad(ffn down | ffn up | attn out, head rows)");
        PASS(dgrad(dlpA, H, H, y.w_ao, H, H, H, B, nullptr, dctx_r, dt, "dgrad(attn out, head rows)"));
        TRY(cpt::tail_scatter2(dctx_r, dpre_r, rm.pos, at(w.dctx), f32(w.dpre), B, L, H, s), "scatter(head rows of dctx, dpre)");
        return attention(l, st, true);      // (Q|K|V's weight gradient alone)
    }

    int layer(int l, BwdState& st) const {
        const cpt_layer& y = m->layers[l];
        const cpt_layer_grads& gy = g->layers[l];
        float* dpre = f32(w.dpre); void* dbig = at(w.dbig);
        // x_out = LN2(pre2); pre2 = h W_out^T + b_out + a
        LnBwdSide f = {};
        f.what = &WHAT_LN2; f.dy = f32(w.dx); f.S = st.dxS; f.Sbf16 = st.dxB; f.pre = w.o_pre2; f.st = w.o_st2; f.kb = w.o_kb2;
        f.g = y.ln2_g; f.dg = gy.ln2_g; f.db = gy.ln2_b; f.dbias = gy.b_out; f.site = 3 + 3 * l; f.out_lp = at(ph ? w.dmask_lp : w.dpre_lp);
        PASS(ln_bwd_side(l, st, f));
        if (fuse_db && l + 1 < d.layers) {      // the layer above is complete now: this launch added its attention-side LayerNorm's sums
            if (st.qjob.S > 1) st.ready_after_triple = 1 + l + 1;      // (... but for its Q|K|V weight gradient, still in partial matrices)
            else bucket(1 + l + 1);
        }
        // h = gelu(u); u = a W_in^T + b_in: bf16 runs the GELU backward in the epilogue of the data-gradient GEMM and sums its columns into the bias gradient (round 3: no colsum
        // launch over the M x I tensor) -- round 6: as PARTIAL rows (one per 32-row wave block, plain stores -- the end-of-launch atomics of round 3's form cost more than the
        // colsum launch), added up by the attention-side LayerNorm backward's spare workgroups (bit 0 of key 18 cleared: the colsum launch)
        int rc = dt == CPT_BF16 ? dgrad(dpre_in(), H, H, y.w_out, I, H, I, M, nullptr, dbig, dt, "dgrad(ffn down)+gelu_bwd+bias", LB(l, w.o_u),
                                        bin_parts ? f32(w.csp) : nullptr, w.csp_rows) : NOT_FUSED;
        if (rc == NOT_FUSED) {
            PASS(dgrad(dpre_in(), H, H, y.w_out, I, H, I, M, nullptr, dbig, dt, "dgrad(ffn down)"));
            TRY(cpt::gelu_bwd(dbig, LB(l, w.o_u), dbig, dt, (size_t)M * I, s), "gelu_bwd");
            TRY(cpt::colsum(dbig, dt, I, gy.b_in, M, I, s), "colsum(b_in)");
        } else if (rc) return rc;
        else if (!bin_parts) TRY(cpt::colsum(dbig, dt, I, gy.b_in, M, I, s), "colsum(b_in)");
        else TRY(col_jobs_push(st.pend, s, f32(w.csp), (M + 31) / 32, I, I, I, gy.b_in), "column-sum jobs (b_in)");
        // weight gradients: the two FFN matrices share one launch here, attention output and Q|K|V one behind the attention backward -- their operands stay untouched until then.
        // triple: the two FFN ones wait for the attention output's and share ONE launch with it behind the attention-side LayerNorm backward (which then writes its
        // low-precision output to a second buffer: the FFN-side one is still an operand); Q|K|V runs alone behind the attention backward
        if (!triple) PASS(wgrad_pair({dpre_in(), H, LB(l, w.o_h), I, gy.w_out, "wgrad(ffn down)"}, {dbig, I, LB(l, w.o_a), H, gy.w_in, "wgrad(ffn up)"}, "wgrad(ffn down | ffn up)"));
        int daS = 1;
        rc = dgrad(dbig, I, I, y.w_in, H, I, H, M, dpre, f32(w.da), CPT_F32, "dgrad(ffn up)+residual", nullptr, nullptr, 0, fuse_db ? &daS : nullptr, 1);
        PASS(rc);
        // a = LN1(pre1); pre1 = ctx W_ao^T + b_ao + x_in
        const void* dao_in = triple ? at(w.dlp2) : dpre_in();      // gradient entering the attention output's dense layer
        LnBwdSide a = {};
        a.what = &WHAT_LN1; a.dy = f32(w.da); a.S = daS; a.pre = w.o_pre1; a.st = w.o_st1; a.kb = w.o_kb1;
        a.Sbf16 = (daS == 2 && M >= 2048) ? 1 : 0;      // (two partial matrices at 2048..6144 rows: the bf16 pair of gemm_nn's split2_bf16; at few rows K splits >= 4 ways in fp32)
        a.g = y.ln1_g; a.dg = gy.ln1_g; a.db = gy.ln1_b; a.dbias = gy.b_ao; a.site = 2 + 3 * l; a.out_lp = triple ? at(w.dlp2) : at(ph ? w.dmask_lp : w.dpre_lp);
        PASS(ln_bwd_side(l, st, a));
        if (triple) {
            TRY(cpt::gemm_tn_triple(dpre_in(), H, LB(l, w.o_h), I, gy.w_out, H, I, dbig, I, LB(l, w.o_a), H, gy.w_in, I, H,
                                    dao_in, H, LB(l, w.o_ctx), H, gy.w_ao, H, H, Mp, M, s, &st.qjob), "wgrad(ffn down | ffn up | attn out) + partial sums of the layer above's wgrad(qkv)");
            st.qjob = cpt::ReduceJob{};
        } else if (st.qjob.S > 1) {
            TRY(cpt::reduce_job_flush(st.qjob, s), "partial sums of wgrad(qkv)");
            st.qjob = cpt::ReduceJob{};
        }
        if (st.ready_after_triple >= 0) { bucket(st.ready_after_triple); st.ready_after_triple = -1; }
        PASS(dgrad(dao_in, H, H, y.w_ao, H, H, H, M, nullptr, at(w.dctx), dt, "dgrad(attn out)"));
        return attention(l, st, triple);
    }

    // region projection and text embeddings
    int embeddings(BwdState& st) const {
        float* dx = f32(w.dx);
        if (dt == CPT_BF16) {      // the last attention-side LayerNorm's sums (and whatever else still waits for a carrier launch)
            if (st.qjob.S > 1) { TRY(cpt::reduce_job_flush(st.qjob, s), "partial sums of wgrad(qkv), first layer"); st.qjob = cpt::ReduceJob{}; }
            if (Li <= 0) {      // (with regions the jobs ride on the region LayerNorm's backward below: no launch of their own)
                TRY(cpt::col_jobs_flush(st.pend, s), "column-sum jobs");
                st.pend = cpt::ColJobs{};
                bucket(1);
            }
        }
        // (round 6: the embedding dropout's backward is applied by the two launches that read dx -- the region LayerNorm's backward and the embedding backward -- as
        // they load their rows: no dropout pass over all rows in front of them)
        const cpt::DropSpec edrop = site(0);
        if (Li > 0) {
            float* dimg = f32(w.dimg);
            const bool iln = d.use_img_ln && m->img_ln_g;
            cpt::LnBwdExtra ei = {};
            if (ph) ei.in_drop = edrop;
            if (dt == CPT_BF16) ei.jobs = &st.pend;      // the first layer's attention-side column sums (and whatever else still waits): spare workgroups of this launch
            TRY(cpt::ln_bwd(dx, f32(w.imgpre), iln ? m->img_ln_g : nullptr, d.img_ln_eps, dimg, dt == CPT_BF16 ? at(w.dimg_lp) : nullptr, dt,
                            iln ? g->img_ln_g : nullptr, iln ? g->img_ln_b : nullptr, R, H, Li, L, Lt, 0, s, nullptr, 0, nullptr, iln ? g->b_img : nullptr, &ei), "ln_bwd(img) + b_img sums + column-sum jobs");
            if (dt == CPT_BF16) { st.pend = cpt::ColJobs{}; bucket(1); }
            if (!iln) TRY(cpt::colsum(dimg, CPT_F32, H, g->b_img, R, H, s), "colsum(b_img)");      // (no region LayerNorm: the launch above is a plain row gather)
            float* gimg = f32(w.gimg);      // (written whole by the weight-gradient GEMM: nothing to clear)
            PASS(wgrad(dt == CPT_BF16 ? at(w.dimg_lp) : (const void*)dimg, dt, H, H, at(w.imgp), Dp, Dp, R, Rp, gimg, Dp, "wgrad(img_embedding)"));
            TRY(cpt::unpad_add(gimg, g->w_img, H, d.img_dim, Dp, s), "unpad(img weight grad)");
        }
        TRY(cpt::embed_bwd(dx, b->input_ids, b->token_type, b->position_ids, m->word_emb, m->pos_emb, m->type_emb, m->emb_ln_g,
                           d.ln_eps, g->word_emb, g->pos_emb, g->type_emb, g->emb_ln_g, g->emb_ln_b, B, Lt, L, H, d.vocab, d.max_pos,
                           d.type_vocab, s, ph ? &edrop : nullptr), "embed_bwd + dropout_bwd(embeddings)");
        bucket(0);
        return CPT_OK;
    }
};

// the head's data gradient enters the encoder: drows scattered into a cleared dx -- once for the three walks below (full, frozen prefix, frozen model).
// (pruned last layer: drows IS the gradient of that layer's compact output)
int head_rows_to_dx(const TrainCtx& t) {
    if (t.tail) return CPT_OK;
    hipError_t e = hipMemsetAsync(t.f32(t.w.dx), 0, (size_t)t.M * t.H * 4, t.s);
    if (e != hipSuccess) return abi_fail(CPT_ERR_HIP - (int)e, "zero dx: %s", hipGetErrorString(e));
    TRY(cpt::scatter_rows_add(t.f32(t.w.drows), t.nsp ? nullptr : t.b->mask_pos, t.f32(t.w.dx), t.Rh, t.L, t.H, t.s, t.b->n_rows > 0 ? t.b->row_seq : nullptr, t.B),
        "scatter([MASK] / [CLS] rows)");
    return CPT_OK;
}

// ---- backward of a frozen model (cpt_train_bwd_soft) ----------------------------------------------------------------------------------------
// The walk of TrainBwd with everything that only a parameter gradient needs taken out: the same head, LayerNorm backwards (LnBwdExtra::no_sums:
// no gain / shift / bias sums, no partial tables, no carried jobs), data-gradient GEMMs with the GELU gradient, attention backward, dropout and
// residual handling under the same plan -- the pruned last layer, the K-split partial matrices the next LayerNorm backward adds, the bf16
// partial pair, the unfused fp32 / bf16x3 branch -- and no weight-gradient GEMM, column sum, zero launch or region-side launch.  It ends in
// the template's gradient (bwd.hip soft_template_bwd), the only tensor outside the workspace it writes.
struct FrozenBwd : TrainCtx {
    const cpt_soft_template* soft; float loss_scale; const float* loss_scale_dev;
    const float* dpre_f() const { return f32(ph ? w.dmask : w.dpre); }
    const void* dpre_in() const { return dt == CPT_BF16 ? at(ph ? w.dmask_lp : w.dpre_lp) : (const void*)dpre_f(); }

    int head_mlm() const {
        float* dt2 = f32(w.dt2); float* duh = f32(w.duh);
        TRY(cpt::scale_cast(f32(w.dlogits), f32(w.loss), loss_scale, loss_scale_dev, at(w.dl_lp), dt, Rh, V, Vp, s), "scale(dlogits)");
        PASS(dgrad(at(w.dl_lp), Vp, Vp, m->w_dec, H, V, H, Rh, nullptr, dt2, CPT_F32, "dgrad(decoder)"));
        cpt::LnBwdExtra e = {};
        e.no_sums = 1;
        TRY(cpt::ln_bwd(dt2, f32(w.uh), m->tr_ln_g, d.ln_eps, duh, dt == CPT_BF16 ? at(w.duh_lp) : nullptr, dt, nullptr, nullptr, Rh, H, Rh, 0, 0, 1, s,
                        nullptr, 0, nullptr, nullptr, &e), "ln_bwd(head)");
        const void* duh_in = dt == CPT_BF16 ? at(w.duh_lp) : (const void*)duh;
        return dgrad(duh_in, H, H, m->w_tr, H, H, H, Rh, nullptr, f32(w.drows), CPT_F32, "dgrad(head transform)");
    }

    // one LayerNorm backward with the dropout mask of the dense output in front of it (TrainBwd::ln_bwd_side without its sums)
    int ln_bwd_side(int l, const LnBwdSide& q) const {
        float* dpre = f32(w.dpre);
        cpt::LnBwdExtra e = {};
        e.no_sums = 1;
        if (!fuse_db) {
            TRY(cpt::ln_bwd(q.dy, LBf(l, q.pre), q.g, d.ln_eps, dpre, nullptr, dt, nullptr, nullptr, M, H, M, 0, 0, 0, s, nullptr, 0, nullptr, nullptr, &e), q.what->ln_bwd);
            if (ph) TRY(cpt::dropout_rows(dpre, nullptr, f32(w.dmask), nullptr, dt, M, H, site(q.site), s), q.what->dropout);
            return CPT_OK;
        }
        const cpt::DropSpec sp = site(q.site);
        e.stats = LBf(l, q.st); e.keep_bits = (const unsigned short*)LB(l, q.kb);
        if (q.S > 1) { e.dy_parts = q.S; e.dy_stride = (size_t)M * H; e.dy_resid = dpre; e.dy_parts_bf16 = q.Sbf16; }
        TRY(cpt::ln_bwd(q.S > 1 ? f32(w.tA) : q.dy, LBf(l, q.pre), q.g, d.ln_eps, dpre, q.out_lp, dt, nullptr, nullptr, M, H, M, 0, 0, 0, s, nullptr, 0,
                        ph ? &sp : nullptr, nullptr, &e), q.what->fused);
        return CPT_OK;
    }

    // attention backward of layer l and the data gradient into dx
    int attention(int l, BwdState& st) const {
        const cpt_layer& y = m->layers[l];
        void* dbig = at(w.dbig);
        const cpt::DropSpec da_spec = site(1 + 3 * l, true);
        if (x3_attn)
            TRY(cpt::attention_bwd_x3(LBf(l, w.o_qkv), b->attn_mask, (const float*)at(w.dctx), (float*)dbig, B, L, d.heads, s, pa ? &da_spec : nullptr, nullptr),
                "attention_bwd (split operands)");
        else
            TRY(cpt::attention_bwd(dt, LB(l, w.o_qkv), b->attn_mask, at(w.dctx), dbig, B, L, d.heads, s, pa ? &da_spec : nullptr, nullptr, m3d,
                                   attn_stats ? LB(l, w.o_ctx) : nullptr, attn_stats ? LBf(l, w.o_ast) : nullptr), "attention_bwd");
        // (layer 0's result feeds the template gradient: complete; above that a K-split launch leaves its partial matrices to the next LayerNorm backward)
        st.dxS = 1;
        const int rc = dgrad(dbig, 3 * H, 3 * H, y.w_qkv, H, 3 * H, H, M, f32(w.dpre), f32(w.dx), CPT_F32, "dgrad(qkv)+residual", nullptr, nullptr, 0, (fuse_db && l > 0) ? &st.dxS : nullptr, 1);
        st.dxB = (st.dxS == 2 && M >= 2048) ? 1 : 0;
        return rc;
    }

    // the pruned last layer on the B head rows (TrainBwd::layer_tail)
    int layer_tail(int l, BwdState& st) const {
        const cpt_layer& y = m->layers[l];
        const cpt::RowMap rm = {b->mask_pos, L, 1};
        const cpt::DropSpec sp2 = site(3 + 3 * l), sp1 = site(2 + 3 * l);
        float* dpre_r = f32(w.t_dpre); float* da_r = f32(w.t_da);
        void* dlpF = at(w.t_dlpF); void* dlpA = at(w.t_dlpA); void* dbig_r = at(w.t_dbig); void* dctx_r = at(w.t_dctx);
        cpt::LnBwdExtra e2 = {};
        e2.no_sums = 1; e2.stats = f32(w.t_st2); e2.drop_rows = rm; e2.keep_bits = (const unsigned short*)at(w.t_kb2);
        TRY(cpt::ln_bwd(f32(w.drows), f32(w.t_pre2), y.ln2_g, d.ln_eps, dpre_r, dlpF, dt, nullptr, nullptr, B, H, B, 0, 0, 0, s, nullptr, 0,
                        ph ? &sp2 : nullptr, nullptr, &e2), "ln_bwd(ffn, head rows)");
        PASS(dgrad(dlpF, H, H, y.w_out, I, H, I, B, nullptr, dbig_r, dt, "dgrad(ffn down)+gelu_bwd (head rows)", at(w.t_u)));
        int daS = 1;
        PASS(dgrad(dbig_r, I, I, y.w_in, H, I, H, B, dpre_r, da_r, CPT_F32, "dgrad(ffn up)+residual (head rows)", nullptr, nullptr, 0, &daS));
        cpt::LnBwdExtra e1 = {};
        e1.no_sums = 1; e1.stats = f32(w.t_st1); e1.drop_rows = rm; e1.keep_bits = (const unsigned short*)at(w.t_kb1);
        if (daS > 1) { e1.dy_parts = daS; e1.dy_stride = (size_t)B * H; e1.dy_resid = dpre_r; }
        TRY(cpt::ln_bwd(daS > 1 ? f32(w.tA) : da_r, f32(w.t_pre1), y.ln1_g, d.ln_eps, dpre_r, dlpA, dt, nullptr, nullptr, B, H, B, 0, 0, 0, s,
                        nullptr, 0, ph ? &sp1 : nullptr, nullptr, &e1), "ln_bwd(attn, head rows)");
        PASS(dgrad(dlpA, H, H, y.w_ao, H, H, H, B, nullptr, dctx_r, dt, "dgrad(attn out, head rows)"));
        TRY(cpt::tail_scatter2(dctx_r, dpre_r, rm.pos, at(w.dctx), f32(w.dpre), B, L, H, s), "scatter(head rows of dctx, dpre)");
        return attention(l, st);
    }

    int layer(int l, BwdState& st) const {
        const cpt_layer& y = m->layers[l];
        float* dpre = f32(w.dpre); void* dbig = at(w.dbig);
        void* lp_out = at(ph ? w.dmask_lp : w.dpre_lp);
        // x_out = LN2(pre2); pre2 = h W_out^T + b_out + a
        LnBwdSide f = {};
        f.what = &WHAT_LN2; f.dy = f32(w.dx); f.S = st.dxS; f.Sbf16 = st.dxB; f.pre = w.o_pre2; f.st = w.o_st2; f.kb = w.o_kb2;
        f.g = y.ln2_g; f.site = 3 + 3 * l; f.out_lp = lp_out;
        PASS(ln_bwd_side(l, f));
        // h = gelu(u); u = a W_in^T + b_in: bf16 runs the GELU backward in the epilogue of the data-gradient GEMM (no bias sums here)
        int rc = dt == CPT_BF16 ? dgrad(dpre_in(), H, H, y.w_out, I, H, I, M, nullptr, dbig, dt, "dgrad(ffn down)+gelu_bwd", LB(l, w.o_u)) : NOT_FUSED;
        if (rc == NOT_FUSED) {
            PASS(dgrad(dpre_in(), H, H, y.w_out, I, H, I, M, nullptr, dbig, dt, "dgrad(ffn down)"));
            TRY(cpt::gelu_bwd(dbig, LB(l, w.o_u), dbig, dt, (size_t)M * I, s), "gelu_bwd");
        } else if (rc) return rc;
        int daS = 1;
        PASS(dgrad(dbig, I, I, y.w_in, H, I, H, M, dpre, f32(w.da), CPT_F32, "dgrad(ffn up)+residual", nullptr, nullptr, 0, fuse_db ? &daS : nullptr, 1));
        // a = LN1(pre1); pre1 = ctx W_ao^T + b_ao + x_in
        LnBwdSide a = {};
        a.what = &WHAT_LN1; a.dy = f32(w.da); a.S = daS; a.pre = w.o_pre1; a.st = w.o_st1; a.kb = w.o_kb1;
        a.Sbf16 = (daS == 2 && M >= 2048) ? 1 : 0;
        a.g = y.ln1_g; a.site = 2 + 3 * l; a.out_lp = lp_out;      // (no weight gradient still reads the FFN side's low-precision rows: one buffer serves both sides)
        PASS(ln_bwd_side(l, a));
        PASS(dgrad(dpre_in(), H, H, y.w_ao, H, H, H, M, nullptr, at(w.dctx), dt, "dgrad(attn out)"));
        return attention(l, st);
    }

    // the template's gradient: the embedding LayerNorm's backward on the slot rows; the region rows of dx and every table go unread and unwritten
    int template_grad() const {
        const cpt::DropSpec edrop = site(0);
        TRY(cpt::soft_template_bwd(f32(w.dx), b->input_ids, b->token_type, b->position_ids, soft->tmpl, soft->n_slots, m->pos_emb, m->type_emb, m->emb_ln_g,
                                   d.ln_eps, soft->g_tmpl, B, Lt, L, H, d.max_pos, d.type_vocab, s, ph ? &edrop : nullptr), "soft_template_bwd + dropout_bwd(embeddings)");
        return CPT_OK;
    }
};

int frozen_bwd_impl(const cpt_model* m, const cpt_soft_template* soft, const cpt_batch* b, float loss_scale, const float* loss_scale_dev,
                    void* workspace, size_t workspace_bytes, void* stream, const cpt_dropout* drop) {
    if (!m || !b || !workspace) return abi_fail(CPT_ERR_NULL, "cpt_train_bwd_soft: null argument");
    PASS(check_soft(m, soft, true, "cpt_train_bwd_soft"));
    PASS(check_drop(drop, "cpt_train_bwd_soft"));
    const TrainPlan p = make_train_plan(m, nullptr, b, drop);
    PASS(check_common(m, b, workspace, workspace_bytes, p, "cpt_train_bwd_soft"));
    FrozenBwd t = {};
    set_ctx(t, p, m, b, workspace, stream, drop, nullptr, nullptr);
    t.soft = soft; t.loss_scale = loss_scale; t.loss_scale_dev = loss_scale_dev;
    PASS(t.head_mlm());
    PASS(head_rows_to_dx(t));
    BwdState st = {};
    st.ready_after_triple = -1; st.dxS = 1;
    for (int l = m->dims.layers - 1; l >= 0; --l) PASS(p.tail && l == m->dims.layers - 1 ? t.layer_tail(l, st) : t.layer(l, st));
    return t.template_grad();
}

// ---- the backward walk: the full step, or a frozen prefix of stages (cpt_train_bwd_from) ---------------------------------------------------
// Stages are the data-parallel buckets: 0 = embedding side, 1 + l = encoder layer l, layers + 1 = pooler and head; stages < first_stage are frozen.
// ONE walk serves every entry point.  first_stage 0 is the full step: head, every layer, embeddings().  With a frozen prefix the walk runs the same
// stage functions down to the boundary layer first_stage - 1 and ends what they leave "for the next launch" there (TrainBwd::flush_boundary).
// Under the boundary: nothing -- or, with a soft template, FrozenBwd's stage functions on the BwdState the boundary layer left (dxS / dxB: its
// data gradient, possibly still in K-split partial matrices), ending in the template's gradient.  who: the entry point, for error reports.
int train_bwd_walk(const char* who, const cpt_model* m, const cpt_rel2* x, const cpt_soft_template* soft, const cpt_batch* b, const cpt_model_grads* g, int first_stage,
                   float loss_scale, const float* loss_scale_dev, void* workspace, size_t workspace_bytes, void* stream, cpt_bucket_fn grads_ready,
                   void* user, const cpt_dropout* drop) {
    if (!m || !b || !g || !workspace) return abi_fail(CPT_ERR_NULL, "%s: null argument", who);
    const int N = m->dims.layers;
    if (first_stage < 0 || first_stage > N + 1) return abi_fail(CPT_ERR_SHAPE, "%s: first_stage %d outside [0, layers + 1 = %d]", who, first_stage, N + 1);
    if (soft && first_stage == 0)
        return abi_fail(CPT_ERR_SHAPE, "%s: a soft template beside a trainable embedding side (first_stage 0) is not supported: the word "
                        "table's lookup gradient would have to skip the slot ids", who);
    if (soft && x) return abi_fail(CPT_ERR_SHAPE, "%s: soft-template tuning runs on the MLM head, not on the two relation heads", who);
    if (soft) PASS(check_soft(m, soft, true, who));
    if (first_stage <= N && !g->layers) return abi_fail(CPT_ERR_NULL, "%s: g->layers is NULL", who);
    PASS(check_drop(drop, who));
    const TrainPlan p = make_train_plan(m, x, b, drop);
    PASS(check_common(m, b, workspace, workspace_bytes, p, who));
    if (p.nsp && b->n_rows > 0) return abi_fail(CPT_ERR_SHAPE, "%s: label grids (n_rows) belong to the MLM head, not the NSP head", who);      // (as the forward: Rh has one meaning)
    if (x && !p.nsp) return abi_fail(CPT_ERR_NULL, "%s: the two-head step needs the pooler and head 0 (w_pool, w_rel) and no MLM head", who);
    TrainBwd t = {};
    set_ctx(t, p, m, b, workspace, stream, drop, grads_ready, user);
    t.x = x; t.g = g; t.loss_scale = loss_scale; t.loss_scale_dev = loss_scale_dev;
    t.stage = first_stage; t.below = soft != nullptr;
    PASS(p.nsp ? t.head_nsp() : t.head_mlm());
    if (!t.head_dx()) {      // the head alone
        t.bucket(N + 1);
        return CPT_OK;
    }
    PASS(head_rows_to_dx(t));
    t.bucket(N + 1);
    BwdState st = {};
    st.ready_after_triple = -1; st.dxS = 1;
    const int lb = std::max(first_stage - 1, 0);      // the lowest layer with a parameter gradient (N: none of them has one)
    for (int l = N - 1; l >= lb; --l) PASS(p.tail && l == N - 1 ? t.layer_tail(l, st) : t.layer(l, st));
    if (first_stage == 0) return t.embeddings(st);      // the full step: the embedding side's launches carry what layer 0 left
    if (lb < N) PASS(t.flush_boundary(lb, st));
    if (!soft) return CPT_OK;
    FrozenBwd f = {};
    set_ctx(f, p, m, b, workspace, stream, drop, nullptr, nullptr);
    f.soft = soft; f.loss_scale = loss_scale; f.loss_scale_dev = loss_scale_dev;
    for (int l = lb - 1; l >= 0; --l) PASS(p.tail && l == N - 1 ? f.layer_tail(l, st) : f.layer(l, st));
    return f.template_grad();
}

int train_bwd_impl(const cpt_model* m, const cpt_rel2* x, const cpt_batch* b, const cpt_model_grads* g, float loss_scale, const float* loss_scale_dev,
                   void* workspace, size_t workspace_bytes, void* stream, cpt_bucket_fn grads_ready, void* user, const cpt_dropout* drop) {
    return train_bwd_walk(x ? "cpt_train_bwd_rel2" : "cpt_train_bwd", m, x, nullptr, b, g, 0, loss_scale, loss_scale_dev, workspace, workspace_bytes, stream, grads_ready, user, drop);
}

}  // namespace

extern "C" {

size_t cpt_train_workspace_bytes(const cpt_dims* d, int B, int Lt, int Li) {
    if (!d || B <= 0 || Lt <= 0 || Li < 0) return 0;
    return plan_shapes(*d, B, Lt, Li, 0).w.total;
}
size_t cpt_train_workspace_bytes_rows(const cpt_dims* d, int B, int Lt, int Li, int n_rows) {
    if (!d || B <= 0 || Lt <= 0 || Li < 0 || n_rows < 0 || (long)n_rows > (long)B * (Lt + Li)) return 0;
    return plan_shapes(*d, B, Lt, Li, n_rows).w.total;
}

int cpt_train_fwd(const cpt_model* m, const cpt_batch* b, const cpt_outputs* o, void* workspace, size_t workspace_bytes, void* stream) {
    return cpt_train_fwd_ex(m, b, o, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr);
}

int cpt_train_bwd(const cpt_model* m, const cpt_batch* b, const cpt_model_grads* g, float loss_scale, void* workspace, size_t workspace_bytes, void* stream) {
    return cpt_train_bwd_ex(m, b, g, loss_scale, nullptr, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr);
}

// What cpt_train_bwd needs cleared, in one launch (+ one memset for a table the chosen head does not overwrite): Linear weight
// gradients are WRITTEN by their GEMMs (and the tied word-embedding table by the decoder's), so only the vectors and small tables
// that take atomic adds are cleared -- 0.3 MB instead of the 447 MB of a whole-buffer fill per step.
// first_stage > 0 (cpt_train_zero_grads_from): stages below it are frozen -- nothing of theirs is read through g or cleared
static int zero_grads_impl(const cpt_model* m, const cpt_rel2* x, const cpt_model_grads* g, int Li, void* stream, int first_stage = 0) {
    if (!m || !g || (!g->layers && first_stage <= m->dims.layers)) return abi_fail(CPT_ERR_NULL, "cpt_train_zero_grads: null argument");
    const cpt_dims& d = m->dims;
    if (first_stage < 0 || first_stage > d.layers + 1) return abi_fail(CPT_ERR_SHAPE, "cpt_train_zero_grads_from: first_stage %d outside [0, layers + 1 = %d]", first_stage, d.layers + 1);
    const bool emb = first_stage == 0;      // the embedding side trains
    hipStream_t s = (hipStream_t)stream;
    const bool nsp = !m->w_tr && !m->w_dec;
    const size_t H = d.hidden, I = d.inter;
    cpt::ZeroSegs z;
    z.count = 0;
    bool ovf = false;
    auto seg = [&](float* p, size_t n) {
        if (!p || !n) return;
        if (z.count >= cpt::ZS_MAX) { ovf = true; return; }
        z.p[z.count] = p; z.n[z.count] = (unsigned)n; ++z.count;
    };
    auto big = [&](float* p, size_t n) -> int {
        if (!p || !n) return CPT_OK;
        hipError_t e = hipMemsetAsync(p, 0, n * 4, s);
        return e == hipSuccess ? CPT_OK : abi_fail(CPT_ERR_HIP - (int)e, "cpt_train_zero_grads: %s", hipGetErrorString(e));
    };
    if (emb) {
        seg(g->pos_emb, (size_t)d.max_pos * H); seg(g->type_emb, (size_t)d.type_vocab * H);
        seg(g->emb_ln_g, H); seg(g->emb_ln_b, H); seg(g->b_img, H); seg(g->img_ln_g, H); seg(g->img_ln_b, H);
    }
    for (int l = std::max(first_stage - 1, 0); l < d.layers; ++l) {
        const cpt_layer_grads& y = g->layers[l];
        seg(y.b_qkv, 3 * H); seg(y.b_ao, H); seg(y.ln1_g, H); seg(y.ln1_b, H);
        seg(y.b_in, I); seg(y.b_out, H); seg(y.ln2_g, H); seg(y.ln2_b, H);
    }
    seg(g->b_tr, H); seg(g->tr_ln_g, H); seg(g->tr_ln_b, H); seg(g->b_dec, (size_t)d.vocab);
    seg(g->b_pool, H); seg(g->b_rel, (size_t)d.n_rel);
    if (x) seg(x->g_b_rel1, (size_t)d.n_rel);
    if (ovf) return abi_fail(CPT_ERR_SHAPE, "cpt_train_zero_grads: more than %d gradient vectors (layers = %d)", cpt::ZS_MAX, d.layers);
    TRY(cpt::zero_segments(z, s), "zero_segments");
    if (nsp) {      // no decoder GEMM writes the word table: the lookup gradient adds into it
        if (emb) PASS(big(g->word_emb, (size_t)d.vocab * H));
        PASS(big(g->w_tr, H * H));
    }
    // (the MLM path leaves the pooler / relation head without a gradient: nothing writes those regions of the caller's gradient buffer and the
    // optimizer skips them (code 0) -- round 6: no per-step fill of them either)
    if (Li <= 0 && emb) PASS(big(g->w_img, H * (size_t)d.img_dim));      // no regions: the projection gets no gradient
    return CPT_OK;
}

int cpt_dropout_mask(const cpt_dropout* drop, int site, int is_attn, unsigned char* out, int n0, int n1, int n2, void* stream) {
    if (!drop || !out) return abi_fail(CPT_ERR_NULL, "cpt_dropout_mask: null argument");
    PASS(check_drop(drop, "cpt_dropout_mask"));
    const cpt::DropSpec sp = drop_spec(drop, site, is_attn != 0);
    if (sp.thresh == 0) return abi_fail(CPT_ERR_SHAPE, "cpt_dropout_mask: the dropout probability of this site is 0");
    return abi_check(cpt::dropout_mask(is_attn ? 1 : 0, out, n0, n1, n2, sp, (hipStream_t)stream), "cpt_dropout_mask");
}

// ---- operator-level backward entry points (ABI 6): thin wrappers over the kernels cpt_train_bwd launches, for per-operator parity tests ----
int cpt_attention_bwd(int dtype, const void* qkv, const int64_t* attn_mask, int mask_3d, const void* dctx, void* dqkv, float* dbias_qkv,
                      int B, int L, int heads, const cpt_dropout* drop, int site, void* stream) {
    if (!qkv || !dctx || !dqkv) return abi_fail(CPT_ERR_NULL, "cpt_attention_bwd: null argument");
    if (B <= 0 || L <= 0 || heads <= 0) return abi_fail(CPT_ERR_SHAPE, "cpt_attention_bwd: bad shape B=%d L=%d heads=%d", B, L, heads);
    PASS(check_drop(drop, "cpt_attention_bwd"));
    const bool pa = drop && drop->p_attn > 0.f;
    const cpt::DropSpec sp = drop_spec(drop, site, true);
    const int m3 = (mask_3d && attn_mask) ? 1 : 0;
    if (dtype == CPT_BF16X3 || dtype == CPT_BF16X3_MASTERS) {
        if (!cpt::attention_bwd_x3_supported(L, m3))
            return abi_fail(CPT_ERR_SHAPE, "cpt_attention_bwd: no split-operand attention backward at L = %d%s", L, m3 ? " with a 3-D mask" : "");
        return abi_check(cpt::attention_bwd_x3((const float*)qkv, attn_mask, (const float*)dctx, (float*)dqkv, B, L, heads, (hipStream_t)stream,
                                               pa ? &sp : nullptr, dbias_qkv), "cpt_attention_bwd (split operands)");
    }
    if (dtype != CPT_F32 && dtype != CPT_BF16) return abi_fail(CPT_ERR_DTYPE, "cpt_attention_bwd: dtype %d", dtype);
    if (!cpt::attention_bwd_supported(dtype, L, pa ? 1 : 0, m3))
        return abi_fail(CPT_ERR_SHAPE, "cpt_attention_bwd: no attention backward for dtype %d at L = %d%s", dtype, L, pa ? " with attention dropout" : "");
    return abi_check(cpt::attention_bwd(dtype, qkv, attn_mask, dctx, dqkv, B, L, heads, (hipStream_t)stream, pa ? &sp : nullptr, dbias_qkv, m3), "cpt_attention_bwd");
}

int cpt_layernorm_bwd(const float* dy, const float* x, const float* g, float eps, float* dx, void* dx_lp, int lp_dtype, float* dg, float* db,
                      int R, int H, const cpt_dropout* drop, int site, float* dbias, void* scratch, size_t scratch_bytes, void* stream) {
    if (!dy || !x || !g || !dx || !dg || !db) return abi_fail(CPT_ERR_NULL, "cpt_layernorm_bwd: null argument");
    if (R <= 0 || H <= 0 || H % 4) return abi_fail(CPT_ERR_SHAPE, "cpt_layernorm_bwd: bad shape R=%d H=%d", R, H);
    if (dx_lp && lp_dtype != CPT_BF16 && lp_dtype != CPT_F32) return abi_fail(CPT_ERR_DTYPE, "cpt_layernorm_bwd: lp_dtype %d", lp_dtype);
    PASS(check_drop(drop, "cpt_layernorm_bwd"));
    const bool ph = drop && drop->p_hidden > 0.f;
    const cpt::DropSpec sp = drop_spec(drop, site, false);
    return abi_check(cpt::ln_bwd(dy, x, g, eps, dx, dx_lp, lp_dtype, dg, db, R, H, R, 0, 0, 0, (hipStream_t)stream, (float*)scratch, scratch_bytes,
                                 ph ? &sp : nullptr, dbias), "cpt_layernorm_bwd");
}

int cpt_embed_ln_bwd(const float* dy, const int64_t* ids, const int64_t* tt, const int64_t* pos, const float* word, const float* posw, const float* typew,
                     const float* g, float eps, float* dword, float* dposw, float* dtypew, float* dg, float* db, int B, int Lt, int L, int H,
                     int vocab, int max_pos, int type_vocab, void* stream) {
    if (!dy || !ids || !word || !posw || !typew || !g || !dword || !dposw || !dtypew || !dg || !db) return abi_fail(CPT_ERR_NULL, "cpt_embed_ln_bwd: null argument");
    if (B <= 0 || Lt <= 0 || L < Lt || H <= 0 || H % 4) return abi_fail(CPT_ERR_SHAPE, "cpt_embed_ln_bwd: bad shape B=%d Lt=%d L=%d H=%d", B, Lt, L, H);
    return abi_check(cpt::embed_bwd(dy, ids, tt, pos, word, posw, typew, g, eps, dword, dposw, dtypew, dg, db, B, Lt, L, H, vocab, max_pos, type_vocab,
                                    (hipStream_t)stream), "cpt_embed_ln_bwd");
}

int cpt_adamw(float* p, const float* g, float* m, float* v, const unsigned char* code, void* shadow_bf16,
              size_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
              float grad_scale, void* stream) {
    return abi_check(cpt::adamw_flat(p, g, m, v, code, shadow_bf16, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                                     (hipStream_t)stream), "cpt_adamw");
}

int cpt_adamw_ex(float* p, const float* g, float* m, float* v, const unsigned char* code, void* shadow_bf16,
                 size_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                 float grad_scale, int flags, void* stream) {
    if (flags & ~(CPT_ADAMW_HF | CPT_ADAMW_NO_BIAS_CORRECTION)) return abi_fail(CPT_ERR_SHAPE, "cpt_adamw_ex: unknown flags %d", flags);
    return abi_check(cpt::adamw_flat(p, g, m, v, code, shadow_bf16, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                                     (hipStream_t)stream, flags), "cpt_adamw_ex");
}

int cpt_train_fwd_ex(const cpt_model* m, const cpt_batch* b, const cpt_outputs* o, void* workspace,
                     size_t workspace_bytes, void* stream, cpt_bucket_fn before_bucket, void* user, const cpt_dropout* drop) {
    return train_fwd_impl(m, nullptr, b, o, workspace, workspace_bytes, stream, before_bucket, user, drop);
}

int cpt_train_bwd_ex(const cpt_model* m, const cpt_batch* b, const cpt_model_grads* g, float loss_scale, const float* loss_scale_dev,
                     void* workspace, size_t workspace_bytes, void* stream, cpt_bucket_fn grads_ready, void* user, const cpt_dropout* drop) {
    return train_bwd_impl(m, nullptr, b, g, loss_scale, loss_scale_dev, workspace, workspace_bytes, stream, grads_ready, user, drop);
}

int cpt_train_zero_grads(const cpt_model* m, const cpt_model_grads* g, int Li, void* stream) {
    return zero_grads_impl(m, nullptr, g, Li, stream);
}

int cpt_train_fwd_rel2(const cpt_model* m, const cpt_rel2* x, const cpt_batch* b, const cpt_outputs* o, void* workspace, size_t workspace_bytes,
                       void* stream, cpt_bucket_fn before_bucket, void* user, const cpt_dropout* drop) {
    if (!x) return abi_fail(CPT_ERR_NULL, "cpt_train_fwd_rel2: the second head (x) is NULL");
    return train_fwd_impl(m, x, b, o, workspace, workspace_bytes, stream, before_bucket, user, drop);
}

int cpt_train_bwd_rel2(const cpt_model* m, const cpt_rel2* x, const cpt_batch* b, const cpt_model_grads* g, float loss_scale,
                       const float* loss_scale_dev, void* workspace, size_t workspace_bytes, void* stream, cpt_bucket_fn grads_ready, void* user,
                       const cpt_dropout* drop) {
    if (!x) return abi_fail(CPT_ERR_NULL, "cpt_train_bwd_rel2: the second head (x) is NULL");
    PASS(check_rel2(m, x, b, "cpt_train_bwd_rel2", stream, false));
    return train_bwd_impl(m, x, b, g, loss_scale, loss_scale_dev, workspace, workspace_bytes, stream, grads_ready, user, drop);
}

int cpt_train_zero_grads_rel2(const cpt_model* m, const cpt_rel2* x, const cpt_model_grads* g, int Li, void* stream) {
    if (!x) return abi_fail(CPT_ERR_NULL, "cpt_train_zero_grads_rel2: the second head (x) is NULL");
    return zero_grads_impl(m, x, g, Li, stream);
}

int cpt_train_fwd_soft(const cpt_model* m, const cpt_soft_template* st, const cpt_batch* b, const cpt_outputs* o, void* workspace,
                       size_t workspace_bytes, void* stream, cpt_bucket_fn before_bucket, void* user, const cpt_dropout* drop) {
    if (!m) return abi_fail(CPT_ERR_NULL, "cpt_train_fwd_soft: null argument");
    PASS(check_soft(m, st, false, "cpt_train_fwd_soft"));
    return train_fwd_impl(m, nullptr, b, o, workspace, workspace_bytes, stream, before_bucket, user, drop, st);
}

int cpt_train_bwd_soft(const cpt_model* m, const cpt_soft_template* st, const cpt_batch* b, float loss_scale, const float* loss_scale_dev,
                       void* workspace, size_t workspace_bytes, void* stream, const cpt_dropout* drop) {
    return frozen_bwd_impl(m, st, b, loss_scale, loss_scale_dev, workspace, workspace_bytes, stream, drop);
}

int cpt_train_bwd_from(const cpt_model* m, const cpt_rel2* x, const cpt_soft_template* soft, const cpt_batch* b, const cpt_model_grads* g, int first_stage,
                       float loss_scale, const float* loss_scale_dev, void* workspace, size_t workspace_bytes, void* stream, cpt_bucket_fn grads_ready,
                       void* user, const cpt_dropout* drop) {
    if (!m || !b) return abi_fail(CPT_ERR_NULL, "cpt_train_bwd_from: null argument");
    if (x) PASS(check_rel2(m, x, b, "cpt_train_bwd_from", stream, false));
    return train_bwd_walk("cpt_train_bwd_from", m, x, soft, b, g, first_stage, loss_scale, loss_scale_dev, workspace, workspace_bytes, stream, grads_ready, user, drop);
}

int cpt_train_zero_grads_from(const cpt_model* m, const cpt_rel2* x, const cpt_model_grads* g, int first_stage, int Li, void* stream) {
    return zero_grads_impl(m, x, g, Li, stream, first_stage);
}

}  // extern "C"
