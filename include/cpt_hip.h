/* cpt_hip.h -- C ABI of libcpt_hip.so: the MI355X (gfx950) implementation of CPT's
 * data-parallel hot path, the Oscar/BertImg forward/backward pass that scores colour-word
 * [MASK] logits over text-token + VinVL region-feature sequences.
 *
 * The reference has no native FFI for this path: it is PyTorch eager code.  Each entry point
 * below replaces the reference Python interface cited next to it (paths relative to
 * /root/reference).  INTEGRATION.md shows the ctypes binding a maintainer adds on the
 * reference side.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     (PyTorch's caching allocator in practice) unless marked host.  The library never
 *     allocates device memory and keeps no pointer after a call returns.
 *   - every call is asynchronous on the hipStream_t passed as `stream` (void* here so the
 *     header needs no HIP include); no internal threads; the compute entry points keep no state between calls and are
 *     re-entrant.  Exceptions, all process-global and meant for A/B measurements and diagnostics only: cpt_set_tuning,
 *     cpt_prof_enable / cpt_prof_read, cpt_debug_gemm_trace.  One process drives one GPU (as torch.distributed launches the
 *     reference): kernel attributes (dynamic LDS sizes) are set once per process.
 *   - return value: CPT_OK (0) or a negative status; cpt_last_error() gives a host string for
 *     the calling thread.  No C++ exception crosses the boundary.
 *   - dtype: CPT_F32 runs every GEMM on v_mfma_f32_32x32x2_f32 (exact fp32; parity mode, matches
 *     the reference CPU path to ~1e-5); CPT_BF16 feeds bf16 operands to v_mfma_f32_32x32x16_bf16
 *     with fp32 accumulation and keeps the residual stream, LayerNorm, softmax, GELU and all
 *     reductions in fp32 (throughput mode); CPT_BF16X3 is the parity mode at MFMA-bf16 rates:
 *     every GEMM operand is split into bf16 hi + lo parts and the product a.w is computed as hi.hi + hi.lo + lo.hi
 *     (three bf16 MFMA terms, fp32 accumulate; relative error ~2^-16 per product instead of 2^-8), laid out as ONE bf16
 *     GEMM over a tripled K: activations [M][hi | hi | lo], weights [N][hi | lo | hi] (cpt_split3).  Everything
 *     outside the GEMMs runs as in CPT_F32 mode.  cpt_model_fwd takes the weight matrices of a CPT_BF16X3 model as
 *     standing split copies; cpt_train_fwd / cpt_train_bwd take them as plain fp32 (as in CPT_F32 mode: they change every
 *     step) under the tag CPT_BF16X3_MASTERS -- a descriptor of the other kind is refused, not misread -- and split both operands of every GEMM -- forward, input gradient, weight gradient -- on the spot.
 */
#ifndef CPT_HIP_H
#define CPT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPT_ABI_VERSION 8     /* 2: CPT_ATTN_MASK_3D, cpt_gemm_ln_prod3 / cpt_resid3_*, cpt_gemm_tn / cpt_gemm_nn (round 2); 3: cpt_layer_fold.w_qkv_t, cpt_retile_k32; 4: cpt_panel_pack, cpt_gemm_ln_prod3_panel (round 3); 5: cpt_train_zero_grads, cpt_batch.n_rows / mask_3d / row_seq;
                               * 6: CPT_BF16X3 in cpt_train_* (fp32 master weights there, NOT the split copies cpt_model_fwd reads under the same tag: the training step's own tag is CPT_BF16X3_MASTERS),
                               *    cpt_set_tuning / cpt_prof_* / cpt_debug_gemm_trace declared in cpt_hip_debug.h, operator-level backward entry points, cpt_comm_*;
                               * 7: cpt_adamw / cpt_adamw_ex take lr, betas, eps and weight decay as doubles (round 6);
                               * 8: cpt_outputs.loss_mean, cpt_outputs.logit_cols / n_logit_cols (round 6) */

enum { CPT_F32 = 0, CPT_BF16 = 1, CPT_BF16X3 = 2,
       CPT_BF16X3_MASTERS = 3 /* ABI 6, cpt_dims.dtype for cpt_train_* only: CPT_BF16X3 arithmetic on plain fp32 weight matrices (split per GEMM) */ };
enum { CPT_EPI_NONE = 0, CPT_EPI_GELU = 1, CPT_EPI_TANH = 2, CPT_EPI_RESID = 3 };
enum {
    CPT_OK = 0,
    CPT_ERR_SHAPE = -1,      /* unsupported / inconsistent sizes */
    CPT_ERR_DTYPE = -2,
    CPT_ERR_ALIGN = -3,      /* pointer not 16-byte aligned or K/ld not a multiple of 16 bytes */
    CPT_ERR_ARCH = -4,       /* device is not gfx950 */
    CPT_ERR_WORKSPACE = -5,  /* workspace too small */
    CPT_ERR_NULL = -6,
    CPT_ERR_HIP = -1000      /* -1000 - hipError_t */
};

int cpt_version(void);
const char* cpt_last_error(void);
/* 0 when device `dev` is gfx950, CPT_ERR_ARCH otherwise. */
int cpt_check_device(int dev);

/* ------------------------------------------------------------------------------------------
 * Model description: what BertImgModel / REC_MLM_CPT hold as nn.Module state
 * (Oscar/oscar/modeling/modeling_bert.py:153-183, modeling_rec.py:101-109).  Matrices are
 * nn.Linear layout (out x in, row-major) in the COMPUTE dtype (fp32 master tensors in CPT_F32
 * mode, a bf16 shadow in CPT_BF16 mode); vectors (biases, LayerNorm gain/shift) and the
 * embedding tables used by the gather are always fp32 -- i.e. the tensors of the state dict.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t hidden;        /* config.hidden_size (multiple of 64) */
    int32_t heads;         /* config.num_attention_heads; hidden / heads must be 64 */
    int32_t inter;         /* config.intermediate_size */
    int32_t layers;        /* config.num_hidden_layers */
    int32_t vocab;         /* config.vocab_size */
    int32_t img_dim;       /* config.img_feature_dim (2054) */
    int32_t img_dim_pad;   /* img_dim rounded up to a multiple of 8: leading dim of w_img */
    int32_t max_pos;       /* config.max_position_embeddings */
    int32_t type_vocab;    /* config.type_vocab_size */
    int32_t use_img_ln;    /* config.use_img_layernorm */
    int32_t n_rel;         /* rows of cls.seq_relationship (num_contrast_classes), 0 if absent */
    int32_t dtype;         /* CPT_F32 | CPT_BF16 | CPT_BF16X3 (matrices then are [N][3K] bf16 split copies, cpt_split3) | CPT_BF16X3_MASTERS (cpt_train_*) */
    float ln_eps;          /* config.layer_norm_eps */
    float img_ln_eps;      /* config.img_layer_norm_eps */
} cpt_dims;

typedef struct {           /* bert.encoder.layer.{i}.* */
    const void* w_qkv;     /* [3H][H]: attention.self.{query,key,value}.weight stacked */
    const float* b_qkv;    /* [3H] */
    const void* w_ao;      /* attention.output.dense.weight [H][H] */
    const float* b_ao;
    const float* ln1_g;    /* attention.output.LayerNorm.{weight,bias} */
    const float* ln1_b;
    const void* w_in;      /* intermediate.dense.weight [I][H] */
    const float* b_in;
    const void* w_out;     /* output.dense.weight [H][I] */
    const float* b_out;
    const float* ln2_g;    /* output.LayerNorm.{weight,bias} */
    const float* ln2_b;
} cpt_layer;

typedef struct {           /* optional LayerNorm-folded operands of layer i (CPT_BF16 only) */
    const void* w_qkv_f;   /* [3H][H] bf16 = output.LayerNorm.weight of layer i-1 (columns) * w_qkv; NULL for layer 0 */
    const float* c_qkv;    /* [3H] sum_k w_qkv_f[n][k] */
    const float* d_qkv;    /* [3H] sum_k output.LayerNorm.bias(i-1)[k] * w_qkv[n][k] + b_qkv[n] */
    const void* w_in_f;    /* [I][H] bf16 = attention.output.LayerNorm.weight of layer i * w_in */
    const float* c_in;     /* [I] */
    const float* d_in;     /* [I] */
    const void* w_qkv_t;   /* ABI 3, optional (NULL: not used): K-tile-major copy [H / 32][3H][32] bf16 (cpt_retile_k32) of the QKV weight this
                            * layer's fused QKV + attention launch reads -- w_qkv_f, or the plain w_qkv for layer 0 */
} cpt_layer_fold;

typedef struct {
    cpt_dims dims;
    const float* word_emb;   /* bert.embeddings.word_embeddings.weight [V][H] fp32 */
    const float* pos_emb;    /* position_embeddings.weight [P][H] */
    const float* type_emb;   /* token_type_embeddings.weight [T][H] */
    const float* emb_ln_g;   /* embeddings.LayerNorm */
    const float* emb_ln_b;
    const void* w_img;       /* bert.img_embedding.weight padded to [H][img_dim_pad], compute dtype */
    const float* b_img;
    const float* img_ln_g;   /* bert.LayerNorm (NULL unless use_img_ln) */
    const float* img_ln_b;
    const cpt_layer* layers; /* HOST array of dims.layers entries */
    const void* w_pool;      /* bert.pooler.dense [H][H] */
    const float* b_pool;
    const void* w_tr;        /* cls.transform.dense [H][H] */
    const float* b_tr;
    const float* tr_ln_g;    /* cls.transform.LayerNorm */
    const float* tr_ln_b;
    const void* w_dec;       /* cls.decoder.weight [V][H] (tied word embeddings), compute dtype */
    const float* b_dec;      /* cls.bias [V] */
    const void* w_rel;       /* cls.seq_relationship.weight [n_rel][H] compute dtype, or NULL */
    const float* b_rel;
    const cpt_layer_fold* fold; /* HOST array of dims.layers entries, or NULL: with it (and CPT_BF16) the encoder's
                                 * LayerNorms are folded into the GEMMs around them instead of running as kernels */
} cpt_model;

/* One batch as the reference drivers hand it to the model
 * (Oscar/oscar/zeroshot/refcoco_cpt.py:213-218): int64 ids / mask, fp32 region features. */
typedef struct {
    int32_t B, Lt, Li;            /* sequences, text length (70), region slots (50); L = Lt + Li */
    const int64_t* input_ids;     /* [B][Lt] */
    const int64_t* token_type;    /* [B][Lt] or NULL (zeros) */
    const int64_t* position_ids;  /* [B][Lt] or NULL (arange) */
    const int64_t* attn_mask;     /* [B][L] 1 = attend, or NULL (ones) */
    const float* img_feats;       /* [B][Li][img_dim] fp32, or NULL when Li == 0 */
    const int64_t* mask_pos;      /* [B] position of [MASK] per sequence (rows mode) or NULL */
    const int64_t* labels;        /* rows mode: [B] target id (-1 ignored); all-rows: [B][L]; or NULL */
    /* ABI 5, training only (0 / NULL: one labelled position per sequence, as above): an arbitrary label grid
     * (masked_lm_labels of modeling_rec.py:147-150 with any number of labelled positions per sequence) as n_rows labelled
     * positions -- position mask_pos[r] of sequence row_seq[r] carries labels[r]; the MLM head, the loss and o->logits
     * [n_rows][V] run over those rows (cpt_train_workspace_bytes_rows sizes the workspace) */
    int32_t n_rows;
    int32_t mask_3d;              /* ABI 5, training only: 1 = attn_mask is [B][L][L], one mask row per query (modeling_bert.py:215-216; inference
                                   * passes CPT_ATTN_MASK_3D instead); the attention backward then runs its generic kernel */
    const int64_t* row_seq;       /* [n_rows] sequence index of every labelled row, ascending; NULL with n_rows = 0 */
} cpt_batch;

enum {
    CPT_OUT_SEQ = 1,        /* sequence_output [B][L][H] fp32 (BertImgModel.forward()[0]) */
    CPT_OUT_POOLED = 2,     /* pooled_output [B][H] fp32 (modeling_bert.py:275) */
    CPT_OUT_MASK_LOGITS = 4,/* prediction scores of the [MASK] rows only [B][V] fp32 */
    CPT_OUT_ALL_LOGITS = 8, /* prediction scores of every position [B][L][V] (modeling_rec.py:143) */
    CPT_OUT_LOSS = 16,      /* CrossEntropy(ignore_index=-1) (modeling_rec.py:147-150) */
    CPT_OUT_REL = 32,       /* cls.seq_relationship(pooled) [B][n_rel] (modeling_vcr.py NSPCPT) */
    CPT_ATTN_MASK_3D = 256  /* input flag: cpt_batch.attn_mask is [B][L][L], one mask row per query (modeling_bert.py:215-216);
                               inference only, attention runs as its own kernel (no QKV fusion) */
};  /* (training keeps its activations through cpt_train_fwd / cpt_train_bwd below, not through a flag here) */

typedef struct {
    float* seq;          /* CPT_OUT_SEQ */
    float* pooled;       /* CPT_OUT_POOLED */
    float* logits;       /* CPT_OUT_MASK_LOGITS [B][V] or CPT_OUT_ALL_LOGITS [B][L][V] */
    float* loss;         /* CPT_OUT_LOSS: [2] = {sum of labelled-row losses, labelled-row count} */
    float* rel;          /* CPT_OUT_REL */
    float* loss_mean;    /* ABI 8, cpt_train_fwd(_ex) only, optional (NULL: not written): [1] = loss[0] / loss[1], the value REC_MLM_CPT.forward /
                          * NSPCPT.forward return (modeling_rec.py:147-150, modeling_vcr.py:126-128), written by the cross-entropy launch itself so that
                          * the host needs no divide kernel behind the forward; cpt_model_fwd ignores the field */
    const int64_t* logit_cols;   /* ABI 8, cpt_model_fwd with CPT_OUT_MASK_LOGITS only, optional (NULL: every column): DEVICE list of n_logit_cols vocabulary ids;
                                  * `logits` is then [B][n_logit_cols] -- the scores of those columns only, in list order.  What the zero- / few-shot
                                  * drivers read of the [B][V] scores is a handful of colour-token columns (zeroshot/refcoco_cpt.py:219,
                                  * fewshot/refcoco_cpt.py:272-291, gqa_cpt.py:598-600): the 47 MB decoder table is not streamed and B x V floats are not written.
                                  * Not with CPT_OUT_LOSS / CPT_OUT_ALL_LOGITS (CPT_ERR_SHAPE).  Ids outside [0, V) are the caller's bug (clamped, never a fault) */
    int64_t n_logit_cols;
} cpt_outputs;

/* Workspace the caller must supply for cpt_model_fwd with these flags (bytes). */
size_t cpt_fwd_workspace_bytes(const cpt_dims* d, int B, int Lt, int Li, int flags);

/* REC_MLM_CPT.forward / BertImgModel.forward (modeling_rec.py:137-152, modeling_bert.py:199-279):
 * embeddings + region projection written into one [B][L][H] buffer, N encoder layers, then the
 * outputs selected by `flags`. */
int cpt_model_fwd(const cpt_model* m, const cpt_batch* b, const cpt_outputs* o, int flags,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * MLM head on a list of rows with the full-vocabulary normaliser (Oscar/oscar/fewshot/vg_cpt.py:271-290: several [MASK]
 * rows per sequence, a softmax over all V columns of each, a handful of columns read).  Added beside ABI 8, no struct changed.
 * ---------------------------------------------------------------------------------------- */
/* Workspace of cpt_model_fwd_rows (bytes); n_cols = 0 sizes the call without a column list. */
size_t cpt_fwd_rows_workspace_bytes(const cpt_dims* d, int B, int Lt, int Li, int n_rows, int n_cols);

/* Inference (CPT_F32, CPT_BF16, CPT_BF16X3): encoder as cpt_model_fwd, then the MLM head on b->n_rows (> 0) rows -- row r is position
 * b->mask_pos[r] of sequence b->row_seq[r] (ascending; a sequence may have any number of rows, none included).  b->labels is ignored;
 * b->mask_3d = 1 means attn_mask is [B][L][L] (as CPT_ATTN_MASK_3D).
 *   logits  [n_rows][n_cols]: the scores of the DEVICE column list `cols` (vocabulary ids, list order, duplicates allowed);
 *           cols == NULL: [n_rows][V], every column.
 *   row_lse [n_rows] or NULL: natural-log log-sum-exp of the row's scores over all V columns (with a column list the [n_rows][V] scores
 *           live in the workspace, cpt_fwd_rows_workspace_bytes).
 * CPT_ERR_SHAPE: n_rows <= 0, row_seq not ascending or outside [0, B), mask_pos outside [0, L), n_cols > V, a column id outside [0, V).
 * The call reads row_seq, mask_pos and cols back to the host to check them (it waits for `stream` once; not for graph capture). */
int cpt_model_fwd_rows(const cpt_model* m, const cpt_batch* b, const int64_t* cols, int n_cols, float* logits, float* row_lse,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Mean log-probability of candidate word-piece lists over k-[MASK] templates (vg_cpt.py:283-289):
 *   out[g][c] = (1 / len) sum_{j < len} (logits[(s + j) * n_cols + cand_cols[c * K + j]] - row_lse[s + j]),
 *   len = cand_len[c], s = slot_row[g * K + len - 1]: the first head row of group g's len-mask template.
 * len == 0 gives 0 (the background slot); s < 0, s + len > n_rows or a cand_cols entry outside [0, n_cols) gives NaN (never read).
 * logits [n_rows][n_cols], row_lse [n_rows], slot_row [G][K], cand_cols [C][K], cand_len [C] (int32), out [G][C]; all device. */
int cpt_mean_logprob_scores(const float* logits, int n_cols, int n_rows, const float* row_lse, const int32_t* slot_row, int G, int K,
                            const int32_t* cand_cols, const int32_t* cand_len, int C, float* out, void* stream);

/* VG Recall@K ranks (Oscar/oscar/utils/vg_eval.py eval_vg), one launch for a whole split; added beside ABI 8, no struct changed.
 * Images come as CSR tables (int32, device):
 *   cand_off [n_img + 1], cand [n_cand][3] = (subject, object, score row): the image's candidates in the reference's dict order;
 *     score row -1 (or any row outside [0, n_rows)) is the all-zero dummy row of an image without predictions;
 *   gt_off [n_img + 1], gt [n_gt][3] = (subject, object, predicate): the image's ground-truth triplets.
 *   scores [n_rows][C] fp32 (device, C >= 2).
 * Per candidate rel = argmax(row[1:]) + 1 (first maximum; NaN counts as the maximum) and score = row[rel]; per image the candidates
 * are ranked by score, descending, ties by candidate order, NaN first (a stable torch.sort(descending=True)).
 * out_rank [n_gt]: the rank of the candidate with the triplet's (subject, object) whose rel equals its predicate, INT32_MAX if there is
 * none (hit@K = rank < K); -1 if the image's offsets are inconsistent or the workspace is too small for it.
 * Images with more candidates than the LDS tile are ranked through `workspace`: cpt_vg_recall_workspace_bytes sizes it from the HOST
 * copy of cand_off (0 when every image fits the tile; workspace may then be NULL). */
size_t cpt_vg_recall_workspace_bytes(const int32_t* cand_off, int n_img);
int cpt_vg_recall_ranks(const float* scores, int n_rows, int C, const int32_t* cand_off, const int32_t* cand, int n_cand, const int32_t* gt_off,
                        const int32_t* gt, int n_gt, int n_img, int32_t* out_rank, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * VCR Q->AR (Oscar/oscar/modeling/modeling_vcr.py:194-251 VCRQAR_NSPCPT, fewshot/vcr_qar_nsp_cpt.py): two relation heads on ONE batch.
 * Added beside ABI 8, no struct changed.  Rows [0, B0) are the Q->A sequences and go through head 0 (cpt_model.w_rel / b_rel, cls_ans), rows
 * [B0, B) are the QA->R sequences and go through head 1 (cpt_rel2.w_rel1 / b_rel1, cls_rat); the encoder and the pooler run once over all B
 * rows.  B0 = B or B0 = 0 is a single-head batch (forward(head="ans" | "rat")).  Head weights: bf16 in CPT_BF16 mode (pooled is rounded to bf16
 * where the head reads it), fp32 in every other mode (CPT_BF16X3 / CPT_BF16X3_MASTERS included); n_rel <= 64.
 * Loss: CrossEntropyLoss(ignore_index=-1) per group, loss = mean over group 0 + mean over group 1 (the driver's q_a_loss + qa_r_loss); a group
 * without rows adds nothing, a group whose rows are all ignored gives NaN.  Labels must lie in [-1, n_rel) (CPT_ERR_SHAPE otherwise): they are
 * checked on the host from labels_host when given, else read back once (the call then waits for its stream).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B0;                  /* rows of head 0: 0 <= B0 <= B */
    const void* w_rel1;          /* head 1 [n_rel][H] (dtype as above) */
    const float* b_rel1;         /* [n_rel] */
    float* g_w_rel1;             /* cpt_train_bwd_rel2: head 1's weight gradient (WRITTEN, as g->w_rel) */
    float* g_b_rel1;             /* cpt_train_bwd_rel2: head 1's bias gradient (ACCUMULATED, as g->b_rel; cpt_train_zero_grads_rel2 clears it) */
    float* score;                /* optional [B] output: 1 - softmax(rel[s])[1], the choice score of evaluate() (vcr_qar_nsp_cpt.py:641,650) */
    const int64_t* labels_host;  /* optional HOST copy of the [B] labels, for the range check without a stream wait */
} cpt_rel2;

/* Workspace of cpt_rel2_scores (bytes): B row losses + the finish ticket.  The ticket word must hold 0 before the first call (a zeroed
 * workspace); every call leaves it 0. */
size_t cpt_rel2_workspace_bytes(int B);
/* The two heads on pooled rows [B][H] fp32 (cpt_model_fwd with CPT_OUT_POOLED), one launch: rel [B][n_rel]; score [B] (optional, n_rel >= 2);
 * with labels [B] (device, optional): loss [2] = {group-0 mean, group-1 mean} and loss_mean [1] = their sum (either may be NULL), dlogits
 * [B][n_rel] (optional) = d loss / d rel.  dtype: CPT_BF16 reads bf16 weights, anything else fp32 weights. */
int cpt_rel2_scores(int dtype, const float* pooled, int B, int H, int n_rel, int B0, const void* w0, const float* b0, const void* w1, const float* b1,
                    const int64_t* labels, const int64_t* labels_host, float* rel, float* score, float* loss, float* loss_mean, float* dlogits,
                    void* workspace, size_t workspace_bytes, void* stream);
/* Q->AR choice of evaluate() (vcr_qar_nsp_cpt.py:657-676) for n_q questions, one launch: q_a [n_q][n_ans] and qa_r [n_q][n_rats] choice scores
 * (device fp32), ans_label / rat_label [n_q] (device int64).  Per question the answer argmax; the rationale argmax over all n_rats scores, or --
 * n_rats > n_ans, the 16-rationale layout -- over the slice [ans_label * n_ans : (ans_label + 1) * n_ans] of them, as written, with Python's
 * slice rules (negative bounds count from the end; an empty slice, where the reference's argmax would raise, gives -1).  torch.argmax rules: first maximum, NaN counts as the maximum.  preds [n_q][2] int64 = (answer,
 * rationale); flags [n_q][3] uint8 = (ans_label == answer, rat_label == rationale, both); counts [3] int32 (optional) += the column sums of
 * flags (device accumulation over evaluation batches). */
int cpt_vcr_qar_choose(const float* q_a, const float* qa_r, int n_q, int n_ans, int n_rats, const int64_t* ans_label, const int64_t* rat_label,
                       int64_t* preds, uint8_t* flags, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * GQA-CPT and VCR Q->A evaluation choices, and global-norm gradient clipping, on the device.  Added beside ABI 8, no struct changed.
 * torch.argmax rules throughout: the first maximum wins, NaN counts as the maximum (the first NaN wins), -0 == +0 is a tie.
 * ---------------------------------------------------------------------------------------- */
/* GQA answer choice of evaluate() (Oscar/oscar/fewshot/gqa_cpt.py:598-612) for R questions, one launch: scores [R][C] fp32 (device), the
 * [MASK]-row logits of the C answer labels in label order.  pred [R] int64 = the argmax column.  Correctness runs on string ids: piece_sid [C]
 * int32 = the id of the string the reference predicts for column c (the label's FIRST word-piece; -2 = equal to no label string), gt_sid [R][G]
 * int32 = the ids of the question's ground-truth label strings, padded with -1.  correct [R] uint8 = any g: gt_sid[r][g] >= 0 and
 * gt_sid[r][g] == piece_sid[pred[r]]; counts [1] int32 (optional) += the number of correct rows (device accumulation over batches). */
int cpt_gqa_choose(const float* scores, int R, int C, const int32_t* piece_sid, const int32_t* gt_sid, int G, int64_t* pred, uint8_t* correct,
                   int32_t* counts, void* stream);
/* VCR Q->A choice of evaluate() (fewshot/vcr_nsp_cpt.py:600-611), one launch: rel [N][n_rel] fp32 relation scores (device, n_rel >= 2), N =
 * n_q * interval sequences (CPT_ERR_SHAPE when interval does not divide N), labels [n_q] int64 (device).  scores [N] = 1 - softmax(rel[i])[1] in
 * fp32 (NaN when the row holds one); pred [n_q] int64 = the argmax inside the question's interval; correct [n_q] uint8 = pred == label; counts
 * [1] int32 (optional) += the number of correct questions. */
int cpt_nsp_choose(const float* rel, int N, int n_rel, int interval, const int64_t* labels, float* scores, int64_t* pred, uint8_t* correct,
                   int32_t* counts, void* stream);
/* torch.nn.utils.clip_grad_norm_(max_norm, error_if_nonfinite=False) on one flat fp32 buffer g [n] (device), in place, two launches and no host
 * synchronisation.  Launch 1 writes per-workgroup partial sums of squares; the last workgroup to finish adds them in index order (the same
 * buffer gives the same norm bit for bit) and writes out [2] fp32 (device) = {norm, coef}, coef = min(1, max_norm / (norm + 1e-6)): a NaN norm
 * gives a NaN coefficient, an infinite norm gives 0.  With sq_in (device double, optional) the norm is sqrt(*sq_in) -- a sum of squares formed
 * elsewhere, e.g. all-reduced over the shards of a data-parallel gradient -- and g is only scaled.  Launch 2 multiplies g by coef (always, also
 * when coef == 1, as torch does).  workspace: cpt_grad_clip_workspace_bytes() bytes (device); its first word is the finish ticket, which must
 * hold 0 before the first call (a zeroed workspace) and is left 0 by every call. */
size_t cpt_grad_clip_workspace_bytes(void);
int cpt_grad_clip(float* g, size_t n, float max_norm, const double* sq_in, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Length-aware evaluation: trim a padded batch to the part any sequence attends to.  Added beside ABI 8, no struct changed.
 * A position whose mask column is 0 in every sequence of the batch is never a key, and its own row is read by no head-row output ([MASK]
 * rows, [CLS] row): dropping it changes only the order of the sums.  Not for outputs that return every position or 3-D masks; training steps
 * take the entries further down (cpt_train_extents).
 * ---------------------------------------------------------------------------------------- */
/* out [2] int32 (device) = {Lt', Li'} of attn_mask [B][Lt + Li] int64 (device): per part (text: columns [0, Lt), regions: [Lt, Lt + Li)) 1 +
 * the last column that is non-zero in any sequence, 0 when there is none -- no prefix form assumed, a hole stays inside.  Lt' >= 1 always.
 * mask_pos [n_pos] int64 (device, optional): head-row positions in [0, Lt + Li); a text position p gives Lt' >= p + 1, a region position keeps
 * the text whole (Lt' = Lt) and gives Li' >= p - Lt + 1, a position outside the sequence keeps both parts whole.  One memset node and one
 * launch, integer max only (the result does not depend on the order of arrival), no host work. */
int cpt_batch_extents(const int64_t* attn_mask, int B, int Lt, int Li, const int64_t* mask_pos, int n_pos, int32_t* out, void* stream);
/* One launch: the contiguous copies input_ids_out / token_type_out / position_ids_out [B][Lt_out] (columns [0, Lt_out) of the [B][Lt] inputs;
 * token_type and position_ids optional, each with its output), attn_mask_out [B][Lt_out + Li_out] (text columns [0, Lt_out), then region columns
 * [Lt, Lt + Li_out) of the [B][Lt + Li] mask) and img_feats_out [B][Li_out][img_dim] fp32 (regions [0, Li_out) of [B][Li][img_dim]; not touched
 * when Li_out == 0).  1 <= Lt_out <= Lt, 0 <= Li_out <= Li.  Feature rows move as 16-byte accesses from 8-byte boundaries when img_dim is even. */
int cpt_trim_batch(const int64_t* input_ids, const int64_t* token_type, const int64_t* position_ids, const int64_t* attn_mask, const float* img_feats,
                   int B, int Lt, int Li, int img_dim, int Lt_out, int Li_out, int64_t* input_ids_out, int64_t* token_type_out,
                   int64_t* position_ids_out, int64_t* attn_mask_out, float* img_feats_out, void* stream);
/* Length-aware TRAINING (added beside ABI 8): the same cut is exact for a training step -- a column no sequence attends to is never a key, no
 * head row reads its row, so the gradient entering it is exactly zero and it adds exact zeros to every weight gradient, column sum and table
 * row -- provided every labelled position stays.
 * cpt_train_extents: out [2] int32 (device) = {Lt', Li'} of attn_mask as cpt_batch_extents defines them, widened by what the loss reads: either
 * label_grid [B][Lt + Li] int64 (device, optional; -1 = no label, any other entry labels its column) or positions [n_pos] int64 (device, optional:
 * the mask_pos / (row_seq, position) list of the training step; row_seq is not needed, only the columns count), or neither (relation heads: the
 * loss reads [CLS] only).  A labelled column follows the head-row rule of cpt_batch_extents: text column p gives Lt' >= p + 1 (so Lt' > every
 * labelled text position and no position moves), a region column keeps the text whole.  ONE launch of ONE workgroup, no memset node, no atomic:
 * 16-byte reads along L, wave reductions, one combine in wave order.  Sized for few-shot training batches (4 x 210 entries): the one workgroup
 * walks all B x (Lt + Li) entries, so the time grows linearly with the batch -- evaluation batches of hundreds of sequences use cpt_batch_extents. */
int cpt_train_extents(const int64_t* attn_mask, int B, int Lt, int Li, const int64_t* label_grid, const int64_t* positions, int n_pos, int32_t* out,
                      void* stream);
/* cpt_trim_batch with a label grid: label_grid_out [B][Lt_out + Li_out] holds text columns [0, Lt_out) and region columns [Lt, Lt + Li_out) of
 * label_grid [B][Lt + Li], exactly as attn_mask_out is cut from attn_mask (the same copy loop, the same launch). */
int cpt_trim_batch_labels(const int64_t* input_ids, const int64_t* token_type, const int64_t* position_ids, const int64_t* attn_mask,
                          const float* img_feats, const int64_t* label_grid, int B, int Lt, int Li, int img_dim, int Lt_out, int Li_out,
                          int64_t* input_ids_out, int64_t* token_type_out, int64_t* position_ids_out, int64_t* attn_mask_out, float* img_feats_out,
                          int64_t* label_grid_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Device-resident evaluation sets.  Added beside ABI 8; no existing struct changed.
 * An evaluation split is uploaded ONCE as packed tables; every step's padded or trimmed batch is then built by one launch from a list of sequence
 * indices, so that a pass uploads nothing but that list.  All pointers are device pointers.
 * Sequences: n_seq sequences with the global indices [seq_base, seq_base + n_seq) (a data-parallel rank stores its shard only), padded Lt + Li:
 *   ids [n_seq][Lt] int32, seg [n_seq][Lt] uint8, mask [n_seq][Lt + Li] uint8 (entries 0 / 1), mask_pos [n_seq] int32 (may be NULL when no call
 *   asks for mask_pos_out), feat_block [n_seq] int32: the block that holds the sequence's region features.
 * Blocks: block b holds block_rows[b] (0 .. Li) feature rows, the rows [block_off[b], block_off[b] + block_rows[b]) of feats; a region at or behind
 *   block_rows reads as +0.0.  Sequences that share their features (the proposals of one image) name the same block.
 * feats [n_rows][pitch] of feat_dtype CPT_F32 or CPT_BF16, img_dim <= pitch, the columns behind img_dim zero (cpt_pad_cast writes a chunk of
 *   fp32 rows into exactly this form).  With feats 16-byte aligned, pitch a multiple of 16 bytes and img_dim even a lane moves 16 bytes per load
 *   and per store; otherwise one element.  The three feature tables may be NULL when Li is 0.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    const void* feats;
    const int32_t* ids; const uint8_t* seg; const uint8_t* mask; const int32_t* mask_pos; const int32_t* feat_block;
    const int32_t* block_rows; const int64_t* block_off;
    int64_t n_rows;
    int32_t feat_dtype, pitch, img_dim, Lt, Li, n_seq, seq_base, n_blocks;
} cpt_resident_store;
/* One launch on `stream`: batch row b is sequence seq_idx[b] (seq_idx [B] int32 on the device: global indices, any order, repeats allowed).
 * Writes what trimming the concatenated host batch gives (cpt_trim_batch): input_ids_out / token_type_out [B][Lt_out] int64 (text columns
 * [0, Lt_out)), attn_mask_out [B][Lt_out + Li_out] int64 (text columns [0, Lt_out), then region columns [Lt, Lt + Li_out)), mask_pos_out [B] int64
 * (or NULL), img_feats_out [B][Li_out][img_dim] fp32 (a bf16 store widened exactly; not touched when Li_out == 0).  1 <= Lt_out <= Lt,
 * 0 <= Li_out <= Li.  EVERY element of every output is written, so the outputs need no initialisation.  The caller validates seq_idx; the kernel
 * clamps an index outside the store (and a block index or block offset outside the tables) and never reads outside the store.
 * CPT_ERR_SHAPE / CPT_ERR_NULL / CPT_ERR_ALIGN / CPT_ERR_DTYPE as cpt_trim_batch. */
int cpt_gather_batch(const cpt_resident_store* store, const int32_t* seq_idx, int B, int Lt_out, int Li_out, int64_t* input_ids_out,
                     int64_t* token_type_out, int64_t* attn_mask_out, int64_t* mask_pos_out, float* img_feats_out, void* stream);
/* Head tables of a resident set, beside cpt_resident_store (added beside ABI 8; no existing struct, entry point or kernel changed): the rows a
 * head reads and their labels, for sets whose sequences hold 0, 1 or several [MASK] rows (VG pairs: 1, 2 or 3), one label per sequence (the
 * relation heads of VCR) or a label grid (the MLM training loops).  All pointers are device pointers; the sequences are the store's, in its order. */
typedef struct {
    const int32_t* head_first;  /* [n_seq + 1]: sequence s owns head rows [head_first[s], head_first[s + 1]) ; counts may be 0 */
    const int32_t* head_pos;    /* [n_heads] position in the PADDED sequence, 0 .. Lt + Li - 1 */
    const int32_t* head_label;  /* [n_heads] label id, -1 = ignored; NULL when the set has no row labels */
    const int32_t* seq_label;   /* [n_seq] one label per sequence (NSP heads); NULL when absent */
    int32_t n_heads;
} cpt_resident_heads;
/* cpt_gather_batch with up to four more outputs, still ONE launch; the five outputs of cpt_gather_batch are written as it writes them.
 * row_first [B + 1] int32 on the device: the exclusive prefix sum of the head counts of the batch's sequences (the host knows it from its tables
 * and sends it with the index lists); R = row_first[B].  Each of the four outputs may be NULL; EVERY element of every other one is written:
 *   head_rows_out   [R][2] int64: row row_first[b] + k = (b, position) of the k-th head row of sequence seq_idx[b] -- the (n, 2) (sequence, position)
 *                   rows cpt_model_fwd_rows takes.  Positions are those of the PADDED sequence, not remapped: the caller chooses Lt_out > p for a
 *                   text position p and Lt_out == Lt when a region position is read (the rule of cpt_batch_extents).
 *   head_labels_out [R] int64: the rows' labels.
 *   label_grid_out  [B][Lt_out + Li_out] int64: -1, and head_label at the row's head positions; cut exactly as attn_mask_out is cut (text column c
 *                   is padded column c, region column Lt_out + j is padded column Lt + j), by the workgroups that write attn_mask_out.
 *   seq_label_out   [B] int64.
 * Indices read from memory are clamped (the sequence, head_first against n_heads, a position against Lt + Li, row_first against R): nothing is read
 * or written outside the arrays.  Error codes as cpt_gather_batch; CPT_ERR_NULL too for an output whose table is NULL (head_label for
 * head_labels_out and label_grid_out, seq_label for seq_label_out, row_first for the row outputs). */
int cpt_gather_batch_heads(const cpt_resident_store* store, const cpt_resident_heads* heads, const int32_t* seq_idx, const int32_t* row_first, int B,
                           int R, int Lt_out, int Li_out, int64_t* input_ids_out, int64_t* token_type_out, int64_t* attn_mask_out,
                           int64_t* mask_pos_out, float* img_feats_out, int64_t* head_rows_out, int64_t* head_labels_out, int64_t* label_grid_out,
                           int64_t* seq_label_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Few-shot training step (Oscar/oscar/fewshot/refcoco_cpt.py:231-249): forward that keeps the
 * activations, backward into caller-owned fp32 gradient tensors laid out like the parameters,
 * fused AdamW.  [MASK]-rows mode only (the loss of modeling_rec.py:147-150 sees only those rows).
 * The plain forms run without dropout; the _ex forms below take the dropout description.
 * ---------------------------------------------------------------------------------------- */
typedef struct {           /* gradients of cpt_layer, all fp32, same shapes */
    float* w_qkv; float* b_qkv; float* w_ao; float* b_ao; float* ln1_g; float* ln1_b;
    float* w_in; float* b_in; float* w_out; float* b_out; float* ln2_g; float* ln2_b;
} cpt_layer_grads;

typedef struct {           /* gradients of cpt_model: the MLM-head fields (w_tr .. b_dec) or the NSP-head fields (w_pool .. b_rel) */
    float* word_emb;       /* [V][H]: tied table, decoder + embedding-lookup contributions */
    float* pos_emb; float* type_emb; float* emb_ln_g; float* emb_ln_b;
    float* w_img;          /* [H][img_dim] (unpadded) */
    float* b_img; float* img_ln_g; float* img_ln_b;
    const cpt_layer_grads* layers;   /* HOST array */
    float* w_tr; float* b_tr; float* tr_ln_g; float* tr_ln_b; float* b_dec;
    float* w_pool; float* b_pool;    /* NSP head (model without w_tr / w_dec but with w_pool and w_rel): bert.pooler.dense */
    float* w_rel; float* b_rel;      /* ... and the relation Linear [n_rel][H] (NSPCPT.cls, modeling_vcr.py:90-92) */
} cpt_model_grads;

size_t cpt_train_workspace_bytes(const cpt_dims* d, int B, int Lt, int Li);
size_t cpt_train_workspace_bytes_rows(const cpt_dims* d, int B, int Lt, int Li, int n_rows);   /* with cpt_batch.n_rows labelled rows (0: B) */
/* forward: o->logits [B][V] and o->loss[2] = {sum of row losses, labelled-row count} are written;
 * b->mask_pos and b->labels ([B], -1 = ignored) are required.
 * A model WITHOUT the MLM head (w_tr, w_dec NULL) but with w_pool and w_rel trains the NSP-CPT head instead
 * (NSPCPT.forward, modeling_vcr.py:115-129; fewshot/vcr_nsp_cpt.py:425-470): pooled [CLS] -> tanh -> Linear(H, n_rel) ->
 * CrossEntropyLoss(ignore_index=-1) over b->labels [B]; o->rel [B][n_rel] is written instead of o->logits, b->mask_pos is not used. */
int cpt_train_fwd(const cpt_model* m, const cpt_batch* b, const cpt_outputs* o, void* workspace,
                  size_t workspace_bytes, void* stream);
/* backward of loss = loss_scale * mean over labelled rows; uses the workspace cpt_train_fwd filled.
 * WRITE / ACCUMULATE contract of g's tensors (ABI 5):
 *   WRITTEN whole by every call (previous contents ignored, never added to): every Linear weight gradient -- w_qkv, w_ao, w_in, w_out of each
 *     layer, w_img and the weights of the model's head (w_tr, or w_pool and w_rel) -- and, with the MLM head, the tied word-embedding / decoder table (decoder gradient written, lookup
 *     gradients added behind it);
 *   ACCUMULATED into with atomics (must hold zeros, or whatever the caller wants added to): every bias and LayerNorm gain / shift vector, the
 *     position and token-type tables, and the word table when the model has no MLM head.
 *   LEFT UNTOUCHED: with the MLM head, w_pool and w_rel -- the pooler and the relation head take no part in that loss, so neither cpt_train_bwd
 *     nor cpt_train_zero_grads writes these two tensors; a caller that reads them must clear them itself.
 * cpt_train_zero_grads clears exactly the second group.  A caller that accumulates micro-batches must therefore ADD the written tensors
 * itself between calls (cpt_amd/train.py keeps a copy and adds it); skipping the zero launch sums the vectors but OVERWRITES the matrices. */
int cpt_train_bwd(const cpt_model* m, const cpt_batch* b, const cpt_model_grads* g, float loss_scale,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Clears what cpt_train_bwd ADDS into -- the bias / LayerNorm gradient vectors and the small embedding tables (atomic
 * accumulation), plus any table the model's head does not overwrite -- in one launch.  Linear weight gradients (and, with the MLM
 * head, the tied word-embedding table) are WRITTEN by cpt_train_bwd, so a caller that runs this before every backward never
 * clears them: 0.3 MB per step instead of the whole 447 MB gradient buffer (replaces optimizer.zero_grad(),
 * Oscar/oscar/fewshot/refcoco_cpt.py:247-249).  Li = region slots of the batch that follows (0: w_img is cleared too). */
int cpt_train_zero_grads(const cpt_model* m, const cpt_model_grads* g, int Li, void* stream);
/* Data-parallel fine-tuning (the reference wraps the model in DistributedDataParallel, whose bucketed gradient
 * all-reduce overlaps backward: Oscar/oscar/fewshot/refcoco_cpt.py:516-522).  The parameters form
 * dims.layers + 2 BUCKETS: 0 = embedding tables + embeddings.LayerNorm + region projection (+ its LayerNorm),
 * 1 + l = encoder layer l, dims.layers + 1 = pooler + MLM head.  The _ex forms call back on the HOST, from inside
 * the call, on the calling thread:
 *   cpt_train_fwd_ex: before_bucket(user, k) BEFORE the first launch that reads bucket k's parameters is enqueued
 *                     (order 0, 1 .. layers, layers + 1) -- the caller makes `stream` wait for k's parameter all-gather;
 *   cpt_train_bwd_ex: grads_ready(user, k) AFTER the last launch that writes bucket k's gradients is enqueued
 *                     (order layers + 1, layers .. 1, 0) -- the caller records an event on `stream` and starts
 *                     bucket k's reduce-scatter on its communication stream while backward continues.
 * The library itself owns no communicator: collectives stay in torch.distributed (RCCL).  NULL callbacks = the plain forms. */
typedef void (*cpt_bucket_fn)(void* user, int bucket);

/* Dropout of the training step (reference: nn.Dropout at modeling_bert.py:57 on the attention probabilities, :266 on the
 * region embeddings, and inside BertEmbeddings / BertSelfOutput / BertOutput; p = config.hidden_dropout_prob /
 * attention_probs_dropout_prob, --drop_out 0.1 in fewshot/refcoco_cpt.py:387,509-512).  Masks are never stored: forward
 * and backward regenerate them from Philox4x32-10 keyed by `seed` with the counter (element block, step, site), so a mask
 * is a pure function of (seed, step, site, element) whatever the tile shapes or the number of GPUs.  Pass the SAME
 * struct to the forward and the backward of a step; ranks of a data-parallel job use different seeds (their batches
 * differ).  NULL, or both probabilities 0, runs exactly the dropout-free kernels.  The rate actually applied is p rounded
 * to 2^-32 (hidden) / 2^-16 (attention), and kept values are scaled by 1 / (1 - that rate). */
typedef struct {
    float p_hidden;      /* embeddings, region embeddings, BertSelfOutput, BertOutput */
    float p_attn;        /* attention probabilities */
    uint64_t seed;
    uint64_t step;       /* training step: a fresh mask every step */
} cpt_dropout;
/* Keep-mask of one dropout site (tests / oracle): site 0 = embeddings; layer l: 1 + 3l attention probabilities,
 * 2 + 3l BertSelfOutput, 3 + 3l BertOutput.  is_attn 0: out[n0 = rows][n1 = hidden]; 1: out[n0 = B*heads][n1 = L][n2 = L].
 * out[i] = 1 keep / 0 drop. */
int cpt_dropout_mask(const cpt_dropout* drop, int site, int is_attn, unsigned char* out, int n0, int n1, int n2, void* stream);

int cpt_train_fwd_ex(const cpt_model* m, const cpt_batch* b, const cpt_outputs* o, void* workspace,
                     size_t workspace_bytes, void* stream, cpt_bucket_fn before_bucket, void* user, const cpt_dropout* drop);
/* loss_scale_dev (optional): DEVICE scalar multiplied into loss_scale -- autograd's incoming gradient of the loss
 * without a host synchronisation. */
int cpt_train_bwd_ex(const cpt_model* m, const cpt_batch* b, const cpt_model_grads* g, float loss_scale,
                     const float* loss_scale_dev, void* workspace, size_t workspace_bytes, void* stream,
                     cpt_bucket_fn grads_ready, void* user, const cpt_dropout* drop);
/* VCR Q->AR (cpt_rel2 above): the training step of VCRQAR_NSPCPT: cpt_train_fwd_ex / cpt_train_bwd_ex / cpt_train_zero_grads with the NSP head (model without the MLM head,
 * with w_pool and w_rel) and the second head in `x`; same workspace (cpt_train_workspace_bytes), dropout, bucket callbacks and write / accumulate
 * contract.  The forward writes o->rel [B][n_rel], o->loss [2] = the two group means, o->loss_mean [1] = their sum (optional), x->score (optional).
 * The backward is that of loss_scale (* *loss_scale_dev) times the summed loss; head 0's gradients go to g->w_rel / g->b_rel, head 1's to
 * x->g_w_rel1 / x->g_b_rel1, the pooler's and the encoder's as in cpt_train_bwd. */
int cpt_train_fwd_rel2(const cpt_model* m, const cpt_rel2* x, const cpt_batch* b, const cpt_outputs* o, void* workspace, size_t workspace_bytes,
                       void* stream, cpt_bucket_fn before_bucket, void* user, const cpt_dropout* drop);
int cpt_train_bwd_rel2(const cpt_model* m, const cpt_rel2* x, const cpt_batch* b, const cpt_model_grads* g, float loss_scale,
                       const float* loss_scale_dev, void* workspace, size_t workspace_bytes, void* stream, cpt_bucket_fn grads_ready, void* user,
                       const cpt_dropout* drop);
int cpt_train_zero_grads_rel2(const cpt_model* m, const cpt_rel2* x, const cpt_model_grads* g, int Li, void* stream);

/* ------------------------------------------------------------------------------------------
 * Soft-template prompt tuning (Oscar/oscar/explore/sgd_to_explore_template.py:26-66 TemplateEmbedding, :389-426 its loop): a trainable
 * table tmpl [n_slots][H] fp32 whose rows 1 .. n_slots - 1 REPLACE the word-embedding rows of the ids 1 .. n_slots - 1 ([unused0] ..)
 * in the text-embedding lookup, while the model itself stays fixed.  Added beside ABI 8, no struct changed.
 *   forward: a text position whose id satisfies 0 < id < n_slots reads its word row from tmpl[id] instead of word_emb[id]; id 0 (padding)
 *     and ids >= n_slots are untouched, tmpl[0] is never read; everything behind the lookup -- and the tied decoder table -- is unchanged.
 *     A NULL struct or tmpl == NULL runs the plain entry point.
 *   cpt_train_bwd_soft: the backward of a FROZEN model -- the data-gradient chain only (head, LayerNorm backwards, data-gradient GEMMs with
 *     the GELU gradient, attention backward, dropout and residual handling as cpt_train_bwd_ex), no weight-gradient GEMM, no bias /
 *     LayerNorm / table column sum, nothing on the region side -- ending in the gradient of the template.
 *     WRITE contract: g_tmpl [n_slots][H] fp32 is WRITTEN WHOLE by every call (previous contents ignored; row 0 and the rows of slots no
 *     position uses are exactly zero), and NOTHING ELSE outside the workspace is written: there is no cpt_model_grads and no zero launch.
 *     A caller that accumulates micro-batches adds g_tmpl to its own sum.  Every slot's sum runs over the text rows in row order
 *     (b * Lt + t) with a fixed association and no float atomics: the same inputs give the same bits.
 *   MLM head only (one [MASK] row per sequence, or a label grid through n_rows / row_seq): a model without it (the NSP-CPT heads) is
 *     CPT_ERR_SHAPE.  Workspace: cpt_train_workspace_bytes(_rows), as the plain step.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    const float* tmpl;     /* [n_slots][H] fp32 */
    float* g_tmpl;         /* cpt_train_bwd_soft: [n_slots][H] fp32, written whole; the other entry points ignore it */
    int n_slots;           /* >= 2 */
} cpt_soft_template;
int cpt_model_fwd_soft(const cpt_model* m, const cpt_soft_template* st, const cpt_batch* b, const cpt_outputs* o, int flags,
                       void* workspace, size_t workspace_bytes, void* stream);
int cpt_model_fwd_rows_soft(const cpt_model* m, const cpt_soft_template* st, const cpt_batch* b, const int64_t* cols, int n_cols, float* logits,
                            float* row_lse, void* workspace, size_t workspace_bytes, void* stream);
int cpt_train_fwd_soft(const cpt_model* m, const cpt_soft_template* st, const cpt_batch* b, const cpt_outputs* o, void* workspace,
                       size_t workspace_bytes, void* stream, cpt_bucket_fn before_bucket, void* user, const cpt_dropout* drop);
int cpt_train_bwd_soft(const cpt_model* m, const cpt_soft_template* st, const cpt_batch* b, float loss_scale, const float* loss_scale_dev,
                       void* workspace, size_t workspace_bytes, void* stream, const cpt_dropout* drop);

/* ------------------------------------------------------------------------------------------
 * Layer freezing: the training step with a frozen PREFIX of stages.  A stage is a data-parallel bucket (above): 0 = the embedding tables,
 * embeddings.LayerNorm and the region projection (+ its LayerNorm), 1 + l = encoder layer l, layers + 1 = pooler and task head.
 * first_stage = s: stages < s are frozen.  s = 0 IS cpt_train_bwd_ex / cpt_train_bwd_rel2 / cpt_train_zero_grads(_rel2) (the same code path);
 * s = 1 freezes the embedding side, s = 1 + k also layers 0 .. k - 1, s = layers + 1 trains the head alone.  Added beside ABI 8, no struct changed.
 * The FORWARD is unchanged -- cpt_train_fwd_ex / cpt_train_fwd_rel2 / cpt_train_fwd_soft, same workspace (the frozen stages' activations are
 * still kept) -- and all three heads are served: MLM (mask_pos or a label grid), NSP, and VCR Q->AR through x (NULL otherwise).
 *   The walk: head, then the layers layers - 1 .. s - 1 exactly as cpt_train_bwd_ex runs them, then it STOPS.  At the stop, what a layer leaves to
 *     the next layer's launches -- column sums waiting for a carrier launch, K-split partial matrices of the Q|K|V weight gradient -- goes out on
 *     launches of its own; the boundary layer's data gradient into the rows below (dgrad(qkv) + residual) is not formed, and with s = layers + 1
 *     neither is the head's.  No embedding-side launch runs for s >= 1.
 *   The tied decoder weight is the word table, stage 0: for every s >= 1 it is frozen -- wgrad(decoder) is not launched and no lookup gradient
 *     exists; cls.bias (b_dec), the transform dense and its LayerNorm stay trainable.  A trainable word table above a frozen embedding side
 *     cannot be expressed.
 *   soft (NULL otherwise; MLM head, s >= 1): the walk keeps the boundary data gradient and continues BELOW the boundary as cpt_train_bwd_soft runs
 *     a frozen model (data-gradient chain only), ending in soft->g_tmpl (written whole, same bits for the same inputs).  soft with s = 0 is
 *     CPT_ERR_SHAPE: the word table's lookup gradient would have to skip the slot ids.
 * WRITE contract: nothing that belongs to a frozen stage is written OR READ through g -- its pointers (word_emb .. img_ln_b, layers[l] for
 *   l < s - 1; g->layers itself with s = layers + 1) may be NULL.  Trainable stages keep the write / accumulate split of cpt_train_bwd.
 *   grads_ready fires for the buckets layers + 1 .. s only, in that order.  cpt_train_zero_grads_from clears only the trainable stages'
 *   accumulate targets (Li is read with s = 0 only).
 * ---------------------------------------------------------------------------------------- */
int cpt_train_bwd_from(const cpt_model* m, const cpt_rel2* x, const cpt_soft_template* soft, const cpt_batch* b, const cpt_model_grads* g, int first_stage,
                       float loss_scale, const float* loss_scale_dev, void* workspace, size_t workspace_bytes, void* stream, cpt_bucket_fn grads_ready,
                       void* user, const cpt_dropout* drop);
int cpt_train_zero_grads_from(const cpt_model* m, const cpt_rel2* x, const cpt_model_grads* g, int first_stage, int Li, void* stream);

/* torch.optim.AdamW update (fewshot/refcoco_cpt.py:343,249) over flat buffers of n fp32 elements
 * (n % 4 == 0).  code[i]: 0 = no gradient on this path (skipped), 1 = weight decay, 2 = no decay
 * (fewshot/refcoco_cpt.py:320-338).  grad is multiplied by grad_scale first (1/world after a
 * sum all-reduce).  shadow_bf16 (optional) receives the bf16 copy of the updated parameters.
 * ABI 7 (round 6): lr, beta1, beta2, eps, weight_decay are DOUBLES, as the reference's optimizers hold them (Python floats): the derived scalars
 * (1 - beta, 1 - lr * weight_decay, lr / (1 - beta1^t), sqrt(1 - beta2^t)) are formed in double on the host and rounded to fp32 ONCE, where torch
 * rounds them -- with float betas 1 - 0.999f was 1.3e-5 off 0.001 (found by the float64 golden vectors of tests/golden/hf_adamw.npz). */
int cpt_adamw(float* p, const float* g, float* m, float* v, const unsigned char* code, void* shadow_bf16,
              size_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
              float grad_scale, void* stream);

/* Round 5 (ABI 6): the same launch with the arithmetic of the GQA / VCR few-shot drivers' optimizer, pytorch_transformers.AdamW
 * (Oscar/oscar/fewshot/vcr_nsp_cpt.py:385, gqa_cpt.py:342; transformers@067923d optimization.py, not vendored):
 *   CPT_ADAMW_HF: m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  p -= lr sqrt(1 - beta2^t) / (1 - beta1^t) m / (sqrt(v) + eps);
 *                 then, for code 1, p -= lr weight_decay p (on the UPDATED p).  eps sits outside the bias correction, the decay behind the step: both differ
 *                 from torch.optim.AdamW (flags = 0 = cpt_adamw) in the last digits only, but a drop-in follows its driver's optimizer.
 *   CPT_ADAMW_NO_BIAS_CORRECTION: correct_bias = False (both corrections 1). */
enum { CPT_ADAMW_HF = 1, CPT_ADAMW_NO_BIAS_CORRECTION = 2 };
int cpt_adamw_ex(float* p, const float* g, float* m, float* v, const unsigned char* code, void* shadow_bf16,
                 size_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                 float grad_scale, int flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * Operator-level entry points (the kernels cpt_model_fwd is built from; also what the parity
 * tests call one by one).
 * ---------------------------------------------------------------------------------------- */

/* out = epi(A[M][K] . W[N][K]^T + bias (+ resid)); A, W in `dtype`; out in `out_dtype`
 * (CPT_F32 always allowed; CPT_BF16 only with dtype CPT_BF16).  Replaces nn.Linear (+gelu /
 * tanh / residual add) at modeling_bert.py:38-40,85,144,145,261,275 and modeling_rec.py:143. */
int cpt_gemm(int dtype, int epi, const void* A, int lda, const void* W, int ldw, const float* bias,
             const float* resid, int ldr, void* out, int out_dtype, int ldo, int M, int N, int K,
             void* stream);

/* BertEmbeddings.forward (call site modeling_bert.py:244-245): LN(word[ids]+pos[pid]+type[tt])
 * for B*Lt tokens, written to rows b*L + t of out_f32 [B*L][H] (and out_lp when non-NULL). */
int cpt_embed_ln(const int64_t* ids, const int64_t* tt, const int64_t* pos, const float* word,
                 const float* posw, const float* typew, const float* g, const float* bta, float eps,
                 float* out_f32, void* out_lp, int lp_dtype, int B, int Lt, int L, int H, int vocab,
                 int max_pos, int type_vocab, void* stream);

/* BertLayerNorm over rows of x[R][H] (fp32), biased variance, eps inside the sqrt.  Input row r
 * goes to output row (r / grp) * grp_stride + grp_off + r % grp (grp = R, stride 0, off 0 for a
 * plain LayerNorm; grp = Li, stride = L, off = Lt places region rows behind the text rows,
 * replacing torch.cat at modeling_bert.py:269).  g == NULL skips the affine+norm (copy/cast). */
int cpt_layernorm_rows(const float* x, const float* g, const float* bta, float eps, float* out_f32,
                       void* out_lp, int lp_dtype, int R, int H, int grp, int grp_stride,
                       int grp_off, void* stream);

/* CaptionBertSelfAttention core (modeling_bert.py:42-67) for head_dim 64: qkv [B*L][3H] ->
 * ctx [B*L][H]; softmax(QK^T/8 + (1-mask)*-10000) V, scores never leave the chip.  L <= 288: MFMA kernels (score strip in registers); 288 < L <= 1024
 * (round 5; the reference accepts 512 text positions + regions, no CPT configuration needs more than 265): a one-wave-per-query coverage kernel, inference only.
 * probs (optional, [B][heads][L][L] in `dtype`) is written only for the backward pass. */
int cpt_attention(int dtype, const void* qkv, const int64_t* attn_mask, void* ctx, void* probs,
                  int B, int L, int heads, void* stream);

/* x[R][K] fp32 -> out[R][Kp] in `dtype`, zero-padded (region features / img weight, K=2054). */
int cpt_pad_cast(const float* x, void* out, int dtype, int R, int K, int Kp, void* stream);

/* Score extraction on the device: only indices go back to the host.
 * cpt_select_regions: per query q, its proposal sequences are rows query_first[q] .. query_first[q+1]-1 of
 * mask_logits [S][V]; sequence s contributes the logits at color_ids[s][0..C) (entries < 0 = trailing padding), in
 * order, divided by its "none" logit when divide_by_none (fewshot/refcoco_cpt.py:291) or raw
 * (zeroshot/refcoco_cpt.py:242); out_idx[q] = position of the maximum inside that concatenation with torch.argmax
 * semantics (first maximum; NaN is maximal), -1 if the query has no colour; out_score[q] (may be NULL) its value.
 * cpt_argmax_columns: out_idx[r] = argmax_j logits[r][ids[j]] (gqa_cpt.py:598-601). */
int cpt_select_regions(const float* mask_logits, int V, const int64_t* color_ids, int C, const int32_t* query_first, int Q,
                       int64_t none_id, int divide_by_none, int64_t* out_idx, float* out_score, void* stream);
int cpt_argmax_columns(const float* logits, int V, const int64_t* ids, int n_ids, int R, int64_t* out_idx, float* out_val,
                       void* stream);

/* RefCOCO REC evaluation of one batch of queries, one launch: the selection of cpt_select_regions, then the two val() post-loops and computeIoU
 * (Oscar/oscar/zeroshot/refcoco_cpt.py:224-246, 267-280; fewshot/refcoco_cpt.py:277-297, 305-315; utils/iou.py:1-13).  Added beside ABI 8, no
 * struct changed.  The split's tables live on the device (built once: cpt_amd/scoring.py rec_eval_table), for Q queries in data set order:
 *   seq_first [Q + 1] int32   first proposal sequence of every query       cols [S_total][C] int32   colour columns of every sequence, -1 = trailing padding
 *   cand_first [Q + 1] int32  first candidate of every query               rects [R_total][4] double  x1, y1, x2, y2 (x2 > x1, y2 > y1: the builder checks)
 *   gt [Q][4] double          the annotation x, y, w, h                    has_gt [Q] uint8
 * scores [S][V] fp32 are the batch's head rows: the sequences of query q_index[0], then of q_index[1], ... (q_index [Qb] int32, global query
 * indices in any order, each once).  A candidate's score is scores[row][col], divided by scores[row][none] when divide_by_none (the fp32 division).
 * Per query, at its GLOBAL index: idx int32 = the argmax inside the query's concatenation (torch.argmax: first maximum, NaN maximal, -0 == +0;
 * -1 for a query without a colour), score fp32 its value, iou double = computeIoU([x1, y1, x2 - x1 + 1, y2 - y1 + 1], gt) in float64 in Python's
 * operation order without contraction (NaN for a query without a colour or without an annotation), correct uint8 = iou > 0.5.  cand_score
 * [R_total] fp32 (may be NULL) takes every candidate's score.  counts [2] int32 += (correct, evaluated) by integer atomics: zero it once per pass;
 * a query without a colour or without an annotation counts in neither. */
int cpt_rec_choose(const float* scores, int S, int V, const int32_t* q_index, int Qb, int Q, const int32_t* seq_first, const int32_t* cols, int C,
                   const int32_t* cand_first, const double* rects, const double* gt, const uint8_t* has_gt, int none, int divide_by_none,
                   int32_t* idx, float* score, double* iou, uint8_t* correct, float* cand_score, int32_t* counts, void* stream);

/* Fold LayerNorm(gamma, beta) into the Linear (W [N][K] fp32, bias [N] or NULL) that consumes its output:
 * Wf = bf16(gamma[k] * W[n][k]), colc[n] = sum_k Wf[n][k], cold[n] = sum_k beta[k] W[n][k] + bias[n]. */
int cpt_fold_ln_weights(const float* W, const float* gamma, const float* beta, const float* bias, void* Wf_bf16,
                        float* colc, float* cold, int N, int K, void* stream);

/* K-tile-major copy of a bf16 weight: dst[K / 32][N][32] = src[N][K] (K % 32 == 0): the layout cpt_layer_fold.w_qkv_t holds.  The
 * fused QKV + attention launch stages K-tiles of 32; out of this copy every 16-row LDS-DMA piece is one contiguous KiB. */
int cpt_retile_k32(const void* src_bf16, void* dst_bf16, int N, int K, void* stream);

/* The two GEMM forms of the fused bf16 encoder, as stand-alone operators (bf16 operands, fp32 accumulate).
 * Row statistics travel as partial sums: st[M][slots][2] (sum, sum of squares), one slot per 96-column block of the
 * `hidden`-wide producer, slots = number of blocks rounded up to even; readers add the slots in index order.
 *   consumer:  out = [gelu]( LayerNorm(A; st_in) . W^T + bias ), with the LayerNorm folded: Wf = gamma (.) W in bf16,
 *              colc / cold from cpt_fold_ln_weights; BertIntermediate (modeling_bert.py:144) and the Q|K|V projections.
 *   producer:  out_f32 = A . W^T + bias + R, R = resid or LayerNorm(resid; st_in, g_in, b_in) when g_in != NULL; also writes
 *              the bf16 copy and st_out (partial row sums of out_f32); BertSelfOutput / BertOutput (:85-86, :145). */
int cpt_gemm_ln_cons(const void* A_bf16, int lda, const void* Wf_bf16, int ldw, const float* st_in, const float* colc,
                     const float* cold, float eps, int hidden, int gelu, void* out_bf16, int ldo, int M, int N, int K, void* stream);
int cpt_gemm_ln_prod(const void* A_bf16, int lda, const void* W_bf16, int ldw, const float* bias, const float* resid, int ldr,
                     const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, float* out_f32,
                     void* out_bf16, float* st_out, int ldo, int M, int N, int K, void* stream);

/* The producer with the residual stream in the 3-byte form (round 2; the form cpt_model_fwd's LayerNorm-folded bf16 encoder runs in;
 * cpt_gemm_ln_prod above is its fp32 + bf16 reference): a pre-LayerNorm sum x travels as T = its fp32 pattern rounded to 24 bits (round half away),
 * hi = (T + 0x80) >> 8 as a plain bf16 tensor (the next GEMM's A operand) and lo = the signed byte T - (hi << 8);
 * x' = ((hi << 8) + lo) << 8, |x' - x| <= 2^-17 |x|.  3 + 3 bytes per element through the epilogue instead of 4 + 6.
 *   cpt_gemm_ln_prod3: as cpt_gemm_ln_prod with resid = (resid_hi bf16, resid_lo int8) [M][ldr], out = (out_hi bf16, out_lo int8) [M][ldo]
 *   cpt_resid3_split:  x fp32 [n] -> hi, lo (n % 4 == 0, 16-byte aligned)
 *   cpt_resid3_merge:  the inverse into out fp32 [R][H]; gather = 0: source row r; gather = 1: source row r * L + pos[r]
 *                      (pos NULL: r * L), the rows the heads read (modeling_rec.py:143, modeling_bert.py:275) */
int cpt_gemm_ln_prod3(const void* A_bf16, int lda, const void* W_bf16, int ldw, const float* bias, const void* resid_hi, const void* resid_lo,
                      int ldr, const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, void* out_hi, void* out_lo,
                      float* st_out, int ldo, int M, int N, int K, void* stream);
int cpt_resid3_split(const float* x, void* hi_bf16, void* lo_i8, size_t n, void* stream);
/* Round 3 (ABI 4): the producer with its A operand in the fragment-major "panel" layout
 *   panel[M / 32][K / 16][64][8] bf16: element (row, k) at (((row / 32) (K / 16) + k / 16) 64 + ((k % 16) / 8) 32 + row % 32) 8 + k % 8
 * (every v_mfma_f32_32x32x16_bf16 A operand of a 32-row block is one contiguous KiB), read straight into registers: only W rides
 * the LDS ring.  Inside cpt_model_fwd the attention kernel and the FFN-up epilogue write ctx / h in this layout; results are
 * bit-identical to cpt_gemm_ln_prod3 on the row-major tensor.  M % 128 == 0, N % 192 == 0, K % 256 == 0, K >= 512.
 *   cpt_panel_pack: row-major bf16 [M][ld] -> panel (to_panel = 1) or back (to_panel = 0, ld = leading dimension of the row-major side);
 *                   M % 32 == 0, K % 16 == 0. */
int cpt_panel_pack(const void* src_bf16, int ld, void* dst_bf16, int M, int K, int to_panel, void* stream);
int cpt_gemm_ln_prod3_panel(const void* A_panel, const void* W_bf16, int ldw, const float* bias, const void* resid_hi, const void* resid_lo,
                            int ldr, const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, void* out_hi, void* out_lo,
                            float* st_out, int ldo, int M, int N, int K, void* stream);
int cpt_resid3_merge(const void* hi_bf16, const void* lo_i8, const int64_t* pos, float* out, int R, int L, int H, int gather, void* stream);
/* Round 5 (ABI 6): the producer with the RESIDUAL STREAM in the panel layout as well -- resid_hi / out_hi as [M / 32][N / 16][64][8] bf16 (the very
 * A-operand panel the next GEMM reads), resid_lo / out_lo as [M / 32][N / 16][64][8] bytes (cpt_panel_pack_bytes: the same index arithmetic on
 * one-byte elements) -- with a register-direct epilogue (swapped MFMA operands, lane = output row; no LDS slab, no barrier behind the K loop).
 * Element for element and slot for slot the same bits as cpt_gemm_ln_prod3_panel / cpt_gemm_ln_prod3 on the row-major tensors.  Inside
 * cpt_model_fwd it is what the fused bf16 encoder runs at panel-eligible shapes (BertSelfOutput / BertOutput, modeling_bert.py:85-86, :145). */
int cpt_panel_pack_bytes(const void* src_i8, int ld, void* dst_i8, int M, int K, int to_panel, void* stream);
int cpt_gemm_ln_prod3_rpanel(const void* A_panel, const void* W_bf16, int ldw, const float* bias, const void* resid_hi_panel, const void* resid_lo_panel,
                             const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, void* out_hi_panel, void* out_lo_panel,
                             float* st_out, int M, int N, int K, int waves, void* stream);
/* (waves: 0 = the library's choice by shape -- 4 x 2 waves of 32 x 96 when the tiles fit one round, 4 x 1 waves of 32 x 192 over several rounds --,
 *  8 / 4 = that shape for THIS call; same bits either way) */

/* Weight-gradient GEMM in the TN form (what cpt_train_bwd runs for dW = dY^T . X, fewshot/refcoco_cpt.py:248's autograd of
 * every nn.Linear): out[M][N] fp32 = sum over k < K of A[k][m] * W[k][n], A bf16 [K][lda], W bf16 [K][ldw] -- both operands
 * as the backward pass holds them (rows = tokens), no transposed copies.  M % 128 == 0, N % 128 == 0 or N % 192 == 0,
 * K % 64 == 0, ldo == N.  k_rows (0: K): token rows that exist when K was rounded up to a multiple of 64 (the rest read as zero).
 * partials (optional, partial_bytes): scratch for split-K partial matrices (up to 8 * M * N * 4
 * bytes are used when the output has few tiles); they are added in split order, so the result is reproducible. */
int cpt_gemm_tn(const void* A_bf16, int lda, const void* W_bf16, int ldw, float* out, int ldo, int M, int N, int K, int k_rows,
                void* partials, size_t partial_bytes, void* stream);
/* Data-gradient GEMM in the NN form (dX = dY . W against an nn.Linear weight as stored): out[M][N] = A[M][K] . W[K][N] (+ resid),
 * A bf16 [M][lda], W bf16 [K][ldw] (row = contraction index = out_features), out fp32 (optionally + fp32 resid [M][ldr]) or bf16.
 * N % 192 == 0 or N % 128 == 0, K % 64 == 0.  w_rows (0: K): rows of W that exist when K was rounded up to a multiple of 64 -- rows beyond read as
 * zero, A's extra columns must hold zeros (the vocabulary-sized decoder, 30522 rows).  partials (optional): scratch for split-K when the
 * output has few tiles and K is long (fp32 output without residual; up to 64 * M * N * 4 bytes used, added in split order). */
int cpt_gemm_nn(const void* A_bf16, int lda, const void* W_bf16, int ldw, const float* resid, int ldr, void* out, int out_dtype, int ldo,
                int M, int N, int K, int w_rows, void* partials, size_t partial_bytes, void* stream);

/* Split-operand copy for CPT_BF16X3: x fp32 [R][K] (leading dimension ld) -> out bf16 [R][3K] holding, per row, the blocks
 * hi | hi | lo (weight_order 0: activations) or hi | lo | hi (weight_order 1: nn.Linear weights), hi = bf16(x),
 * lo = bf16(x - hi).  A bf16 GEMM of the two over K' = 3K is x.w to ~2^-16 relative. */
int cpt_split3(const float* x, int ld, void* out_bf16, int R, int K, int weight_order, void* stream);

/* out[b][:] = src[b*L + pos[b]][:] (pos NULL = row 0): the [MASK] rows
 * (zeroshot/refcoco_cpt.py:219) and the [CLS] rows of BertPooler. */
int cpt_gather_rows(const void* src, int dtype, const int64_t* pos, void* out, int B, int L, int H,
                    void* stream);

/* CrossEntropyLoss(ignore_index=-1) over rows of logits[R][V] (modeling_rec.py:147-150).
 * loss[0] += sum of row losses, loss[1] += labelled-row count (caller zeroes loss first);
 * dlogits (optional) = softmax - onehot for labelled rows, 0 otherwise (caller scales by 1/count). */
int cpt_ce_rows(const float* logits, const int64_t* labels, float* loss, float* dlogits, int R, int V,
                void* stream);

/* ------------------------------------------------------------------------------------------
 * Operator-level BACKWARD entry points (ABI 6; SURVEY 8(b): attention_bwd, bias_residual_ln_bwd, embed_ln_bwd): the kernels cpt_train_bwd
 * launches, one by one -- what autograd runs under loss.backward() (Oscar/oscar/fewshot/refcoco_cpt.py:248) for the blocks of
 * Oscar/oscar/modeling/modeling_bert.py:30-70 (self-attention), :85-86 / :145 (BertSelfOutput / BertOutput LayerNorm) and :244-245 (BertEmbeddings).
 * `drop` / `site` as in cpt_train_*_ex (NULL or p = 0: no dropout): masks are regenerated from (seed, step, site), never stored.
 *
 * cpt_attention_bwd: qkv [B*L][3H] and dctx [B*L][H] -> dqkv [B*L][3H] (written) for ctx = dropout(softmax(q k^T / 8 + mask)) v per head, the probabilities
 *   recomputed.  dtype CPT_F32: fp32 tensors; CPT_BF16: bf16 tensors (MFMA kernel, L <= 288); CPT_BF16X3: fp32 tensors through the split-operand
 *   MFMA kernel.  dbias_qkv (optional, [3H] fp32): += column sums of dqkv (the stacked Q | K | V bias gradient).  mask_3d: attn_mask is [B][L][L].
 * cpt_layernorm_bwd: y = LayerNorm(x; g, b) over rows of x [R][H] fp32 (x = the stored pre-LayerNorm sum): dx [R][H] fp32 written; dg, db += their sums
 *   (atomics: zero them first); dx_lp (optional): the copy of dx in lp_dtype THROUGH the hidden-site dropout mask of `site` when drop is given
 *   (the gradient entering the dense layer in front of the residual add), dbias (optional, [H]) += its column sums.  scratch (optional,
 *   >= (R / 4) * 3 * H * 4 bytes): two-stage column sums instead of per-block atomics.
 * cpt_embed_ln_bwd: backward of cpt_embed_ln for dy = rows b * L + t of a [B*L][H] fp32 gradient: LayerNorm backward, then scatter-add into dword
 *   (rows of padding_idx 0 skipped, as nn.Embedding), dposw, dtypew; dg, db += (zero everything first).
 * ---------------------------------------------------------------------------------------- */
int cpt_attention_bwd(int dtype, const void* qkv, const int64_t* attn_mask, int mask_3d, const void* dctx, void* dqkv, float* dbias_qkv,
                      int B, int L, int heads, const cpt_dropout* drop, int site, void* stream);
int cpt_layernorm_bwd(const float* dy, const float* x, const float* g, float eps, float* dx, void* dx_lp, int lp_dtype, float* dg, float* db,
                      int R, int H, const cpt_dropout* drop, int site, float* dbias, void* scratch, size_t scratch_bytes, void* stream);
int cpt_embed_ln_bwd(const float* dy, const int64_t* ids, const int64_t* tt, const int64_t* pos, const float* word, const float* posw, const float* typew,
                     const float* g, float eps, float* dword, float* dposw, float* dtypew, float* dg, float* db, int B, int Lt, int L, int H,
                     int vocab, int max_pos, int type_vocab, void* stream);

/* ------------------------------------------------------------------------------------------
 * Communicator block (ABI 6) for hosts that are NOT PyTorch.  cpt_amd itself keeps its collectives in torch.distributed
 * (backend "nccl" = RCCL over xGMI) and starts them from the bucket callbacks of cpt_train_fwd_ex / cpt_train_bwd_ex; a host without
 * torch.distributed drives the same data-parallel step through these calls instead: sum the flat gradient (cpt_allreduce_grads, or
 * cpt_reduce_scatter + cpt_allgather around a sharded cpt_adamw) where the reference's DistributedDataParallel all-reduces it
 * (Oscar/oscar/fewshot/refcoco_cpt.py:516-522), and gather the per-rank result arrays where the reference all_gathers pickled dicts
 * (Oscar/oscar/utils/comm.py:102-142).  RCCL is bound at run time (dlopen of librccl.so.1: no link-time dependency; inside a PyTorch
 * process the soname resolves to the copy torch loaded).  ONE communicator per process, on the device current at cpt_comm_init; rank 0
 * creates the 128-byte id with cpt_comm_unique_id and the host ships it to the other ranks out of band (a file, a socket, MPI).
 * All collectives are asynchronous on `stream`; dtype CPT_F32 or CPT_BF16; counts in elements; in-place allowed where RCCL allows it.
 * ---------------------------------------------------------------------------------------- */
int cpt_comm_unique_id(void* id128);                              /* host buffer of 128 bytes */
int cpt_comm_init(int rank, int nranks, const void* id128);
int cpt_comm_rank(int* rank, int* nranks);
int cpt_allreduce_grads(void* buf, size_t count, int dtype, void* stream);                                     /* in-place sum over ranks */
int cpt_reduce_scatter(const void* send, void* recv, size_t recv_count, int dtype, void* stream);              /* send holds nranks * recv_count elements */
int cpt_allgather(const void* send, void* recv, size_t send_count, int dtype, void* stream);                   /* recv holds nranks * send_count elements */
int cpt_comm_destroy(void);

/* Per-kernel event timing, the A/B switches of the kernels (cpt_set_tuning) and the per-workgroup trace live in cpt_hip_debug.h: they are
 * measurement and development entry points of the same library, not part of the interface a host binds for the hot path. */

#ifdef __cplusplus
}
#endif
#endif /* CPT_HIP_H */
