/* libcpt_hip.so -- measurement and development entry points (round 4: split out of cpt_hip.h).
 *
 * Exported by the same library; NOT part of the hot-path interface of cpt_hip.h.  bench.py's roofline leg uses the per-kernel event
 * timing; tools/ and the A/B tests use cpt_set_tuning and the per-workgroup trace.  A product host never needs to call any of them.
 * The kernel-variant switches are process-global state only in the DEVELOPMENT build of the library (-DCPT_ABLATION,
 * cpt_amd/libcpt_hip_abl.so, selected by CPT_AMD_ABLATION=1); in the product build they are compile-time constants, the code behind the
 * losing settings is not compiled, and cpt_set_tuning refuses every key but -1 (cpt_build_info tells the two apart).
 */
#ifndef CPT_HIP_DEBUG_H
#define CPT_HIP_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 * ---------------------------------------------------------------------------------------- */
enum { CPT_K_GEMM_QKV = 0, CPT_K_ATTN, CPT_K_GEMM_AO, CPT_K_LN, CPT_K_GEMM_FFN1, CPT_K_GEMM_FFN2,
       CPT_K_EMBED, CPT_K_IMG, CPT_K_HEAD, CPT_K_OP /* any operator-level call */, CPT_K_COUNT };
int cpt_prof_enable(int on);                          /* resets accumulators */
int cpt_prof_read(int kernel_id, double* total_ms, int64_t* launches); /* synchronises */

/* Operator-level entry points with a PER-CALL kernel choice (round 5; product and development build alike): which of the SHIPPED tile
 * configurations / wave shapes serves a GEMM is normally the library's choice by shape; the parity and race tests walk through all of them on
 * small problems with these.  The choice is an argument of the call (thread-local for its duration): no state survives it.
 *   tile (cpt_gemm_tile, cpt_gemm_ln_cons_tile): 3 = by shape; 0 = generic register-staged kernel; 13 = 128x192 (3-stage), 11 = 192x192, 10 = 128x384,
 *     14 = 384x192, 15 = 128x192 two workgroups per CU, 18 = 64x192, 19 = 384x256 one pass; consumers also 20 = two-pass 384x256, 21 = 4-wave 192x256
 *   tile (cpt_gemm_ln_prod_tile, cpt_gemm_ln_prod3_tile): 3 = by shape; 13 = 128x192, 18 = 64x192, 11 = 192x192, 10 = 128x384; cpt_gemm_ln_prod3_tile also
 *     15 = 128x192 two workgroups per CU.  The LayerNorm-producer epilogue has no other instantiation: any other id above 3 (14, 19, ...; 15 for
 *     cpt_gemm_ln_prod_tile) runs the 128x192 kernel, and so does 10 at a width whose last 384-column tile would reach past the row-sum table's
 *     slots (N mod 384 in 1..192); an id below 3 chooses by shape
 *   waves (cpt_gemm_ln_prod3_panel_waves; also an argument of cpt_gemm_ln_prod3_rpanel in cpt_hip.h): 0 = by shape, 8 = 4x2 waves of 32x96, 4 = 4x1 waves of 32x192 */
int cpt_gemm_tile(int tile, int dtype, int epi, const void* A, int lda, const void* W, int ldw, const float* bias,
                  const float* resid, int ldr, void* out, int out_dtype, int ldo, int M, int N, int K, void* stream);
int cpt_gemm_ln_cons_tile(int tile, const void* A_bf16, int lda, const void* Wf_bf16, int ldw, const float* st_in, const float* colc,
                          const float* cold, float eps, int hidden, int gelu, void* out_bf16, int ldo, int M, int N, int K, void* stream);
int cpt_gemm_ln_prod_tile(int tile, const void* A_bf16, int lda, const void* W_bf16, int ldw, const float* bias, const float* resid, int ldr,
                          const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, float* out_f32, void* out_bf16,
                          float* st_out, int ldo, int M, int N, int K, void* stream);
int cpt_gemm_ln_prod3_tile(int tile, const void* A_bf16, int lda, const void* W_bf16, int ldw, const float* bias, const void* resid_hi, const void* resid_lo,
                           int ldr, const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, void* out_hi, void* out_lo,
                           float* st_out, int ldo, int M, int N, int K, void* stream);
int cpt_gemm_ln_prod3_panel_waves(int waves, const void* A_panel, const void* W_bf16, int ldw, const float* bias, const void* resid_hi, const void* resid_lo,
                                  int ldr, const float* st_in, const float* g_in, const float* b_in, float eps, int hidden, void* out_hi, void* out_lo,
                                  float* st_out, int ldo, int M, int N, int K, void* stream);

/* 0 = product build (libcpt_hip.so: every kernel-variant switch below is a compile-time constant, cpt_set_tuning refuses every key but -1);
 * bit 0 set = the CPT_ABLATION development build (libcpt_hip_abl.so), where the switches are process-global (round 5). */
int cpt_build_info(void);

/* Kernel-variant switches for A/B measurements (CPT_ABLATION build only); defaults are the shipped configuration.  The AUTHORITATIVE list is the
 * table in cpt_amd/csrc/switches.h (key, variable, default, legal range, description): the library's declarations, this call's lookup and its
 * reset are generated from it, and tests/test_abi_cpu.py holds the list below to the same keys.  A value outside a key's range is clamped into it.
 * Switches are process-global: they must NOT change between a training forward (cpt_train_fwd*) and its backward (cpt_train_bwd*) -- both
 * derive the step's launches and buffers from them, and the backward reads what the forward wrote.  Set them before a step, restore them after.
 *   key 0  (default 3) GEMM tile: 3 = by shape; 0 = generic register-staged kernel; a tile id of cpt_gemm_tile forces that tile where legal
 *   key 1  (default 0) knock-out bits of the pipelined GEMMs (1 no operand DMA, 2 no fragment reads, 4 no MFMA, 8 no epilogue) and of the fused QKV + attention
 *          kernel (32 no attention phase); results are garbage unless 0
 *   key 2  (default 1) attention backward, bf16: 1 = transpose-read MFMA kernels (L <= 288); 0 = generic kernel always; 2 = L <= 128 through the older MFMA
 *          kernel with transposed tile copies
 *   key 3  (default 384) generic GEMM path: workgroup count the split-K factor aims at
 *   key 6  (default 3) bf16, L <= 128: QKV projection + attention in one kernel (0 = two kernels; 1 = one workgroup per (sequence, head), two per CU; 2 = same,
 *          one per CU; 3 = one workgroup per (sequence, three heads) where heads % 3 == 0, else 1)
 *   key 10 (default 1) training backward: bf16 weight gradients through the TN GEMM (operands read as stored, split-K partials reduced in order); 0 = explicit
 *          operand transposes + NT GEMM
 *   key 13 (default 0) knock-out experiments of the panel producer (gemm_prod.hip prod3_panel_kernel: 1 half the A loads, 2 no A loads, 3 no W DMA, ...); results
 *          are garbage unless 0
 *   key 14 (default 1) fused bf16 encoder: ctx and the FFN activation in the fragment-major panel layout where the shapes allow (gemm_prod.hip); 0 = row-major
 *          tensors
 *   key 16 (default 192) FFN-up two-pass kernel (and with it panel mode) from this many 384 x 256 tiles on
 *   key 17 (default 0) LayerNorm backward, two-stage column-sum form: rows per workgroup (0 = 8 from 2048 rows on, else 4 = one row per wave)
 *   key 18 (default 3) training backward, bias-gradient column sums inside their producers: bit 0 = b_in (GELU-gradient epilogue), bit 1 = b_qkv (attention
 *          backward); a cleared bit runs the stand-alone column-sum launch
 *   key 19 (default 2) training backward, a layer's weight gradients: 2 = FFN down | FFN up | attention output in one launch + Q|K|V alone where the shapes fit
 *          one round (else as 1), 1 = two paired launches, 0 = four single launches
 *   key 20 (default 1) stand-alone LayerNorm-consumer QKV projection: the GELU-less two-pass 384 x 256 kernel when its tiles fill the chip; 0 = the 384 x 192
 *          pipelined kernel
 *   key 22 (default 1) training forward, FFN-down at 2048..6144 rows: 128 x 192 tiles with K split over two workgroups, partial matrices summed by the LayerNorm
 *          pass; 0 = 64 x 192 tiles over the whole K
 *   key 24 (default 0) wave shape of the panel LayerNorm producers' 128 x 192 tile: 0 = by shape (4 when the tiles run several rounds), 4 = 4 x 1 waves of 32 x
 *          192, 8 = 4 x 2 waves of 32 x 96; same bits
 *   key 25 (default 1) fused bf16 encoder: text embedding + region-feature pad/cast in one launch; 0 = two launches
 *   key 26 (default 40) MLM head on the [MASK] rows: percent of the decoder table prefetched by the head's first launch (the rest: by its reduce + GELU +
 *          LayerNorm launch)
 *   key 27 (default 1) bf16x3 parity mode: attention on bf16 MFMA with split operands; 0 = the fp32 MFMA kernel + a split3 pass over ctx
 *   key 28 (default 1) panel layout for the FFN activation also when the producers run several rounds of tiles; 0 = row-major there
 *   key 29 (default 1) 4-wave 192 x 256 LayerNorm-consumer kernel (gemm_ffn4.hip) in place of the two-pass 384 x 256 kernel: 1 = where its tiles fill their
 *          rounds at least 10 % better, 2 = wherever legal, 0 = nowhere; same bits
 *   key 30 (default 1) fused bf16 encoder at the full-panel shapes: the residual stream itself in the panel layout, register-direct producer epilogue
 *          (gemm_prod.hip RP); 0 = row-major 3-byte stream; same bits
 *   key 31 (default 1) only [MASK] (or only [CLS]) rows read behind the encoder: the last layer's attention output / FFN / LayerNorms on those rows alone; 0 =
 *          every row
 *   key 34 (default 1) training backward, data-gradient GEMMs in front of a LayerNorm backward at 2048..6144 rows: two K-split bf16 partial matrices of 128 x 192
 *          tiles; 0 = 64 x 192 tiles over the whole K, fp32 out
 *   key 36 (default 1) training forward with hidden dropout: LayerNorm launches write no fp32 output, the next row pass re-forms the residual; 0 = fp32 outputs
 *          written and read back
 *   key 37 (default 1) training backward: Q|K|V weight-gradient partial sums added up inside the next layer's three-problem weight-gradient launch; 0 = a
 *          reduction launch of their own
 * Two more calls that are not switches: cpt_set_tuning(-1, 0) restores the default of every key above (and the trace filter);
 * cpt_set_tuning(8, epilogue_id | K << 8) narrows cpt_debug_gemm_trace to the launches of one epilogue id / one K (255: all).
 * Any other key fails with CPT_ERR_SHAPE; the product build refuses every key but -1. */
int cpt_set_tuning(int key, int value);
/* Debug: when buf != NULL the pipelined GEMM writes 8 int64 per workgroup (shader-clock stamps at
 * start / after prologue issue / after K loop / after staging / end, and the XCC id). */
int cpt_debug_gemm_trace(void* buf);

#ifdef __cplusplus
}
#endif
#endif /* CPT_HIP_DEBUG_H */
