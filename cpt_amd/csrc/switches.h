#pragma once
// Kernel-variant switches (include/cpt_hip_debug.h, cpt_set_tuning): THE table.  A switch is written down here and nowhere else; the declarations
// below, cpt_set_tuning's lookup and its reset (key -1) are generated from it (cpt_abi.hip).  In the PRODUCT build (libcpt_hip.so) every switch
// is a compile-time constant holding the shipped configuration: the library carries no process-global state that changes which kernel runs,
// the compiler drops the code behind the losing settings, and cpt_set_tuning refuses every key.  The development build (-DCPT_ABLATION,
// libcpt_hip_abl.so; CPT_AMD_ABLATION=1 selects it in cpt_amd._lib) keeps them as process-global ints for same-box A/B measurements and the
// bit-identity tests between variants.
//
// Row: X(key, variable, default, lowest, highest legal value, description).  cpt_set_tuning clamps a value into [lowest, highest]; key 24 alone
// also maps every value that is not one of its three onto 8 (cpt_abi.hip).  Key numbers are never re-used: tests and tools pass them as
// literals, and a retired switch leaves a hole.  Key 8 (trace filter of cpt_debug_gemm_trace) is a diagnostic, not a switch, and has no row.
#define CPT_SWITCH_TABLE(X) \
    X( 0, g_gemm_variant_sw,     3,   0,  21, "GEMM tile: 3 = by shape; 0 = generic register-staged kernel; a tile id of cpt_gemm_tile forces that tile where legal") \
    X( 1, g_gemm_abl,            0,   0, 0x7fffffff, "knock-out bits of the pipelined GEMMs (1 no operand DMA, 2 no fragment reads, 4 no MFMA, 8 no epilogue) and of the fused QKV + attention kernel (32 no attention phase); results are garbage unless 0") \
    X( 2, g_attn_bwd_variant,    1,   0,   2, "attention backward, bf16: 1 = transpose-read MFMA kernels (L <= 288); 0 = generic kernel always; 2 = L <= 128 through the older MFMA kernel with transposed tile copies") \
    X( 3, g_splitk_target,     384,   1, 0x7fffffff, "generic GEMM path: workgroup count the split-K factor aims at") \
    X( 6, g_fuse_attn,           3,   0,   3, "bf16, L <= 128: QKV projection + attention in one kernel (0 = two kernels; 1 = one workgroup per (sequence, head), two per CU; 2 = same, one per CU; 3 = one workgroup per (sequence, three heads) where heads % 3 == 0, else 1)") \
    X(10, g_wgrad_tn,            1,   0,   1, "training backward: bf16 weight gradients through the TN GEMM (operands read as stored, split-K partials reduced in order); 0 = explicit operand transposes + NT GEMM") \
    X(13, g_prod_abl,            0,   0,   4, "knock-out experiments of the panel producer (gemm_prod.hip prod3_panel_kernel: 1 half the A loads, 2 no A loads, 3 no W DMA, ...); results are garbage unless 0") \
    X(14, g_panel,               1,   0,   1, "fused bf16 encoder: ctx and the FFN activation in the fragment-major panel layout where the shapes allow (gemm_prod.hip); 0 = row-major tensors") \
    X(16, g_ffn_2pass_min_tiles, 192, 0, 0x7fffffff, "FFN-up two-pass kernel (and with it panel mode) from this many 384 x 256 tiles on") \
    X(17, g_lnb_rpb,             0,   0, 0x7fffffff, "LayerNorm backward, two-stage column-sum form: rows per workgroup (0 = 8 from 2048 rows on, else 4 = one row per wave)") \
    X(18, g_bias_fuse,           3,   0,   3, "training backward, bias-gradient column sums inside their producers: bit 0 = b_in (GELU-gradient epilogue), bit 1 = b_qkv (attention backward); a cleared bit runs the stand-alone column-sum launch") \
    X(19, g_wgrad_pair,          2,   0,   2, "training backward, a layer's weight gradients: 2 = FFN down | FFN up | attention output in one launch + Q|K|V alone where the shapes fit one round (else as 1), 1 = two paired launches, 0 = four single launches") \
    X(20, g_qkv_2pass,           1,   0,   1, "stand-alone LayerNorm-consumer QKV projection: the GELU-less two-pass 384 x 256 kernel when its tiles fill the chip; 0 = the 384 x 192 pipelined kernel") \
    X(22, g_fwd_split2,          1,   0,   1, "training forward, FFN-down at 2048..6144 rows: 128 x 192 tiles with K split over two workgroups, partial matrices summed by the LayerNorm pass; 0 = 64 x 192 tiles over the whole K") \
    X(24, g_prod_waves,          0,   0,   8, "wave shape of the panel LayerNorm producers' 128 x 192 tile: 0 = by shape (4 when the tiles run several rounds), 4 = 4 x 1 waves of 32 x 192, 8 = 4 x 2 waves of 32 x 96; same bits") \
    X(25, g_embed_pad,           1,   0,   1, "fused bf16 encoder: text embedding + region-feature pad/cast in one launch; 0 = two launches") \
    X(26, g_dec_pf_pct,         40,   0, 100, "MLM head on the [MASK] rows: percent of the decoder table prefetched by the head's first launch (the rest: by its reduce + GELU + LayerNorm launch)") \
    X(27, g_x3_attn,             1,   0,   1, "bf16x3 parity mode: attention on bf16 MFMA with split operands; 0 = the fp32 MFMA kernel + a split3 pass over ctx") \
    X(28, g_panel_ffn_multi,     1,   0,   1, "panel layout for the FFN activation also when the producers run several rounds of tiles; 0 = row-major there") \
    X(29, g_lncons4,             1,   0,   2, "4-wave 192 x 256 LayerNorm-consumer kernel (gemm_ffn4.hip) in place of the two-pass 384 x 256 kernel: 1 = where its tiles fill their rounds at least 10 % better, 2 = wherever legal, 0 = nowhere; same bits") \
    X(30, g_rpanel,              1,   0,   1, "fused bf16 encoder at the full-panel shapes: the residual stream itself in the panel layout, register-direct producer epilogue (gemm_prod.hip RP); 0 = row-major 3-byte stream; same bits") \
    X(31, g_tail,                1,   0,   1, "only [MASK] (or only [CLS]) rows read behind the encoder: the last layer's attention output / FFN / LayerNorms on those rows alone; 0 = every row") \
    X(34, g_nn_split2,           1,   0,   1, "training backward, data-gradient GEMMs in front of a LayerNorm backward at 2048..6144 rows: two K-split bf16 partial matrices of 128 x 192 tiles; 0 = 64 x 192 tiles over the whole K, fp32 out") \
    X(36, g_ln_lean,             1,   0,   1, "training forward with hidden dropout: LayerNorm launches write no fp32 output, the next row pass re-forms the residual; 0 = fp32 outputs written and read back") \
    X(37, g_qkv_defer,           1,   0,   1, "training backward: Q|K|V weight-gradient partial sums added up inside the next layer's three-problem weight-gradient launch; 0 = a reduction launch of their own")

namespace cpt {
#ifdef CPT_ABLATION
#define CPT_SWITCH_DECL(key, name, dflt, lo, hi, desc) extern int name;      // the one definition: cpt_abi.hip
#else
#define CPT_SWITCH_DECL(key, name, dflt, lo, hi, desc) constexpr int name = dflt;
#endif
CPT_SWITCH_TABLE(CPT_SWITCH_DECL)
#undef CPT_SWITCH_DECL
}  // namespace cpt
