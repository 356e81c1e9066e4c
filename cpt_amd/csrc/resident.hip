// Device-resident evaluation sets (cpt_gather_batch): a split lives on the GPU as packed tables (cpt_resident_store, include/cpt_hip.h) and ONE
// launch builds a step's padded or trimmed batch out of it from a list of sequence indices -- what batching.trim(torch.cat(...)) holds on the
// host, element for element.
//   features: the hot part, a pure gather bound by HBM.  A destination row is D floats at (b Li' + r) D, so with D even (2054) it starts on an
//             8-byte boundary only; a store row starts on a 16-byte boundary (its pitch is D rounded up to 16 bytes, the padding zero).  A lane
//             moves one 16-byte piece of a store row: one 16-byte load from a 16-byte-aligned address -- the last piece of a row too, its
//             surplus is the row's own padding -- and 16-byte stores declared 8-byte aligned (fp32: one, bf16: two, the bf16 widened exactly),
//             the tail of a row as pairs of floats.  Four pieces per lane are in flight before the first store (the index chain of a piece --
//             seq_idx -> feat_block -> block_rows / block_off -- is three dependent reads of small cached tables; the four chains run side by
//             side).  A row at or behind its block's block_rows is written as +0.0 (its lanes read one shared line and drop it).  Odd D or an unaligned operand: one
//             element per lane, grid-strided.
//   int64 rows: ids (int32), token types and mask (uint8) widened to int64, [MASK] positions (int32): small, on extra workgroups of the same
//             launch, as trim_batch_kernel carries its rows.
// Every index that comes from memory is clamped before it is used: a sequence index outside the store, a block index outside the block table or
// a block that reaches past the feature rows reads the nearest valid entry or is written as zeros; nothing is read outside the store.
#include "common.h"
#include "kernels.h"

namespace cpt {

constexpr int GB_THREADS = 256;
constexpr int GB_UNR = 4;

struct GatherArgs {
    const void* feats;
    const int32_t* ids;
    const uint8_t *seg, *mask;
    const int32_t *mask_pos, *feat_block, *block_rows;
    const int64_t* block_off;
    long long n_rows;
    int pitch, D, Lt, Li, S, base, NB;
    const int32_t* seq_idx;
    int B, Lt2, Li2;
    int64_t *ids_o, *type_o, *mask_o, *mpos_o;
    float* img_o;
    unsigned nfeat;                          // workgroups [0, nfeat) gather the region features, the others the int64 rows
};

// the store-local sequence of batch entry b, clamped into [0, S)
__device__ __forceinline__ int gather_seq(const GatherArgs& a, unsigned b) {
    const long long s = (long long)a.seq_idx[b] - a.base;
    return (int)(s < 0 ? 0 : (s >= a.S ? a.S - 1 : s));
}

// first feature row of sequence `seq`'s block and whether region r of it is stored (else the row is +0.0)
__device__ __forceinline__ bool gather_row(const GatherArgs& a, int seq, unsigned r, long long& row) {
    int blk = a.feat_block[seq];
    blk = blk < 0 ? 0 : (blk >= a.NB ? a.NB - 1 : blk);
    const long long off = a.block_off[blk];
    row = off + r;
    return (long long)r < a.block_rows[blk] && off >= 0 && row < a.n_rows;
}

template <typename T>
__device__ __forceinline__ void gather_feats_vec(const GatherArgs& a, unsigned block) {
    typedef f32x4 f32x4_a8 __attribute__((aligned(8)));
    typedef f32x2 f32x2_a8 __attribute__((aligned(8)));
    constexpr unsigned EPC = 16 / sizeof(T);                          // elements per 16-byte piece of a store row
    const unsigned cpr = ((unsigned)a.D + EPC - 1) / EPC;             // pieces per row
    const unsigned rows = (unsigned)a.B * (unsigned)a.Li2, total = rows * cpr;     // (< 2^31: checked by the host)
    const unsigned stride = a.nfeat * GB_THREADS, idx0 = block * GB_THREADS + threadIdx.x;
    if (a.n_rows <= 0) {                                              // a store without a feature row: every region is +0.0
        for (size_t i = idx0; i < (size_t)rows * a.D / 2; i += stride) reinterpret_cast<f32x2_a8*>(a.img_o)[i] = f32x2{0.f, 0.f};
        return;
    }
    // The index chain of a piece is three dependent reads (seq_idx -> feat_block -> block_rows, block_off) in front of its 16-byte load.  The
    // four pieces of a lane walk the chain in step, one table at a time, so that each table costs ONE wait for all four and the four feature
    // loads are issued back to back; a piece behind the end of the work follows the last piece's chain and is dropped at the store.
    unsigned orow[GB_UNR], c[GB_UNR], r[GB_UNR];
    int v[GB_UNR];
    long long off[GB_UNR];
    u32x4_t raw[GB_UNR];
#pragma unroll
    for (int u = 0; u < GB_UNR; ++u) {
        const unsigned idx = min(idx0 + u * stride, total - 1);
        orow[u] = idx / cpr;
        c[u] = (idx - orow[u] * cpr) * EPC;
        const unsigned b = orow[u] / (unsigned)a.Li2;
        r[u] = orow[u] - b * (unsigned)a.Li2;
        v[u] = a.seq_idx[b];
    }
#pragma unroll
    for (int u = 0; u < GB_UNR; ++u) {
        const long long s = (long long)v[u] - a.base;
        v[u] = a.feat_block[s < 0 ? 0 : (s >= a.S ? a.S - 1 : s)];
    }
#pragma unroll
    for (int u = 0; u < GB_UNR; ++u) {
        const int blk = v[u] < 0 ? 0 : (v[u] >= a.NB ? a.NB - 1 : v[u]);
        v[u] = a.block_rows[blk];
        off[u] = a.block_off[blk];
    }
    // a row at or behind block_rows (or outside the store) is +0.0: its lanes read the store's first 16 bytes instead -- one line for the whole
    // wave -- and drop them, so that the four loads stay unconditional and in flight together (a load under a branch is waited for at its join)
    bool live[GB_UNR];
#pragma unroll
    for (int u = 0; u < GB_UNR; ++u) {
        const long long row = off[u] + r[u];
        live[u] = (long long)r[u] < v[u] && off[u] >= 0 && row < a.n_rows;
        const size_t at = live[u] ? (size_t)row * a.pitch + c[u] : 0;
        raw[u] = *reinterpret_cast<const u32x4_t*>(static_cast<const T*>(a.feats) + at);
    }
#pragma unroll
    for (int u = 0; u < GB_UNR; ++u)
        if (!live[u]) raw[u] = u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u < GB_UNR; ++u) {
        if (idx0 + u * stride >= total) continue;
        float* dst = a.img_o + (size_t)orow[u] * a.D + c[u];
        float f[EPC];
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = __uint_as_float(raw[u][e]);
        } else {                                                       // bf16 -> fp32: the 16 bits become the upper half, exact
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                f[2 * e] = __uint_as_float(raw[u][e] << 16);
                f[2 * e + 1] = __uint_as_float(raw[u][e] & 0xffff0000u);
            }
        }
#pragma unroll
        for (unsigned g = 0; g < EPC; g += 4) {
            if (c[u] + g + 4 <= (unsigned)a.D) *reinterpret_cast<f32x4_a8*>(dst + g) = f32x4{f[g], f[g + 1], f[g + 2], f[g + 3]};
            else {                                                     // the tail of a row: D is even here, so it is whole pairs
#pragma unroll
                for (unsigned e = 0; e < 4; e += 2)
                    if (c[u] + g + e < (unsigned)a.D) *reinterpret_cast<f32x2_a8*>(dst + g + e) = f32x2{f[g + e], f[g + e + 1]};
            }
        }
    }
}

template <typename T>
__device__ __forceinline__ void gather_feats_scalar(const GatherArgs& a, unsigned block) {
    const size_t total = (size_t)a.B * a.Li2 * a.D, stride = (size_t)a.nfeat * GB_THREADS;
    for (size_t idx = (size_t)block * GB_THREADS + threadIdx.x; idx < total; idx += stride) {
        const size_t orow = idx / a.D;
        const unsigned c = (unsigned)(idx % a.D);
        long long row;
        float v = 0.f;
        if (gather_row(a, gather_seq(a, (unsigned)(orow / a.Li2)), (unsigned)(orow % a.Li2), row))
            v = to_f32(static_cast<const T*>(a.feats)[(size_t)row * a.pitch + c]);
        a.img_o[idx] = v;
    }
}

__device__ __forceinline__ void gather_rows_block(const GatherArgs& a, unsigned block, unsigned nblocks) {
    const unsigned L = a.Lt + a.Li, L2 = a.Lt2 + a.Li2;
    const size_t n_text = (size_t)a.B * a.Lt2, n_mask = (size_t)a.B * L2, n = n_text + n_mask + (a.mpos_o ? (size_t)a.B : 0);
    const size_t stride = (size_t)nblocks * GB_THREADS;
    for (size_t idx = (size_t)block * GB_THREADS + threadIdx.x; idx < n; idx += stride) {
        if (idx < n_text) {
            const unsigned b = (unsigned)(idx / a.Lt2), t = (unsigned)(idx % a.Lt2);
            const size_t src = (size_t)gather_seq(a, b) * a.Lt + t;
            a.ids_o[idx] = a.ids[src];
            a.type_o[idx] = a.seg[src];
        } else if (idx < n_text + n_mask) {
            const size_t j = idx - n_text;
            const unsigned b = (unsigned)(j / L2), c = (unsigned)(j % L2);
            a.mask_o[j] = a.mask[(size_t)gather_seq(a, b) * L + (c < (unsigned)a.Lt2 ? c : a.Lt + (c - a.Lt2))];
        } else {
            const unsigned b = (unsigned)(idx - n_text - n_mask);
            a.mpos_o[b] = a.mask_pos[gather_seq(a, b)];
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(GB_THREADS) void gather_batch_kernel(GatherArgs a) {
    if (blockIdx.x < a.nfeat) {
        if constexpr (VEC) gather_feats_vec<T>(a, blockIdx.x);
        else gather_feats_scalar<T>(a, blockIdx.x);
    } else gather_rows_block(a, blockIdx.x - a.nfeat, gridDim.x - a.nfeat);
}

// ---- cpt_gather_batch_heads: the same launch with the head rows, the labels and the label grid ------------------------------------------------
// A set with head tables (cpt_resident_heads) names, per sequence, the positions a head reads ([MASK] rows) and their labels.  The feature
// workgroups are those of gather_batch_kernel.  The int64-row workgroups write, beside the rows above:
//   label grid  (B, Lt' + Li') of -1 with head_label at the row's head positions, by the workgroups that write the mask row and with the mask's index
//               arithmetic (text column c is padded column c, region column Lt' + j is padded column Lt + j); per element the sequence's few head
//               entries are walked, so that every element is written exactly once: no atomics, no fill in front.
//   head rows   row_first[b] + k = (b, position) of the k-th head entry of sequence seq_idx[b], with its label; one lane per row, the batch entry
//               found by bisection of row_first ([B + 1], the exclusive prefix sum of the head counts of the batch, built by the host).
//   sequence labels  one per batch entry (the relation heads).
// Every index read from memory is clamped: head_first into [0, n_heads], a position into [0, Lt + Li), row_first into [0, R].
struct GatherHeadArgs {
    GatherArgs g;
    const int32_t *head_first, *head_pos, *head_label, *seq_label, *row_first;
    int n_heads, R;
    int64_t *rows_o, *hlab_o, *grid_o, *slab_o;
};

__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the head entries [h0, h1) of store-local sequence `seq`, inside [0, n_heads]
__device__ __forceinline__ void head_range(const GatherHeadArgs& a, int seq, int& h0, int& h1) {
    h0 = clamp_i(a.head_first[seq], 0, a.n_heads);
    h1 = clamp_i(a.head_first[seq + 1], h0, a.n_heads);
}

__device__ __forceinline__ void gather_rows_heads_block(const GatherHeadArgs& a, unsigned block, unsigned nblocks) {
    const GatherArgs& g = a.g;
    const unsigned L = g.Lt + g.Li, L2 = g.Lt2 + g.Li2;
    const size_t n_text = (size_t)g.B * g.Lt2, n_mask = (size_t)g.B * L2, n_pos = g.mpos_o ? (size_t)g.B : 0, n_slab = a.slab_o ? (size_t)g.B : 0;
    const size_t n_rows = (a.rows_o || a.hlab_o) ? (size_t)a.R : 0, n = n_text + n_mask + n_pos + n_slab + n_rows;
    const size_t stride = (size_t)nblocks * GB_THREADS;
    for (size_t idx = (size_t)block * GB_THREADS + threadIdx.x; idx < n; idx += stride) {
        if (idx < n_text) {
            const unsigned b = (unsigned)(idx / g.Lt2), t = (unsigned)(idx % g.Lt2);
            const size_t src = (size_t)gather_seq(g, b) * g.Lt + t;
            g.ids_o[idx] = g.ids[src];
            g.type_o[idx] = g.seg[src];
        } else if (idx < n_text + n_mask) {
            const size_t j = idx - n_text;
            const unsigned b = (unsigned)(j / L2), c = (unsigned)(j % L2);
            const int seq = gather_seq(g, b);
            const unsigned pc = c < (unsigned)g.Lt2 ? c : g.Lt + (c - g.Lt2);          // the padded column of output column c
            g.mask_o[j] = g.mask[(size_t)seq * L + pc];
            if (a.grid_o) {
                int h0, h1;
                head_range(a, seq, h0, h1);
                long long lab = -1;
                for (int h = h0; h < h1; ++h)
                    if ((unsigned)a.head_pos[h] == pc) lab = a.head_label[h];
                a.grid_o[j] = lab;
            }
        } else if (idx < n_text + n_mask + n_pos) {
            const unsigned b = (unsigned)(idx - n_text - n_mask);
            g.mpos_o[b] = g.mask_pos[gather_seq(g, b)];
        } else if (idx < n_text + n_mask + n_pos + n_slab) {
            const unsigned b = (unsigned)(idx - n_text - n_mask - n_pos);
            a.slab_o[b] = a.seq_label[gather_seq(g, b)];
        } else {
            const int r = (int)(idx - n_text - n_mask - n_pos - n_slab);
            int lo = 0, hi = g.B - 1;                                                  // the last batch entry whose first row is <= r
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (clamp_i(a.row_first[mid], 0, a.R) <= r) lo = mid;
                else hi = mid - 1;
            }
            int h0, h1;
            head_range(a, gather_seq(g, (unsigned)lo), h0, h1);
            const int k = r - clamp_i(a.row_first[lo], 0, a.R);
            long long pos = 0, lab = -1;                                               // (a sequence without an entry: tables that disagree)
            if (h1 > h0) {
                const int h = h0 + clamp_i(k, 0, h1 - h0 - 1);
                pos = clamp_i(a.head_pos[h], 0, (int)L - 1);
                if (a.hlab_o) lab = a.head_label[h];
            }
            if (a.rows_o) {
                a.rows_o[2 * (size_t)r] = lo;
                a.rows_o[2 * (size_t)r + 1] = pos;
            }
            if (a.hlab_o) a.hlab_o[r] = lab;
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(GB_THREADS) void gather_batch_heads_kernel(GatherHeadArgs a) {
    if (blockIdx.x < a.g.nfeat) {
        if constexpr (VEC) gather_feats_vec<T>(a.g, blockIdx.x);
        else gather_feats_scalar<T>(a.g, blockIdx.x);
    } else gather_rows_heads_block(a, blockIdx.x - a.g.nfeat, gridDim.x - a.g.nfeat);
}

// the checks of a launch, its feature form and its grid: shared by gather_batch and gather_batch_heads (extra: int64 elements beside the rows
// of gather_batch)
static int gather_plan(const cpt_resident_store* st, const int32_t* seq_idx, int B, int Lt2, int Li2, int64_t* ids_o, int64_t* type_o, int64_t* mask_o,
                       int64_t* mpos_o, float* img_o, size_t extra, GatherArgs& a, bool& vec, size_t& nrow) {
    if (!st || !seq_idx || !ids_o || !type_o || !mask_o) return CPT_ERR_NULL;
    const int Lt = st->Lt, Li = st->Li, D = st->img_dim;
    if (B <= 0 || Lt <= 0 || Li < 0 || Lt2 <= 0 || Lt2 > Lt || Li2 < 0 || Li2 > Li || st->n_seq <= 0) return CPT_ERR_SHAPE;
    if (!st->ids || !st->seg || !st->mask || (mpos_o && !st->mask_pos)) return CPT_ERR_NULL;
    if (st->feat_dtype != CPT_F32 && st->feat_dtype != CPT_BF16) return CPT_ERR_DTYPE;
    const size_t esz = st->feat_dtype == CPT_BF16 ? 2 : 4;
    vec = false;
    size_t nfeat = 0;
    if (Li2 > 0) {
        if (D <= 0 || st->pitch < D || st->n_blocks <= 0 || st->n_rows < 0) return CPT_ERR_SHAPE;
        if (!img_o || !st->feat_block || !st->block_rows || !st->block_off || (st->n_rows > 0 && !st->feats)) return CPT_ERR_NULL;
        if ((uintptr_t)img_o % 4 || (uintptr_t)st->feats % esz) return CPT_ERR_ALIGN;
        // 16-byte loads want 16-byte-aligned store rows; 16-byte stores declared 8-byte aligned want D even and an 8-byte-aligned destination
        vec = D % 2 == 0 && ((uintptr_t)st->feats % 16) == 0 && ((size_t)st->pitch * esz) % 16 == 0 && ((uintptr_t)img_o % 8) == 0;
        const size_t epc = 16 / esz;
        const size_t work = vec ? (size_t)B * Li2 * (((size_t)D + epc - 1) / epc) : (size_t)B * Li2 * D;
        if (vec && work >= 0x7fff0000u) return CPT_ERR_SHAPE;          // (the vector form indexes its pieces in 32 bits)
        // vector form: exactly GB_UNR pieces per lane (its loop is unrolled, not grid-strided); scalar form: grid-strided behind a cap
        nfeat = (work + (size_t)GB_THREADS * GB_UNR - 1) / ((size_t)GB_THREADS * GB_UNR);
        if (!vec && nfeat > 4096) nfeat = 4096;
    }
    const size_t rows = (size_t)B * Lt2 + (size_t)B * (Lt2 + Li2) + (size_t)B + extra;
    nrow = (rows + (size_t)GB_THREADS * 4 - 1) / ((size_t)GB_THREADS * 4);
    nrow = nrow < 1 ? 1 : (nrow > 1024 ? 1024 : nrow);
    a = GatherArgs{st->feats, st->ids, st->seg, st->mask, st->mask_pos, st->feat_block, st->block_rows, st->block_off, (long long)st->n_rows,
                   st->pitch, D, Lt, Li, st->n_seq, st->seq_base, st->n_blocks, seq_idx, B, Lt2, Li2, ids_o, type_o, mask_o, mpos_o, img_o, (unsigned)nfeat};
    return CPT_OK;
}

int gather_batch(const cpt_resident_store* st, const int32_t* seq_idx, int B, int Lt2, int Li2, int64_t* ids_o, int64_t* type_o, int64_t* mask_o,
                 int64_t* mpos_o, float* img_o, hipStream_t s) {
    GatherArgs a;
    bool vec;
    size_t nrow;
    const int rc = gather_plan(st, seq_idx, B, Lt2, Li2, ids_o, type_o, mask_o, mpos_o, img_o, 0, a, vec, nrow);
    if (rc != CPT_OK) return rc;
    const dim3 grid((unsigned)(a.nfeat + nrow)), block(GB_THREADS);
    if (st->feat_dtype == CPT_BF16) {
        if (vec) gather_batch_kernel<bf16, true><<<grid, block, 0, s>>>(a);
        else gather_batch_kernel<bf16, false><<<grid, block, 0, s>>>(a);
    } else {
        if (vec) gather_batch_kernel<float, true><<<grid, block, 0, s>>>(a);
        else gather_batch_kernel<float, false><<<grid, block, 0, s>>>(a);
    }
    return CPT_OK;
}

int gather_batch_heads(const cpt_resident_store* st, const cpt_resident_heads* hd, const int32_t* seq_idx, const int32_t* row_first, int B, int R,
                       int Lt2, int Li2, int64_t* ids_o, int64_t* type_o, int64_t* mask_o, int64_t* mpos_o, float* img_o, int64_t* rows_o,
                       int64_t* hlab_o, int64_t* grid_o, int64_t* slab_o, hipStream_t s) {
    if (!hd) return CPT_ERR_NULL;
    if (R < 0 || hd->n_heads < 0) return CPT_ERR_SHAPE;
    const bool rows = (rows_o || hlab_o) && R > 0;                     // (R = 0: the row outputs are empty, nothing of theirs is read)
    if ((rows || grid_o) && (!hd->head_first || (hd->n_heads > 0 && !hd->head_pos))) return CPT_ERR_NULL;
    if (rows && !row_first) return CPT_ERR_NULL;
    if (((hlab_o && R > 0) || grid_o) && !hd->head_label) return CPT_ERR_NULL;
    if (slab_o && !hd->seq_label) return CPT_ERR_NULL;
    if (rows && hd->n_heads == 0) return CPT_ERR_SHAPE;                // (rows to write and no entry to take them from)
    GatherHeadArgs a;
    bool vec;
    size_t nrow;
    const size_t extra = (slab_o ? (size_t)B : 0) + (rows ? (size_t)R : 0) + (grid_o && st ? (size_t)B * (size_t)(Lt2 + Li2 > 0 ? Lt2 + Li2 : 0) : 0);
    const int rc = gather_plan(st, seq_idx, B, Lt2, Li2, ids_o, type_o, mask_o, mpos_o, img_o, extra, a.g, vec, nrow);
    if (rc != CPT_OK) return rc;
    a.head_first = hd->head_first, a.head_pos = hd->head_pos, a.head_label = hd->head_label, a.seq_label = hd->seq_label, a.row_first = row_first;
    a.n_heads = hd->n_heads, a.R = rows ? R : 0;
    a.rows_o = rows ? rows_o : nullptr, a.hlab_o = rows ? hlab_o : nullptr, a.grid_o = grid_o, a.slab_o = slab_o;
    const dim3 grid((unsigned)(a.g.nfeat + nrow)), block(GB_THREADS);
    if (st->feat_dtype == CPT_BF16) {
        if (vec) gather_batch_heads_kernel<bf16, true><<<grid, block, 0, s>>>(a);
        else gather_batch_heads_kernel<bf16, false><<<grid, block, 0, s>>>(a);
    } else {
        if (vec) gather_batch_heads_kernel<float, true><<<grid, block, 0, s>>>(a);
        else gather_batch_heads_kernel<float, false><<<grid, block, 0, s>>>(a);
    }
    return CPT_OK;
}

}  // namespace cpt
