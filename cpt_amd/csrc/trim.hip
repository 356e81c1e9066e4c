// Length-aware evaluation on padded device batches (cpt_batch_extents, cpt_trim_batch): how far the attended part of a batch reaches, and
// the contiguous copy of that part.
//   batch_extents: one pass over the (B, Lt + Li) int64 mask, 16 bytes per lane where the mask allows it.  Every lane keeps the largest
//                  1 + index of a non-zero entry of either part, a wave reduces by shuffles, a workgroup through LDS, and one integer
//                  atomic max per workgroup and part lands in out[2] (zeroed by a memset node in front).  Integer max only: the result
//                  does not depend on the order of arrival.
//   trim_batch:    one launch.  The first workgroups copy the region features: per sequence the Li' x D floats that stay are contiguous
//                  in the source and in the destination, and with D even (2054) both start on 8-byte boundaries, so they move as
//                  16-byte accesses declared 8-byte aligned (as pad_cast reads them), a scalar tail behind; four chunks per lane in
//                  flight before the first store.  The other workgroups copy the int64 rows (ids, token types, position ids, mask -- and,
//                  for cpt_trim_batch_labels, a (B, Lt + Li) label grid cut exactly as the mask is).
// Length-aware training (cpt_train_extents, cpt_trim_batch_labels):
//   train_extents: the extents of a mask TOGETHER with what the loss reads: a (B, Lt + Li) label grid (-1 = no label) or a list of labelled
//                  positions.  ONE workgroup, no memset node and no atomic of any kind: every lane walks the flat mask (and grid) in 16-byte
//                  reads, consecutive lanes on consecutive addresses along L, a wave reduces by shuffles, the four wave results meet in LDS
//                  and lane 0 combines them in wave order and stores the two words.  A few-shot training batch is 4 x 210 entries.
#include "common.h"
#include "kernels.h"

namespace cpt {

typedef long long i64x2 __attribute__((ext_vector_type(2)));

constexpr int TR_THREADS = 256;
constexpr int EXT_MAX_GROUPS = 1024;        // grid cap of the extents pass: the rest is grid-strided

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// position p of a head row: a text position must survive the trim; a region position (or one outside the sequence) keeps the text whole
__device__ __forceinline__ void extent_of_pos(long long p, int Lt, int Li, int& tmax, int& imax) {
    if (p >= 0 && p < Lt) tmax = max(tmax, (int)p + 1);
    else {
        tmax = Lt;
        imax = (p >= Lt && p < (long long)Lt + Li) ? max(imax, (int)(p - Lt) + 1) : Li;
    }
}

__global__ __launch_bounds__(TR_THREADS) void batch_extents_kernel(const int64_t* __restrict__ mask, int B, int Lt, int Li,
                                                                   const int64_t* __restrict__ mask_pos, int n_pos, int* __restrict__ out, int vec) {
    __shared__ int lds[2][TR_THREADS / 64];
    const int L = Lt + Li;
    const size_t total = (size_t)B * L;
    const size_t tid = (size_t)blockIdx.x * TR_THREADS + threadIdx.x, stride = (size_t)gridDim.x * TR_THREADS;
    int tmax = 1, imax = 0;                 // (the [CLS] row always stays)
    auto see = [&](size_t idx, long long v) {
        if (v == 0) return;
        const int c = (int)(idx % L);
        if (c < Lt) tmax = max(tmax, c + 1);
        else imax = max(imax, c - Lt + 1);
    };
    if (vec) {                              // mask 16-byte aligned: pairs of entries, the odd last one by thread 0
        const i64x2* m2 = reinterpret_cast<const i64x2*>(mask);
        const size_t n2 = total / 2;
        for (size_t i = tid; i < n2; i += stride) {
            const i64x2 v = m2[i];
            see(2 * i, v[0]);
            see(2 * i + 1, v[1]);
        }
        if (tid == 0 && (total & 1)) see(total - 1, mask[total - 1]);
    } else {
        for (size_t i = tid; i < total; i += stride) see(i, mask[i]);
    }
    if (mask_pos)
        for (size_t i = tid; i < (size_t)n_pos; i += stride) extent_of_pos(mask_pos[i], Lt, Li, tmax, imax);
    tmax = wave_max_i(tmax);
    imax = wave_max_i(imax);
    if ((threadIdx.x & 63) == 0) { lds[0][threadIdx.x >> 6] = tmax; lds[1][threadIdx.x >> 6] = imax; }
    __syncthreads();
    if (threadIdx.x < 2) {
        int v = lds[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < TR_THREADS / 64; ++w) v = max(v, lds[threadIdx.x][w]);
        atomicMax(out + threadIdx.x, v);
    }
}

int batch_extents(const int64_t* mask, int B, int Lt, int Li, const int64_t* mask_pos, int n_pos, int32_t* out, hipStream_t s) {
    if (B <= 0 || Lt <= 0 || Li < 0 || n_pos < 0) return CPT_ERR_SHAPE;
    if (!mask || !out || (n_pos > 0 && !mask_pos)) return CPT_ERR_NULL;
    if ((uintptr_t)mask % 8 || (uintptr_t)out % 4) return CPT_ERR_ALIGN;
    const hipError_t e = hipMemsetAsync(out, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) return CPT_ERR_HIP - (int)e;
    const size_t total = (size_t)B * (Lt + Li);
    const int vec = ((uintptr_t)mask % 16) == 0;
    const size_t per = (size_t)TR_THREADS * (vec ? 2 : 1) * 4;                            // at least four accesses per lane before the grid grows
    size_t groups = (total + per - 1) / per;
    groups = groups < 1 ? 1 : (groups > (size_t)EXT_MAX_GROUPS ? (size_t)EXT_MAX_GROUPS : groups);
    batch_extents_kernel<<<dim3((unsigned)groups), dim3(TR_THREADS), 0, s>>>(mask, B, Lt, Li, n_pos > 0 ? mask_pos : nullptr, n_pos, out, vec);
    return CPT_OK;
}

// ---- train_extents ----
// One workgroup.  flat: the (B, L) array; LABELS: an entry counts when it is != -1 and follows the head-row rule (extent_of_pos), else when it
// is != 0 and follows the mask rule.  vec: the array is 16-byte aligned.
template <bool LABELS>
__device__ __forceinline__ void extent_scan(const int64_t* __restrict__ flat, size_t total, int L, int Lt, int Li, int vec, int& tmax, int& imax) {
    auto see = [&](size_t idx, long long v) {
        if (LABELS ? v == -1 : v == 0) return;
        const int c = (int)(idx % L);
        if (LABELS) extent_of_pos(c, Lt, Li, tmax, imax);
        else if (c < Lt) tmax = max(tmax, c + 1);
        else imax = max(imax, c - Lt + 1);
    };
    if (vec) {
        const i64x2* m2 = reinterpret_cast<const i64x2*>(flat);
        const size_t n2 = total / 2;
        for (size_t i = threadIdx.x; i < n2; i += TR_THREADS) {
            const i64x2 v = m2[i];
            see(2 * i, v[0]);
            see(2 * i + 1, v[1]);
        }
        if (threadIdx.x == 0 && (total & 1)) see(total - 1, flat[total - 1]);
    } else {
        for (size_t i = threadIdx.x; i < total; i += TR_THREADS) see(i, flat[i]);
    }
}

__global__ __launch_bounds__(TR_THREADS) void train_extents_kernel(const int64_t* __restrict__ mask, int B, int Lt, int Li,
                                                                   const int64_t* __restrict__ grid, const int64_t* __restrict__ pos, int n_pos,
                                                                   int* __restrict__ out, int vec_mask, int vec_grid) {
    __shared__ int lds[2][TR_THREADS / 64];
    const int L = Lt + Li;
    const size_t total = (size_t)B * L;
    int tmax = 1, imax = 0;                 // (the [CLS] row always stays)
    extent_scan<false>(mask, total, L, Lt, Li, vec_mask, tmax, imax);
    if (grid) extent_scan<true>(grid, total, L, Lt, Li, vec_grid, tmax, imax);
    if (pos)
        for (int i = threadIdx.x; i < n_pos; i += TR_THREADS) extent_of_pos(pos[i], Lt, Li, tmax, imax);
    tmax = wave_max_i(tmax);
    imax = wave_max_i(imax);
    if ((threadIdx.x & 63) == 0) { lds[0][threadIdx.x >> 6] = tmax; lds[1][threadIdx.x >> 6] = imax; }
    __syncthreads();
    if (threadIdx.x == 0) {                 // the fixed-order combine: waves 0, 1, 2, 3
        int t = lds[0][0], r = lds[1][0];
#pragma unroll
        for (int w = 1; w < TR_THREADS / 64; ++w) { t = max(t, lds[0][w]); r = max(r, lds[1][w]); }
        out[0] = t;
        out[1] = r;
    }
}

int train_extents(const int64_t* mask, int B, int Lt, int Li, const int64_t* grid, const int64_t* pos, int n_pos, int32_t* out, hipStream_t s) {
    if (B <= 0 || Lt <= 0 || Li < 0 || n_pos < 0) return CPT_ERR_SHAPE;
    if (!mask || !out || (n_pos > 0 && !pos)) return CPT_ERR_NULL;
    if ((uintptr_t)mask % 8 || (grid && (uintptr_t)grid % 8) || (uintptr_t)out % 4) return CPT_ERR_ALIGN;
    train_extents_kernel<<<dim3(1), dim3(TR_THREADS), 0, s>>>(mask, B, Lt, Li, grid, n_pos > 0 ? pos : nullptr, n_pos, out,
                                                              ((uintptr_t)mask % 16) == 0, grid && ((uintptr_t)grid % 16) == 0);
    return CPT_OK;
}

// ---- trim_batch ----
constexpr int TB_UNR = 4;

struct TrimArgs {
    const int64_t *ids, *type, *pos, *mask;
    const float* img;
    int64_t *ids_o, *type_o, *pos_o, *mask_o;
    float* img_o;
    const int64_t* grid;                     // optional (B, Lt + Li) label grid, cut as the mask is (cpt_trim_batch_labels)
    int64_t* grid_o;
    int B, Lt, Li, D, Lt2, Li2;
    unsigned nfeat;                          // workgroups [0, nfeat) copy the region features, the others the int64 rows
};

template <bool VEC>
__device__ __forceinline__ void trim_feats_block(const TrimArgs& a, unsigned block) {
    const size_t seg = (size_t)a.Li2 * a.D;                           // floats kept per sequence: contiguous on both sides
    const size_t src_seq = (size_t)a.Li * a.D;
    if constexpr (VEC) {
        typedef f32x4 f32x4_a8 __attribute__((aligned(8)));
        const size_t cps = (seg + 3) / 4;                             // chunks of four floats per sequence, the last one possibly short
        const size_t total = (size_t)a.B * cps, stride = (size_t)a.nfeat * TR_THREADS;
        const size_t idx0 = (size_t)block * TR_THREADS + threadIdx.x;
        f32x4 v[TB_UNR];
#pragma unroll
        for (int u = 0; u < TB_UNR; ++u) {
            const size_t idx = idx0 + u * stride;
            if (idx >= total) continue;
            const size_t b = idx / cps, c = (idx % cps) * 4;
            const float* src = a.img + b * src_seq + c;
            if (c + 4 <= seg) v[u] = *reinterpret_cast<const f32x4_a8*>(src);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[u][e] = c + e < seg ? src[e] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < TB_UNR; ++u) {
            const size_t idx = idx0 + u * stride;
            if (idx >= total) continue;
            const size_t b = idx / cps, c = (idx % cps) * 4;
            float* dst = a.img_o + b * seg + c;
            if (c + 4 <= seg) *reinterpret_cast<f32x4_a8*>(dst) = v[u];
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < seg) dst[e] = v[u][e];
            }
        }
    } else {
        const size_t total = (size_t)a.B * seg, stride = (size_t)a.nfeat * TR_THREADS;
        for (size_t idx = (size_t)block * TR_THREADS + threadIdx.x; idx < total; idx += stride) {
            const size_t b = idx / seg, c = idx % seg;
            a.img_o[idx] = a.img[b * src_seq + c];
        }
    }
}

__device__ __forceinline__ void trim_rows_block(const TrimArgs& a, unsigned block, unsigned nblocks) {
    const int L2 = a.Lt2 + a.Li2;
    const size_t n_text = (size_t)a.B * a.Lt2, n_mask = (size_t)a.B * L2;
    const size_t stride = (size_t)nblocks * TR_THREADS;
    for (size_t idx = (size_t)block * TR_THREADS + threadIdx.x; idx < n_text + n_mask; idx += stride) {
        if (idx < n_text) {
            const size_t b = idx / a.Lt2, src = b * a.Lt + idx % a.Lt2;
            a.ids_o[idx] = a.ids[src];
            if (a.type) a.type_o[idx] = a.type[src];
            if (a.pos) a.pos_o[idx] = a.pos[src];
        } else {
            const size_t j = idx - n_text, b = j / L2;
            const int c = (int)(j % L2);
            const size_t src = b * (a.Lt + a.Li) + (c < a.Lt2 ? c : a.Lt + (c - a.Lt2));
            a.mask_o[j] = a.mask[src];
            if (a.grid) a.grid_o[j] = a.grid[src];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(TR_THREADS) void trim_batch_kernel(TrimArgs a) {
    if (blockIdx.x < a.nfeat) trim_feats_block<VEC>(a, blockIdx.x);
    else trim_rows_block(a, blockIdx.x - a.nfeat, gridDim.x - a.nfeat);
}

int trim_batch(const int64_t* ids, const int64_t* type, const int64_t* pos, const int64_t* mask, const float* img, int B, int Lt, int Li, int D,
               int Lt2, int Li2, int64_t* ids_o, int64_t* type_o, int64_t* pos_o, int64_t* mask_o, float* img_o, hipStream_t s,
               const int64_t* lab, int64_t* lab_o) {
    if (B <= 0 || Lt <= 0 || Li < 0 || Lt2 <= 0 || Lt2 > Lt || Li2 < 0 || Li2 > Li || (Li2 > 0 && D <= 0)) return CPT_ERR_SHAPE;
    if (!ids || !mask || !ids_o || !mask_o || (type && !type_o) || (pos && !pos_o) || (Li2 > 0 && (!img || !img_o)) || (lab && !lab_o))
        return CPT_ERR_NULL;
    const size_t seg = (size_t)Li2 * D;
    const bool vec = seg > 0 && D % 2 == 0 && ((uintptr_t)img % 8) == 0 && ((uintptr_t)img_o % 8) == 0;
    const size_t work = seg == 0 ? 0 : (vec ? (size_t)B * ((seg + 3) / 4) : (size_t)B * seg);
    // vector form: exactly TB_UNR chunks per lane (its loop is unrolled, not grid-strided); scalar form: grid-strided behind a cap
    size_t nfeat = (work + (size_t)TR_THREADS * TB_UNR - 1) / ((size_t)TR_THREADS * TB_UNR);
    if (!vec && nfeat > 4096) nfeat = 4096;
    if (nfeat > 0x7fff0000u) return CPT_ERR_SHAPE;
    const size_t rows = (size_t)B * Lt2 + (size_t)B * (Lt2 + Li2);
    size_t nrow = (rows + (size_t)TR_THREADS * 4 - 1) / ((size_t)TR_THREADS * 4);
    nrow = nrow < 1 ? 1 : (nrow > 1024 ? 1024 : nrow);
    TrimArgs a{ids, type, pos, mask, img, ids_o, type_o, pos_o, mask_o, img_o, lab, lab ? lab_o : nullptr, B, Lt, Li, D, Lt2, Li2, (unsigned)nfeat};
    const dim3 grid((unsigned)(nfeat + nrow)), block(TR_THREADS);
    if (vec) trim_batch_kernel<true><<<grid, block, 0, s>>>(a);
    else trim_batch_kernel<false><<<grid, block, 0, s>>>(a);
    return CPT_OK;
}

}  // namespace cpt
