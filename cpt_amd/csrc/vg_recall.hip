// VG-CPT Recall@K on the device (Oscar/oscar/utils/vg_eval.py eval_vg, the per-image loop): one workgroup per image.
//   Each candidate (subject, object, score row) takes rel = argmax(row[1:]) + 1 (torch.argmax: first maximum, NaN counts as the maximum)
//   and score = row[rel]; the image's candidates are ranked by score, descending, ties by candidate order, NaN first (a stable
//   torch.sort(descending=True)); every ground-truth triplet (s, o, r) gets the rank of the candidate with the same (s, o) whose
//   predicted relation is r, INT32_MAX if there is none.  Hit@K of a triplet is then rank < K for any K.
//   Ranking: a candidate's sort word is (~ordered(score) << 32 | index), unique per image, ascending = the rank order.
//     n <= VGR_TILE: bitonic sort of the words in LDS (a power of two >= n, padded with ~0).
//     n >  VGR_TILE: the words go to a workspace slice the workgroup claims with one atomic; a candidate's rank is the count of
//                    smaller words, counted against VGR_TILE-word chunks staged through LDS.  Exact, O(n^2 / 256) per image.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace cpt {

constexpr int VGR_THREADS = 256;
constexpr int VGR_TILE = 4096;          // 32 KiB of sort words + 16 KiB of relations: VG150's 62-box images (3782 ordered pairs) fit

// float -> uint32, ascending with the float order; every NaN is the largest value and -0 equals +0 (torch.sort's comparisons)
__device__ __forceinline__ uint32_t vgr_ordered(float f) {
    if (f != f) return 0xFFFFFFFFu;
    if (f == 0.f) f = 0.f;
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// rel = argmax(row[1:]) + 1 and its score; row < 0 (or outside [0, n_rows)): the reference's all-zero dummy row -> rel 1, score 0
__device__ __forceinline__ uint64_t vgr_word(const float* __restrict__ scores, int n_rows, int C, int row, uint32_t j, int* rel_out) {
    int rel = 1;
    float best = 0.f;
    if (row >= 0 && row < n_rows) {
        const float* x = scores + (size_t)row * C;
        best = x[1];
        for (int c = 2; c < C; ++c) {
            const float v = x[c];
            if (best != best) break;                       // the first NaN wins
            if (v > best || v != v) { best = v; rel = c; }
        }
    }
    *rel_out = rel;
    return ((uint64_t)(~vgr_ordered(best)) << 32) | j;
}

__device__ __forceinline__ void vgr_match(const int32_t* __restrict__ cand, const int32_t* __restrict__ gt, int32_t* __restrict__ out_rank,
                                          int c, int rel, int g0, int ng, int rank) {
    const int s = cand[3 * c], o = cand[3 * c + 1];
    for (int g = 0; g < ng; ++g) {
        const int32_t* t = gt + 3 * (g0 + g);
        if (t[0] == s && t[1] == o && t[2] == rel) atomicMin(out_rank + g0 + g, rank);   // (several candidates of one (s, o): the best rank)
    }
}

__global__ __launch_bounds__(VGR_THREADS) void vg_recall_kernel(const float* __restrict__ scores, int n_rows, int C,
                                                                const int32_t* __restrict__ cand_off, const int32_t* __restrict__ cand, int n_cand,
                                                                const int32_t* __restrict__ gt_off, const int32_t* __restrict__ gt, int n_gt,
                                                                int32_t* __restrict__ out_rank, unsigned long long* __restrict__ counter,
                                                                uint64_t* __restrict__ ws_word, int32_t* __restrict__ ws_rel, long long ws_cap) {
    __shared__ uint64_t word[VGR_TILE];
    __shared__ int32_t rel_s[VGR_TILE];
    __shared__ long long base_s;
    const int img = blockIdx.x, tid = threadIdx.x;
    const int c0 = cand_off[img], c1 = cand_off[img + 1], g0 = gt_off[img], g1 = gt_off[img + 1];
    if (g0 < 0 || g1 < g0 || g1 > n_gt) return;                                   // (the host builds the tables; never fault)
    const int ng = g1 - g0;
    const bool bad = c0 < 0 || c1 < c0 || c1 > n_cand;
    const int n = bad ? 0 : c1 - c0;
    for (int g = tid; g < ng; g += VGR_THREADS) out_rank[g0 + g] = bad ? -1 : INT32_MAX;
    if (bad || n == 0) return;
    if (n <= VGR_TILE) {
        int P = 2;
        while (P < n) P <<= 1;
        for (int j = tid; j < P; j += VGR_THREADS) {
            if (j < n) {
                int r;
                word[j] = vgr_word(scores, n_rows, C, cand[3 * (c0 + j) + 2], (uint32_t)j, &r);
                rel_s[j] = r;
            } else {
                word[j] = ~0ull;
            }
        }
        __syncthreads();                                    // (also orders the INT32_MAX stores before the atomics below)
        for (int k = 2; k <= P; k <<= 1) {
            for (int h = k >> 1; h > 0; h >>= 1) {
                for (int i = tid; i < P; i += VGR_THREADS) {
                    const int p = i ^ h;
                    if (p > i) {
                        const uint64_t a = word[i], b = word[p];
                        if ((a > b) == ((i & k) == 0)) { word[i] = b; word[p] = a; }
                    }
                }
                __syncthreads();
            }
        }
        for (int p = tid; p < n; p += VGR_THREADS) {
            const int j = (int)(uint32_t)word[p];
            vgr_match(cand, gt, out_rank, c0 + j, rel_s[j], g0, ng, p);
        }
        return;
    }
    // more candidates than the tile: words in a claimed workspace slice, ranks by counting
    if (tid == 0) base_s = (counter && (long long)n <= ws_cap) ? (long long)atomicAdd(counter, (unsigned long long)n) : ws_cap;
    __syncthreads();
    const long long base = base_s;
    if (base + n > ws_cap) {                                // workspace too small for this split: -1 marks the image's triplets
        for (int g = tid; g < ng; g += VGR_THREADS) out_rank[g0 + g] = -1;
        return;
    }
    uint64_t* w = ws_word + base;
    int32_t* rl = ws_rel + base;
    for (int j = tid; j < n; j += VGR_THREADS) {
        int r;
        w[j] = vgr_word(scores, n_rows, C, cand[3 * (c0 + j) + 2], (uint32_t)j, &r);
        rl[j] = r;
    }
    __syncthreads();
    for (int jb = 0; jb < n; jb += VGR_THREADS) {
        const int j = jb + tid;
        const uint64_t mine = j < n ? w[j] : 0ull;
        int cnt = 0;
        for (int cs = 0; cs < n; cs += VGR_TILE) {
            const int m = min(VGR_TILE, n - cs);
            __syncthreads();
            for (int i = tid; i < m; i += VGR_THREADS) word[i] = w[cs + i];
            __syncthreads();
            if (j < n)
                for (int i = 0; i < m; ++i) cnt += word[i] < mine;
        }
        if (j < n) vgr_match(cand, gt, out_rank, c0 + j, rl[j], g0, ng, cnt);
    }
}

size_t vg_recall_ws_bytes(long long n_big) { return n_big > 0 ? 16 + (size_t)n_big * 12 : 0; }

int vg_recall(const float* scores, int n_rows, int C, const int32_t* cand_off, const int32_t* cand, int n_cand, const int32_t* gt_off,
              const int32_t* gt, int n_gt, int n_img, int32_t* out_rank, void* ws, size_t ws_bytes, hipStream_t s) {
    if (n_img <= 0 || C < 2 || n_rows < 0 || n_cand < 0 || n_gt < 0) return CPT_ERR_SHAPE;
    if (!cand_off || !gt_off || (n_rows > 0 && !scores) || (n_cand > 0 && !cand) || (n_gt > 0 && (!gt || !out_rank))) return CPT_ERR_NULL;
    if (n_gt == 0) return CPT_OK;
    unsigned long long* counter = nullptr;
    uint64_t* words = nullptr;
    int32_t* rels = nullptr;
    long long cap = 0;
    if (ws && ws_bytes >= 16 + 12) {
        cap = (long long)((ws_bytes - 16) / 12);
        counter = (unsigned long long*)ws;
        words = (uint64_t*)((char*)ws + 16);
        rels = (int32_t*)(words + cap);
        hipError_t e = hipMemsetAsync(counter, 0, sizeof(unsigned long long), s);
        if (e != hipSuccess) return CPT_ERR_HIP - (int)e;
    }
    vg_recall_kernel<<<dim3(n_img), dim3(VGR_THREADS), 0, s>>>(scores, n_rows, C, cand_off, cand, n_cand, gt_off, gt, n_gt, out_rank, counter,
                                                               words, rels, cap);
    return CPT_OK;
}

int vg_recall_tile() { return VGR_TILE; }

}  // namespace cpt
