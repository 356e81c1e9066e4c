// RefCOCO REC evaluation on the device (cpt_rec_choose): selection, IoU and the accuracy counts of one batch of queries in one launch.
//   Replaces the two val() post-loops (Oscar/oscar/zeroshot/refcoco_cpt.py:224-246, 267-280; fewshot/refcoco_cpt.py:277-297, 305-315) and
//   computeIoU (utils/iou.py:1-13).  The split's tables are uploaded once (scoring.rec_eval_table); per batch only q_index arrives.
//   One wave per query of the batch:
//     * the batch row of the query's first proposal sequence = the sequence counts of the queries before it in q_index, summed by the wave;
//     * lanes stride the query's candidates in concatenation order (sequence by sequence, colour by colour), 64 per trip.  A candidate's
//       sequence comes from registers: per block of 64 sequences every lane counts the colours of one sequence, an inclusive scan over the
//       lanes gives the candidate offsets, and a six-step search over them by shuffles places the lane's candidate -- so all loads of a trip
//       are in flight together and nothing walks the sequences one after the other; the score is the raw logit at
//       the candidate's colour column, or that logit / the sequence's "none" logit (the fp32 division cpt_select_regions performs); each lane
//       keeps its first maximum and a cross-lane (value, index) reduction applies torch.argmax's rule: a NaN beats any number, then the larger
//       value, then the lower index, -0 == +0;
//     * lane 0 turns the chosen x1, y1, x2, y2 into [x1, y1, x2 - x1 + 1, y2 - y1 + 1] and computes computeIoU against the annotation in float64,
//       operation by operation as Python does (no contraction: a fused w1 * h1 + w2 * h2 would round once where Python rounds twice), sets
//       correct = iou > 0.5 and bumps counts[0] (correct) / counts[1] (evaluated) with integer atomics.
//   The table builder has already refused degenerate rectangles, so there is no error path here; rows, columns and query indices outside
//   their arrays are skipped, never read or written.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace cpt {

constexpr int RC_THREADS = 256;
constexpr int RC_QUERIES = RC_THREADS / 64;   // one wave per query
constexpr int RC_NONE = 0x7fffffff;            // "no candidate": loses every comparison on the index

// (value, index) a is the better argmax candidate than b
static __device__ __forceinline__ bool rec_better(float va, int ia, float vb, int ib) {
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return (na && nb) ? ia < ib : na;
    if (va != vb) return va > vb;
    return ia < ib;
}

// Python's max(a, b) / min(a, b): the first argument unless the second is strictly larger / smaller
static __device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
static __device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }

// utils/iou.py:1-13 on box1 = [x1, y1, x2 - x1 + 1, y2 - y1 + 1] (refcoco_cpt.py:273) and box2 = the annotation [x, y, w, h]
static __device__ __forceinline__ double rec_iou(const double* __restrict__ r, const double* __restrict__ g) {
#pragma clang fp contract(off)
    const double b0 = r[0], b1 = r[1], b2 = r[2] - r[0] + 1.0, b3 = r[3] - r[1] + 1.0;
    const double g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
    const double ix1 = py_max(b0, g0);
    const double iy1 = py_max(b1, g1);
    const double ix2 = py_min(b0 + b2 - 1.0, g0 + g2 - 1.0);
    const double iy2 = py_min(b1 + b3 - 1.0, g1 + g3 - 1.0);
    double inter = 0.0;
    if (ix1 < ix2 && iy1 < iy2) inter = (ix2 - ix1 + 1.0) * (iy2 - iy1 + 1.0);
    const double area1 = b2 * b3;
    const double area2 = g2 * g3;
    const double uni = area1 + area2 - inter;
    return inter / uni;
}

__global__ __launch_bounds__(RC_THREADS) void rec_choose_kernel(const float* __restrict__ scores, int S, int V, const int32_t* __restrict__ q_index,
                                                                int Qb, int Q, const int32_t* __restrict__ seq_first,
                                                                const int32_t* __restrict__ cols, int C, const int32_t* __restrict__ cand_first,
                                                                const double* __restrict__ rects, const double* __restrict__ gt,
                                                                const uint8_t* __restrict__ has_gt, int none, int divide_by_none,
                                                                int32_t* __restrict__ idx, float* __restrict__ score, double* __restrict__ iou,
                                                                uint8_t* __restrict__ correct, float* __restrict__ cand_score, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * RC_QUERIES + (threadIdx.x >> 6);
    if (w >= Qb) return;                               // (wave-uniform)
    const int q = q_index[w];
    if (q < 0 || q >= Q) return;                       // (wave-uniform)
    // batch row of the query's first sequence: the queries before it in the batch, in q_index order
    int row0 = 0;
    for (int j = lane; j < w; j += 64) {
        const int p = q_index[j];
        if (p >= 0 && p < Q) row0 += seq_first[p + 1] - seq_first[p];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) row0 += __shfl_xor(row0, d, 64);
    const int s0 = seq_first[q], s1 = seq_first[q + 1];
    const int c0 = cand_first[q], n_cand = cand_first[q + 1] - c0;
    float bv = -INFINITY;
    int bi = RC_NONE;
    int base = 0;                                      // candidates before the current block of 64 sequences (uniform)
    for (int sb = s0; sb < s1; sb += 64) {             // (uniform)
        // the lane's sequence of the block: its colour count (padding is trailing, so the count of entries >= 0), all lanes' loads in flight at once
        const int sm = sb + lane;
        int n_own = 0;
        if (sm < s1)
            for (int c = 0; c < C; ++c) n_own += cols[(size_t)sm * C + c] >= 0;
        int incl = n_own;                              // inclusive scan over the lanes: candidates up to and including the lane's sequence
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        const int first = incl - n_own;
        const int T = __shfl(incl, 63, 64);            // candidates of the block (uniform)
        for (int t = 0; t < T; t += 64) {              // one trip per 64 candidates; ascending: the lane keeps the first maximum of its stride
            const int kl = t + lane;
            int j = 0;                                 // the candidate's sequence: the number of lanes whose inclusive count is <= kl
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1)
                if (__shfl(incl, j + step - 1, 64) <= kl) j += step;
            const int fj = __shfl(first, j, 64);
            const int k = base + kl;
            if (kl >= T || k >= n_cand) continue;
            const int s = sb + j;
            const int row = row0 + (s - s0);
            const int col = cols[(size_t)s * C + (kl - fj)];
            if (row >= S || col < 0 || col >= V) continue;
            const float* x = scores + (size_t)row * V;
            float v = x[col];
            if (divide_by_none) v = v / x[none];
            if (cand_score) cand_score[(size_t)c0 + k] = v;
            if (rec_better(v, k, bv, bi)) { bv = v; bi = k; }
        }
        base += T;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(bv, d, 64);
        const int oi = __shfl_xor(bi, d, 64);
        if (rec_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        const bool chosen = bi != RC_NONE;
        const bool judged = chosen && has_gt[q];
        double u = __longlong_as_double(0x7ff8000000000000LL);      // not judged: the quiet NaN of float("nan")
        if (judged) u = rec_iou(rects + ((size_t)c0 + bi) * 4, gt + (size_t)q * 4);
        const int ok = judged && u > 0.5;
        idx[q] = chosen ? bi : -1;
        score[q] = bv;
        iou[q] = u;
        correct[q] = (uint8_t)ok;
        if (judged) atomicAdd(counts + 1, 1);
        if (ok) atomicAdd(counts, 1);
    }
}

int rec_choose(const float* scores, int S, int V, const int32_t* q_index, int Qb, int Q, const int32_t* seq_first, const int32_t* cols, int C,
               const int32_t* cand_first, const double* rects, const double* gt, const uint8_t* has_gt, int none, int divide_by_none, int32_t* idx,
               float* score, double* iou, uint8_t* correct, float* cand_score, int* counts, hipStream_t s) {
    rec_choose_kernel<<<dim3((Qb + RC_QUERIES - 1) / RC_QUERIES), dim3(RC_THREADS), 0, s>>>(scores, S, V, q_index, Qb, Q, seq_first, cols, C, cand_first,
                                                                                             rects, gt, has_gt, none, divide_by_none, idx, score, iou,
                                                                                             correct, cand_score, counts);
    return CPT_OK;
}

}  // namespace cpt
