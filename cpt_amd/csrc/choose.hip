// Evaluation choices of the GQA-CPT and VCR Q->A drivers, and global-norm gradient clipping, each without a host round trip.
//   gqa_choose:  gqa_cpt.py:598-612 -- per question the first-maximum argmax over the label-order columns (one wave per row, lanes stride the
//                columns, a cross-lane (value, index) reduction that breaks ties to the lower index), the multi-ground-truth correctness on
//                string ids, and the count of correct rows (integer atomic).
//   nsp_choose:  vcr_nsp_cpt.py:600-611 -- choice score 1 - softmax(rel)[1] per sequence, first-maximum argmax inside each question's `interval`
//                sequences, correctness against the question's label, count.
//   grad_clip:   torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False) on one flat fp32 buffer, two launches: per-workgroup partial sums of
//                squares, added in a FIXED order by the last workgroup to finish (ticket) -> norm, coef = min(1, max_norm / (norm + 1e-6));
//                then g *= coef with 16-byte accesses.  No float atomics: the same buffer gives the same norm bit for bit.
// torch.argmax rules everywhere: the first maximum wins, NaN counts as the maximum (the first NaN wins), -0 == +0 is a tie.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace cpt {

// (value, index) a is the better argmax candidate than b
__device__ __forceinline__ bool arg_better(float va, int ia, float vb, int ib) {
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return (na && nb) ? ia < ib : na;
    if (va != vb) return va > vb;
    return ia < ib;
}

constexpr int GC_THREADS = 256;
constexpr int GC_ROWS = GC_THREADS / 64;      // one wave per row

__global__ __launch_bounds__(GC_THREADS) void gqa_choose_kernel(const float* __restrict__ scores, int R, int C, const int32_t* __restrict__ piece_sid,
                                                                const int32_t* __restrict__ gt_sid, int G, int64_t* __restrict__ pred,
                                                                uint8_t* __restrict__ correct, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * GC_ROWS + (threadIdx.x >> 6);
    if (r >= R) return;                         // (wave-uniform)
    const float* x = scores + (size_t)r * C;
    float bv = -INFINITY;
    int bi = 0x7fffffff;                        // a lane without columns loses every comparison
    for (int c = lane; c < C; c += 64) {        // ascending columns: `better` keeps the first maximum of the lane's stride
        const float v = x[c];
        if (arg_better(v, c, bv, bi)) { bv = v; bi = c; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(bv, d, 64);
        const int oi = __shfl_xor(bi, d, 64);
        if (arg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        const int ps = piece_sid[bi];
        int ok = 0;
        for (int g = 0; g < G; ++g) {
            const int t = gt_sid[(size_t)r * G + g];
            ok |= (t >= 0 && t == ps);
        }
        pred[r] = bi;
        correct[r] = (uint8_t)ok;
        if (counts && ok) atomicAdd(counts, 1);
    }
}

__global__ __launch_bounds__(64) void nsp_choose_kernel(const float* __restrict__ rel, int n_q, int interval, int n_rel, const int64_t* __restrict__ labels,
                                                        float* __restrict__ scores, int64_t* __restrict__ pred, uint8_t* __restrict__ correct,
                                                        int* __restrict__ counts) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n_q) return;
    float bv = 0.f;
    int bi = 0;
    for (int j = 0; j < interval; ++j) {
        const size_t s = (size_t)q * interval + j;
        const float* x = rel + s * n_rel;
        float m = x[0];
        for (int c = 1; c < n_rel; ++c) m = fmaxf(m, x[c]);
        bool nan = false;
        float sum = 0.f, e1 = 0.f;
        for (int c = 0; c < n_rel; ++c) {
            nan |= x[c] != x[c];                // (fmaxf drops NaN; softmax of a row holding one is NaN throughout)
            const float e = expf(x[c] - m);
            sum += e;
            if (c == 1) e1 = e;
        }
        const float v = nan ? NAN : 1.f - e1 / sum;
        scores[s] = v;
        if (j == 0 || arg_better(v, j, bv, bi)) { bv = v; bi = j; }
    }
    const int ok = labels[q] == bi;
    pred[q] = bi;
    correct[q] = (uint8_t)ok;
    if (counts && ok) atomicAdd(counts, 1);
}

// ---- global-norm clipping ----
constexpr int CL_THREADS = 256;
constexpr int CL_MAX_GROUPS = 1024;           // more workgroups than the final stage has lanes: it strides the partials
constexpr size_t CL_PER_GROUP = 16384;        // elements a workgroup takes before the grid is capped

// the sum of v over the workgroup, pairings fixed by the thread layout alone
__device__ __forceinline__ float clip_block_sum(float v, float* lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < CL_THREADS / 64; ++w) t += lds[w];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(CL_THREADS) void clip_norm_kernel(const float* __restrict__ g, size_t n, float max_norm, const double* __restrict__ sq_in,
                                                               float* partial, unsigned* ticket, float* __restrict__ out) {
    __shared__ float lds[CL_THREADS / 64];
    __shared__ double dl[CL_THREADS];
    __shared__ int last;
    if (!sq_in) {
        // 16-byte chunks of the aligned body, the unaligned head and the tail by the first / last threads of the grid stride
        const size_t head = min(n, (size_t)((16 - ((uintptr_t)g & 15)) & 15) / 4);
        const size_t n4 = (n - head) / 4;
        const f32x4* g4 = reinterpret_cast<const f32x4*>(g + head);
        const size_t tid = (size_t)blockIdx.x * CL_THREADS + threadIdx.x, stride = (size_t)gridDim.x * CL_THREADS;
        float acc = 0.f;
        for (size_t i = tid; i < n4; i += stride) {
            const f32x4 v = g4[i];
            acc = fmaf(v[0], v[0], acc); acc = fmaf(v[1], v[1], acc); acc = fmaf(v[2], v[2], acc); acc = fmaf(v[3], v[3], acc);
        }
        if (tid < head) acc = fmaf(g[tid], g[tid], acc);
        const size_t t0 = head + n4 * 4;
        if (tid < n - t0) acc = fmaf(g[t0 + tid], g[t0 + tid], acc);
        const float bs = clip_block_sum(acc, lds);
        if (threadIdx.x == 0) {
            partial[blockIdx.x] = bs;
            __threadfence();
            last = atomicAdd(ticket, 1u) == gridDim.x - 1;
        }
        __syncthreads();
        if (!last) return;
        __threadfence();
    }
    // ---- the last workgroup (or the only one, with sq_in): the partials in index order, in double ----
    double t = 0.0;
    if (!sq_in)
        for (unsigned i = threadIdx.x; i < gridDim.x; i += CL_THREADS) t += (double)partial[i];
    dl[threadIdx.x] = t;
    __syncthreads();
    for (int w = CL_THREADS / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) dl[threadIdx.x] += dl[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(sq_in ? sq_in[0] : dl[0]);
        float coef = max_norm / (norm + 1e-6f);
        if (coef == coef) coef = fminf(coef, 1.f);          // (fminf would drop a NaN coefficient: torch.clamp keeps it)
        out[0] = norm;
        out[1] = coef;
        if (!sq_in) *ticket = 0u;
    }
}

__global__ __launch_bounds__(CL_THREADS) void clip_scale_kernel(float* __restrict__ g, size_t n, const float* __restrict__ out) {
    const float coef = out[1];
    const size_t head = min(n, (size_t)((16 - ((uintptr_t)g & 15)) & 15) / 4);
    const size_t n4 = (n - head) / 4;
    f32x4* g4 = reinterpret_cast<f32x4*>(g + head);
    const size_t tid = (size_t)blockIdx.x * CL_THREADS + threadIdx.x, stride = (size_t)gridDim.x * CL_THREADS;
    for (size_t i = tid; i < n4; i += stride) {
        f32x4 v = g4[i];
        v[0] *= coef; v[1] *= coef; v[2] *= coef; v[3] *= coef;
        g4[i] = v;
    }
    if (tid < head) g[tid] *= coef;
    const size_t t0 = head + n4 * 4;
    if (tid < n - t0) g[t0 + tid] *= coef;
}

int gqa_choose(const float* scores, int R, int C, const int32_t* piece_sid, const int32_t* gt_sid, int G, int64_t* pred, uint8_t* correct, int* counts,
               hipStream_t s) {
    gqa_choose_kernel<<<dim3((R + GC_ROWS - 1) / GC_ROWS), dim3(GC_THREADS), 0, s>>>(scores, R, C, piece_sid, gt_sid, G, pred, correct, counts);
    return CPT_OK;
}

int nsp_choose(const float* rel, int n_q, int interval, int n_rel, const int64_t* labels, float* scores, int64_t* pred, uint8_t* correct, int* counts,
               hipStream_t s) {
    nsp_choose_kernel<<<dim3((n_q + 63) / 64), dim3(64), 0, s>>>(rel, n_q, interval, n_rel, labels, scores, pred, correct, counts);
    return CPT_OK;
}

static unsigned clip_groups(size_t n) {
    const size_t g = (n + CL_PER_GROUP - 1) / CL_PER_GROUP;
    return (unsigned)(g < 1 ? 1 : (g > (size_t)CL_MAX_GROUPS ? (size_t)CL_MAX_GROUPS : g));
}

size_t grad_clip_ws_bytes() { return 256 + (size_t)CL_MAX_GROUPS * sizeof(float); }      // [0, 256): the finish ticket; then the partials

int grad_clip(float* g, size_t n, float max_norm, const double* sq_in, float* out, void* ws, hipStream_t s) {
    unsigned* ticket = (unsigned*)ws;
    float* partial = (float*)((char*)ws + 256);
    const unsigned groups = clip_groups(n);
    clip_norm_kernel<<<dim3(sq_in ? 1u : groups), dim3(CL_THREADS), 0, s>>>(g, n, max_norm, sq_in, partial, ticket, out);
    clip_scale_kernel<<<dim3(groups), dim3(CL_THREADS), 0, s>>>(g, n, out);
    return CPT_OK;
}

}  // namespace cpt
