// VCR Q->AR (Oscar/oscar/modeling/modeling_vcr.py:194-251 VCRQAR_NSPCPT, fewshot/vcr_qar_nsp_cpt.py): two relation heads on one batch.
// Rows [0, B0) are Q->A sequences and go through head 0 (cls_ans), rows [B0, B) are QA->R sequences and go through head 1 (cls_rat); the
// encoder and the pooler have run once over all B rows.
//   rel2_fwd:    rel[s] = pooled[s] . W_h(s)^T + b_h(s) (one wave per row, fp32 accumulation), the choice score 1 - softmax(rel[s])[1] and, with
//                labels, CrossEntropyLoss(ignore_index=-1) per group: loss = mean(group 0) + mean(group 1) -- the driver's q_a_loss + qa_r_loss.  A
//                group without rows adds nothing; a group whose rows are all ignored gives NaN (torch's mean over no rows).  dlogits is written
//                already divided by its group's labelled-row count.  The last workgroup to finish (ticket) sums the row losses in a fixed order.
//   rel2_bwd:    dpooled[s] = dlogits[s] . W_h(s), dW_h = sum over the group's rows of dlogits[s]^T pooled[s] (written), db_h += sum of dlogits[s];
//                every sum runs in a fixed order by one thread: no float atomics, the gradients repeat bit for bit.
//   qar_choose:  per question the answer argmax, the rationale slice and the rationale argmax of evaluate() (vcr_qar_nsp_cpt.py:657-676),
//                torch.argmax rules (first maximum, NaN counts as the maximum), three correctness flags and their counts.
// bf16 mode: weights are the bf16 shadows and pooled is rounded to bf16 where it is read (as the relation GEMM's operand); every other mode
// reads fp32 weights (bf16x3 included: the head is a few dot products, not a GEMM worth splitting).
#include <math.h>

#include <vector>

#include "common.h"
#include "kernels.h"

namespace cpt {

constexpr int R2_THREADS = 256;
constexpr int R2_ROWS = R2_THREADS / 64;      // one wave per row

template <typename W>
__device__ __forceinline__ float r2_w(const W* w, size_t i) { return (float)w[i]; }

__device__ __forceinline__ float r2_p(const float* p, size_t i, bool lp) {
    const float v = p[i];
    return lp ? (float)(bf16)v : v;
}

template <typename W>
__global__ __launch_bounds__(R2_THREADS) void rel2_fwd_kernel(const float* __restrict__ pooled, int B, int H, int n_rel, int B0,
                                                              const W* __restrict__ w0, const float* __restrict__ b0, const W* __restrict__ w1,
                                                              const float* __restrict__ b1, const int64_t* __restrict__ labels,
                                                              float* __restrict__ rel, float* __restrict__ score, float* __restrict__ dlogits,
                                                              float* __restrict__ rowloss, unsigned* __restrict__ ticket, float* __restrict__ loss2,
                                                              float* __restrict__ loss_mean, int lp) {
    __shared__ int last;
    __shared__ float gsum[2], gcnt[2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int s = blockIdx.x * R2_ROWS + wv;
    if (s < B) {
        const bool h1 = s >= B0;
        const W* w = h1 ? w1 : w0;
        const float* bias = h1 ? b1 : b0;
        const float* p = pooled + (size_t)s * H;
        float mine = -INFINITY;                    // lane c holds rel[s][c]
        for (int c = 0; c < n_rel; ++c) {
            float acc = 0.f;
            for (int k = lane; k < H; k += 64) acc += r2_p(p, k, lp != 0) * r2_w(w, (size_t)c * H + k);
            acc = wave_sum(acc);
            if (lane == c) mine = acc + bias[c];
        }
        const bool valid = lane < n_rel;
        if (valid) rel[(size_t)s * n_rel + lane] = mine;
        const float m = wave_max(valid ? mine : -INFINITY);
        const float e = valid ? expf(mine - m) : 0.f;
        const float sum = wave_sum(e);
        if (score) {
            const float e1 = __shfl(e, 1, 64);
            if (lane == 0) score[s] = 1.f - e1 / sum;
        }
        if (labels) {
            const long lab = labels[s];
            const bool use = lab >= 0 && lab < n_rel;          // (-1: ignored; the entry points reject anything else)
            const float xl = __shfl(mine, use ? (int)lab : 0, 64);
            if (valid) dlogits[(size_t)s * n_rel + lane] = use ? e / sum - (lane == lab ? 1.f : 0.f) : 0.f;
            if (lane == 0) rowloss[s] = use ? (m + logf(sum)) - xl : 0.f;
        }
    }
    if (!labels) return;
    // ---- the last workgroup: per-group means in row order, dlogits divided by the group's count ----
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    if (wv < 2) {
        const int lo = wv == 0 ? 0 : B0, hi = wv == 0 ? B0 : B;
        float sm = 0.f, cn = 0.f;
        for (int r = lo + lane; r < hi; r += 64) {
            const long lab = labels[r];
            if (lab >= 0 && lab < n_rel) { sm += rowloss[r]; cn += 1.f; }
        }
        sm = wave_sum(sm);
        cn = wave_sum(cn);
        if (lane == 0) { gsum[wv] = sm; gcnt[wv] = cn; }
    }
    __syncthreads();
    const float inv0 = gcnt[0] > 0.f ? 1.f / gcnt[0] : 0.f, inv1 = gcnt[1] > 0.f ? 1.f / gcnt[1] : 0.f;
    for (int i = threadIdx.x; i < B * n_rel; i += R2_THREADS) dlogits[i] *= (i / n_rel) < B0 ? inv0 : inv1;
    if (threadIdx.x == 0) {
        const float m0 = gsum[0] / gcnt[0], m1 = gsum[1] / gcnt[1];      // 0 / 0 = NaN: a group whose rows are all ignored
        if (loss2) { loss2[0] = B0 > 0 ? m0 : 0.f; loss2[1] = B > B0 ? m1 : 0.f; }
        if (loss_mean) loss_mean[0] = (B0 > 0 ? m0 : 0.f) + (B > B0 ? m1 : 0.f);
        *ticket = 0u;
    }
}

template <typename W>
__global__ __launch_bounds__(R2_THREADS) void rel2_bwd_kernel(const float* __restrict__ pooled, int B, int H, int n_rel, int B0,
                                                              const W* __restrict__ w0, const W* __restrict__ w1, const float* __restrict__ dlogits,
                                                              float scale, const float* __restrict__ scale_dev, float* __restrict__ dpooled,
                                                              float* __restrict__ gw0, float* __restrict__ gb0, float* __restrict__ gw1,
                                                              float* __restrict__ gb1, int lp) {
    const long i = (long)blockIdx.x * R2_THREADS + threadIdx.x;
    const float sc = scale_dev ? scale * scale_dev[0] : scale;
    const long nA = (long)B * H, nW = 2L * n_rel * H, nb = 2L * n_rel;
    if (i < nA) {                                  // dpooled[s][k] = sum_c dlogits[s][c] W_h(s)[c][k]
        const int s = (int)(i / H), k = (int)(i % H);
        const W* w = s >= B0 ? w1 : w0;
        float acc = 0.f;
        for (int c = 0; c < n_rel; ++c) acc += (dlogits[(size_t)s * n_rel + c] * sc) * r2_w(w, (size_t)c * H + k);
        dpooled[i] = acc;
    } else if (i < nA + nW) {                      // dW_h[c][k] = sum over the group's rows, in row order
        const long j = i - nA;
        const int h = (int)(j / ((long)n_rel * H)), c = (int)((j / H) % n_rel), k = (int)(j % H);
        const int lo = h ? B0 : 0, hi = h ? B : B0;
        float acc = 0.f;
        for (int s = lo; s < hi; ++s) acc += (dlogits[(size_t)s * n_rel + c] * sc) * r2_p(pooled, (size_t)s * H + k, lp != 0);
        (h ? gw1 : gw0)[(size_t)c * H + k] = acc;
    } else if (i < nA + nW + nb) {                 // db_h[c] += sum over the group's rows
        const int j = (int)(i - nA - nW);
        const int h = j / n_rel, c = j % n_rel;
        const int lo = h ? B0 : 0, hi = h ? B : B0;
        float acc = 0.f;
        for (int s = lo; s < hi; ++s) acc += dlogits[(size_t)s * n_rel + c] * sc;
        float* gb = h ? gb1 : gb0;
        gb[c] += acc;
    }
}

// torch.argmax over x[0..n): first maximum, NaN counts as the maximum (the first NaN wins)
__device__ __forceinline__ int qar_argmax(const float* x, int n) {
    int bi = 0;
    float bv = x[0];
    for (int i = 1; i < n && bv == bv; ++i) {
        const float v = x[i];
        if (v != v || v > bv) { bv = v; bi = i; }
    }
    return bi;
}

__global__ __launch_bounds__(64) void qar_choose_kernel(const float* __restrict__ q_a, const float* __restrict__ qa_r, int n_q, int n_ans, int n_rats,
                                                        const int64_t* __restrict__ ans_label, const int64_t* __restrict__ rat_label,
                                                        int64_t* __restrict__ preds, uint8_t* __restrict__ flags, int* __restrict__ counts) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n_q) return;
    const long al = ans_label[q], rl = rat_label[q];
    const int a = qar_argmax(q_a + (size_t)q * n_ans, n_ans);
    // the rationale slice: all n_rats scores, or -- 16-rationale layout -- x[al * n_ans : (al + 1) * n_ans] of them with Python's slice rules
    // (a negative bound counts from the end, then both bounds are clamped to [0, n_rats])
    int lo = 0, hi = n_rats;
    if (n_rats > n_ans) {
        auto bound = [n_rats](long v) -> int {
            if (v < 0) v += n_rats;
            return (int)(v < 0 ? 0 : (v > n_rats ? n_rats : v));
        };
        lo = bound(al * n_ans);
        hi = bound((al + 1) * n_ans);
    }
    const int r = hi > lo ? qar_argmax(qa_r + (size_t)q * n_rats + lo, hi - lo) : -1;      // (-1: the reference's argmax of an empty slice raises)
    preds[2 * (size_t)q] = a;
    preds[2 * (size_t)q + 1] = r;
    const int fa = al == a, fr = r >= 0 && rl == r, fq = fa && fr;
    flags[3 * (size_t)q] = (uint8_t)fa;
    flags[3 * (size_t)q + 1] = (uint8_t)fr;
    flags[3 * (size_t)q + 2] = (uint8_t)fq;
    if (counts) {
        if (fa) atomicAdd(&counts[0], 1);
        if (fr) atomicAdd(&counts[1], 1);
        if (fq) atomicAdd(&counts[2], 1);
    }
}

int rel2_fwd(int lp, const float* pooled, int B, int H, int n_rel, int B0, const void* w0, const float* b0, const void* w1, const float* b1,
             const int64_t* labels, float* rel, float* score, float* dlogits, float* rowloss, unsigned* ticket, float* loss2, float* loss_mean,
             hipStream_t s) {
    const dim3 grid((B + R2_ROWS - 1) / R2_ROWS), block(R2_THREADS);
    if (lp)
        rel2_fwd_kernel<bf16><<<grid, block, 0, s>>>(pooled, B, H, n_rel, B0, (const bf16*)w0, b0, (const bf16*)w1, b1, labels, rel, score, dlogits,
                                                     rowloss, ticket, loss2, loss_mean, 1);
    else
        rel2_fwd_kernel<float><<<grid, block, 0, s>>>(pooled, B, H, n_rel, B0, (const float*)w0, b0, (const float*)w1, b1, labels, rel, score, dlogits,
                                                      rowloss, ticket, loss2, loss_mean, 0);
    return CPT_OK;
}

int rel2_bwd(int lp, const float* pooled, int B, int H, int n_rel, int B0, const void* w0, const void* w1, const float* dlogits, float scale,
             const float* scale_dev, float* dpooled, float* gw0, float* gb0, float* gw1, float* gb1, hipStream_t s) {
    const long n = (long)B * H + 2L * n_rel * H + 2L * n_rel;
    const dim3 grid((unsigned)((n + R2_THREADS - 1) / R2_THREADS)), block(R2_THREADS);
    if (lp)
        rel2_bwd_kernel<bf16><<<grid, block, 0, s>>>(pooled, B, H, n_rel, B0, (const bf16*)w0, (const bf16*)w1, dlogits, scale, scale_dev, dpooled,
                                                     gw0, gb0, gw1, gb1, 1);
    else
        rel2_bwd_kernel<float><<<grid, block, 0, s>>>(pooled, B, H, n_rel, B0, (const float*)w0, (const float*)w1, dlogits, scale, scale_dev, dpooled,
                                                      gw0, gb0, gw1, gb1, 0);
    return CPT_OK;
}

int abi_fail(int code, const char* fmt, ...);

// labels in [-1, n_rel): checked on the host copy when the caller has one, else the device labels are read back (one stream wait)
int rel2_check_labels(const int64_t* labels, const int64_t* labels_host, int B, int n_rel, const char* who, hipStream_t s) {
    std::vector<int64_t> tmp;
    const int64_t* h = labels_host;
    if (!h) {
        tmp.resize(B > 0 ? B : 1);
        hipError_t e = hipMemcpyAsync(tmp.data(), labels, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return abi_fail(CPT_ERR_HIP - (int)e, "%s: reading the labels back: %s", who, hipGetErrorString(e));
        h = tmp.data();
    }
    for (int i = 0; i < B; ++i)
        if (h[i] < -1 || h[i] >= n_rel) return abi_fail(CPT_ERR_SHAPE, "%s: label %lld of row %d outside [-1, %d)", who, (long long)h[i], i, n_rel);
    return CPT_OK;
}

int qar_choose(const float* q_a, const float* qa_r, int n_q, int n_ans, int n_rats, const int64_t* ans_label, const int64_t* rat_label,
               int64_t* preds, uint8_t* flags, int* counts, hipStream_t s) {
    qar_choose_kernel<<<dim3((n_q + 63) / 64), dim3(64), 0, s>>>(q_a, qa_r, n_q, n_ans, n_rats, ans_label, rat_label, preds, flags, counts);
    return CPT_OK;
}

}  // namespace cpt
