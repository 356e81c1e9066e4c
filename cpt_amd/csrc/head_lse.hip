// MLM head on a list of rows with the full-vocabulary normaliser (VG-CPT predicate scoring, vg_cpt.py:271-290).
//   row_lse: natural-log log-sum-exp of full fp32 score rows [R][V] (the decoder GEMM writes them into the workspace).
//     (A decoder GEMM that reduced its tiles to (max, sum) pairs in the epilogue without writing the scores was built: one workgroup per
//     64-column tile of the table held in LDS.  It took 82 us at 192 rows of Oscar-base where the plain decoder GEMM writing all
//     [192][30522] scores takes 30 us -- 97 KB of LDS per workgroup leaves one per CU, 477 tiles need two rounds -- so it is not used.)
//   gather_cols: listed columns of full score rows.
//   mean_logprob: the predicate scores of vg_cpt.py:283-289 from the listed columns and the row normalisers.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace cpt {

constexpr float LOG2E_F = 1.4426950408889634f;
constexpr float LN2_F = 0.6931471805599453f;
// one 1024-thread workgroup per row of full fp32 scores [R][V] (V <= 32 K: every vocabulary here), the row read ONCE into registers
// (32 values per thread) for the maximum and the sum of exp2 -- as ce_rows_reg_kernel (rowops.hip).  A one-pass running (max, sum)
// per 256-thread row took 44 us at 192 rows of 30522: two dependent exponentials per element.
constexpr int LSE_NV = 32;
__global__ __launch_bounds__(1024) void row_lse_kernel(const float* __restrict__ x, float* __restrict__ lse, int V) {
    __shared__ float red[32];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* xr = x + (size_t)r * V;
    float xv[LSE_NV];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < LSE_NV; ++i) {
        const int c = i * 1024 + tid;
        xv[i] = c < V ? xr[c] * LOG2E_F : -INFINITY;
        m = fmaxf(m, xv[i]);
    }
    m = wave_max(m);
    if (lane == 0) red[w] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) m = fmaxf(m, red[k]);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LSE_NV; ++i) s += exp2f(xv[i] - m);      // exp2(-inf) = 0 beyond V
    s = wave_sum(s);
    if (lane == 0) red[16 + w] = s;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[16 + k];
        lse[r] = (m + log2f(t)) * LN2_F;
    }
}
// V beyond 32 K: 256 threads, two passes over the row
__global__ __launch_bounds__(256) void row_lse_wide_kernel(const float* __restrict__ x, float* __restrict__ lse, int V) {
    __shared__ float red[8];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* xr = x + (size_t)r * V;
    float m = -INFINITY;
    for (int c = tid; c < V; c += 256) m = fmaxf(m, xr[c] * LOG2E_F);
    m = wave_max(m);
    if (lane == 0) red[w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f;
    for (int c = tid; c < V; c += 256) s += exp2f(xr[c] * LOG2E_F - m);
    s = wave_sum(s);
    if (lane == 0) red[4 + w] = s;
    __syncthreads();
    if (tid == 0) lse[r] = (m + log2f(red[4] + red[5] + red[6] + red[7])) * LN2_F;
}

__global__ __launch_bounds__(256) void gather_cols_kernel(const float* __restrict__ x, const int64_t* __restrict__ cols, float* __restrict__ out,
                                                          int n, int V) {
    const int r = blockIdx.x;
    for (int j = threadIdx.x; j < n; j += 256) {
        long c = cols[j];
        c = c < 0 ? 0 : (c >= V ? V - 1 : c);      // (the host checks the list; never fault)
        out[(size_t)r * n + j] = x[(size_t)r * V + c];
    }
}

// one thread per (group, candidate)
__global__ __launch_bounds__(256) void mean_logprob_kernel(const float* __restrict__ logits, int n_cols, int n_rows, const float* __restrict__ lse,
                                                           const int32_t* __restrict__ slot_row, int G, int K, const int32_t* __restrict__ cand_cols,
                                                           const int32_t* __restrict__ cand_len, int C, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= G * C) return;
    const int g = i / C, c = i - g * C;
    const int len = cand_len[c];
    if (len == 0) { out[i] = 0.f; return; }                    // the background slot (vg_cpt.py: logits = zeros(len(idx2pred) + 1))
    const int s = (len > 0 && len <= K) ? slot_row[g * K + len - 1] : -1;
    if (s < 0 || s + len > n_rows) { out[i] = NAN; return; }   // no template of that length (or a bad length): never read
    float acc = 0.f;
    for (int j = 0; j < len; ++j) {
        const int col = cand_cols[c * K + j];
        if (col < 0 || col >= n_cols) { acc = NAN; break; }
        acc += logits[(size_t)(s + j) * n_cols + col] - lse[s + j];
    }
    out[i] = acc / (float)len;
}

int row_lse(const float* x, float* lse, int R, int V, hipStream_t s) {
    if (R <= 0 || V <= 0) return CPT_ERR_SHAPE;
    if (!x || !lse) return CPT_ERR_NULL;
    if (V <= LSE_NV * 1024) row_lse_kernel<<<dim3(R), dim3(1024), 0, s>>>(x, lse, V);
    else row_lse_wide_kernel<<<dim3(R), dim3(256), 0, s>>>(x, lse, V);
    return CPT_OK;
}

int gather_cols(const float* x, const int64_t* cols, float* out, int R, int n, int V, hipStream_t s) {
    if (R <= 0 || n <= 0 || V <= 0) return CPT_ERR_SHAPE;
    if (!x || !cols || !out) return CPT_ERR_NULL;
    gather_cols_kernel<<<dim3(R), dim3(256), 0, s>>>(x, cols, out, n, V);
    return CPT_OK;
}

int mean_logprob(const float* logits, int n_cols, int n_rows, const float* lse, const int32_t* slot_row, int G, int K, const int32_t* cand_cols,
                 const int32_t* cand_len, int C, float* out, hipStream_t s) {
    if (n_cols <= 0 || n_rows <= 0 || G <= 0 || K <= 0 || C <= 0 || (long)G * C > (1L << 30)) return CPT_ERR_SHAPE;
    if (!logits || !lse || !slot_row || !cand_cols || !cand_len || !out) return CPT_ERR_NULL;
    mean_logprob_kernel<<<dim3((G * C + 255) / 256), dim3(256), 0, s>>>(logits, n_cols, n_rows, lse, slot_row, G, K, cand_cols, cand_len, C, out);
    return CPT_OK;
}

}  // namespace cpt
