// gcn_dense.hip — a dense fp32 [n_rows, n_cols] adjacency to CSR on the device (gfx950), with the two
// sparsifications a co-visit matrix calls for: a value bound, and the `keep` strongest entries of every row.
//
// The fork never builds a sparse adjacency: its live scripts load the co-visit matrix as a dense [N, N] float
// tensor (reference pygcn/utils.py:124-131) and hand that to every model.  This is the front end that brings such
// a matrix onto the CSR path: two streaming reads of the matrix, the caller's scan of the row counts between them.
//     dense_count_kernel   row_count[i] = the number of kept entries of row i
//     dense_fill_kernel    the kept entries of row i at rowptr[i] + 0, 1, ..., ascending column
// The rule of what is kept is in include/gcn_spmm.h ("Dense adjacency ingest"); classify() below is its one
// statement on the device.  With a per-row threshold (thr, count_gt: gcn_select_kth's answers at kth = keep, the
// matrix being exactly its [batch = n_rows, n_rows = n_cols] layout) the entries whose key EQUALS the threshold all
// share one answer of the value rule — equal keys are equal floats up to the sign of zero and the payload of a NaN,
// and neither rule tells those apart — so a wave's share of the kept entries follows from two totals, (above the
// threshold and passing the rule, equal to it), and one barrier per chunk is enough.
//
// SHAPE.  One 256-thread block per row, rows grid-stride from a grid of at most GCN_DENSE_SWEEP_ROWS blocks.  A row
// is walked in chunks of 1024 columns: thread t holds the four columns 4t .. 4t + 3 of the chunk, loaded as ONE
// 16-byte access where the row base is 16-byte aligned (A aligned and lda a multiple of 4), else element by element.
// The fill compacts a chunk in order the way select_write_kernel (gcn_select.hip) does: one ballot per held column,
// popcounts below the lane, the four wave totals through LDS with a parity double buffer, and the running totals of
// the row in registers.  A matrix of few very long rows leaves most of the chip idle (one block per row); a co-visit
// matrix has as many rows as columns, and the 8192-block sweep fills the chip from N = 2048 up.
// No atomics; nothing is read by the host; two runs give the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

constexpr int64_t kSweepRows = GCN_DENSE_SWEEP_ROWS;      // blocks of a launch = rows of one sweep of the grid
constexpr int kChunk = 1024;                              // columns per chunk: 256 threads x 4

__device__ __forceinline__ bool value_rule(float a, int rule, float bound)
{
    return rule == GCN_DENSE_GREATER ? a > bound : !(a == 0.0f);
}

// what a row's selection needs, block-uniform
struct RowRule {
    int rule;
    float bound;
    bool topk;            // a threshold was given
    bool eq_kept;         // the value rule's answer for the entries equal to the threshold
    uint32_t T;           // order_key(thr[i])
    int64_t need_eq;      // how many of those are selected: keep - count_gt[i], lowest columns first
    __device__ __forceinline__ RowRule(int rule_, float bound_, const float *thr, const int32_t *count_gt,
                                       int64_t keep, int64_t i)
        : rule(rule_), bound(bound_), topk(thr != nullptr), eq_kept(false), T(0u), need_eq(0)
    {
        if (topk) {
            const float t = thr[i];
            T = order_key(t);
            eq_kept = value_rule(t, rule, bound);
            need_eq = max(keep - (int64_t)count_gt[i], (int64_t)0);
        }
    }
    // gt: kept whatever came before it in the row; eq: equal to the threshold (kept iff eq_kept and fewer than
    // need_eq equal entries lie before it)
    __device__ __forceinline__ void classify(float a, bool &gt, bool &eq) const
    {
        const bool ok = value_rule(a, rule, bound);
        if (topk) {
            const uint32_t t = order_key(a);
            gt = ok && t > T;
            eq = t == T;
        } else {
            gt = ok;
            eq = false;
        }
    }
    __device__ __forceinline__ int64_t eq_kept_of(int64_t eq_before) const
    {
        return eq_kept ? min(eq_before, need_eq) : (int64_t)0;
    }
};

// columns c0 .. c0 + 3 of the row at w; returns how many of them exist (0 .. 4), the others read as 0
__device__ __forceinline__ int load4(const float *w, int64_t c0, int64_t n_cols, bool vec, float (&x)[4])
{
    const int64_t left = n_cols - c0;
    const int n = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    if (vec && n == 4) {
        Run4<float>::load(w + c0, x);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = e < n ? w[c0 + e] : 0.0f;
    }
    return n;
}

__global__ __launch_bounds__(256) void dense_count_kernel(const float *__restrict__ A, int64_t lda, int64_t n_rows,
                                                          int64_t n_cols, int rule, float bound,
                                                          const float *__restrict__ thr,
                                                          const int32_t *__restrict__ count_gt, int64_t keep,
                                                          int32_t *__restrict__ row_count)
{
    __shared__ int red[2][2][4];          // [row parity][gt, eq][wave]
    int it = 0;
    for (int64_t i = blockIdx.x; i < n_rows; i += gridDim.x, ++it) {     // (block-uniform)
        const RowRule rr(rule, bound, thr, count_gt, keep, i);
        const float *w = A + i * lda;
        const bool vec = ((uintptr_t)w & 15) == 0;
        int gt = 0, eq = 0;
        for (int64_t c0 = (int64_t)threadIdx.x * 4; c0 < n_cols; c0 += kChunk) {
            float x[4];
            const int n = load4(w, c0, n_cols, vec, x);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bool g, q;
                rr.classify(x[e], g, q);
                gt += (e < n) && g;
                eq += (e < n) && q;
            }
        }
        for (int m = 1; m < 64; m <<= 1) {
            gt += __shfl_xor(gt, m, 64);
            eq += __shfl_xor(eq, m, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            red[it & 1][0][threadIdx.x >> 6] = gt;
            red[it & 1][1][threadIdx.x >> 6] = eq;
        }
        __syncthreads();                  // (the other parity is the previous row's: one barrier per row)
        if (threadIdx.x == 0) {
            const int (&r)[2][4] = red[it & 1];
            const int64_t all_g = r[0][0] + r[0][1] + r[0][2] + r[0][3];
            const int64_t all_e = r[1][0] + r[1][1] + r[1][2] + r[1][3];
            row_count[i] = (int32_t)(all_g + rr.eq_kept_of(all_e));
        }
    }
}

template <typename RP>
__global__ __launch_bounds__(256) void dense_fill_kernel(const float *__restrict__ A, int64_t lda, int64_t n_rows,
                                                         int64_t n_cols, int rule, float bound,
                                                         const float *__restrict__ thr,
                                                         const int32_t *__restrict__ count_gt, int64_t keep,
                                                         const RP *__restrict__ rowptr, int32_t *__restrict__ col,
                                                         float *__restrict__ val)
{
    __shared__ int wave_tot[2][2][4];     // [chunk parity][gt, eq][wave]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int it = 0;                           // chunks this block has walked, over all its rows
    for (int64_t i = blockIdx.x; i < n_rows; i += gridDim.x) {           // (block-uniform)
        const RowRule rr(rule, bound, thr, count_gt, keep, i);
        const float *w = A + i * lda;
        const bool vec = ((uintptr_t)w & 15) == 0;
        const int64_t e_first = (int64_t)rowptr[i];
        const int64_t row_len = (int64_t)rowptr[i + 1] - e_first;        // nothing is written past the row's slots
        int64_t gt_before = 0, eq_before = 0;
        for (int64_t base = 0; base < n_cols; base += kChunk, ++it) {    // (block-uniform trip count)
            const int64_t c0 = base + (int64_t)threadIdx.x * 4;
            float x[4];
            const int n = load4(w, c0, n_cols, vec, x);
            bool g[4], q[4];
            unsigned long long mg[4], me[4];
            int wave_g = 0, wave_e = 0, lane_g = 0, lane_e = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                rr.classify(x[e], g[e], q[e]);
                g[e] = g[e] && e < n;
                q[e] = q[e] && e < n;
                mg[e] = __ballot(g[e]);
                me[e] = __ballot(q[e]);
                wave_g += __popcll(mg[e]);
                wave_e += __popcll(me[e]);
                lane_g += __popcll(mg[e] & below);
                lane_e += __popcll(me[e] & below);
            }
            if (lane == 0) {
                wave_tot[it & 1][0][wave] = wave_g;
                wave_tot[it & 1][1][wave] = wave_e;
            }
            __syncthreads();              // (the other parity is the previous chunk's: one barrier per chunk)
            int64_t g0 = gt_before + lane_g, e0 = eq_before + lane_e;
            int all_g = 0, all_e = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int a = wave_tot[it & 1][0][s], b = wave_tot[it & 1][1][s];
                if (s < wave) { g0 += a; e0 += b; }
                all_g += a;
                all_e += b;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {                 // the lane's columns in ascending order
                if (g[e] || (q[e] && rr.eq_kept && e0 < rr.need_eq)) {
                    const int64_t pos = g0 + rr.eq_kept_of(e0);
                    if (pos < row_len) {                  // (always, when rowptr is the scan of the count sweep)
                        col[e_first + pos] = (int32_t)(c0 + e);
                        val[e_first + pos] = x[e];
                    }
                }
                g0 += g[e];
                e0 += q[e];
            }
            gt_before += all_g;
            eq_before += all_e;
        }
    }
}

// everything the two entry points check alike; 0, or the code that was recorded under `who`
int check_matrix(const char *who, const float *A, int64_t lda, int64_t n_rows, int64_t n_cols, int rule,
                 const float *thr, const int32_t *count_gt, int64_t keep)
{
    if (n_rows < 0) return bad(who, GCN_E_BADARG, "n_rows < 0");
    if (n_cols < 1 || n_cols > (int64_t)INT32_MAX) return bad(who, GCN_E_BADARG, "needs 1 <= n_cols < 2^31");
    if (lda < n_cols) return bad(who, GCN_E_BADARG, "lda < n_cols");
    if (rule != GCN_DENSE_NONZERO && rule != GCN_DENSE_GREATER) return bad(who, GCN_E_BADARG, "unknown rule");
    if (thr != nullptr && count_gt == nullptr) return bad(who, GCN_E_BADARG, "thr without count_gt");
    if (thr != nullptr && (keep < 1 || keep > n_cols)) return bad(who, GCN_E_BADARG, "needs 1 <= keep <= n_cols");
    if (n_rows > 0 && A == nullptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if ((uintptr_t)A % 4 != 0 || (uintptr_t)thr % 4 != 0 || (uintptr_t)count_gt % 4 != 0)
        return bad(who, GCN_E_ALIGN, "A, thr, count_gt: 4-byte alignment required");
    return 0;
}

dim3 row_grid(int64_t n_rows) { return dim3((unsigned)std::min<int64_t>(n_rows, kSweepRows)); }

}   // namespace

extern "C" {

int gcn_dense_to_csr_count(const float *A, int64_t lda, int64_t n_rows, int64_t n_cols, int rule, float bound,
                           const float *thr, const int32_t *count_gt, int64_t keep, int32_t *row_count, void *stream)
{
    const char *who = "gcn_dense_to_csr_count";
    if (int rc = check_matrix(who, A, lda, n_rows, n_cols, rule, thr, count_gt, keep)) return rc;
    if (n_rows > 0 && row_count == nullptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if ((uintptr_t)row_count % 4 != 0) return bad(who, GCN_E_ALIGN, "row_count: 4-byte alignment required");
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(dense_count_kernel, row_grid(n_rows), dim3(256), 0, (hipStream_t)stream, A, lda, n_rows, n_cols,
                       rule, bound, thr, count_gt, keep, row_count);
    return launched(who);
}

int gcn_dense_to_csr_fill(const float *A, int64_t lda, int64_t n_rows, int64_t n_cols, int rule, float bound,
                          const float *thr, const int32_t *count_gt, int64_t keep, const void *rowptr, int rowptr_is64,
                          int32_t *col, float *val, void *stream)
{
    const char *who = "gcn_dense_to_csr_fill";
    if (int rc = check_matrix(who, A, lda, n_rows, n_cols, rule, thr, count_gt, keep)) return rc;
    if (n_rows > 0 && (rowptr == nullptr || col == nullptr || val == nullptr))
        return bad(who, GCN_E_BADARG, "NULL pointer");
    if ((uintptr_t)rowptr % (rowptr_is64 ? 8 : 4) != 0 || (uintptr_t)col % 4 != 0 || (uintptr_t)val % 4 != 0)
        return bad(who, GCN_E_ALIGN, "rowptr: its element size, col, val: 4-byte alignment required");
    if (n_rows == 0) return 0;
    pick_index(rowptr_is64 != 0, [&](auto t) {
        typedef typename decltype(t)::type RP;
        hipLaunchKernelGGL(dense_fill_kernel<RP>, row_grid(n_rows), dim3(256), 0, (hipStream_t)stream, A, lda, n_rows,
                           n_cols, rule, bound, thr, count_gt, keep, (const RP *)rowptr, col, val);
    });
    return launched(who);
}

}   // extern "C"
