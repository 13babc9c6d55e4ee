// gcn_symmetric.hip — what a GCN user gets from a SYMMETRIC adjacency (gfx950).
//
//   D^-1/2 (A + I) D^-1/2     Kipf & Welling's normalisation (the reference's `normalize` is the row form
//                             D^-1 (A + I), pygcn/utils.py:390-397)            -> gcn_sym_normalize_device
//   CSR(A^T) without a sort   when the pattern of A is symmetric, CSR(A^T) has A's rowptr and col, and its
//                             values are A's values read through the mirror permutation
//                             (i, j) -> (j, i)                  -> gcn_csr_mirror_device, gcn_gather_f32
//
// The mirror search is ENTRY-parallel: one thread per stored entry, its row found by binary search in rowptr (as
// pack_entries_kernel of gcn_ingest.hip does), its mirror by binary search in the row of its column.  A row of
// 10^5 entries is then 10^5 independent threads, not one wavefront walking it; consecutive threads read
// consecutive col / val and write consecutive mirror.  No float atomics anywhere; the four check counts are
// integer sums (per-wavefront shuffle tree, then one integer atomic per wavefront and non-zero count), so they
// do not depend on scheduling either.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

constexpr char kNorm[] = "gcn_sym_normalize_device";
constexpr char kMirror[] = "gcn_csr_mirror_device";
constexpr char kGather[] = "gcn_gather_f32";

size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

__device__ __forceinline__ double wave_sum(double s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

// deg[r] = sum of row r in double: one wavefront per row (grid-stride), lane l adds the entries e0 + l, e0 + l + 64,
// ... in that order, then the xor tree — a fixed order, whatever the grid (row_normalize_kernel's scheme in double)
template <typename IdxT>
__global__ __launch_bounds__(256) void sym_degree_kernel(const IdxT *__restrict__ rowptr,
                                                         const float *__restrict__ val, int64_t n,
                                                         double *__restrict__ deg)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n; r += n_waves) {
        const int64_t e0 = (int64_t)rowptr[r], e1 = (int64_t)rowptr[r + 1];
        double s = 0.0;
        for (int64_t e = e0 + lane; e < e1; e += 64) s += (double)val[e];
        s = wave_sum(s);
        if (lane == 0) deg[r] = s;
    }
}

// val[e] <- (float)(w / sqrt(d_i * d_j)) for e = (i, j).  The product is formed FIRST: d_i * d_j and d_j * d_i are
// the same double, so (i, j) and (j, i) evaluate one expression on the same operands and equal weights stay
// equal bit for bit, whatever sqrt rounds to.  A product of 0 gives 0 (Kipf's d_inv_sqrt[isinf] = 0); a NaN
// degree makes the entries of its row and column NaN; a negative product gives NaN (sqrt), as numpy's power does.
// A column outside [0, n) — not a square matrix — is left as it is.
template <typename IdxT>
__global__ __launch_bounds__(256) void sym_scale_kernel(const IdxT *__restrict__ rowptr,
                                                        const int32_t *__restrict__ col,
                                                        float *__restrict__ val, int64_t n,
                                                        const double *__restrict__ deg)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n; r += n_waves) {
        const int64_t e0 = (int64_t)rowptr[r], e1 = (int64_t)rowptr[r + 1];
        const double di = deg[r];
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            const int64_t j = (int64_t)col[e];
            if (j < 0 || j >= n) continue;
            const double p = di * deg[j];
            val[e] = p == 0.0 ? 0.f : (float)((double)val[e] / sqrt(p));
        }
    }
}

// adds this thread's count to *counter: shuffle tree over the wavefront, one atomic per wavefront that has any
__device__ __forceinline__ void count_add(int c, int64_t *counter)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd((unsigned long long *)counter, (unsigned long long)c);
}

// first row r of [lo, hi] with rowptr[r + 1] > e (hi itself is the answer when no earlier row qualifies)
__device__ __forceinline__ int32_t row_of_entry(const int32_t *__restrict__ rowptr, int32_t lo, int32_t hi, int32_t e)
{
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (rowptr[mid + 1] > e)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// mirror[e] = storage position of (j, i) for e = (i, j), or -1: lower bound of i among the columns of row j, a
// hit if that position holds i.  Every probe lies in [rowptr[j], rowptr[j + 1]) clamped to [0, nnz).
// counts[2] += entries whose column is not above their left neighbour's in the same row.
// All sizes are below 2^31 here (the entry point checks).  (Narrowing the row lookup to the rows of a block's
// first and last entry changed nothing measurable: the random probes of row j are the cost.)
__global__ __launch_bounds__(256) void mirror_search_kernel(const int32_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ col, int32_t n, int32_t nnz,
                                                            int32_t *__restrict__ mirror,
                                                            int64_t *__restrict__ counts)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int unsorted = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nnz; t += stride) {
        const int32_t e = (int32_t)t;
        const int32_t i = row_of_entry(rowptr, 0, n, e);
        const int32_t j = col[e];
        if (i < n && e > rowptr[i] && col[e - 1] >= j) ++unsorted;
        int32_t m = -1;
        if (i < n && j >= 0 && j < n) {
            const int32_t r1 = std::min(std::max(rowptr[j + 1], 0), nnz);
            int32_t a = std::min(std::max(rowptr[j], 0), r1), b = r1;
            while (a < b) {
                const int32_t mid = a + ((b - a) >> 1);
                if (col[mid] < i)
                    a = mid + 1;
                else
                    b = mid;
            }
            if (a < r1 && col[a] == i) m = a;
        }
        mirror[e] = m;
    }
    count_add(unsorted, counts + 2);
}

// counts[0] += entries without a mirror, [1] += entries whose mirror's mirror is another entry (duplicates),
// [3] += entries whose value differs bitwise from its mirror's.  mirror is never indexed with -1.
__global__ __launch_bounds__(256) void mirror_check_kernel(const int32_t *__restrict__ mirror,
                                                           const float *__restrict__ val, int64_t nnz,
                                                           int64_t *__restrict__ counts)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int none = 0, twice = 0, differ = 0;
    for (int64_t e = tid; e < nnz; e += stride) {
        const int64_t m = (int64_t)mirror[e];
        if (m < 0 || m >= nnz) {
            ++none;
            continue;
        }
        if ((int64_t)mirror[m] != e) ++twice;
        if (__float_as_uint(val[m]) != __float_as_uint(val[e])) ++differ;
    }
    count_add(none, counts + 0);
    count_add(twice, counts + 1);
    count_add(differ, counts + 3);
}

__global__ __launch_bounds__(256) void gather_f32_kernel(const float *__restrict__ src,
                                                         const int32_t *__restrict__ index, int64_t n,
                                                         int64_t src_len, float *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int64_t k = (int64_t)index[e];
        out[e] = (k >= 0 && k < src_len) ? src[k] : 0.f;
    }
}

unsigned entry_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 32); }   // (256 threads)

}   // namespace

extern "C" {

size_t gcn_sym_normalize_workspace_bytes(int64_t n_rows)
{
    return n_rows <= 0 ? 256 : align_up((size_t)n_rows * sizeof(double));
}

int gcn_sym_normalize_device(const void *rowptr, int rowptr_is64, const int32_t *col, float *val, int64_t n_rows,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    if (rowptr == nullptr || n_rows < 0 || n_rows >= INT32_MAX) return bad(kNorm, GCN_E_BADARG, "bad arguments");
    if (n_rows == 0) return 0;
    if (col == nullptr || val == nullptr) return bad(kNorm, GCN_E_BADARG, "col or val is NULL");
    if (workspace == nullptr || workspace_bytes < gcn_sym_normalize_workspace_bytes(n_rows))
        return bad(kNorm, GCN_E_WORKSPACE, "workspace too small");
    if (((uintptr_t)workspace & 7) != 0) return bad(kNorm, GCN_E_ALIGN, "workspace must be 8-byte aligned");
    double *deg = (double *)workspace;
    const unsigned blocks = (unsigned)std::min<int64_t>((n_rows + 3) / 4, 256 * 64);
    hipStream_t s = (hipStream_t)stream;
    pick_index(rowptr_is64 != 0, [&](auto i) {
        typedef typename decltype(i)::type I;
        hipLaunchKernelGGL(sym_degree_kernel<I>, dim3(blocks), dim3(256), 0, s, (const I *)rowptr, val, n_rows, deg);
        hipLaunchKernelGGL(sym_scale_kernel<I>, dim3(blocks), dim3(256), 0, s, (const I *)rowptr, col, val, n_rows,
                           deg);
    });
    return launched(kNorm);
}

int gcn_csr_mirror_device(const int32_t *rowptr, const int32_t *col, const float *val, int64_t n_rows, int64_t nnz,
                          int32_t *mirror, int64_t *counts, void *stream)
{
    if (rowptr == nullptr || counts == nullptr || n_rows < 0 || nnz < 0 || n_rows >= INT32_MAX || nnz >= INT32_MAX)
        return bad(kMirror, GCN_E_BADARG, "bad sizes, or NULL rowptr / counts");
    if (nnz > 0 && (col == nullptr || val == nullptr || mirror == nullptr))
        return bad(kMirror, GCN_E_BADARG, "NULL entry arrays");
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s);
    if (e != hipSuccess || nnz == 0) return launched(kMirror, e);
    const unsigned blocks = entry_blocks(nnz);
    hipLaunchKernelGGL(mirror_search_kernel, dim3(blocks), dim3(256), 0, s, rowptr, col, (int32_t)n_rows,
                       (int32_t)nnz, mirror, counts);
    hipLaunchKernelGGL(mirror_check_kernel, dim3(blocks), dim3(256), 0, s, (const int32_t *)mirror, val, nnz, counts);
    return launched(kMirror);
}

int gcn_gather_f32(const float *src, const int32_t *index, int64_t n, int64_t src_len, float *out, void *stream)
{
    if (n < 0 || src_len < 0) return bad(kGather, GCN_E_BADARG, "negative length");
    if (n == 0) return 0;
    if (src == nullptr || index == nullptr || out == nullptr) return bad(kGather, GCN_E_BADARG, "NULL array");
    hipLaunchKernelGGL(gather_f32_kernel, dim3(entry_blocks(n)), dim3(256), 0, (hipStream_t)stream, src, index, n,
                       src_len, out);
    return launched(kGather);
}

}   // extern "C"
