// gcn_rows.hip — what a forward pass restricted to the loss rows' receptive field needs beside the
// products (pygcn_amd/fused.py, GCN2RestrictedFunction), for gfx950:
//
//   gcn_dropout_rows    the dropout of include/gcn_spmm.h, struct gcn_epilogue, applied IN PLACE to a
//                       compact [m, F] tensor whose row r stands for row rows[r] of the full matrix: the
//                       keep bit is the header's function of (seed, drop_row_base + rows[r], f), so a
//                       compact pass draws the mask the full-height pass draws at the same seed.
//   gcn_csr_take_rows   rows of a CSR matrix as a CSR matrix of their own, columns optionally renumbered.
//
// Dropout.  The keep function (block, field, one-bit form) is specified in gcn_internal.h above
// philox4x32_10; every call made here serves ALL the columns it covers:
//   T != 32768  one thread per (row, block): two runs of four consecutive elements; consecutive lanes take
//               consecutive blocks, so the first accesses of a wave cover the lower halves of its 64-byte
//               groups and the second the upper halves.
//   T == 32768  a workgroup of 256 threads takes 128 rows of one 256-column span s: thread t draws the
//               call (row t >> 1, b = t & 1) into LDS, then the workgroup sweeps the 128 x 256 window four
//               rows at a time, a wave per row and four consecutive columns per lane (one 16-byte access at
//               fp32), each lane picking its four bits out of LDS.
// A run of four is one vector access when base address and pitch allow and the run lies inside the row,
// else element by element: any F >= 1, any pitch.  Nothing outside the m x F window is touched.
//
// gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kBitRows = kBlock / 2;      // rows of one workgroup of the one-bit form

// one element of a row <-> a float, where a run of four cannot travel as one access
__device__ __forceinline__ float get(const float *p) { return *p; }
__device__ __forceinline__ void put(float *p, float x) { *p = x; }
__device__ __forceinline__ float get(const bf16_t *p) { return __uint_as_float(((uint32_t)*p) << 16); }
__device__ __forceinline__ void put(bf16_t *p, float x) { *p = (bf16_t)(pack_bf16x2(x, 0.f) & 0xffffu); }

// h[f .. f + 4) of one row (p points at column f; `left` = F - f > 0 columns remain) under four keep
// flags: kept elements are multiplied by s in fp32 and rounded once, the others become +0
template <typename T>
__device__ __forceinline__ void drop_run(T *p, int64_t left, bool vec, const bool (&keep)[4], float s)
{
    if (vec && left >= 4) {
        float x[4];
        Run4<T>::load(p, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = keep[j] ? x[j] * s : 0.f;
        Run4<T>::store_rounded(p, x);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < left) put(p + j, keep[j] ? get(p + j) * s : 0.f);
    }
}

struct DropParams {
    const int64_t *rows;       // NULL: row r is r
    int64_t m, F, ld;
    int64_t row_base;
    const uint64_t *seed_dev;  // NULL: seed_lo / seed_hi
    uint32_t seed_lo, seed_hi;
    uint32_t thresh;
    float scale;
    int32_t vec;               // runs of four may travel as one vector access
};

__device__ __forceinline__ void seed_of(const DropParams &p, uint32_t &k0, uint32_t &k1)
{
    k0 = p.seed_lo; k1 = p.seed_hi;
    if (p.seed_dev != nullptr) {     // the seed as of execution time (a captured launch)
        const uint64_t sd = *p.seed_dev;
        k0 = (uint32_t)sd; k1 = (uint32_t)(sd >> 32);
    }
}

// T != 32768: one thread per (row, blk), grid-stride over m * G pairs, G = 2 * ceil(F / 16)
template <typename T>
__global__ __launch_bounds__(kBlock) void dropout_rows_fields_kernel(T *__restrict__ h, DropParams p)
{
    uint32_t k0, k1;
    seed_of(p, k0, k1);
    const int64_t G = 2 * ((p.F + 15) / 16), total = p.m * G;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / G;
        const uint32_t blk = (uint32_t)(i - r * G);
        const int64_t f0 = 16 * (int64_t)(blk >> 1) + 4 * (blk & 1u);
        if (f0 >= p.F) continue;
        const int64_t row = (p.rows != nullptr ? p.rows[r] : r) + p.row_base;
        uint32_t w[4];
        philox4x32_10<kPhiloxMulPair>((uint32_t)row, (uint32_t)((uint64_t)row >> 32), blk, 0u, k0, k1, w);
        T *base = h + r * p.ld;
#pragma unroll
        for (int half = 0; half < 2; ++half) {      // fields 0..3 = columns f0 + (0..3), 4..7 = f0 + 8 + (0..3)
            const int64_t f = f0 + 8 * half;
            if (f >= p.F) break;
            const uint32_t w0 = w[2 * half], w1 = w[2 * half + 1];
            const bool keep[4] = {(w0 & 0xFFFFu) >= p.thresh, (w0 >> 16) >= p.thresh,
                                  (w1 & 0xFFFFu) >= p.thresh, (w1 >> 16) >= p.thresh};
            drop_run<T>(base + f, p.F - f, p.vec != 0, keep, p.scale);
        }
    }
}

// T == 32768: blockIdx.x = 128-row slab, blockIdx.y = 256-column span
template <typename T>
__global__ __launch_bounds__(kBlock) void dropout_rows_bits_kernel(T *__restrict__ h, DropParams p)
{
    __shared__ uint32_t bits[kBitRows * 2][4];
    uint32_t k0, k1;
    seed_of(p, k0, k1);
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kBitRows;
    const uint32_t span = blockIdx.y;
    {
        const int64_t r = r0 + (t >> 1);
        if (r < p.m) {
            const int64_t row = (p.rows != nullptr ? p.rows[r] : r) + p.row_base;
            uint32_t w[4];
            philox4x32_10<kPhiloxMulPair>((uint32_t)row, (uint32_t)((uint64_t)row >> 32),
                                          (span << 1) | (uint32_t)(t & 1), 0u, k0, k1, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) bits[t][j] = w[j];
        }
    }
    __syncthreads();
    const int lane = t & 63;
    const int64_t f = 256 * (int64_t)span + 4 * lane;
    if (f >= p.F) return;
    // columns f .. f + 3: b = bit 2 of f = lane & 1, index = ((f & 255) >> 3) << 2 = (lane >> 1) << 2
    const int b = lane & 1, idx = (lane >> 1) << 2;
    for (int lr = t >> 6; lr < kBitRows; lr += kBlock / 64) {
        const int64_t r = r0 + lr;
        if (r >= p.m) break;
        const uint32_t nib = bits[2 * lr + b][idx >> 5] >> (idx & 31);
        const bool keep[4] = {(nib & 1u) != 0, (nib & 2u) != 0, (nib & 4u) != 0, (nib & 8u) != 0};
        drop_run<T>(h + r * p.ld + f, p.F - f, p.vec != 0, keep, p.scale);
    }
}

// ------------------------------------------------------------------------------------------------
// rows of a CSR matrix: one thread per OUTPUT entry, its row found by binary search in rowptr_out
// ------------------------------------------------------------------------------------------------
template <typename P>
__device__ __forceinline__ int64_t at(const void *a, int64_t i) { return (int64_t)((const P *)a)[i]; }

template <typename PI, typename PO>
__global__ __launch_bounds__(kBlock) void take_rows_kernel(const void *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const float *__restrict__ val, const int64_t *__restrict__ rows,
                                                           int64_t m, const int32_t *__restrict__ col_map,
                                                           const void *__restrict__ rowptr_out, int32_t *__restrict__ col_out,
                                                           float *__restrict__ val_out, int32_t *__restrict__ n_unmapped)
{
    const int64_t total = at<PO>(rowptr_out, m);
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        // the LAST r with rowptr_out[r] <= e (rows without entries repeat a value: they are passed over)
        int64_t lo = 0, hi = m;            // invariant: rowptr_out[lo] <= e < rowptr_out[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (at<PO>(rowptr_out, mid) <= e) lo = mid; else hi = mid;
        }
        const int64_t src_row = rows[lo];
        const int64_t off = e - at<PO>(rowptr_out, lo);
        const int64_t s0 = at<PI>(rowptr, src_row), s1 = at<PI>(rowptr, src_row + 1);
        int32_t c = 0;
        float v = 0.f;
        if (off < s1 - s0) {               // (a rowptr_out that is not the scan of the row lengths reads nothing out of range)
            c = col[s0 + off];
            v = val[s0 + off];
            if (col_map != nullptr) {
                c = col_map[c];
                if (c < 0) {
                    c = 0;
                    v = 0.f;
                    if (n_unmapped != nullptr) atomicAdd(n_unmapped, 1);
                }
            }
        }
        col_out[e] = c;
        val_out[e] = v;
    }
}

}   // namespace

extern "C" {

int gcn_dropout_rows(int dtype, void *h, int64_t ld, const int64_t *rows, int64_t m, int64_t F, float dropout_p,
                     uint64_t seed, const uint64_t *seed_dev, int64_t drop_row_base, void *stream)
{
    if (dtype != GCN_DTYPE_F32 && dtype != GCN_DTYPE_BF16)
        return gcn_internal_fail(GCN_E_BADARG, "gcn_dropout_rows: dtype must be GCN_DTYPE_F32 or GCN_DTYPE_BF16");
    if (!(dropout_p >= 0.f && dropout_p < 1.f))
        return gcn_internal_fail(GCN_E_BADARG, "gcn_dropout_rows: dropout_p must lie in [0, 1)");
    if (m < 0 || F < 1 || ld < F)
        return gcn_internal_fail(GCN_E_BADARG, "gcn_dropout_rows: need m >= 0, F >= 1 and ld >= F");
    if (m == 0 || dropout_p == 0.f) return 0;
    if (h == nullptr) return gcn_internal_fail(GCN_E_BADARG, "gcn_dropout_rows: NULL pointer");
    const size_t esize = pick_dtype(dtype, [](auto t) { return sizeof(typename decltype(t)::type); });
    if (((uintptr_t)h) % esize != 0) return gcn_internal_fail(GCN_E_ALIGN, "gcn_dropout_rows: h is not element-aligned");
    DropParams p;
    p.rows = rows; p.m = m; p.F = F; p.ld = ld; p.row_base = drop_row_base;
    p.seed_dev = seed_dev; p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32);
    p.thresh = gcn_dropout_threshold16(dropout_p);
    p.scale = gcn_dropout_scale16(p.thresh);
    p.vec = (((uintptr_t)h) % (4 * esize) == 0 && ld % 4 == 0) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    if (p.thresh == 32768u) {
        const int64_t slabs = (m + kBitRows - 1) / kBitRows, spans = (F + 255) / 256;
        if (slabs > INT_MAX || spans > 65535)
            return gcn_internal_fail(GCN_E_BADARG, "gcn_dropout_rows: m or F too large for one launch");
        const dim3 grid((unsigned)slabs, (unsigned)spans), block(kBlock);
        pick_dtype(dtype, [&](auto t) {
            typedef typename decltype(t)::type T;
            hipLaunchKernelGGL(dropout_rows_bits_kernel<T>, grid, block, 0, s, (T *)h, p);
        });
    } else {
        const int64_t G = 2 * ((F + 15) / 16);
        if (G > INT_MAX || m > INT64_MAX / G)
            return gcn_internal_fail(GCN_E_BADARG, "gcn_dropout_rows: m * F too large");
        const int64_t blocks = std::min<int64_t>((m * G + kBlock - 1) / kBlock, 1 << 20);   // (grid-stride beyond)
        const dim3 grid((unsigned)blocks), block(kBlock);
        pick_dtype(dtype, [&](auto t) {
            typedef typename decltype(t)::type T;
            hipLaunchKernelGGL(dropout_rows_fields_kernel<T>, grid, block, 0, s, (T *)h, p);
        });
    }
    return launched("gcn_dropout_rows launch");
}

int gcn_csr_take_rows(const void *rowptr, int rowptr_is64, const int32_t *col, const float *val, const int64_t *rows,
                      int64_t m, const int32_t *col_map, const void *rowptr_out, int out_is64, int32_t *col_out,
                      float *val_out, int32_t *n_unmapped, void *stream)
{
    if (m < 0) return gcn_internal_fail(GCN_E_BADARG, "gcn_csr_take_rows: m < 0");
    if (m == 0) return 0;
    if (rowptr == nullptr || rows == nullptr || rowptr_out == nullptr)
        return gcn_internal_fail(GCN_E_BADARG, "gcn_csr_take_rows: NULL pointer");
    // (col / val / col_out / val_out may be NULL when no selected row holds an entry: nothing is then touched)
    const dim3 grid(4096), block(kBlock);       // grid-stride: the entry count is rowptr_out[m], on the device
    hipStream_t s = (hipStream_t)stream;
    pick_index(rowptr_is64 != 0, [&](auto pi) {
        pick_index(out_is64 != 0, [&](auto po) {
            hipLaunchKernelGGL((take_rows_kernel<typename decltype(pi)::type, typename decltype(po)::type>), grid,
                               block,
                               0, s, rowptr, col, val, rows, m, col_map, rowptr_out, col_out, val_out, n_unmapped);
        });
    });
    return launched("gcn_csr_take_rows launch");
}

}   // extern "C"
