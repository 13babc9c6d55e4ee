// gcn_eval.hip — the input side of the fork's evaluator GCN_OVER_MLP as one read sweep of x and one
// write sweep of dx (gfx950).
//
// The evaluator's input is ONE tensor x [batch, n_rows, F] (reference pygcn/gnn-over-mlp.py:219-237,
// F = 9 or 17): its GCN reads the columns [0, d) of every sample (reference pygcn/models.py:345), the
// columns [d, F-1) are pooled as they are (:351, :272-279), and the last column is the 0/1 vertex flag
// PoolLayer multiplies by and whose non-zero count it divides by (:272, :279).  With e = F - 1 - d and
// m(j, n) = flag[j, n] when a separate flag is given, x[j, n, F-1] otherwise:
//     eval_ingest_kernel      reads x (and flag) once ->
//         wide[n, j*d + c]   = x[j, n, c]                  c < d     the [n_rows, batch*d] layout of
//                                                                    GraphConvolution.forward_wide
//         mask[j, n]         = m(j, n)                                the layout gcn_masked_colsum reads
//         esum[j*e + c - d]  = sum_n m(j, n) * x[j, n, c]  d <= c < F-1   double
//         nonzero[j]         = #{n : m(j, n) != 0}                    int64 (NaN counts, as torch.nonzero)
//     eval_ingest_bwd_kernel  reads x (flag), d_wide, d_mask, d_esum once, writes dx (and dflag) once
//         dx[j, n, c < d]        = d_wide[n, j*d + c]
//         dx[j, n, d <= c < F-1] = m(j, n) * d_esum[j, c - d]         one fp32 product
//         dm(j, n)               = d_mask[j, n] + sum_c x[j, n, c] * d_esum[j, c - d]   in double, rounded once
//                                  -> dx[j, n, F-1], or -> dflag[j, n] with dx[j, n, F-1] = 0
//
// WHY LDS.  This is a transposition between sample-major rows of 4*F bytes (36 bytes at F = 9: not even
// 16-byte aligned) and vertex-major rows of 4*batch*d bytes.  A lane per row on either side touches a cache
// line per few bytes.  So a 256-thread block stages a TILE of TV = 64 consecutive vertices x BS samples:
//   * sample s of the tile is the TV*F CONSECUTIVE floats x[j0+s, t0 .. t0+TV, :]: read as consecutive dwords,
//     a wave instruction covering 256 contiguous bytes;
//   * row n of `wide` receives the BS*d CONSECUTIVE floats [j0*d, (j0+BS)*d): written as consecutive dwords;
//   * mask, flag, d_mask and dflag are TV consecutive floats of one sample: one wave, one sample.
// The backward kernel mirrors it: d_wide segments in, the tile assembled in LDS, flat dx rows out.
//
// LDS IMAGE.  Sample s, vertex v, column c lives at tile[s*SP + v*P + c] with the vertex pitch P = F | 1 (odd)
// and the sample pitch SP = TV*P + d.
//   * ds_write_b32 / ds_read_b32 bank = dword address mod 32, conflicts within a 32-lane half.  The flat fill
//     writes consecutive dwords (odd F: pos = idx; even F: pos = idx + idx / F, one skipped dword per row):
//     conflict-free.  Lane-per-vertex accesses of one column (the mask column, the backward's per-vertex pass)
//     have stride P: odd, so 32 lanes hit 32 banks — with the natural pitch of an even F (P = F) they would be
//     2- to 32-way.
//   * the `wide` side walks (s, c) with c fastest: TV*P is a multiple of 32, so SP mod 32 = d and the lane
//     q = s*d + c sits on bank (q + v*P) mod 32: consecutive lanes, consecutive banks.
// The tile is 32 KiB (kTileFloats), so BS = as many samples as fit, at most ceil(batch / groups) so that the
// sample groups on gridDim.y are balanced; F = 9, batch = 20: 2 groups of 10 samples, 320-byte segments of
// `wide`.  34.3 KiB of LDS per workgroup: 4 workgroups = 16 waves per CU of the 160 KiB.
//
// SUMS.  esum products and sums are carried in double (a product of two fp32 numbers is exact in double):
// thread (vs, s, c) adds the vertices vs, vs + VS, ... of its column over every tile of the block's slab, the
// VS slices are added in slice order through LDS, each block writes one partial row, and eval_finish_kernel adds
// the partial rows in a fixed order — no float atomics, bitwise reproducible.  The mask MULTIPLIES:
// 0 * NaN = NaN, as in the fork.  The non-zero count is a ballot + popcount per wave, integer adds only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

constexpr int TV = 64;                   // vertices per tile: one wave = one sample's mask segment
constexpr int kTileFloats = 8192;        // the LDS image, 32 KiB
constexpr int64_t kMaxF = 64;

struct Shape {
    int P, SP, BS, groups, rows_per_block;
    int64_t blocks;
    Shape(int64_t n_rows, int64_t F, int64_t d, int64_t batch)
    {
        P = (int)F | 1;
        SP = TV * P + (int)d;
        const int64_t fit = std::max<int64_t>(1, kTileFloats / SP);
        groups = (int)((batch + fit - 1) / fit);
        BS = (int)((batch + groups - 1) / groups);
        groups = (int)((batch + BS - 1) / BS);
        const TileSlabs sl(n_rows, TV);
        blocks = sl.slabs;
        rows_per_block = sl.rows_per_block;
    }
};

// the block's place: its slab of rows and its group of samples
struct Place {
    int P, SP, e, j0, bs;
    int64_t r0, r1;
    __device__ __forceinline__ Place(int64_t n_rows, int F, int d, int batch, int BS, int rows_per_block)
    {
        P = F | 1;
        SP = TV * P + d;
        e = F - 1 - d;
        j0 = (int)blockIdx.y * BS;
        bs = min(BS, batch - j0);
        r0 = (int64_t)blockIdx.x * rows_per_block;
        r1 = min(r0 + (int64_t)rows_per_block, n_rows);
    }
};

__global__ __launch_bounds__(256) void eval_ingest_kernel(const float *__restrict__ x, const float *__restrict__ flag,
                                                          float *__restrict__ wide, float *__restrict__ mask,
                                                          double *__restrict__ part_sum,
                                                          long long *__restrict__ part_cnt, int64_t n_rows, int F,
                                                          int d, int batch, int BS, int rows_per_block)
{
    __shared__ float tile[kTileFloats];
    __shared__ double red[256];
    __shared__ int cnt[64];
    const Place p(n_rows, F, d, batch, BS, rows_per_block);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float rF = 1.0f / (float)F;
    // the thread's column sum: slice vs of the tile's vertices, pair pr = (sample, column)
    const int pairs = part_sum != nullptr ? p.bs * p.e : 0;      // < 128: bs * P <= kTileFloats / TV
    int VS = 1, vs = 0, pr = 0, sum_base = 0, sum_col = 0;
    bool sums = false;
    if (pairs > 0) {
        VS = min(TV, 256 / pairs);
        sums = t < pairs * VS;
        vs = t / pairs;
        pr = t - vs * pairs;
        const int ps = pr / p.e;
        sum_base = ps * p.SP;
        sum_col = d + (pr - ps * p.e);
    }
    double acc = 0.0;
    if (t < 64) cnt[t] = 0;                                     // (first used after the fill's barrier)
    for (int64_t t0 = p.r0; t0 < p.r1; t0 += TV) {
        const int nv = (int)min((int64_t)TV, p.r1 - t0);
        const int nvF = nv * F;
        for (int s = 0; s < p.bs; ++s) {                        // fill: consecutive dwords of each sample
            const float *xs = x + ((int64_t)(p.j0 + s) * n_rows + t0) * F;
            float *ts = tile + s * p.SP;
#pragma unroll 4
            for (int idx = t; idx < nvF; idx += 256) ts[(F & 1) ? idx : idx + fdiv(idx, rF)] = xs[idx];
        }
        __syncthreads();
        for (int s = wave; s < p.bs; s += 4) {                  // mask and count: one wave, one sample
            const bool live = lane < nv;
            const int at = s * p.SP + lane * p.P + F - 1;
            float m = 0.f;
            if (live) {
                const int64_t o = (int64_t)(p.j0 + s) * n_rows + t0 + lane;
                if (flag != nullptr) {
                    m = flag[o];
                    tile[at] = m;                               // (x's last column is not read when a flag is given)
                } else {
                    m = tile[at];
                }
                if (mask != nullptr) mask[o] = m;
            }
            const unsigned long long nz = __ballot(live && m != 0.f);     // NaN != 0
            if (lane == 0) cnt[s] += __popcll(nz);              // (sample s belongs to this wave alone)
        }
        if (flag != nullptr) __syncthreads();
        if (sums) {
            for (int v = vs; v < nv; v += VS) {
                const int row = sum_base + v * p.P;
                const double m = (double)tile[row + F - 1];
                acc = fma(m, (double)tile[row + sum_col], acc);           // 0 * NaN = NaN, as torch's product
            }
        }
        if (wide != nullptr) {                                  // rows of `wide`: (sample, column) fastest
            const int D = p.bs * d, total = nv * D;
            const float rD = 1.0f / (float)D, rd = 1.0f / (float)d;
            const int64_t ld = (int64_t)batch * d;
            float *ws = wide + t0 * ld + (int64_t)p.j0 * d;
#pragma unroll 4
            for (int el = t; el < total; el += 256) {
                const int v = fdiv(el, rD), q = el - v * D;
                const int s = fdiv(q, rd), c = q - s * d;
                ws[v * ld + q] = tile[s * p.SP + v * p.P + c];
            }
        }
        __syncthreads();
    }
    red[t] = acc;
    __syncthreads();
    if (sums && vs == 0) {
        for (int k = 1; k < VS; ++k) acc += red[k * pairs + pr];           // fixed order
        part_sum[((int64_t)blockIdx.x * batch + p.j0) * p.e + pr] = acc;
    }
    if (part_cnt != nullptr && t < p.bs) part_cnt[(int64_t)blockIdx.x * batch + p.j0 + t] = cnt[t];
}

// esum[col] = sum over the blocks' partial rows part_sum[n_blocks][We]; nonzero[col] the same of
// part_cnt[n_blocks][Wc].  A 256-thread block owns 32 columns of the We + Wc; thread (g, c) adds the partial rows
// g, g + 8, ... of its column, then the 8 group sums are added in group order through LDS: a fixed order.
__global__ __launch_bounds__(256) void eval_finish_kernel(const double *__restrict__ part_sum,
                                                          const long long *__restrict__ part_cnt, int n_blocks,
                                                          int64_t We, int64_t Wc, double *__restrict__ esum,
                                                          long long *__restrict__ nonzero)
{
    __shared__ double rs[8][33];
    __shared__ long long rc[8][33];
    const int c = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int64_t col = (int64_t)blockIdx.x * 32 + c;
    double a = 0.0;
    long long n = 0;
    if (col < We) {
        if (esum != nullptr)
            for (int k = grp; k < n_blocks; k += 8) a += part_sum[(int64_t)k * We + col];
    } else if (col < We + Wc) {
        if (nonzero != nullptr)
            for (int k = grp; k < n_blocks; k += 8) n += part_cnt[(int64_t)k * Wc + (col - We)];
    }
    rs[grp][c] = a;
    rc[grp][c] = n;
    __syncthreads();
    if (grp == 0) {
        for (int k = 1; k < 8; ++k) {
            a += rs[k][c];
            n += rc[k][c];
        }
        if (col < We) {
            if (esum != nullptr) esum[col] = a;
        } else if (col < We + Wc) {
            if (nonzero != nullptr) nonzero[col - We] = n;
        }
    }
}

__global__ __launch_bounds__(256) void eval_ingest_bwd_kernel(const float *__restrict__ x,
                                                              const float *__restrict__ flag,
                                                              const float *__restrict__ d_wide,
                                                              const float *__restrict__ d_mask,
                                                              const float *__restrict__ d_esum,
                                                              float *__restrict__ dx, float *__restrict__ dflag,
                                                              int64_t n_rows, int F, int d, int batch, int BS,
                                                              int rows_per_block)
{
    __shared__ float tile[kTileFloats];
    const Place p(n_rows, F, d, batch, BS, rows_per_block);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float rF = 1.0f / (float)F;
    const bool need_x = p.e > 0 && d_esum != nullptr;           // (a NULL d_esum is zero: nothing of x matters)
    for (int64_t t0 = p.r0; t0 < p.r1; t0 += TV) {
        const int nv = (int)min((int64_t)TV, p.r1 - t0);
        const int nvF = nv * F;
        if (need_x) {                                           // fill with what dm needs: the columns >= d
            for (int s = 0; s < p.bs; ++s) {
                const float *xs = x + ((int64_t)(p.j0 + s) * n_rows + t0) * F;
                float *ts = tile + s * p.SP;
#pragma unroll 4
                for (int idx = t; idx < nvF; idx += 256) {
                    const int v = fdiv(idx, rF);
                    if (idx - v * F >= d) ts[idx + v * (p.P - F)] = xs[idx];
                }
            }
            __syncthreads();
        }
        for (int s = wave; s < p.bs; s += 4) {                  // per vertex: one wave, one sample
            if (lane < nv) {
                const int j = p.j0 + s;
                const int64_t o = (int64_t)j * n_rows + t0 + lane;
                float *row = tile + s * p.SP + lane * p.P;
                double a = d_mask != nullptr ? (double)d_mask[o] : 0.0;
                if (need_x) {
                    const float m = flag != nullptr ? flag[o] : row[F - 1];
                    for (int c = d; c < F - 1; ++c) {
                        const float de = d_esum[(int64_t)j * p.e + (c - d)];
                        a = fma((double)row[c], (double)de, a);
                        if (dx != nullptr) row[c] = m * de;
                    }
                } else if (dx != nullptr) {
                    for (int c = d; c < F - 1; ++c) row[c] = 0.f;
                }
                const float dm = (float)a;                      // rounded once
                if (flag != nullptr) {
                    if (dflag != nullptr) dflag[o] = dm;
                    if (dx != nullptr) row[F - 1] = 0.f;
                } else {
                    row[F - 1] = dm;                            // (dx is not NULL without a flag)
                }
            }
        }
        if (dx != nullptr) {
            if (d > 0) {                                        // segments of d_wide's rows -> the columns < d
                const int D = p.bs * d, total = nv * D;
                const float rD = 1.0f / (float)D, rd = 1.0f / (float)d;
                const int64_t ld = (int64_t)batch * d;
                const float *ws = d_wide != nullptr ? d_wide + t0 * ld + (int64_t)p.j0 * d : nullptr;
#pragma unroll 4
                for (int el = t; el < total; el += 256) {
                    const int v = fdiv(el, rD), q = el - v * D;
                    const int s = fdiv(q, rd), c = q - s * d;
                    tile[s * p.SP + v * p.P + c] = ws != nullptr ? ws[v * ld + q] : 0.f;
                }
            }
            __syncthreads();
            for (int s = 0; s < p.bs; ++s) {                    // flat rows of dx: consecutive dwords
                float *xs = dx + ((int64_t)(p.j0 + s) * n_rows + t0) * F;
                const float *ts = tile + s * p.SP;
#pragma unroll 4
                for (int idx = t; idx < nvF; idx += 256) xs[idx] = ts[(F & 1) ? idx : idx + fdiv(idx, rF)];
            }
        }
        __syncthreads();
    }
}

bool shape_ok(int64_t n_rows, int64_t F, int64_t d, int64_t batch)
{
    return n_rows >= 1 && n_rows <= (int64_t)INT32_MAX * kSlabBlocks && F >= 2 && F <= kMaxF && d >= 0 && d <= F - 1 &&
           batch >= 1 && batch <= kMaxBatch;
}

bool off(const void *ptr, uintptr_t a) { return (uintptr_t)ptr % a != 0; }

}  // namespace

size_t gcn_eval_workspace_bytes(int64_t n_rows, int64_t F, int64_t d, int64_t batch)
{
    if (!shape_ok(n_rows, F, d, batch)) return 0;
    // per block: batch * e partial sums (double) and batch partial counts (int64); e + 1 = F - d
    return (size_t)Shape(n_rows, F, d, batch).blocks * (size_t)batch * (size_t)(F - d) * sizeof(double);
}

int gcn_eval_ingest(const float *x, const float *flag, int64_t n_rows, int64_t F, int64_t d, int64_t batch,
                    float *wide, float *mask, double *esum, int64_t *nonzero, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    const char *who = "gcn_eval_ingest";
    if (!shape_ok(n_rows, F, d, batch))
        return bad(who, GCN_E_BADARG, "needs n_rows >= 1, 2 <= F <= 64, 0 <= d <= F - 1 and 1 <= batch <= 65535");
    if (x == nullptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if (off(x, 4) || off(flag, 4) || off(wide, 4) || off(mask, 4) || off(esum, 8) || off(nonzero, 8))
        return bad(who, GCN_E_ALIGN, "4-byte alignment required (esum, nonzero: 8)");
    const int64_t e = F - 1 - d;
    if (d == 0) wide = nullptr;                                  // (nothing to copy)
    if (e == 0) esum = nullptr;                                  // (no column to sum)
    const bool reduces = esum != nullptr || nonzero != nullptr;
    if (reduces && (workspace == nullptr || workspace_bytes < gcn_eval_workspace_bytes(n_rows, F, d, batch)))
        return bad(who, GCN_E_WORKSPACE, "workspace too small");
    if (reduces && off(workspace, 16)) return bad(who, GCN_E_ALIGN, "16-byte alignment required");
    if (wide == nullptr && mask == nullptr && !reduces) return 0;
    const Shape sh(n_rows, F, d, batch);
    hipStream_t s = (hipStream_t)stream;
    double *part_sum = esum != nullptr ? (double *)workspace : nullptr;
    long long *part_cnt =
        nonzero != nullptr ? (long long *)((double *)workspace + sh.blocks * batch * e) : nullptr;
    hipLaunchKernelGGL(eval_ingest_kernel, dim3((unsigned)sh.blocks, (unsigned)sh.groups), dim3(256), 0, s, x, flag,
                       wide, mask, part_sum, part_cnt, n_rows, (int)F, (int)d, (int)batch, sh.BS, sh.rows_per_block);
    if (reduces) {
        const int64_t We = batch * e, Wc = batch;
        hipLaunchKernelGGL(eval_finish_kernel, dim3((unsigned)((We + Wc + 31) / 32)), dim3(256), 0, s,
                           (const double *)part_sum, (const long long *)part_cnt, (int)sh.blocks, We, Wc, esum,
                           (long long *)nonzero);
    }
    return launched(who);
}

int gcn_eval_ingest_backward(const float *x, const float *flag, const float *d_wide, const float *d_mask,
                             const float *d_esum, int64_t n_rows, int64_t F, int64_t d, int64_t batch, float *dx,
                             float *dflag, void *stream)
{
    const char *who = "gcn_eval_ingest_backward";
    if (!shape_ok(n_rows, F, d, batch))
        return bad(who, GCN_E_BADARG, "needs n_rows >= 1, 2 <= F <= 64, 0 <= d <= F - 1 and 1 <= batch <= 65535");
    if (x == nullptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if (dx == nullptr && (flag == nullptr || dflag == nullptr))
        return bad(who, GCN_E_BADARG, "dx may be NULL only when flag and dflag are given");
    if (dflag != nullptr && flag == nullptr) return bad(who, GCN_E_BADARG, "dflag needs flag");
    if (off(x, 4) || off(flag, 4) || off(d_wide, 4) || off(d_mask, 4) || off(d_esum, 4) || off(dx, 4) ||
        off(dflag, 4))
        return bad(who, GCN_E_ALIGN, "4-byte alignment required");
    const Shape sh(n_rows, F, d, batch);
    hipLaunchKernelGGL(eval_ingest_bwd_kernel, dim3((unsigned)sh.blocks, (unsigned)sh.groups), dim3(256), 0,
                       (hipStream_t)stream, x, flag, d_wide, d_mask, d_esum, dx, dflag, n_rows, (int)F, (int)d,
                       (int)batch, sh.BS, sh.rows_per_block);
    return launched(who);
}
