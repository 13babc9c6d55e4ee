// gcn_norm.hip — ReLU + training-mode BatchNorm over a [n_rows, F] activation as four full-height
// sweeps (gfx950).
//
// The reference fork's live model normalises the output of its first two layers,
//     x = apply_bn(F.relu(gc(x, adj)))          reference pygcn/models.py:49,53
//     apply_bn = nn.BatchNorm1d(x.size(1)).cuda()(x)                     :41-45
// i.e. batch statistics over all vertices, per feature column.  With x = relu ? relu(z) : z:
//     forward   bn_stats_kernel     reads z              -> mean, var (biased), rstd          1 stream
//               bn_apply_kernel     reads z, writes y    y = (x - mean) * rstd * gamma + beta 2 streams
//     backward  bn_bwd_sums_kernel  reads g, z           -> sum g, sum g * xhat, coef         2 streams
//               bn_bwd_apply_kernel reads g, z, writes dz                                     3 streams
//     dx = gamma * rstd * (g - sum_g / n - xhat * sum_gxhat / n),   dz = relu && z <= 0 ? 0 : dx
// The ReLU and its backward mask ride in the loads; xhat is recomputed from z, never stored.
//
// BACKWARD IN DOUBLE: dx is what is left of g after its components along 1 and xhat are taken out,
// plus a term of relative size eps * rstd^2.  Over few rows (n = 2: xhat = +-1 exactly spans the rest)
// the projection cancels to that term, and every fp32 rounding on the way — of mean, of rstd, of the
// two sums, of the products in the apply sweep — comes out multiplied by 1 / (eps * rstd^2): 3e-5 of
// max|dz| at 2 x 16 standard normal rows, in torch's own fp32 evaluation as much as in an fp32 sweep
// here.  So the backward pair does not pass fp32 through: bn_bwd_sums_kernel, which reads z anyway,
// also carries sum t and sum t^2 of t = x - mean (exact in double, and centred, so nothing cancels),
// and its finish kernel derives from them the mean's rounding error, var and rstd in double, and hands
// the apply sweep four DOUBLE columns coef[4][F] = { mean, rstd, sum_g / n, rstd^2 * sum g (x - mean) / n };
// bn_bwd_apply_kernel evaluates dx in double from them and rounds once, in the store.  That is
// 5 FP64 instructions per element pair loaded, on a part whose FP64 vector rate is half its FP32 one:
// the sweeps stay HBM-bound (DESIGN.md has the times).  sum_g / sum_gxhat (dbeta / dgamma) stay fp32 [F].
//
// Geometry of every sweep (that of bwd_colsum_kernel, gcn_backward.hip): a 256-thread block owns a
// contiguous slab of rows; thread t owns the 16 bytes (V = 4 fp32 / 8 bf16 columns) at column group
// t % CG (CG = F / V) of every (256 / CG)-th row of the slab, so its per-column constants live in
// registers for the whole slab.
//
// ACCUMULATION: the running sums (sum x, sum x^2; sum g, sum g * (x - mean)) are carried in DOUBLE,
// per thread, per block and in the finish kernel.  A product of two fp32 numbers is exact in double,
// so var = sum x^2 / n - mean^2 loses nothing to cancellation that fp32 could see (a column
// 1000 + N(0,1) keeps its variance: the stored fp32 var is 6e-8 of float64, its own rounding; plain fp32
// sums miss it by 9e-2).  Each block writes one
// partial row [2][F]; bn_finish_kernel adds the partial rows in a fixed order — no float atomics,
// bitwise reproducible.  The sweeps are HBM-bound: 3 FP64 instructions per element loaded.
//
// COLUMN WINDOWS (the *_batched entry points): k samples over the same vertices lie side by side as
// [n_rows, k * F] (GraphConvolution's batched layout), and per-sample BatchNorm is per-column BatchNorm of
// that matrix.  gridDim.y walks the k windows [j * F, (j + 1) * F): a block sweeps its slab of ONE window
// with the row pitch k * F, so the window width obeys the shape rule and k is free.  The slabs, the lane
// of every thread, the partial layout of a window and every summation order are those of the 2-D sweep
// (which is the k = 1 launch of the same kernels): a window's results are, bit for bit, what the 2-D
// entry point returns on a contiguous copy of the window.
//
// MASKED MEAN POOL (the fork's PoolLayer, reference pygcn/models.py:267-286) over the same layout:
// pool_colsum_kernel is bn_stats_kernel with a per-row, per-window weight mask[j, r] and one sum;
// pool_broadcast_kernel writes its gradient mask[j, r] * coef[j * C + c] in one sweep.  The mask stays
// [k, n_rows], as the caller holds it: a block's slab reads consecutive floats of ONE mask row.  (As
// [n_rows, k] every row of a window fetched 4 bytes of a line of its own: measured at 10^6 x (20 x 32)
// fp32, 4.6 instead of 5.8 TB/s for the sum and 3.8 instead of 4.8 for the broadcast.)
//
// VERTEX ATTENTION (the head of the fork's SoftGenerator, reference pygcn/models.py:324-329:
// attn = softmax over the vertices of torch.mul(key, x).sum(dim=1)) over the same layout, one key [C] per
// window, every per-row vector [k, n_rows] as the pool's mask:
//     forward   attn_scores_kernel    reads h      -> s[j, r] = key_j . h[r, window j], rounded once to fp32,
//                                                     and per block (max, sum exp(s - max)) of the ROUNDED scores
//               attn_finish_kernel    merges the per-block pairs in a fixed order -> (M, Z) per window, double
//               attn_normalize_kernel [k, n_rows] floats: attn = exp(s - M) / Z
//     backward  attn_backward_kernel  reads h, ds  -> writes dh = ds[r] * key, sums dkey = sum_r ds[r] * h[r, :]
//                                                     as pool_colsum_kernel does (then bn_finish_kernel<1>)
// ds = attn * (g - sum g attn) is [k, n_rows]-sized work left to the caller.  The dot of a row is carried in
// double by the CG threads of the row and added by cross-lane moves (and through LDS where a row spans 2 or
// 4 waves); the exponentials are double, evaluated once per row with all lanes busy.  A NaN score makes the
// window's Z, and with it every attn of the window, NaN — torch's softmax — and touches no other window.
//
// NaN / inf follow torch: relu keeps NaN (z < 0 ? 0 : z), an inf in a column gives mean = inf and
// var = rstd = NaN for that column only, and the backward mask is torch's threshold_backward
// (z <= 0 ? 0 : dx), so a NaN z lets its (NaN) dx through.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

// where a thread stands in its block's slab, and the slab in the matrix: blockIdx.y is the column
// window [w0, w0 + F) of a [n_rows, gridDim.y * F] matrix (one window, pitch F: the 2-D entry points)
struct Place {
    int CG, RL, cg, rl;
    int64_t r0, r1, ld;
    int c0;                               // the thread's first column in the whole matrix
    __device__ __forceinline__ Place(int F, int V, int64_t n_rows, int rows_per_block)
    {
        CG = F / V; RL = 256 / CG;
        cg = threadIdx.x % CG; rl = threadIdx.x / CG;
        r0 = (int64_t)blockIdx.x * rows_per_block;
        r1 = min(r0 + (int64_t)rows_per_block, n_rows);
        ld = (int64_t)gridDim.y * F;
        c0 = (int)blockIdx.y * F + V * cg;
    }
    __device__ __forceinline__ int64_t at(int64_t r) const { return r * ld + c0; }
    // the block's partial row: window after window, each laid out as the 2-D sweep's [gridDim.x][NS][F]
    __device__ __forceinline__ int64_t slot() const { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }
};

// sums of the block's 256 / CG row lanes, added in lane order, written to dst[V * cg ..]
template <int V>
__device__ __forceinline__ void block_combine(double (&acc)[V], double *red, const Place &p, double *dst)
{
    __syncthreads();                      // (red may still be read from the previous call)
#pragma unroll
    for (int i = 0; i < V; ++i) red[threadIdx.x * V + i] = acc[i];
    __syncthreads();
    if (p.rl == 0) {
        for (int k = 1; k < p.RL; ++k)    // fixed order
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] += red[(k * p.CG + p.cg) * V + i];
#pragma unroll
        for (int i = 0; i < V; ++i) dst[V * p.cg + i] = acc[i];
    }
}

// partial[block][0][F] = sum x, partial[block][1][F] = sum x^2 over the block's slab
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_kernel(const T *__restrict__ z, double *__restrict__ partial,
                                                       int64_t n_rows, int F, int relu, int rows_per_block)
{
    constexpr int V = Lane<T>::V;
    typedef typename Lane<T>::Raw Raw;
    __shared__ double red[256 * V];
    const Place p(F, V, n_rows, rows_per_block);
    double s[V], q[V];
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = q[i] = 0.0;
    for (int64_t r = p.r0 + p.rl; r < p.r1; r += p.RL) {
        float x[V];
        Lane<T>::unpack(*(const Raw *)(z + p.at(r)), x);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const double d = (double)act(x[i], relu);
            s[i] += d;
            q[i] = fma(d, d, q[i]);
        }
    }
    double *row = partial + p.slot() * 2 * F;
    block_combine<V>(s, red, p, row);
    block_combine<V>(q, red, p, row + F);
}

// partial[block][0..3][F] = sum g, sum g * t, sum t, sum t^2 over the block's slab, t = x - mean
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const T *__restrict__ g, const T *__restrict__ z,
                                                          double *__restrict__ partial, int64_t n_rows, int F,
                                                          int relu, int rows_per_block,
                                                          const float *__restrict__ mean)
{
    constexpr int V = Lane<T>::V;
    typedef typename Lane<T>::Raw Raw;
    __shared__ double red[256 * V];
    const Place p(F, V, n_rows, rows_per_block);
    double mu[V], s[V], q[V], st[V], stt[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        mu[i] = (double)mean[p.c0 + i];
        s[i] = q[i] = st[i] = stt[i] = 0.0;
    }
    for (int64_t r = p.r0 + p.rl; r < p.r1; r += p.RL) {
        const int64_t off = p.at(r);
        float x[V], gg[V];
        Lane<T>::unpack(*(const Raw *)(g + off), gg);
        Lane<T>::unpack(*(const Raw *)(z + off), x);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const double d = (double)gg[i];
            const double t = (double)act(x[i], relu) - mu[i];
            s[i] += d;
            q[i] = fma(d, t, q[i]);
            st[i] += t;
            stt[i] = fma(t, t, stt[i]);
        }
    }
    double *row = partial + p.slot() * 4 * F;
    block_combine<V>(s, red, p, row);
    block_combine<V>(q, red, p, row + F);
    block_combine<V>(st, red, p, row + 2 * F);
    block_combine<V>(stt, red, p, row + 3 * F);
}

// y = (x - mean) * (rstd * gamma) + beta
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T *__restrict__ z, T *__restrict__ y, int64_t n_rows,
                                                       int F, int relu, int rows_per_block,
                                                       const float *__restrict__ mean,
                                                       const float *__restrict__ rstd,
                                                       const float *__restrict__ gamma,
                                                       const float *__restrict__ beta)
{
    constexpr int V = Lane<T>::V;
    typedef typename Lane<T>::Raw Raw;
    const Place p(F, V, n_rows, rows_per_block);
    float mu[V], sc[V], sh[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int f = p.c0 + i;
        mu[i] = mean[f];
        sc[i] = gamma ? rstd[f] * gamma[f] : rstd[f];
        sh[i] = beta ? beta[f] : 0.f;
    }
    for (int64_t r = p.r0 + p.rl; r < p.r1; r += p.RL) {
        const int64_t off = p.at(r);
        float x[V];
        Lane<T>::unpack(*(const Raw *)(z + off), x);
#pragma unroll
        for (int i = 0; i < V; ++i) x[i] = fmaf(act(x[i], relu) - mu[i], sc[i], sh[i]);
        *(Raw *)(y + off) = Lane<T>::pack(x);
    }
}

// dz = mask * gamma * rstd * (g - sum_g / n - (x - mean) * rstd^2 * sum g (x - mean) / n), in double from
// coef[4][ld] (see the file header); dz may alias g (a thread reads its 16 bytes of g before it writes
// the same 16 bytes of dz)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T *g, const T *__restrict__ z, T *dz,
                                                           int64_t n_rows, int F, int relu, int rows_per_block,
                                                           const float *__restrict__ gamma,
                                                           const double *__restrict__ coef)
{
    constexpr int V = Lane<T>::V;
    typedef typename Lane<T>::Raw Raw;
    const Place p(F, V, n_rows, rows_per_block);
    double mu[V], a[V], b[V], c[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int f = p.c0 + i;
        mu[i] = coef[f];
        a[i] = gamma ? coef[p.ld + f] * (double)gamma[f] : coef[p.ld + f];
        b[i] = coef[2 * p.ld + f];
        c[i] = coef[3 * p.ld + f];
    }
    for (int64_t r = p.r0 + p.rl; r < p.r1; r += p.RL) {
        const int64_t off = p.at(r);
        float x[V], gg[V];
        Lane<T>::unpack(*(const Raw *)(g + off), gg);
        Lane<T>::unpack(*(const Raw *)(z + off), x);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const double t = (double)act(x[i], relu) - mu[i];
            const float dx = (float)(a[i] * fma(-t, c[i], (double)gg[i] - b[i]));
            gg[i] = (relu && x[i] <= 0.f) ? 0.f : dx;     // torch's threshold_backward: NaN z passes dx
        }
        *(Raw *)(dz + off) = Lane<T>::pack(gg);
    }
}

// partial[window][n_blocks][NS][F] -> per-column results of window blockIdx.y, written at columns
// [window * F, (window + 1) * F) of vectors of length gridDim.y * F.  A 1024-thread block owns 32 columns;
// thread (g, c) adds the partial rows g, g+32, ... of column c, then the 32 group sums are added in group
// order through LDS: a fixed order, the same for a window as for the 2-D sweep (gridDim.y = 1).
//   NS = 2 (forward):  (sum x, sum x^2) -> mean, biased var, rstd                       fp32
//   NS = 4 (backward): (sum g, sum g t, sum t, sum t^2), t = x - mean32 -> sum_g, sum_gxhat fp32 and
//                      coef[4][gridDim.y * F] in double: the mean, var and rstd of the column to double
//                      precision (mean = mean32 + sum t / n; var = sum t^2 / n - (sum t / n)^2, centred)
//   NS = 1 (pool):     the sum itself, in double -> coef
template <int NS>
__global__ __launch_bounds__(1024) void bn_finish_kernel(const double *__restrict__ partial, int n_blocks, int F,
                                                         double n, float eps, const float *__restrict__ mean_in,
                                                         float *__restrict__ out0, float *__restrict__ out1,
                                                         float *__restrict__ out2, double *__restrict__ coef)
{
    __shared__ double red[NS][32][33];
    const int c = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int f = blockIdx.x * 32 + c;
    const int64_t ld = (int64_t)gridDim.y * F;
    const int64_t o = (int64_t)blockIdx.y * F + f;       // the column in the whole matrix
    partial += (int64_t)blockIdx.y * n_blocks * NS * F;
    double a[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) a[j] = 0.0;
    if (f < F) {
#pragma unroll 4
        for (int k = grp; k < n_blocks; k += 32)
#pragma unroll
            for (int j = 0; j < NS; ++j) a[j] += partial[((int64_t)k * NS + j) * F + f];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) red[j][grp][c] = a[j];
    __syncthreads();
    if (grp == 0 && f < F) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            a[j] = 0.0;
            for (int k = 0; k < 32; ++k) a[j] += red[j][k][c];
        }
        if constexpr (NS == 1) {
            coef[o] = a[0];
        } else if constexpr (NS == 2) {
            const double m = a[0] / n;
            double v = a[1] / n - m * m;
            v = v < 0.0 ? 0.0 : v;                       // (keeps NaN)
            out0[o] = (float)m;
            out1[o] = (float)v;
            out2[o] = (float)(1.0 / sqrt(v + (double)eps));
        } else {
            // (nl_finish of gcn_normlin.hip repeats these lines: the two must agree to the bit)
            const double d = a[2] / n;                   // mean - mean32
            double v = a[3] / n - d * d;
            v = v < 0.0 ? 0.0 : v;
            const double rs = 1.0 / sqrt(v + (double)eps);
            const double sgx = a[1] - d * a[0];          // sum g (x - mean)
            out0[o] = (float)a[0];
            out1[o] = (float)(sgx * rs);
            coef[o] = (double)mean_in[o] + d;
            coef[ld + o] = rs;
            coef[2 * ld + o] = a[0] / n;
            coef[3 * ld + o] = rs * rs * (sgx / n);
        }
    }
}

// masked column sums of window blockIdx.y: partial[slot][F] = sum_r mask[window, r] * h[r, window's columns]
// over the block's slab (a product of two fp32 numbers is exact in double)
template <typename T>
__global__ __launch_bounds__(256) void pool_colsum_kernel(const T *__restrict__ h, const float *__restrict__ mask,
                                                          double *__restrict__ partial, int64_t n_rows, int F,
                                                          int rows_per_block)
{
    constexpr int V = Lane<T>::V;
    typedef typename Lane<T>::Raw Raw;
    __shared__ double red[256 * V];
    const Place p(F, V, n_rows, rows_per_block);
    double s[V];
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = 0.0;
    for (int64_t r = p.r0 + p.rl; r < p.r1; r += p.RL) {
        const double m = (double)mask[(int64_t)blockIdx.y * n_rows + r];
        float x[V];
        Lane<T>::unpack(*(const Raw *)(h + p.at(r)), x);
#pragma unroll
        for (int i = 0; i < V; ++i) s[i] = fma(m, (double)x[i], s[i]);   // 0 * NaN = NaN, as torch's product
    }
    block_combine<V>(s, red, p, partial + p.slot() * F);
}

// dh[r, window's columns] = mask[window, r] * coef[window's columns]
template <typename T>
__global__ __launch_bounds__(256) void pool_broadcast_kernel(const float *__restrict__ mask,
                                                             const float *__restrict__ coef, T *__restrict__ dh,
                                                             int64_t n_rows, int F, int rows_per_block)
{
    constexpr int V = Lane<T>::V;
    typedef typename Lane<T>::Raw Raw;
    const Place p(F, V, n_rows, rows_per_block);
    float c[V];
#pragma unroll
    for (int i = 0; i < V; ++i) c[i] = coef[p.c0 + i];
    for (int64_t r = p.r0 + p.rl; r < p.r1; r += p.RL) {
        const float m = mask[(int64_t)blockIdx.y * n_rows + r];
        float x[V];
#pragma unroll
        for (int i = 0; i < V; ++i) x[i] = m * c[i];
        *(Raw *)(dh + p.at(r)) = Lane<T>::pack(x);
    }
}

// ---- vertex attention: attn = softmax over the rows of (h . key), per window (file header)
//
// a running (max, sum of exp(s - max)) of a set of scores, in double.  z == 0 marks the empty set (a
// non-empty one has z >= 1 or NaN), so an empty slab or lane drops out instead of giving exp(-inf + inf)
struct MaxSum {
    double m, z;
    __device__ __forceinline__ void add(float s)
    {
        const double d = (double)s;
        const double e = exp(-fabs(d - m));              // NaN s: e = NaN, the comparison fails, z = NaN
        if (d > m) { z = fma(z, e, 1.0); m = d; }
        else z += e;
    }
    __device__ __forceinline__ void merge(double m2, double z2)
    {
        if (z2 == 0.0) return;
        if (z == 0.0) { m = m2; z = z2; return; }
        const double top = m2 > m ? m2 : m;
        z = z * exp(m - top) + z2 * exp(m2 - top);
        m = top;
    }
};

// the 256 MaxSums of a block merged as a fixed tree through LDS; the result is thread 0's
__device__ __forceinline__ void block_merge(MaxSum &a, double *red_m, double *red_z)
{
    red_m[threadIdx.x] = a.m;
    red_z[threadIdx.x] = a.z;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            a.merge(red_m[threadIdx.x + s], red_z[threadIdx.x + s]);
            red_m[threadIdx.x] = a.m;
            red_z[threadIdx.x] = a.z;
        }
        __syncthreads();
    }
}

// scores[window, r] = (float) sum_c key[window's columns] * h[r, window's columns], and the block's
// MaxSum of its slab's ROUNDED scores -> partial[slot][2].
// The CG threads of a row are consecutive lanes.  Their partial dots (double) are added by a butterfly
// of cross-lane moves over min(CG, 64) lanes — a + b = b + a, so every lane of the row holds the same
// bits — and for CG = 128 / 256 the 2 / 4 wave sums of the row are added in wave order through LDS.
// The row's lane (iteration % min(CG, 64)) of its first wave rounds, stores and keeps the score; every
// min(CG, 64) iterations all lanes fold the score they keep into their MaxSum at once, so the double
// exp costs one evaluation per 64 rows and not one per row.  Every trip count is block-uniform.
template <typename T>
__global__ __launch_bounds__(256) void attn_scores_kernel(const T *__restrict__ h, const float *__restrict__ key,
                                                          float *__restrict__ scores, double *__restrict__ partial,
                                                          int64_t n_rows, int C, int rows_per_block)
{
    constexpr int V = Lane<T>::V;
    typedef typename Lane<T>::Raw Raw;
    __shared__ double wsum[2][4];
    __shared__ double red_m[256], red_z[256];
    const Place p(C, V, n_rows, rows_per_block);
    const int W = p.CG < 64 ? p.CG : 64;                 // lanes of a row within one wave
    const int wave = threadIdx.x >> 6;
    double kk[V];
#pragma unroll
    for (int i = 0; i < V; ++i) kk[i] = (double)key[p.c0 + i];
    MaxSum acc = {-INFINITY, 0.0};
    float kept = 0.f;
    bool keeps = false;
    int it = 0;
    for (int64_t base = p.r0; base < p.r1; base += p.RL, ++it) {
        const int64_t r = base + p.rl;
        const bool live = r < p.r1;
        double d = 0.0;
        if (live) {
            float x[V];
            Lane<T>::unpack(*(const Raw *)(h + p.at(r)), x);
#pragma unroll
            for (int i = 0; i < V; ++i) d = fma(kk[i], (double)x[i], d);
        }
        for (int m = 1; m < W; m <<= 1) d += __shfl_xor(d, m, 64);
        if (p.CG > 64) {                                 // (block-uniform)
            if ((threadIdx.x & 63) == 0) wsum[it & 1][wave] = d;
            __syncthreads();                             // (the other buffer is the previous iteration's)
            const int w0 = p.rl * (p.CG >> 6);
            d = wsum[it & 1][w0];
            for (int w = 1; w < (p.CG >> 6); ++w) d += wsum[it & 1][w0 + w];
        }
        const int turn = it & (W - 1);
        if (live && p.cg == turn) {                      // (cg < W: the row's first wave)
            kept = (float)d;
            keeps = true;
            scores[(int64_t)blockIdx.y * n_rows + r] = kept;
        }
        if (turn == W - 1) {
            if (keeps) acc.add(kept);
            keeps = false;
        }
    }
    if (keeps) acc.add(kept);
    block_merge(acc, red_m, red_z);
    if (threadIdx.x == 0) {
        partial[p.slot() * 2] = acc.m;
        partial[p.slot() * 2 + 1] = acc.z;
    }
}

// stats[window] = (M, Z) of the window's n_blocks partial pairs: thread t merges the pairs t, t + 256, ...
// in that order, then the 256 threads merge as block_merge's tree — a fixed order, the same for every batch
__global__ __launch_bounds__(256) void attn_finish_kernel(const double *__restrict__ partial, int n_blocks,
                                                          double *__restrict__ stats)
{
    __shared__ double red_m[256], red_z[256];
    partial += (int64_t)blockIdx.x * n_blocks * 2;
    MaxSum acc = {-INFINITY, 0.0};
    for (int b = threadIdx.x; b < n_blocks; b += 256) acc.merge(partial[2 * b], partial[2 * b + 1]);
    block_merge(acc, red_m, red_z);
    if (threadIdx.x == 0) {
        stats[2 * blockIdx.x] = acc.m;
        stats[2 * blockIdx.x + 1] = acc.z;
    }
}

// attn[window, r] = (float)(exp(s - M) / Z); attn may alias scores (a thread reads its float before it
// writes the same float)
__global__ __launch_bounds__(256) void attn_normalize_kernel(const float *scores, const double *__restrict__ stats,
                                                             float *attn, int64_t n_rows)
{
    const double M = stats[2 * blockIdx.y], Z = stats[2 * blockIdx.y + 1];
    const int64_t w = (int64_t)blockIdx.y * n_rows;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256)
        attn[w + r] = (float)(exp((double)scores[w + r] - M) / Z);
}

// dh[r, window's columns] = ds[window, r] * key[window's columns] (skipped when dh is NULL) and
// partial[slot][C] = sum_r ds[window, r] * h[r, window's columns] over the block's slab, accumulated as
// pool_colsum_kernel accumulates its masked sums
template <typename T>
__global__ __launch_bounds__(256) void attn_backward_kernel(const T *__restrict__ h, const float *__restrict__ ds,
                                                            const float *__restrict__ key, T *__restrict__ dh,
                                                            double *__restrict__ partial, int64_t n_rows, int C,
                                                            int rows_per_block)
{
    constexpr int V = Lane<T>::V;
    typedef typename Lane<T>::Raw Raw;
    __shared__ double red[256 * V];
    const Place p(C, V, n_rows, rows_per_block);
    float kk[V];
    double s[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        kk[i] = key[p.c0 + i];
        s[i] = 0.0;
    }
    for (int64_t r = p.r0 + p.rl; r < p.r1; r += p.RL) {
        const int64_t off = p.at(r);
        const float d = ds[(int64_t)blockIdx.y * n_rows + r];
        float x[V];
        Lane<T>::unpack(*(const Raw *)(h + off), x);
#pragma unroll
        for (int i = 0; i < V; ++i) s[i] = fma((double)d, (double)x[i], s[i]);
        if (dh != nullptr) {
#pragma unroll
            for (int i = 0; i < V; ++i) x[i] = d * kk[i];
            *(Raw *)(dh + off) = Lane<T>::pack(x);
        }
    }
    block_combine<V>(s, red, p, partial + p.slot() * C);
}

bool rows_ok(int64_t n_rows, int64_t min_rows) { return n_rows >= min_rows && n_rows <= (int64_t)INT32_MAX * kSlabBlocks; }

bool shape_ok(int64_t n_rows, int64_t F, int dtype) { return rows_ok(n_rows, 2) && lane_width_ok(F, dtype); }

bool batch_ok(int64_t batch) { return batch >= 1 && batch <= kMaxBatch; }

// how few rows a sweep takes, and the sentence that says so: BatchNorm needs two, the pool and attention sweeps one
struct RowsRule {
    int64_t min_rows;
    const char *text;
};
constexpr RowsRule kBnRows = {2, "needs n_rows >= 2 and F a multiple of the 16-byte lane width with F/width dividing 256"};
constexpr RowsRule kPoolRows = {1, "needs n_rows >= 1 and C a multiple of the 16-byte lane width with C/width dividing 256"};

// the argument checks every entry point of this file with a [n_rows, batch * F] tensor shares; 0 = go on
int check(const char *who, const RowsRule &rule, int dtype, int64_t n_rows, int64_t F, int64_t batch, bool null_ptr,
          uintptr_t tensors)
{
    if (dtype != GCN_DTYPE_F32 && dtype != GCN_DTYPE_BF16) return bad(who, GCN_E_BADARG, "unknown dtype");
    if (!rows_ok(n_rows, rule.min_rows) || !lane_width_ok(F, dtype)) return bad(who, GCN_E_BADARG, rule.text);
    if (!batch_ok(batch)) return bad(who, GCN_E_BADARG, "needs 1 <= batch <= 65535");
    if (null_ptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if (tensors % 16 != 0) return bad(who, GCN_E_ALIGN, "16-byte alignment required");
    return 0;
}

dim3 finish_grid(int64_t F, int64_t batch) { return dim3((unsigned)((F + 31) / 32), (unsigned)batch); }

// The four sweeps over `batch` column windows of width F; the 2-D entry points are batch = 1.
int stats(const char *who, int dtype, const void *z, int64_t n_rows, int64_t F, int64_t batch, int relu, float eps,
          float *mean, float *var, float *rstd, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check(who, kBnRows, dtype, n_rows, F, batch,
                       z == nullptr || mean == nullptr || var == nullptr || rstd == nullptr, (uintptr_t)z))
        return rc;
    if (workspace == nullptr || workspace_bytes < gcn_bn_batched_workspace_bytes(n_rows, F, batch, dtype))
        return bad(who, GCN_E_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace % 16 != 0) return bad(who, GCN_E_ALIGN, "16-byte alignment required");
    const RowSlabs sl(n_rows);
    const dim3 grid((unsigned)sl.blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)workspace;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(bn_stats_kernel<T>, grid, block, 0, s, (const T *)z, part, n_rows, (int)F, relu,
                           sl.rows_per_block);
    });
    hipLaunchKernelGGL(bn_finish_kernel<2>, finish_grid(F, batch), dim3(1024), 0, s, (const double *)part,
                       (int)sl.blocks, (int)F, (double)n_rows, eps, (const float *)nullptr, mean, var, rstd,
                       (double *)nullptr);
    return launched(who);
}

int apply(const char *who, int dtype, const void *z, void *y, int64_t n_rows, int64_t F, int64_t batch, int relu,
          const float *mean, const float *rstd, const float *gamma, const float *beta, void *stream)
{
    if (int rc = check(who, kBnRows, dtype, n_rows, F, batch,
                       z == nullptr || y == nullptr || mean == nullptr || rstd == nullptr,
                       (uintptr_t)z | (uintptr_t)y))
        return rc;
    const RowSlabs sl(n_rows);
    const dim3 grid((unsigned)sl.blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(bn_apply_kernel<T>, grid, block, 0, s, (const T *)z, (T *)y, n_rows, (int)F, relu,
                           sl.rows_per_block, mean, rstd, gamma, beta);
    });
    return launched(who);
}

int backward_sums(const char *who, int dtype, const void *g, const void *z, int64_t n_rows, int64_t F,
                  int64_t batch, int relu, float eps, const float *mean, float *sum_g, float *sum_gxhat,
                  double *coef, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check(who, kBnRows, dtype, n_rows, F, batch,
                       g == nullptr || z == nullptr || mean == nullptr || sum_g == nullptr ||
                           sum_gxhat == nullptr || coef == nullptr,
                       (uintptr_t)g | (uintptr_t)z))
        return rc;
    if (workspace == nullptr || workspace_bytes < gcn_bn_batched_workspace_bytes(n_rows, F, batch, dtype))
        return bad(who, GCN_E_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace % 16 != 0 || (uintptr_t)coef % 8 != 0)
        return bad(who, GCN_E_ALIGN, "16-byte alignment required (coef: 8)");
    const RowSlabs sl(n_rows);
    const dim3 grid((unsigned)sl.blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)workspace;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(bn_bwd_sums_kernel<T>, grid, block, 0, s, (const T *)g, (const T *)z, part, n_rows, (int)F,
                           relu, sl.rows_per_block, mean);
    });
    hipLaunchKernelGGL(bn_finish_kernel<4>, finish_grid(F, batch), dim3(1024), 0, s, (const double *)part,
                       (int)sl.blocks, (int)F, (double)n_rows, eps, mean, sum_g, sum_gxhat, (float *)nullptr, coef);
    return launched(who);
}

int backward_apply(const char *who, int dtype, const void *g, const void *z, void *dz, int64_t n_rows, int64_t F,
                   int64_t batch, int relu, const float *gamma, const double *coef, void *stream)
{
    if (int rc = check(who, kBnRows, dtype, n_rows, F, batch,
                       g == nullptr || z == nullptr || dz == nullptr || coef == nullptr,
                       (uintptr_t)g | (uintptr_t)z | (uintptr_t)dz))
        return rc;
    if ((uintptr_t)coef % 8 != 0) return bad(who, GCN_E_ALIGN, "coef: 8-byte alignment required");
    const RowSlabs sl(n_rows);
    const dim3 grid((unsigned)sl.blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, grid, block, 0, s, (const T *)g, (const T *)z, (T *)dz, n_rows,
                           (int)F, relu, sl.rows_per_block, gamma, coef);
    });
    return launched(who);
}

}   // namespace

extern "C" {

size_t gcn_bn_workspace_bytes(int64_t n_rows, int64_t F, int dtype)
{
    if (!shape_ok(n_rows, F, dtype)) return 0;
    return (size_t)RowSlabs(n_rows).blocks * 4 * (size_t)F * sizeof(double);    // backward: 4 sums per block
}

size_t gcn_bn_batched_workspace_bytes(int64_t n_rows, int64_t F, int64_t batch, int dtype)
{
    return batch_ok(batch) ? (size_t)batch * gcn_bn_workspace_bytes(n_rows, F, dtype) : 0;
}

int gcn_bn_stats(int dtype, const void *z, int64_t n_rows, int64_t F, int relu, float eps, float *mean,
                 float *var, float *rstd, void *workspace, size_t workspace_bytes, void *stream)
{
    return stats("gcn_bn_stats", dtype, z, n_rows, F, 1, relu, eps, mean, var, rstd, workspace, workspace_bytes,
                 stream);
}

int gcn_bn_apply(int dtype, const void *z, void *y, int64_t n_rows, int64_t F, int relu, const float *mean,
                 const float *rstd, const float *gamma, const float *beta, void *stream)
{
    return apply("gcn_bn_apply", dtype, z, y, n_rows, F, 1, relu, mean, rstd, gamma, beta, stream);
}

int gcn_bn_backward_sums(int dtype, const void *g, const void *z, int64_t n_rows, int64_t F, int relu, float eps,
                         const float *mean, float *sum_g, float *sum_gxhat, double *coef, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    return backward_sums("gcn_bn_backward_sums", dtype, g, z, n_rows, F, 1, relu, eps, mean, sum_g, sum_gxhat, coef,
                         workspace, workspace_bytes, stream);
}

int gcn_bn_backward_apply(int dtype, const void *g, const void *z, void *dz, int64_t n_rows, int64_t F, int relu,
                          const float *gamma, const double *coef, void *stream)
{
    return backward_apply("gcn_bn_backward_apply", dtype, g, z, dz, n_rows, F, 1, relu, gamma, coef, stream);
}

int gcn_bn_stats_batched(int dtype, const void *z, int64_t n_rows, int64_t F, int64_t batch, int relu, float eps,
                         float *mean, float *var, float *rstd, void *workspace, size_t workspace_bytes,
                         void *stream)
{
    return stats("gcn_bn_stats_batched", dtype, z, n_rows, F, batch, relu, eps, mean, var, rstd, workspace,
                 workspace_bytes, stream);
}

int gcn_bn_apply_batched(int dtype, const void *z, void *y, int64_t n_rows, int64_t F, int64_t batch, int relu,
                         const float *mean, const float *rstd, const float *gamma, const float *beta, void *stream)
{
    return apply("gcn_bn_apply_batched", dtype, z, y, n_rows, F, batch, relu, mean, rstd, gamma, beta, stream);
}

int gcn_bn_backward_sums_batched(int dtype, const void *g, const void *z, int64_t n_rows, int64_t F, int64_t batch,
                                 int relu, float eps, const float *mean, float *sum_g, float *sum_gxhat,
                                 double *coef, void *workspace, size_t workspace_bytes, void *stream)
{
    return backward_sums("gcn_bn_backward_sums_batched", dtype, g, z, n_rows, F, batch, relu, eps, mean, sum_g,
                         sum_gxhat, coef, workspace, workspace_bytes, stream);
}

int gcn_bn_backward_apply_batched(int dtype, const void *g, const void *z, void *dz, int64_t n_rows, int64_t F,
                                  int64_t batch, int relu, const float *gamma, const double *coef, void *stream)
{
    return backward_apply("gcn_bn_backward_apply_batched", dtype, g, z, dz, n_rows, F, batch, relu, gamma, coef,
                          stream);
}

size_t gcn_pool_workspace_bytes(int64_t n_rows, int64_t C, int64_t batch, int dtype)
{
    if (!rows_ok(n_rows, 1) || !lane_width_ok(C, dtype) || !batch_ok(batch)) return 0;
    return (size_t)batch * (size_t)RowSlabs(n_rows).blocks * (size_t)C * sizeof(double);   // one sum per block
}

int gcn_masked_colsum(int dtype, const void *h, const float *mask, int64_t n_rows, int64_t C, int64_t batch,
                      double *sums, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gcn_masked_colsum";
    if (int rc = check(who, kPoolRows, dtype, n_rows, C, batch, h == nullptr || mask == nullptr || sums == nullptr,
                            (uintptr_t)h))
        return rc;
    if (workspace == nullptr || workspace_bytes < gcn_pool_workspace_bytes(n_rows, C, batch, dtype))
        return bad(who, GCN_E_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace % 16 != 0 || (uintptr_t)sums % 8 != 0 || (uintptr_t)mask % 4 != 0)
        return bad(who, GCN_E_ALIGN, "16-byte alignment required (sums: 8, mask: 4)");
    const RowSlabs sl(n_rows);
    const dim3 grid((unsigned)sl.blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)workspace;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(pool_colsum_kernel<T>, grid, block, 0, s, (const T *)h, mask, part, n_rows, (int)C,
                           sl.rows_per_block);
    });
    hipLaunchKernelGGL(bn_finish_kernel<1>, finish_grid(C, batch), dim3(1024), 0, s, (const double *)part,
                       (int)sl.blocks, (int)C, 1.0, 0.f, (const float *)nullptr, (float *)nullptr, (float *)nullptr,
                       (float *)nullptr, sums);
    return launched(who);
}

int gcn_masked_broadcast(int dtype, const float *mask, const float *coef, void *dh, int64_t n_rows, int64_t C,
                         int64_t batch, void *stream)
{
    const char *who = "gcn_masked_broadcast";
    if (int rc = check(who, kPoolRows, dtype, n_rows, C, batch, mask == nullptr || coef == nullptr || dh == nullptr,
                            (uintptr_t)dh))
        return rc;
    if ((uintptr_t)mask % 4 != 0 || (uintptr_t)coef % 4 != 0)
        return bad(who, GCN_E_ALIGN, "mask, coef: 4-byte alignment required");
    const RowSlabs sl(n_rows);
    const dim3 grid((unsigned)sl.blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(pool_broadcast_kernel<T>, grid, block, 0, s, mask, coef, (T *)dh, n_rows, (int)C,
                           sl.rows_per_block);
    });
    return launched(who);
}

size_t gcn_attn_workspace_bytes(int64_t n_rows, int64_t C, int64_t batch, int dtype)
{
    if (!rows_ok(n_rows, 1) || !lane_width_ok(C, dtype) || !batch_ok(batch)) return 0;
    // scores: one (max, sum) pair per block; backward: one partial row [C] per block
    return (size_t)batch * (size_t)RowSlabs(n_rows).blocks * (size_t)std::max<int64_t>(C, 2) * sizeof(double);
}

int gcn_attn_scores(int dtype, const void *h, const float *key, int64_t n_rows, int64_t C, int64_t batch,
                    float *scores, double *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gcn_attn_scores";
    if (int rc = check(who, kPoolRows, dtype, n_rows, C, batch,
                            h == nullptr || key == nullptr || scores == nullptr || stats == nullptr, (uintptr_t)h))
        return rc;
    if (workspace == nullptr || workspace_bytes < gcn_attn_workspace_bytes(n_rows, C, batch, dtype))
        return bad(who, GCN_E_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace % 16 != 0 || (uintptr_t)stats % 8 != 0 || (uintptr_t)key % 4 != 0 ||
        (uintptr_t)scores % 4 != 0)
        return bad(who, GCN_E_ALIGN, "16-byte alignment required (stats: 8, key, scores: 4)");
    const RowSlabs sl(n_rows);
    const dim3 grid((unsigned)sl.blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)workspace;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(attn_scores_kernel<T>, grid, block, 0, s, (const T *)h, key, scores, part, n_rows, (int)C,
                           sl.rows_per_block);
    });
    hipLaunchKernelGGL(attn_finish_kernel, dim3((unsigned)batch), block, 0, s, (const double *)part, (int)sl.blocks,
                       stats);
    return launched(who);
}

int gcn_attn_normalize(const float *scores, const double *stats, float *attn, int64_t n_rows, int64_t batch,
                       void *stream)
{
    const char *who = "gcn_attn_normalize";
    if (!rows_ok(n_rows, 1)) return bad(who, GCN_E_BADARG, "needs n_rows >= 1");
    if (!batch_ok(batch)) return bad(who, GCN_E_BADARG, "needs 1 <= batch <= 65535");
    if (scores == nullptr || stats == nullptr || attn == nullptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if ((uintptr_t)stats % 8 != 0 || (uintptr_t)scores % 4 != 0 || (uintptr_t)attn % 4 != 0)
        return bad(who, GCN_E_ALIGN, "stats: 8-byte, scores, attn: 4-byte alignment required");
    const dim3 grid((unsigned)std::min<int64_t>((n_rows + 255) / 256, 4096), (unsigned)batch);
    hipLaunchKernelGGL(attn_normalize_kernel, grid, dim3(256), 0, (hipStream_t)stream, scores, stats, attn, n_rows);
    return launched(who);
}

int gcn_attn_backward(int dtype, const void *h, const float *ds, const float *key, void *dh, double *dkey,
                      int64_t n_rows, int64_t C, int64_t batch, void *workspace, size_t workspace_bytes,
                      void *stream)
{
    const char *who = "gcn_attn_backward";
    if (int rc = check(who, kPoolRows, dtype, n_rows, C, batch,
                            h == nullptr || ds == nullptr || key == nullptr || dkey == nullptr,
                            (uintptr_t)h | (uintptr_t)dh))
        return rc;
    if (workspace == nullptr || workspace_bytes < gcn_attn_workspace_bytes(n_rows, C, batch, dtype))
        return bad(who, GCN_E_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace % 16 != 0 || (uintptr_t)dkey % 8 != 0 || (uintptr_t)key % 4 != 0 ||
        (uintptr_t)ds % 4 != 0)
        return bad(who, GCN_E_ALIGN, "16-byte alignment required (dkey: 8, key, ds: 4)");
    const RowSlabs sl(n_rows);
    const dim3 grid((unsigned)sl.blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)workspace;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(attn_backward_kernel<T>, grid, block, 0, s, (const T *)h, ds, key, (T *)dh, part, n_rows,
                           (int)C, sl.rows_per_block);
    });
    hipLaunchKernelGGL(bn_finish_kernel<1>, finish_grid(C, batch), dim3(1024), 0, s, (const double *)part,
                       (int)sl.blocks, (int)C, 1.0, 0.f, (const float *)nullptr, (float *)nullptr, (float *)nullptr,
                       (float *)nullptr, dkey);
    return launched(who);
}

}   // extern "C"
