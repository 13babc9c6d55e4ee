// gcn_head.hip — the per-vertex score head of the fork's Generator and Hierarchical_Generator as fused sweeps
// (gfx950).
//
//     score = linear3( bn(relu( linear2( bn(relu( linear1( cat(h, x[:, d : d + T]) ))) )) ))      [n_rows, 1]
//
// (reference pygcn/models.py:368-370, :391-393, the two MLPs :195-241; bn = the fork's FRESH BatchNorm1d: batch
// statistics over all rows, biased variance, eps 1e-5, gamma = 1, beta = 0 — or no bn at all, the plain MLPLayers.)
// The concatenation never exists, the hidden activations are RECOMPUTED in every sweep and never written, and
// nothing of size [n_rows, H] is kept for the backward pass.
//
// GEOMETRY (that of gcn_eval.hip).  A block of up to 4 waves owns a slab of rows, a multiple of TV = 64; wave w takes
// the tiles w, w + 4, ... of the slab.  A tile — 64 vertices of h [C] and of the tail x[:, d : d + T] — is staged
// through LDS with runs of consecutive dwords and then read A LANE PER VERTEX: vertex v, column k at
// tile[v * P + k], P = (C + T) | 1.  ds_read_b32 banks are dword address mod 32 and conflicts count within a
// 32-lane half: P odd puts 32 lanes reading column k of 32 vertices on 32 banks.  The weights live in LDS,
// transposed and zero-padded to the compile-time width HP (16 / 32 / 64, both hidden layers): W1s[k * HP + j],
// W2s[i * HP + j] — row k is read by all lanes at once (one address: a broadcast, ds_read_b128, rows 16-byte
// aligned) while lane v holds z[0 .. HP) in registers:  z[j] = fmaf(a[v][k], W1s[k][j], z[j]), k ascending.
// The chain is written ONCE (layer1 / relu_mask / normalise / layer2 / score_of below) and every sweep calls it:
// explicit fmaf in a fixed order and `fp contract(off)`, so the ReLU masks and xhat of a backward sweep are bit for
// bit those the statistics were taken over.
//
// OUTER PRODUCTS AND COLUMN SUMS.  A per-vertex vector that is needed ACROSS vertices (relu(z) for the statistics,
// dz for the weight gradients) goes to a second LDS tile, vertex v at s[v * SP + j], SP = HP + 4: the row stays
// 16-byte aligned for the broadcast reads, the lane-per-vertex store of one column has stride 36 / 20 / 68 dwords
// (4-way conflicts, HP stores per tile).  Then
//   * column sums: lane (sl, j) adds the vertices sl, sl + 64 / HP, ... of column j IN DOUBLE, over every tile of
//     its wave; (consecutive lanes, consecutive banks)
//   * grad W1 [K, H1]: lane k holds row k of the sum  sum_v a[v][k] * dz1[v][.]  in HP fp32 registers (rows 64 ..
//     95: 32 lanes x 2 half rows), a[v][k] from the staged tile (consecutive lanes, consecutive banks), dz1[v][.]
//     a broadcast row;  grad W2 [H1, H2] the same with y1 in a tile, HP * HP / 64 registers per lane.
//   fp32 per wave over its slab, the waves of a block added in wave order, one partial row per block (doubles for
//   the column sums, floats for the outer products), and vmlp_finish_kernel adds the <= 2048 partial rows in a
//   fixed order IN DOUBLE.  No float atomics: bitwise reproducible.  vmlp_epilogue_kernel (one block) turns the
//   totals into statistics, coefficients and parameter gradients.
//
// SWEEPS.  forward, bn:  1  z1 -> sum, sum^2 of relu(z1)   2  .. y1 -> z2 -> sum, sum^2 of relu(z2)   3  -> score
//          forward, no bn: 1.
//          backward, bn: 1  .. y2: sum ds, grad W3[j] = sum ds * y2[j]  (sum dy2 = W3 * sum ds, sum dy2 * xhat2 =
//                           W3 * grad W3: the BatchNorm-2 sums need nothing else)
//                        2  dz2 -> grad W2, grad b2 (the BatchNorm-1 sums  sum dy1 = W2^T grad b2  and
//                           sum dy1 * y1 [i] = sum_j W2[j][i] grad W2[j][i]  are formed from the double totals)
//                        3  dz2 -> dy1 = W2^T dz2 -> dz1 -> grad W1, grad b1, dh = (W1^T dz1)[:C]
//          backward, no bn: 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "gcn_spmm.h"
#include "gcn_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int TV = 64;                   // vertices per tile: one wave, a lane per vertex
constexpr int64_t kMaxC = 64, kMaxT = 32, kMaxH = 64, kMinRows = 64;
constexpr int kStat = 64;                // pitch of the statistics and coefficient vectors
constexpr size_t kLdsDefault = 64 * 1024;          // what a launch may ask for without opting in
constexpr size_t kLdsLimit = 159 * 1024;           // of the CU's 160 KiB, room left for the kernels' static LDS

enum Mode { kFwdAll = 0, kFwdStats1 = 1, kFwdStats2 = 2, kFwdScore = 3, kBwdAll = 10, kBwdSums = 11, kBwdMid = 12,
            kBwdLast = 13 };

struct Params {
    const float *h, *x, *W1, *b1, *W2, *b2, *W3, *b3, *stats, *coef, *ds;
    float *score, *dh;
    long long *mask1, *mask2;
    double *partD;
    float *partF;
    int64_t n, ldx;
    int C, T, d, H1, H2, rows_per_block;
};

// LDS traffic of a wave's OWN tiles: program order within the wave is enough, no workgroup barrier
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__host__ __device__ constexpr int row_doubles(int HP) { return 1 + 3 * HP; }      // sum ds; 3 column vectors
__host__ __device__ inline int row_floats(int K, int HP) { return K * HP + HP * HP; }   // grad W1^T, grad W2^T

// floats of LDS: the weights, then per wave the staged tile and `tiles` [64][HP + 4] tiles
__host__ __device__ inline int weight_floats(int K, int HP) { return K * HP + HP * HP + 11 * HP; }
__host__ __device__ inline int wave_floats(int K, int HP, int tiles) { return TV * (K | 1) + tiles * TV * (HP + 4); }

template <int HP>
struct Lds {
    static constexpr int SP = HP + 4;
    float *W1s, *W2s, *b1s, *b2s, *W3s, *st, *cf, *wave0;
    int K, P, wstride;
    float b3;
    __device__ __forceinline__ Lds(float *base, const Params &p, int tiles)
    {
        K = p.C + p.T;
        P = K | 1;
        W1s = base;
        W2s = W1s + K * HP;
        b1s = W2s + HP * HP;
        b2s = b1s + HP;
        W3s = b2s + HP;
        st = W3s + HP;
        cf = st + 4 * HP;
        wave0 = cf + 4 * HP;
        wstride = wave_floats(K, HP, tiles);
        b3 = p.b3 != nullptr ? p.b3[0] : 0.f;
    }
    // The same view behind an offset of 0 the compiler cannot see through.  Taken once per tile: the weights never
    // change, so without it their reads — HP * HP + K * HP floats — are hoisted out of the tile loop into registers
    // they do not fit.
    __device__ __forceinline__ Lds per_tile() const
    {
        int o = 0;
        asm volatile("" : "+s"(o));
        Lds t = *this;
        t.W1s += o, t.W2s += o, t.b1s += o, t.b2s += o, t.W3s += o, t.st += o, t.cf += o;
        return t;
    }
    __device__ __forceinline__ float *tile(int w) const { return wave0 + w * wstride; }
    __device__ __forceinline__ float *s0(int w) const { return tile(w) + TV * P; }
    __device__ __forceinline__ float *s1(int w) const { return s0(w) + TV * SP; }
    // nn.Linear layouts W1 [H1, K], W2 [H2, H1], W3 [1, H2] -> transposed, zero-padded to HP
    __device__ __forceinline__ void load(const Params &p) const
    {
        const int t = threadIdx.x, nt = blockDim.x;
        for (int idx = t; idx < K * HP; idx += nt) {
            const int k = idx / HP, j = idx % HP;
            W1s[idx] = j < p.H1 ? p.W1[j * K + k] : 0.f;
        }
        for (int idx = t; idx < HP * HP; idx += nt) {
            const int i = idx / HP, j = idx % HP;
            W2s[idx] = (i < p.H1 && j < p.H2) ? p.W2[j * p.H1 + i] : 0.f;
        }
        for (int j = t; j < HP; j += nt) {
            b1s[j] = (p.b1 != nullptr && j < p.H1) ? p.b1[j] : 0.f;
            b2s[j] = (p.b2 != nullptr && j < p.H2) ? p.b2[j] : 0.f;
            W3s[j] = j < p.H2 ? p.W3[j] : 0.f;
            for (int q = 0; q < 4; ++q) {
                st[q * HP + j] = p.stats != nullptr ? p.stats[q * kStat + j] : 0.f;
                cf[q * HP + j] = p.coef != nullptr ? p.coef[q * kStat + j] : 0.f;
            }
        }
    }
};

// ------------------------------------------------------------------------------------------- the staged tile
// vertices [t0, t0 + nv) of h and of the tail -> tile[v * P + k]; global reads are runs of consecutive dwords
template <int HP>
__device__ __forceinline__ void fill_tile(const Params &p, const Lds<HP> &L, float *tile, int64_t t0, int nv, int lane)
{
    const int C = p.C, T = p.T, P = L.P;
    const float rC = 1.0f / (float)C;
    const float *hs = p.h + t0 * C;
#pragma unroll 4
    for (int idx = lane; idx < nv * C; idx += 64) {
        const int v = fdiv(idx, rC);
        tile[v * P + (idx - v * C)] = hs[idx];
    }
    if (T > 0) {
        const float rT = 1.0f / (float)T;
        const float *xs = p.x + t0 * p.ldx + p.d;
#pragma unroll 4
        for (int idx = lane; idx < nv * T; idx += 64) {
            const int v = fdiv(idx, rT);
            tile[v * P + C + (idx - v * T)] = xs[(int64_t)v * p.ldx + (idx - v * T)];
        }
    }
}

// ------------------------------------------------------------------------------------ rows of W floats in LDS
// A row is read as W / 4 ds_read_b128 (16-byte aligned).  Every product below is software-pipelined by hand — row
// k + 1 is requested before the W fused multiply-adds of row k, and a scheduling barrier ends each step — because
// left alone the scheduler hoists the reads of ALL rows of an unrolled product (HP * HP floats) ahead of their
// use and spills.  One wave per SIMD (the LDS tiles set the occupancy) has nobody else to hide the LDS latency.
template <int W>
struct Row {
    float4 q[W / 4];
    __device__ __forceinline__ void load(const float *src)
    {
#pragma unroll
        for (int c = 0; c < W / 4; ++c) q[c] = *(const float4 *)(src + 4 * c);
    }
    __device__ __forceinline__ float at(int j) const
    {
        const float4 v = q[j >> 2];
        return (j & 3) == 0 ? v.x : (j & 3) == 1 ? v.y : (j & 3) == 2 ? v.z : v.w;
    }
    __device__ __forceinline__ void fma_into(float a, float (&acc)[W]) const
    {
#pragma unroll
        for (int j = 0; j < W; ++j) acc[j] = fmaf(a, at(j), acc[j]);
    }
    // four partial sums over j = 0, 4, ..; 1, 5, ..; .. added as (s0 + s1) + (s2 + s3)
    __device__ __forceinline__ float dot(const float (&v)[W]) const
    {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < W; ++j) a[j & 3] = fmaf(v[j], at(j), a[j & 3]);
        return (a[0] + a[1]) + (a[2] + a[3]);
    }
};

__device__ __forceinline__ void step_end() { __builtin_amdgcn_sched_barrier(0); }

// acc[j] = fmaf(sc[k * sstride], rows[k * rstride + j], acc[j]) for k = 0 .. n - 1 in this order, n >= 1
template <int W>
__device__ __forceinline__ void fma_rows(float (&acc)[W], const float *rows, int rstride, const float *sc, int sstride,
                                         int n)
{
    Row<W> ra, rb;
    float a = sc[0], b;
    ra.load(rows);
    int k = 0;
    for (; k + 1 < n; k += 2) {
        rb.load(rows + (k + 1) * rstride);
        b = sc[(k + 1) * sstride];
        ra.fma_into(a, acc);
        step_end();
        const int k2 = min(k + 2, n - 1);
        ra.load(rows + k2 * rstride);
        a = sc[k2 * sstride];
        rb.fma_into(b, acc);
        step_end();
    }
    if (k < n) ra.fma_into(a, acc);
    step_end();
}

// ----------------------------------------------------------------------------------------- the chain, once
template <int HP>
__device__ __forceinline__ void layer1(const Lds<HP> &L, const float *arow, float (&z)[HP])
{
#pragma unroll
    for (int j = 0; j < HP; ++j) z[j] = L.b1s[j];
    fma_rows<HP>(z, L.W1s, HP, arow, 1, L.K);
}

// z -> relu(z) in place (a NaN stays a NaN, as torch.relu), the padded columns forced to 0; bit j = z[j] > 0
template <int HP>
__device__ __forceinline__ unsigned long long relu_mask(float (&z)[HP], int H)
{
    unsigned long long m = 0;
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        const float v = z[j];
        if (j < H && v > 0.f) m |= 1ull << j;
        z[j] = j < H ? (v <= 0.f ? 0.f : v) : 0.f;
    }
    return m;
}

template <int HP>
__device__ __forceinline__ void normalise(float (&r)[HP], const float *mean, const float *rstd)
{
#pragma unroll
    for (int c = 0; c < HP / 4; ++c) {                                   // (four columns a step: two ds_read_b128)
        Row<4> m, s;
        m.load(mean + 4 * c);
        s.load(rstd + 4 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) r[4 * c + j] = (r[4 * c + j] - m.at(j)) * s.at(j);      // (padded: (0 - 0) * 0)
    }
}

template <int HP>
__device__ __forceinline__ void layer2(const Lds<HP> &L, const float (&y)[HP], float (&z)[HP])
{
#pragma unroll
    for (int j = 0; j < HP; ++j) z[j] = L.b2s[j];
    Row<HP> cur, nxt;
    cur.load(L.W2s);
#pragma unroll
    for (int i = 0; i < HP; ++i) {
        if (i + 1 < HP) nxt.load(L.W2s + (i + 1) * HP);
        cur.fma_into(y[i], z);
        step_end();
        cur = nxt;
    }
}

template <int HP>
__device__ __forceinline__ float score_of(const Lds<HP> &L, const float (&y)[HP])
{
    float s = L.b3;
#pragma unroll
    for (int j = 0; j < HP; ++j) s = fmaf(y[j], L.W3s[j], s);
    return s;
}

// the chain up to y2 (and y1), with the masks: what every backward sweep and the score sweep start with
template <int HP, bool BN>
__device__ __forceinline__ void chain(const Params &p, const Lds<HP> &L, const float *arow, float (&y1)[HP],
                                      float (&y2)[HP], unsigned long long &m1, unsigned long long &m2)
{
    layer1<HP>(L, arow, y1);
    m1 = relu_mask<HP>(y1, p.H1);
    if (BN) normalise<HP>(y1, L.st, L.st + HP);
    layer2<HP>(L, y1, y2);
    m2 = relu_mask<HP>(y2, p.H2);
    if (BN) normalise<HP>(y2, L.st + 2 * HP, L.st + 3 * HP);
}

// ----------------------------------------------------------------------------------- across the vertices
template <int HP>
__device__ __forceinline__ void store_tile(float *s, int lane, const float (&v)[HP])
{
#pragma unroll
    for (int j = 0; j < HP; ++j) s[lane * (HP + 4) + j] = v[j];
}

// lane (sl, j), j = lane % HP: the vertices sl, sl + 64 / HP, ... of column j
template <int HP>
__device__ __forceinline__ void column_sums(const float *s, int nv, int lane, double &sum, double &sumsq)
{
    constexpr int NSL = 64 / HP;
    const int j = lane & (HP - 1);
    for (int v = lane / HP; v < nv; v += NSL) {
        const double x = (double)s[v * (HP + 4) + j];
        sum += x;
        sumsq = fma(x, x, sumsq);
    }
}

// the same of ds[v] * s[v][j], ds[v] in the tile's pad slot HP
template <int HP>
__device__ __forceinline__ void column_sums_weighted(const float *s, int nv, int lane, double &sum)
{
    constexpr int NSL = 64 / HP;
    const int j = lane & (HP - 1);
    for (int v = lane / HP; v < nv; v += NSL)
        sum = fma((double)s[v * (HP + 4) + HP], (double)s[v * (HP + 4) + j], sum);
}

// the block's partial row of column vector q: the waves in wave order, the slices in slice order
template <int HP>
__device__ __forceinline__ void reduce_columns(const Params &p, double *const *dred_of_wave, int nw, int nq)
{
    constexpr int NSL = 64 / HP;
    for (int t = threadIdx.x; t < nq * HP; t += blockDim.x) {     // (a block may have fewer than 4 waves)
        const int q = t / HP, j = t % HP;
        double a = 0.0;
        for (int w = 0; w < nw; ++w)
            for (int sl = 0; sl < NSL; ++sl) a += dred_of_wave[w][q * 64 + sl * HP + j];
        p.partD[(int64_t)blockIdx.x * row_doubles(HP) + 1 + q * HP + j] = a;
    }
}

// ---------------------------------------------------------------------------------------------- forward
template <int HP, int MODE>
__global__ __launch_bounds__(256) void vmlp_fwd_kernel(Params p)
{
    extern __shared__ __align__(16) float lds[];
    constexpr bool BN = MODE != kFwdAll;
    const Lds<HP> L0(lds, p, 1);
    L0.load(p);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
    const int64_t r1 = min(r0 + (int64_t)p.rows_per_block, p.n);
    float *tile = L0.tile(wave), *s0 = L0.s0(wave);
    const float *arow = tile + lane * L0.P;
    double sum = 0.0, sumsq = 0.0;
    for (int64_t t0 = r0 + (int64_t)wave * TV; t0 < r1; t0 += (int64_t)nw * TV) {
        const int nv = (int)min((int64_t)TV, r1 - t0);
        const Lds<HP> L = L0.per_tile();
        fill_tile<HP>(p, L, tile, t0, nv, lane);
        wave_sync();
        float y1[HP];
        layer1<HP>(L, arow, y1);
        const unsigned long long m1 = relu_mask<HP>(y1, p.H1);
        if (MODE == kFwdStats1) {
            store_tile<HP>(s0, lane, y1);
            wave_sync();
            column_sums<HP>(s0, nv, lane, sum, sumsq);
            wave_sync();
            continue;
        }
        if (BN) normalise<HP>(y1, L.st, L.st + HP);
        float y2[HP];
        layer2<HP>(L, y1, y2);
        const unsigned long long m2 = relu_mask<HP>(y2, p.H2);
        if (MODE == kFwdStats2) {
            store_tile<HP>(s0, lane, y2);
            wave_sync();
            column_sums<HP>(s0, nv, lane, sum, sumsq);
            wave_sync();
            continue;
        }
        if (BN) normalise<HP>(y2, L.st + 2 * HP, L.st + 3 * HP);
        float s = score_of<HP>(L, y2);
        asm volatile("" : "+v"(s));       // (the chain stays HERE: sunk into the branch below it would leave its
                                          //  scheduling barriers behind, and every weight read with them)
        if (lane < nv) {
            p.score[t0 + lane] = s;
            if (p.mask1 != nullptr) {
                p.mask1[t0 + lane] = (long long)m1;
                p.mask2[t0 + lane] = (long long)m2;
            }
        }
        wave_sync();
    }
    if (MODE == kFwdStats1 || MODE == kFwdStats2) {
        __shared__ double *dred_of_wave[4];
        __syncthreads();
        double *dred = (double *)s0;
        dred[lane] = sum;
        dred[64 + lane] = sumsq;
        if (lane == 0) dred_of_wave[wave] = dred;
        __syncthreads();
        reduce_columns<HP>(p, dred_of_wave, nw, 2);
    }
}

// --------------------------------------------------------------------------------------------- backward
// dz2[j] = [z2[j] > 0] * (bn: rstd2[j] * (dy2[j] - mean_v dy2[j] - y2[j] * mean_v dy2[j] y2[j]), dy2[j] = ds * W3[j]),
// the two means as the coefficient vectors cf[0], cf[1] of the first backward sweep
template <int HP, bool BN>
__device__ __forceinline__ void dz2_of(const Lds<HP> &L, const float (&y2)[HP], unsigned long long m2, float ds,
                                       float (&dz)[HP])
{
#pragma unroll
    for (int c = 0; c < HP / 4; ++c) {
        Row<4> w3, rs, c1, c2;
        w3.load(L.W3s + 4 * c);
        if (BN) rs.load(L.st + 3 * HP + 4 * c), c1.load(L.cf + 4 * c), c2.load(L.cf + HP + 4 * c);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = 4 * c + jj;
            float g = ds * w3.at(jj);
            if (BN) g = rs.at(jj) * ((g - c1.at(jj)) - y2[j] * c2.at(jj));
            dz[j] = ((m2 >> j) & 1ull) ? g : 0.f;
        }
    }
}

// dz1[i] = [z1[i] > 0] * (bn: rstd1[i] * (dy1[i] - cf[2][i] - y1[i] * cf[3][i])), dy1 = W2^T dz2 (Row::dot), straight
// to the lane's row of the tile the outer product reads (four columns a store) — not held in registers
template <int HP, bool BN>
__device__ __forceinline__ void dz1_of(const Lds<HP> &L, const float (&y1)[HP], unsigned long long m1,
                                       const float (&dz2)[HP], float *srow)
{
    float4 out;
    Row<HP> cur, nxt;
    cur.load(L.W2s);
#pragma unroll
    for (int i = 0; i < HP; ++i) {
        if (i + 1 < HP) nxt.load(L.W2s + (i + 1) * HP);
        float g = cur.dot(dz2);
        step_end();
        cur = nxt;
        if (BN) g = L.st[HP + i] * ((g - L.cf[2 * HP + i]) - y1[i] * L.cf[3 * HP + i]);
        g = ((m1 >> i) & 1ull) ? g : 0.f;
        if ((i & 3) == 0) out.x = g;
        if ((i & 3) == 1) out.y = g;
        if ((i & 3) == 2) out.z = g;
        if ((i & 3) == 3) out.w = g, *(float4 *)(srow + (i & ~3)) = out;
    }
}

template <int HP, int MODE>
__global__ __launch_bounds__(256) void vmlp_bwd_kernel(Params p)
{
    extern __shared__ __align__(16) float lds[];
    constexpr bool BN = MODE != kBwdAll;
    constexpr int SP = HP + 4, NSL = 64 / HP, J2 = HP / NSL;       // J2 = HP * HP / 64 columns of grad W2 per lane
    constexpr bool kW3 = MODE == kBwdAll || MODE == kBwdSums, kW2 = MODE == kBwdAll || MODE == kBwdMid,
                   kW1 = MODE == kBwdAll || MODE == kBwdLast;
    const Lds<HP> L0(lds, p, 2);
    L0.load(p);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
    const int64_t r1 = min(r0 + (int64_t)p.rows_per_block, p.n);
    const int K = L0.K, P = L0.P, C = p.C;
    float *tile = L0.tile(wave), *s0 = L0.s0(wave), *s1 = L0.s1(wave);
    float *arow = tile + lane * P;
    // grad W1: lane k < 64 holds row k; rows 64 .. 95: lane (half, k - 64) holds HP / 2 columns
    const int ka = min(lane, K - 1), kb = min(64 + (lane & 31), K - 1), jb = (lane >> 5) * (HP / 2);
    const int i2 = lane & (HP - 1), j2 = (lane / HP) * J2;          // grad W2: row i2, columns j2 ..
    float g1a[HP], g1b[HP / 2], g2[J2];                          // (dead, and gone, in the sweeps that do not use them)
#pragma unroll
    for (int j = 0; j < HP; ++j) g1a[j] = 0.f;
#pragma unroll
    for (int j = 0; j < HP / 2; ++j) g1b[j] = 0.f;
#pragma unroll
    for (int j = 0; j < J2; ++j) g2[j] = 0.f;
    double sum_ds = 0.0, cW3 = 0.0, cb2 = 0.0, cb1 = 0.0, unused = 0.0;
    for (int64_t t0 = r0 + (int64_t)wave * TV; t0 < r1; t0 += (int64_t)nw * TV) {
        const int nv = (int)min((int64_t)TV, r1 - t0);
        const Lds<HP> L = L0.per_tile();
        fill_tile<HP>(p, L, tile, t0, nv, lane);
        wave_sync();
        const float ds = lane < nv ? p.ds[t0 + lane] : 0.f;
        float y1[HP], y2[HP], dz2[HP];
        unsigned long long m1, m2;
        chain<HP, BN>(p, L, arow, y1, y2, m1, m2);
        if (kW3) {                                              // sum ds, grad W3[j] = sum ds * y2[j]
            sum_ds += (double)ds;
            store_tile<HP>(s1, lane, y2);
            s1[lane * SP + HP] = ds;
            wave_sync();
            column_sums_weighted<HP>(s1, nv, lane, cW3);
            wave_sync();
        }
        if (MODE == kBwdSums) continue;
        dz2_of<HP, BN>(L, y2, m2, ds, dz2);
        if (kW2) {                                              // grad W2^T[i][j] += y1[v][i] * dz2[v][j], grad b2
            store_tile<HP>(s0, lane, y1);
            store_tile<HP>(s1, lane, dz2);
            wave_sync();
            fma_rows<J2>(g2, s1 + j2, SP, s0 + i2, SP, nv);
            column_sums<HP>(s1, nv, lane, cb2, unused);
            wave_sync();
        }
        if (kW1) {
            dz1_of<HP, BN>(L, y1, m1, dz2, s1 + lane * SP);
            wave_sync();
            fma_rows<HP>(g1a, s1, SP, tile + ka, P, nv);        // grad W1^T[k][j] += a[v][k] * dz1[v][j]
            if (K > 64) fma_rows<HP / 2>(g1b, s1 + jb, SP, tile + kb, P, nv);
            column_sums<HP>(s1, nv, lane, cb1, unused);
            wave_sync();                                        // (the tile's rows were read across lanes)
            if (p.dh != nullptr) {                              // dh[v][k] = sum_j W1[j][k] dz1[j], into the tile
                float dz1[HP];
                Row<HP> ra, rb;
                ra.load(s1 + lane * SP);
#pragma unroll
                for (int j = 0; j < HP; ++j) dz1[j] = ra.at(j);
                ra.load(L.W1s);
                int k = 0;
                for (; k + 1 < C; k += 2) {
                    rb.load(L.W1s + (k + 1) * HP);
                    arow[k] = ra.dot(dz1);
                    step_end();
                    ra.load(L.W1s + min(k + 2, C - 1) * HP);
                    arow[k + 1] = rb.dot(dz1);
                    step_end();
                }
                if (k < C) arow[k] = ra.dot(dz1);
                wave_sync();
                const float rC = 1.0f / (float)C;
                float *dhs = p.dh + t0 * C;
#pragma unroll 4
                for (int idx = lane; idx < nv * C; idx += 64) {
                    const int v = fdiv(idx, rC);
                    dhs[idx] = tile[v * P + (idx - v * C)];
                }
            }
        }
        wave_sync();
    }
    // the block's partial row: each wave's registers to its own tiles, then the waves in wave order
    __shared__ double *dred_of_wave[4];
    __syncthreads();
    if (kW1) {
        if (lane < K) {
#pragma unroll
            for (int j = 0; j < HP; ++j) tile[lane * HP + j] = g1a[j];
        }
        if (64 + (lane & 31) < K) {
#pragma unroll
            for (int j = 0; j < HP / 2; ++j) tile[(64 + (lane & 31)) * HP + jb + j] = g1b[j];
        }
    }
    if (kW2) {
#pragma unroll
        for (int j = 0; j < J2; ++j) s0[i2 * HP + j2 + j] = g2[j];
    }
    double *dred = (double *)s1;
    dred[lane] = cW3;
    dred[64 + lane] = cb2;
    dred[128 + lane] = cb1;
    dred[192 + lane] = sum_ds;
    if (lane == 0) dred_of_wave[wave] = dred;
    __syncthreads();
    const int t = threadIdx.x, nt = blockDim.x;
    float *rowF = p.partF + (int64_t)blockIdx.x * row_floats(K, HP);
    if (kW1) {
        for (int idx = t; idx < K * HP; idx += nt) {
            float a = L0.tile(0)[idx];
            for (int w = 1; w < nw; ++w) a += L0.tile(w)[idx];
            rowF[idx] = a;
        }
    }
    if (kW2) {
        for (int idx = t; idx < HP * HP; idx += nt) {
            float a = L0.s0(0)[idx];
            for (int w = 1; w < nw; ++w) a += L0.s0(w)[idx];
            rowF[K * HP + idx] = a;
        }
    }
    reduce_columns<HP>(p, dred_of_wave, nw, 3);
    if (kW3 && t == 0) {
        double a = 0.0;
        for (int w = 0; w < nw; ++w)
            for (int l = 0; l < 64; ++l) a += dred_of_wave[w][192 + l];
        p.partD[(int64_t)blockIdx.x * row_doubles(HP)] = a;
    }
}

// ------------------------------------------------------------------------------------- the partial rows
// tot[c] = sum over the blocks' partial rows, in double: the columns [d0, d0 + nd) of partD [n_blocks][rowD] and
// the columns [f0, f0 + nf) of partF [n_blocks][rowF] (-> tot[rowD + f0 ..]).  The scheme of eval_finish_kernel: a
// block owns 32 columns, thread (g, c) adds the rows g, g + 8, ..., the 8 group sums are added in group order.
__global__ __launch_bounds__(256) void vmlp_finish_kernel(const double *__restrict__ partD,
                                                          const float *__restrict__ partF, int n_blocks, int rowD,
                                                          int rowF, int d0, int nd, int f0, int nf,
                                                          double *__restrict__ tot)
{
    __shared__ double rs[8][33];
    const int c = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int col = (int)blockIdx.x * 32 + c;
    double a = 0.0;
    if (col < nd) {
        for (int k = grp; k < n_blocks; k += 8) a += partD[(int64_t)k * rowD + d0 + col];
    } else if (col < nd + nf) {
        for (int k = grp; k < n_blocks; k += 8) a += (double)partF[(int64_t)k * rowF + f0 + (col - nd)];
    }
    rs[grp][c] = a;
    __syncthreads();
    if (grp == 0 && col < nd + nf) {
        for (int k = 1; k < 8; ++k) a += rs[k][c];
        tot[col < nd ? d0 + col : rowD + f0 + (col - nd)] = a;
    }
}

struct Epilogue {
    const double *tot;
    const float *W2, *W3;
    float *stats, *coef, *gW1, *gb1, *gW2, *gb2, *gW3, *gb3;
    int64_t n;
    int mode, HP, K, H1, H2;
};

// one block: the totals -> statistics (forward), coefficient vectors and parameter gradients (backward)
__global__ __launch_bounds__(256) void vmlp_epilogue_kernel(Epilogue e)
{
    const int t = threadIdx.x, HP = e.HP, K = e.K, H1 = e.H1, H2 = e.H2;
    const double inv_n = 1.0 / (double)e.n;
    const double *D = e.tot + 1, *F1 = e.tot + row_doubles(HP), *F2 = F1 + K * HP;
    if (e.mode == kFwdStats1 || e.mode == kFwdStats2) {         // mean and 1 / sqrt(biased var + eps) of relu(z)
        const int l = e.mode - kFwdStats1, H = l == 0 ? H1 : H2;
        if (t < kStat) {
            float mean = 0.f, rstd = 0.f;
            if (t < H) {
                const double m = D[t] * inv_n;
                const double var = fmax(D[HP + t] * inv_n - m * m, 0.0);
                mean = (float)m;
                rstd = (float)(1.0 / sqrt(var + 1e-5));
            }
            e.stats[(2 * l) * kStat + t] = mean;
            e.stats[(2 * l + 1) * kStat + t] = rstd;
        }
        return;
    }
    if (e.mode == kBwdAll || e.mode == kBwdSums) {
        if (t < H2 && e.gW3 != nullptr) e.gW3[t] = (float)D[t];
        if (t == 0 && e.gb3 != nullptr) e.gb3[0] = (float)e.tot[0];
        if (e.mode == kBwdSums && t < kStat) {
            const double w = t < H2 ? (double)e.W3[t] : 0.0;
            e.coef[t] = t < H2 ? (float)(w * e.tot[0] * inv_n) : 0.f;
            e.coef[kStat + t] = t < H2 ? (float)(w * D[t] * inv_n) : 0.f;
        }
    }
    if (e.mode == kBwdAll || e.mode == kBwdMid) {
        if (e.gW2 != nullptr)
            for (int idx = t; idx < H2 * H1; idx += 256) e.gW2[idx] = (float)F2[(idx % H1) * HP + idx / H1];
        if (t < H2 && e.gb2 != nullptr) e.gb2[t] = (float)D[HP + t];
        if (e.mode == kBwdMid && t < kStat) {                   // sum_v dy1[i] and sum_v dy1[i] * y1[i], over n
            double a = 0.0, b = 0.0;
            if (t < H1) {
                for (int j = 0; j < H2; ++j) {
                    const double w = (double)e.W2[j * H1 + t];
                    a = fma(w, D[HP + j], a);
                    b = fma(w, F2[t * HP + j], b);
                }
            }
            e.coef[2 * kStat + t] = (float)(a * inv_n);
            e.coef[3 * kStat + t] = (float)(b * inv_n);
        }
    }
    if (e.mode == kBwdAll || e.mode == kBwdLast) {
        if (e.gW1 != nullptr)
            for (int idx = t; idx < H1 * K; idx += 256) e.gW1[idx] = (float)F1[(idx % K) * HP + idx / K];
        if (t < H1 && e.gb1 != nullptr) e.gb1[t] = (float)D[2 * HP + t];
    }
}

// ------------------------------------------------------------------------------------------------- host
int pad_width(int64_t H1, int64_t H2)
{
    const int64_t H = std::max(H1, H2);
    return H <= 16 ? 16 : H <= 32 ? 32 : 64;
}

bool shape_ok(int64_t n_rows, int64_t C, int64_t T, int64_t H1, int64_t H2)
{
    return n_rows >= kMinRows && n_rows <= (int64_t)INT32_MAX * 32 && C >= 1 && C <= kMaxC && T >= 0 && T <= kMaxT &&
           H1 >= 1 && H1 <= kMaxH && H2 >= 1 && H2 <= kMaxH;
}

struct Shape {
    int HP, K, rowD, rowF, rows_per_block;
    int64_t blocks;
    size_t offF, offTot, offCoef, bytes;
    Shape(int64_t n_rows, int64_t C, int64_t T, int64_t H1, int64_t H2)
    {
        HP = pad_width(H1, H2);
        K = (int)(C + T);
        rowD = row_doubles(HP);
        rowF = row_floats(K, HP);
        // the workspace holds B = min(tiles, 2048) partial rows; the launch uses the blocks that have rows
        const TileSlabs sl(n_rows, TV);
        const int64_t B = sl.slabs;
        rows_per_block = sl.rows_per_block;
        blocks = (n_rows + rows_per_block - 1) / rows_per_block;
        auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
        offF = up((size_t)B * rowD * sizeof(double));
        offTot = offF + up((size_t)B * rowF * sizeof(float));
        offCoef = offTot + up((size_t)(rowD + rowF) * sizeof(double));
        bytes = offCoef + 4 * kStat * sizeof(float);
    }
    // waves per block: as many of 4 as fit `cap` bytes of LDS
    int waves(int tiles, size_t cap, size_t *lds_bytes) const
    {
        for (int nw = 4;; nw >>= 1) {
            *lds_bytes = ((size_t)weight_floats(K, HP) + (size_t)nw * wave_floats(K, HP, tiles)) * sizeof(float);
            if (*lds_bytes <= cap || nw == 1) return nw;
        }
    }
};

bool off(const void *ptr, uintptr_t a) { return (uintptr_t)ptr % a != 0; }

template <int HP, int MODE>
hipError_t launch_sweep(const Shape &sh, const Params &p, hipStream_t s)
{
    constexpr bool fwd = MODE < kBwdAll;
    size_t lds_bytes = 0;
    int nw = sh.waves(fwd ? 1 : 2, kLdsLimit, &lds_bytes);
    void (*kernel)(Params);
    if constexpr (fwd) kernel = vmlp_fwd_kernel<HP, MODE>;
    else kernel = vmlp_bwd_kernel<HP, MODE>;
    // more than 64 KiB of dynamic LDS is an opt-in of the CURRENT device: asked for at every such launch (a host
    // call, no state kept here); a runtime that refuses it gets blocks of fewer waves
    if (lds_bytes > kLdsDefault &&
        hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit) !=
            hipSuccess) {
        (void)hipGetLastError();
        nw = sh.waves(fwd ? 1 : 2, kLdsDefault, &lds_bytes);
        if (lds_bytes > kLdsDefault) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)sh.blocks), dim3(64 * nw), lds_bytes, s, p);
    return hipSuccess;
}

template <int MODE>
hipError_t launch_sweep(const Shape &sh, const Params &p, hipStream_t s)
{
    return sh.HP == 16   ? launch_sweep<16, MODE>(sh, p, s)
           : sh.HP == 32 ? launch_sweep<32, MODE>(sh, p, s)
                         : launch_sweep<64, MODE>(sh, p, s);
}

// the partial rows of a sweep -> totals -> the epilogue of `mode`
void finish(const Shape &sh, const Params &p, Epilogue e, int d0, int nd, int f0, int nf, hipStream_t s)
{
    double *tot = (double *)e.tot;
    hipLaunchKernelGGL(vmlp_finish_kernel, dim3((unsigned)((nd + nf + 31) / 32)), dim3(256), 0, s,
                       (const double *)p.partD, (const float *)p.partF, (int)sh.blocks, sh.rowD, sh.rowF, d0, nd,
                       f0, nf, tot);
    hipLaunchKernelGGL(vmlp_epilogue_kernel, dim3(1), dim3(256), 0, s, e);
}

int check_args(const char *who, const float *h, const float *x, int64_t ldx, int64_t d, int64_t n_rows, int64_t C,
               int64_t T, const float *W1, int64_t H1, const float *W2, int64_t H2, const float *W3,
               const void *workspace, size_t workspace_bytes)
{
    if (n_rows < 0 || C < 0 || T < 0 || H1 < 0 || H2 < 0 || d < 0)
        return bad(who, GCN_E_BADARG, "negative size");
    if (!shape_ok(n_rows, C, T, H1, H2))
        return bad(who, GCN_E_BADARG, "needs n_rows >= 64, 1 <= C <= 64, 0 <= T <= 32 and 1 <= H1, H2 <= 64");
    if (h == nullptr || W1 == nullptr || W2 == nullptr || W3 == nullptr || (T > 0 && x == nullptr))
        return bad(who, GCN_E_BADARG, "NULL pointer");
    if (T > 0 && ldx < d + T) return bad(who, GCN_E_BADARG, "ldx < d + T: the tail does not fit a row of x");
    if (workspace == nullptr || workspace_bytes < Shape(n_rows, C, T, H1, H2).bytes)
        return bad(who, GCN_E_WORKSPACE, "workspace too small");
    if (off(workspace, 16)) return bad(who, GCN_E_ALIGN, "16-byte alignment required");
    return 0;
}

}  // namespace

size_t gcn_vmlp_workspace_bytes(int64_t n_rows, int64_t C, int64_t T, int64_t H1, int64_t H2)
{
    if (!shape_ok(n_rows, C, T, H1, H2)) return 0;
    return Shape(n_rows, C, T, H1, H2).bytes;
}

int gcn_vmlp_forward(const float *h, const float *x, int64_t ldx, int64_t d, int64_t n_rows, int64_t C, int64_t T,
                     const float *W1, const float *b1, int64_t H1, const float *W2, const float *b2, int64_t H2,
                     const float *W3, const float *b3, int batch_norm, float *stats, float *scores, int64_t *mask1,
                     int64_t *mask2, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gcn_vmlp_forward";
    if (const int rc = check_args(who, h, x, ldx, d, n_rows, C, T, W1, H1, W2, H2, W3, workspace, workspace_bytes))
        return rc;
    if (scores == nullptr || (batch_norm && stats == nullptr)) return bad(who, GCN_E_BADARG, "NULL pointer");
    if ((mask1 == nullptr) != (mask2 == nullptr)) return bad(who, GCN_E_BADARG, "both masks or neither");
    if (off(h, 4) || off(x, 4) || off(scores, 4) || off(stats, 4) || off(mask1, 8) || off(mask2, 8))
        return bad(who, GCN_E_ALIGN, "4-byte alignment required (masks: 8)");
    const Shape sh(n_rows, C, T, H1, H2);
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    Params p = {};
    p.h = h, p.x = x, p.W1 = W1, p.b1 = b1, p.W2 = W2, p.b2 = b2, p.W3 = W3, p.b3 = b3;
    p.score = scores, p.mask1 = (long long *)mask1, p.mask2 = (long long *)mask2;
    p.partD = (double *)ws, p.partF = (float *)(ws + sh.offF);
    p.n = n_rows, p.ldx = ldx, p.C = (int)C, p.T = (int)T, p.d = (int)d, p.H1 = (int)H1, p.H2 = (int)H2;
    p.rows_per_block = sh.rows_per_block;
    hipError_t e = hipSuccess;
    if (!batch_norm) {
        e = launch_sweep<kFwdAll>(sh, p, s);
        return launched(who, e);
    }
    Epilogue ep = {};
    ep.tot = (const double *)(ws + sh.offTot), ep.stats = stats, ep.n = n_rows;
    ep.HP = sh.HP, ep.K = sh.K, ep.H1 = (int)H1, ep.H2 = (int)H2;
    p.stats = stats;
    e = launch_sweep<kFwdStats1>(sh, p, s);
    if (e != hipSuccess) return launched(who, e);
    ep.mode = kFwdStats1;
    finish(sh, p, ep, 1, 2 * sh.HP, 0, 0, s);
    e = launch_sweep<kFwdStats2>(sh, p, s);
    if (e != hipSuccess) return launched(who, e);
    ep.mode = kFwdStats2;
    finish(sh, p, ep, 1, 2 * sh.HP, 0, 0, s);
    e = launch_sweep<kFwdScore>(sh, p, s);
    return launched(who, e);
}

int gcn_vmlp_backward(const float *h, const float *x, int64_t ldx, int64_t d, int64_t n_rows, int64_t C, int64_t T,
                      const float *W1, const float *b1, int64_t H1, const float *W2, const float *b2, int64_t H2,
                      const float *W3, const float *b3, int batch_norm, const float *stats, const float *dscores,
                      float *dh, float *gW1, float *gb1, float *gW2, float *gb2, float *gW3, float *gb3,
                      void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gcn_vmlp_backward";
    if (const int rc = check_args(who, h, x, ldx, d, n_rows, C, T, W1, H1, W2, H2, W3, workspace, workspace_bytes))
        return rc;
    if (dscores == nullptr || (batch_norm && stats == nullptr))
        return bad(who, GCN_E_BADARG, "NULL pointer");
    if (off(h, 4) || off(x, 4) || off(dscores, 4) || off(stats, 4) || off(dh, 4))
        return bad(who, GCN_E_ALIGN, "4-byte alignment required");
    const Shape sh(n_rows, C, T, H1, H2);
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    Params p = {};
    p.h = h, p.x = x, p.W1 = W1, p.b1 = b1, p.W2 = W2, p.b2 = b2, p.W3 = W3, p.b3 = b3, p.ds = dscores, p.dh = dh;
    p.partD = (double *)ws, p.partF = (float *)(ws + sh.offF);
    p.n = n_rows, p.ldx = ldx, p.C = (int)C, p.T = (int)T, p.d = (int)d, p.H1 = (int)H1, p.H2 = (int)H2;
    p.rows_per_block = sh.rows_per_block;
    Epilogue ep = {};
    ep.tot = (const double *)(ws + sh.offTot), ep.W2 = W2, ep.W3 = W3, ep.coef = (float *)(ws + sh.offCoef);
    ep.gW1 = gW1, ep.gb1 = gb1, ep.gW2 = gW2, ep.gb2 = gb2, ep.gW3 = gW3, ep.gb3 = gb3, ep.n = n_rows;
    ep.HP = sh.HP, ep.K = sh.K, ep.H1 = (int)H1, ep.H2 = (int)H2;
    const int HP = sh.HP, K = sh.K;
    hipError_t e = hipSuccess;
    if (!batch_norm) {
        e = launch_sweep<kBwdAll>(sh, p, s);
        if (e != hipSuccess) return launched(who, e);
        ep.mode = kBwdAll;
        finish(sh, p, ep, 0, sh.rowD, 0, sh.rowF, s);
        return launched(who, e);
    }
    p.stats = stats;
    e = launch_sweep<kBwdSums>(sh, p, s);
    if (e != hipSuccess) return launched(who, e);
    ep.mode = kBwdSums;
    finish(sh, p, ep, 0, 1 + HP, 0, 0, s);
    p.coef = ep.coef;
    e = launch_sweep<kBwdMid>(sh, p, s);
    if (e != hipSuccess) return launched(who, e);
    ep.mode = kBwdMid;
    finish(sh, p, ep, 1 + HP, HP, K * HP, HP * HP, s);
    e = launch_sweep<kBwdLast>(sh, p, s);
    if (e != hipSuccess) return launched(who, e);
    ep.mode = kBwdLast;
    finish(sh, p, ep, 1 + 2 * HP, HP, 0, K * HP, s);
    return launched(who, e);
}
