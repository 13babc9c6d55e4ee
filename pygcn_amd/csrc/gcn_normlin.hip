// gcn_normlin.hip — BN(relu(z)) · W for 32-wide layers as ONE node that never forms the normalised
// activation (gfx950).
//
// The fork's live model (reference pygcn/models.py:49-56) feeds apply_bn(F.relu(gc(x, adj))) straight into the
// next layer's X·W.  As separate nodes that is y = BN(relu(z)) written by one sweep only so that a GEMM can read
// it back, and y kept for the backward pass beside z.  Here, for k samples side by side (z [n_rows, k * 32], the
// layout of gcn_bn_*_batched), with x = relu ? relu(z) : z and xhat = (x - mean) * rstd per column of a window:
//     forward    gcn_bn_stats_batched (gcn_norm.hip, unchanged)  reads z          -> mean, rstd        1 stream
//                nl_forward_kernel      reads z, writes s = xhat · W                                   2 streams
//     backward   nl_bwd_sums_kernel     reads dS, z  -> grad_W = sum over windows and rows of xhat^T · dS,
//                                                       and the double coef [4][k * 32] of BatchNorm's backward
//                                                                                                      2 streams
//                nl_bwd_apply_kernel    reads dS, z, writes dz                                         3 streams
//     dy = dS · W^T (registers only),  dz = [z > 0] * rstd * (dy - sum dy / n - xhat * sum (dy xhat) / n)
//
// MFMA MAPPING.  The products are v_mfma_f32_32x32x2_f32: f32 in, f32 accumulate, bitwise an fmaf chain over the
// contraction index in issue order.  A wave owns a slab of rows of ONE window and walks it in tiles of 32 rows,
// so the window's per-column constants are registers and no sum mixes samples.  With h = lane >> 5, c = lane & 31:
//   A layout  lane holds the 64 contiguous bytes  m[row c][16 h .. 16 h + 16)  of a tile (4 x 16-byte loads);
//             MFMA step s takes A = m[row c][16 h + s], so the contraction index runs 0, 16, 1, 17, ... — a
//             permutation both operands share.
//   C layout  register g of a lane is  m[row (g & 3) + 8 (g >> 2) + 4 h][column c]: what the 32x32 MFMA returns,
//             and two full 128-byte row segments per load / store instruction when memory is accessed that way.
//   forward   A = xhat (z in the A layout), B = W[16 h + s][c]  -> s in the C layout, stored as it lies.
//   dy        A = dS (A layout), B = W[c][16 h + s]             -> dy in the C layout; z is loaded in the C layout
//             too, so dy, xhat and dz meet element by element without a cross-lane move.
//   grad_W    P[i][j] += sum over two rows of xhat[r][i] dS[r][j]: step g takes A = xhat and B = dS, both in the
//             C layout (rows (g & 3) + 8 (g >> 2) and that + 4 are the step's two contraction indices); 16 steps
//             cover the tile.  dS is therefore read in both layouts; the second read is the wave's own tile again.
// No LDS on the streaming path.
//
// xhat is formed as bn_apply_kernel forms it, (x - mean) * rstd in fp32 with contraction off, from the fp32 mean
// and rstd of gcn_bn_stats_batched: with W a signed permutation of powers of two, s is bitwise the permuted,
// scaled columns of gcn_bn_apply_batched's result.
//
// BACKWARD IN DOUBLE, as gcn_norm.hip argues: dz is what is left of dy after its components along 1 and xhat are
// taken out, and over few rows that projection cancels.  The two sums are therefore sums of the SAME fp32 dy
// values the apply sweep forms again (the same MFMA chain, bit for bit), accumulated in double next to sum t and
// sum t^2 (t = x - mean32), so that dy's own rounding is projected out with it.  (The identities
// sum_r dy[r][i] = sum_j W[i][j] colsum(dS)[j] and sum_r dy[r][i] xhat[r][i] = sum_j W[i][j] P[i][j] give the sums
// of the EXACT dy instead: the difference to the rounded dy of the apply sweep is not projected, and at n = 2 it
// comes out multiplied by 1 / (eps * rstd^2).  tests/test_normlin_cpu.py states the identities; the kernels do
// not use them.)
//
// ACCUMULATION.  grad_W: fp32 in the MFMA accumulator over one wave's slab (32 * T rows), the 4 waves of a block
// added in wave order in double, one partial row [1024 + 4 * 32] doubles per (window, block); nl_finish_blocks
// adds the partial rows of a window in a fixed order in double, nl_finish adds the windows in window order and
// rounds once.  No float atomics; bitwise reproducible; the geometry does not depend on k, so a window's s, coef
// and dz are bitwise those of the k = 1 call on a contiguous copy of the window.
//
// GEOMETRY.  T = ceil(n_rows / (128 * 512)) tiles per wave, R = 128 * T rows per block, B = ceil(n_rows / R)
// blocks (<= 512) on gridDim.x, the k windows on gridDim.y; wave w of block b owns the rows
// [b R + 32 T w, b R + 32 T (w + 1)) below n_rows.
//
// NaN / inf follow gcn_norm.hip: relu keeps NaN, the backward mask is z <= 0 ? 0 : dx, and a non-finite column
// touches its own window only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

constexpr int kF = 32;                    // the one width built
constexpr int kWaves = 4;                 // per block
constexpr int kThreads = 64 * kWaves;
constexpr int64_t kMaxBlocks = 512;
constexpr int kRow = kF * kF + 4 * kF;    // doubles per partial row: P[32][32], sum dy, sum dy t, sum t, sum t^2

// (x - mean) * rstd, rounded after the subtraction and after the product (bn_apply_kernel's expression)
__device__ __forceinline__ float normalised(float x, float mu, float rs)
{
#pragma clang fp contract(off)
    const float t = x - mu;
    return t * rs;
}

// the row of a tile that accumulator register g of a lane in half h holds
__device__ __forceinline__ int c_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

struct Slab {                             // the rows of this wave, and where its window lies
    int lane, wave, h, c;
    int64_t r0, r1, ld;
    int w0;
    __device__ __forceinline__ Slab(int64_t n_rows, int tiles)
    {
        lane = threadIdx.x & 63; wave = threadIdx.x >> 6; h = lane >> 5; c = lane & 31;
        r0 = ((int64_t)blockIdx.x * kWaves + wave) * 32 * tiles;
        r1 = min(r0 + (int64_t)32 * tiles, n_rows);
        ld = (int64_t)gridDim.y * kF;
        w0 = (int)blockIdx.y * kF;
    }
    // the lane's 64 bytes of the tile at row0 in the A layout.  A row below the slab's end reads the slab's last
    // row instead (always inside the matrix, no branch around the loads): rows of an MFMA result are independent
    // of each other, and what such a row yields is never stored or summed.
    __device__ __forceinline__ void load_a(const float *__restrict__ m, int64_t row0, float (&a)[16]) const
    {
        const f32x4 *q = (const f32x4 *)(m + clamp(row0 + c) * ld + w0 + 16 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 v = q[i];
            a[4 * i] = v.x; a[4 * i + 1] = v.y; a[4 * i + 2] = v.z; a[4 * i + 3] = v.w;
        }
    }
    // the same with zeros below the slab's end (the forward sweep: one branch per tile, four loads behind it)
    __device__ __forceinline__ void load_a_or_zero(const float *__restrict__ m, int64_t row0, float (&a)[16]) const
    {
        const int64_t r = row0 + c;
        f32x4 q[4];
        if (r < r1) {
            const f32x4 *p = (const f32x4 *)(m + r * ld + w0 + 16 * h);
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = p[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[4 * i] = q[i].x; a[4 * i + 1] = q[i].y; a[4 * i + 2] = q[i].z; a[4 * i + 3] = q[i].w;
        }
    }
    __device__ __forceinline__ int64_t clamp(int64_t r) const { return r < r1 ? r : r1 - 1; }
    // element (row, column c of the window) of a matrix in the C layout, the row clamped as above
    __device__ __forceinline__ int64_t at(int64_t r) const { return clamp(r) * ld + w0 + c; }
};

__device__ __forceinline__ f32x16 zero16()
{
    f32x16 v;
#pragma unroll
    for (int g = 0; g < 16; ++g) v[g] = 0.f;
    return v;
}

// dy = dS · W^T of a tile, in the C layout; a = the tile of dS in the A layout, wT[s] = W[c][16 h + s]
__device__ __forceinline__ f32x16 tile_dy(const float (&a)[16], const float (&wT)[16])
{
    f32x16 dy = zero16();
#pragma unroll
    for (int s = 0; s < 16; ++s) dy = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], wT[s], dy, 0, 0, 0);
    return dy;
}

// s = xhat · W
__global__ __launch_bounds__(kThreads) void nl_forward_kernel(const float *__restrict__ z,
                                                              const float *__restrict__ W,
                                                              const float *__restrict__ mean,
                                                              const float *__restrict__ rstd, float *__restrict__ out,
                                                              int64_t n_rows, int tiles, int relu)
{
    const Slab p(n_rows, tiles);
    float wB[16], mu[16], rs[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        wB[s] = W[(16 * p.h + s) * kF + p.c];
        mu[s] = mean[p.w0 + 16 * p.h + s];
        rs[s] = rstd[p.w0 + 16 * p.h + s];
    }
    for (int64_t row0 = p.r0; row0 < p.r1; row0 += 32) {
        float a[16];
        p.load_a_or_zero(z, row0, a);
        f32x16 acc = zero16();
#pragma unroll
        for (int s = 0; s < 16; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(normalised(act(a[s], relu), mu[s], rs[s]), wB[s], acc, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int64_t r = row0 + c_row(g, p.h);
            if (r < p.r1) out[r * p.ld + p.w0 + p.c] = acc[g];
        }
    }
}

// partial[window][block][kRow]: P = xhat^T · dS, and per column of z the sums of dy, dy t, t, t^2 (t = x - mean32)
__global__ __launch_bounds__(kThreads) void nl_bwd_sums_kernel(const float *__restrict__ ds,
                                                               const float *__restrict__ z,
                                                               const float *__restrict__ W,
                                                               const float *__restrict__ mean,
                                                               const float *__restrict__ rstd,
                                                               double *__restrict__ partial, int64_t n_rows, int tiles,
                                                               int relu)
{
    __shared__ float pw[kWaves][kF * kF];
    __shared__ double sw[kWaves][4][kF];
    const Slab p(n_rows, tiles);
    float wT[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) wT[s] = W[p.c * kF + 16 * p.h + s];
    const float mu = mean[p.w0 + p.c], rs = rstd[p.w0 + p.c];
    const double mud = (double)mu;
    f32x16 P = zero16();
    double a_dy = 0.0, a_dyt = 0.0, a_t = 0.0, a_tt = 0.0;
    for (int64_t row0 = p.r0; row0 < p.r1; row0 += 32) {
        float a[16], zc[16], gc[16];
        p.load_a(ds, row0, a);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int64_t off = p.at(row0 + c_row(g, p.h));
            zc[g] = z[off];
            gc[g] = ds[off];
        }
        // every load of the tile is in flight before its first use: one memory latency per tile, not one per
        // group of loads the scheduler would otherwise sink next to their uses
        __builtin_amdgcn_sched_barrier(0);
        const f32x16 dy = tile_dy(a, wT);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const bool live = row0 + c_row(g, p.h) < p.r1;
            const float x = act(zc[g], relu);
            const float gg = live ? gc[g] : 0.f;            // (a row below the end adds xhat * 0)
            P = __builtin_amdgcn_mfma_f32_32x32x2f32(normalised(x, mu, rs), gg, P, 0, 0, 0);
            const double t = live ? (double)x - mud : 0.0, d = live ? (double)dy[g] : 0.0;
            a_dy += d;
            a_dyt = fma(d, t, a_dyt);
            a_t += t;
            a_tt = fma(t, t, a_tt);
        }
    }
    // the two halves of a wave hold different rows of the same column: a + b = b + a, both get the same bits
    a_dy += __shfl_xor(a_dy, 32, 64);
    a_dyt += __shfl_xor(a_dyt, 32, 64);
    a_t += __shfl_xor(a_t, 32, 64);
    a_tt += __shfl_xor(a_tt, 32, 64);
#pragma unroll
    for (int g = 0; g < 16; ++g) pw[p.wave][c_row(g, p.h) * kF + p.c] = P[g];
    if (p.h == 0) {
        sw[p.wave][0][p.c] = a_dy;
        sw[p.wave][1][p.c] = a_dyt;
        sw[p.wave][2][p.c] = a_t;
        sw[p.wave][3][p.c] = a_tt;
    }
    __syncthreads();
    double *row = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kRow;
    for (int e = threadIdx.x; e < kRow; e += kThreads) {
        double acc = 0.0;
        if (e < kF * kF) {
#pragma unroll
            for (int w = 0; w < kWaves; ++w) acc += (double)pw[w][e];               // wave order
        } else {
#pragma unroll
            for (int w = 0; w < kWaves; ++w) acc += (&sw[w][0][0])[e - kF * kF];
        }
        row[e] = acc;
    }
}

// dz = mask * rstd * (dy - sum dy / n - t * rstd^2 * sum dy t / n), in double from coef[4][ld] as bn_bwd_apply_kernel
__global__ __launch_bounds__(kThreads) void nl_bwd_apply_kernel(const float *__restrict__ ds,
                                                                const float *__restrict__ z,
                                                                const float *__restrict__ W,
                                                                const double *__restrict__ coef,
                                                                float *__restrict__ dz, int64_t n_rows, int tiles,
                                                                int relu)
{
    const Slab p(n_rows, tiles);
    float wT[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) wT[s] = W[p.c * kF + 16 * p.h + s];
    const int f = p.w0 + p.c;
    const double mu = coef[f], a = coef[p.ld + f], b = coef[2 * p.ld + f], cc = coef[3 * p.ld + f];
    for (int64_t row0 = p.r0; row0 < p.r1; row0 += 32) {
        float ga[16], zc[16];
        p.load_a(ds, row0, ga);
#pragma unroll
        for (int g = 0; g < 16; ++g) zc[g] = z[p.at(row0 + c_row(g, p.h))];
        __builtin_amdgcn_sched_barrier(0);                  // (all loads in flight before the first use)
        const f32x16 dy = tile_dy(ga, wT);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int64_t r = row0 + c_row(g, p.h);
            const float x = zc[g];
            const double t = (double)act(x, relu) - mu;
            const float dx = (float)(a * fma(-t, cc, (double)dy[g] - b));
            if (r < p.r1) dz[r * p.ld + p.w0 + p.c] = (relu && x <= 0.f) ? 0.f : dx;   // threshold_backward: NaN z passes dx
        }
    }
}

// tot[window][kRow] = the window's n_blocks partial rows added in a fixed order: thread (grp, c) of a 1024-thread
// block adds the rows grp, grp + 32, ... of column blockIdx.x * 32 + c, then the 32 group sums are added in group
// order (bn_finish_kernel's order)
__global__ __launch_bounds__(1024) void nl_finish_blocks(const double *__restrict__ partial, int n_blocks,
                                                         double *__restrict__ tot)
{
    __shared__ double red[32][33];
    const int c = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + c;                       // (kRow is a multiple of 32)
    partial += (int64_t)blockIdx.y * n_blocks * kRow;
    double a = 0.0;
#pragma unroll 4
    for (int k = grp; k < n_blocks; k += 32) a += partial[(int64_t)k * kRow + e];
    red[grp][c] = a;
    __syncthreads();
    if (grp == 0) {
        a = 0.0;
        for (int k = 0; k < 32; ++k) a += red[k][c];
        tot[(int64_t)blockIdx.y * kRow + e] = a;
    }
}

// grad_W = the windows' P added in window order, rounded once; coef[4][batch * 32] from a window's four sums as
// bn_finish_kernel<4> derives it (mean, var and rstd of the column to double precision, centred on mean32)
__global__ __launch_bounds__(1024) void nl_finish(const double *__restrict__ tot, int batch, double n, float eps,
                                                  const float *__restrict__ mean, float *__restrict__ grad_w,
                                                  double *__restrict__ coef)
{
    const int e = threadIdx.x;
    double g = 0.0;
    for (int w = 0; w < batch; ++w) g += tot[(int64_t)w * kRow + e];
    grad_w[e] = (float)g;
    const int64_t ld = (int64_t)batch * kF;
    for (int64_t o = threadIdx.x; o < ld; o += 1024) {
        const double *s = tot + (o / kF) * kRow + kF * kF + (o % kF);
        const double s_dy = s[0], s_dyt = s[kF], s_t = s[2 * kF], s_tt = s[3 * kF];
        const double d = s_t / n;                            // mean - mean32
        double v = s_tt / n - d * d;
        v = v < 0.0 ? 0.0 : v;                               // (keeps NaN)
        const double rs = 1.0 / sqrt(v + (double)eps);
        const double sgx = s_dyt - d * s_dy;                 // sum dy (x - mean)
        coef[o] = (double)mean[o] + d;
        coef[ld + o] = rs;
        coef[2 * ld + o] = s_dy / n;
        coef[3 * ld + o] = rs * rs * (sgx / n);
    }
}

struct Geometry {
    int tiles;                            // per wave
    int64_t rows_per_block, blocks;
    explicit Geometry(int64_t n_rows)
    {
        tiles = (int)((n_rows + 32 * kWaves * kMaxBlocks - 1) / (32 * kWaves * kMaxBlocks));
        rows_per_block = (int64_t)32 * kWaves * tiles;
        blocks = (n_rows + rows_per_block - 1) / rows_per_block;
    }
};

bool shape_ok(int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch)
{
    return n_rows >= 2 && n_rows <= ((int64_t)1 << 40) && Fin == kF && Fout == kF && batch >= 1 &&
           batch <= kMaxBatch;
}

int check(const char *who, int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch, bool null_ptr,
          uintptr_t tensors, uintptr_t doubles)
{
    if (!shape_ok(n_rows, Fin, Fout, batch))
        return bad(who, GCN_E_BADARG, "needs n_rows >= 2, Fin = Fout = 32 and 1 <= batch <= 65535");
    if (null_ptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if (tensors % 16 != 0 || doubles % 8 != 0)
        return bad(who, GCN_E_ALIGN, "16-byte alignment required (coef: 8)");
    return 0;
}

}   // namespace

extern "C" {

size_t gcn_bn_linear_workspace_bytes(int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch)
{
    if (!shape_ok(n_rows, Fin, Fout, batch)) return 0;
    return (size_t)batch * (size_t)(Geometry(n_rows).blocks + 1) * kRow * sizeof(double);
}

int gcn_bn_linear_forward(const float *z, const float *weight, const float *mean, const float *rstd, float *s,
                          int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch, int relu, void *stream)
{
    const char *who = "gcn_bn_linear_forward";
    if (int rc = check(who, n_rows, Fin, Fout, batch,
                       z == nullptr || weight == nullptr || mean == nullptr || rstd == nullptr || s == nullptr,
                       (uintptr_t)z | (uintptr_t)s | (uintptr_t)weight, 0))
        return rc;
    const Geometry g(n_rows);
    hipLaunchKernelGGL(nl_forward_kernel, dim3((unsigned)g.blocks, (unsigned)batch), dim3(kThreads), 0,
                       (hipStream_t)stream, z, weight, mean, rstd, s, n_rows, g.tiles, relu);
    return launched(who);
}

int gcn_bn_linear_backward_sums(const float *ds, const float *z, const float *weight, const float *mean,
                                const float *rstd, int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch,
                                int relu, float eps, float *grad_w, double *coef, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    const char *who = "gcn_bn_linear_backward_sums";
    if (int rc = check(who, n_rows, Fin, Fout, batch,
                       ds == nullptr || z == nullptr || weight == nullptr || mean == nullptr || rstd == nullptr ||
                           grad_w == nullptr || coef == nullptr,
                       (uintptr_t)ds | (uintptr_t)z | (uintptr_t)weight, (uintptr_t)coef))
        return rc;
    if (workspace == nullptr || workspace_bytes < gcn_bn_linear_workspace_bytes(n_rows, Fin, Fout, batch))
        return bad(who, GCN_E_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace % 16 != 0) return bad(who, GCN_E_ALIGN, "16-byte alignment required (coef: 8)");
    const Geometry g(n_rows);
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    double *tot = part + (int64_t)batch * g.blocks * kRow;
    hipLaunchKernelGGL(nl_bwd_sums_kernel, dim3((unsigned)g.blocks, (unsigned)batch), dim3(kThreads), 0, st, ds, z,
                       weight, mean, rstd, part, n_rows, g.tiles, relu);
    hipLaunchKernelGGL(nl_finish_blocks, dim3(kRow / 32, (unsigned)batch), dim3(1024), 0, st, (const double *)part,
                       (int)g.blocks, tot);
    hipLaunchKernelGGL(nl_finish, dim3(1), dim3(1024), 0, st, (const double *)tot, (int)batch, (double)n_rows, eps,
                       mean, grad_w, coef);
    return launched(who);
}

int gcn_bn_linear_backward_apply(const float *ds, const float *z, const float *weight, const double *coef, float *dz,
                                 int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch, int relu, void *stream)
{
    const char *who = "gcn_bn_linear_backward_apply";
    if (int rc = check(who, n_rows, Fin, Fout, batch,
                       ds == nullptr || z == nullptr || weight == nullptr || coef == nullptr || dz == nullptr,
                       (uintptr_t)ds | (uintptr_t)z | (uintptr_t)dz | (uintptr_t)weight, (uintptr_t)coef))
        return rc;
    const Geometry g(n_rows);
    hipLaunchKernelGGL(nl_bwd_apply_kernel, dim3((unsigned)g.blocks, (unsigned)batch), dim3(kThreads), 0,
                       (hipStream_t)stream, ds, z, weight, coef, dz, n_rows, g.tiles, relu);
    return launched(who);
}

}   // extern "C"
