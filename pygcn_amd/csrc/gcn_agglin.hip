// gcn_agglin.hip — the dense half of an aggregate-first input layer, (Â·X)·W + b, for narrow inputs (gfx950).
//
// The fork's live models start with a narrow layer: 4, 8 or 16 input columns into a 32-wide GCN (reference
// pygcn/gnn-over-mlp.py:221-237, policy-generator.py:330-350), and the input of that layer needs no gradient.
// Evaluated the reference's way, Â·(X·W) + b (pygcn/layers.py:33-38), the sparse product gathers rows of k·32
// floats and the backward pass needs a transpose product of the same width only to form grad_W.  Evaluated as
// (Â·X)·W + b, the sparse product gathers k·Fin floats per stored entry and, with z = Â·X kept,
//     y      = act(z · W + b)                                                   gcn_agg_linear_forward
//     grad_W = z^T · gp,  grad_b = colsum(gp),  gp = relu ? g · [y > 0] : g      gcn_agg_linear_backward
// are two dense sweeps: layer 1 has no sparse product in its backward pass at all.  There is no input gradient.
//
// LAYOUT.  z [n_rows, batch·Fin] and y, g [n_rows, batch·32] are contiguous fp32 with sample j in the columns
// [j·F, (j+1)·F): row r, sample j is UNIT u = r·batch + j, whose Fin floats of z start at z + u·Fin and whose 32
// floats of y at y + u·32.  Both sweeps walk the M = n_rows·batch units as one flat [M, Fin] · [Fin, 32] product;
// no sum of the forward sweep mixes units, so a sample's y is bitwise that of the batch = 1 call on a contiguous
// copy of its columns.
//
// FORWARD, THE ORDER (the bitwise tests rest on it).  For every element
//     acc = fmaf(z[u][0], W[0][c], 0.0f);  acc = fmaf(z[u][i], W[i][c], acc) for i = 1 .. Fin-1 ascending;
//     if (bias) acc = acc + b[c];  if (relu) acc = acc < 0 ? 0 : acc          (torch.relu: NaN stays NaN)
// in fp32, plain VALU FMAs.  8 lanes share a unit; a lane owns the four adjacent columns 4·(lane & 7) .. + 3 and
// keeps its [Fin][4] slice of W in registers for the whole sweep; the lanes of a unit read the same z floats
// (16-byte loads that the memory pipeline serves once); a wave stores 8 units = 1 KiB contiguous, 16 bytes per
// lane.  Blocks of 256 threads walk the units with a grid stride.
//
// BACKWARD, THE ORDER.  Everything is accumulated in DOUBLE (an fp32 × fp32 product is exact in double, so each
// step rounds once, at 2^-53).  Block b owns the units [b·R, min((b+1)·R, M)), its wave w the units
// [b·R + 16·P·w, b·R + 16·P·(w+1)) of them; lane (h = lane >> 5, c = lane & 31) owns column c and walks the wave's
// units of parity h (first + h, first + h + 2, ...) in ascending order: acc[i] = fma(z[u][i], gp[u][c], acc[i]),
// accb += gp[u][c] (the loads of 8 / 4 / 2 units, for Fin <= 8 / <= 16 / <= 32, are issued together; the additions
// keep their order).  Then half 0 + half 1 (one addition, commutative), the 4 waves in wave order, one partial row
// of Fin·32 + 32 doubles per block (grad_W row-major, then grad_b).  The finishing launch adds the partial rows
// in block order 0, 1, 2, ... and rounds once to fp32.  No atomics; the result does not depend on which block
// ran first.  g, z (and y when relu) are read once.
//
// GEOMETRY of the backward sweep (gcn_agg_linear_partial_rows documents it in include/gcn_spmm.h):
//     M = n_rows·batch,  P = ceil(M / (64 · 2048)),  R = 64·P units per block,  B = ceil(M / R) <= 2048 blocks.
//
// The mask is y <= 0 ? 0 : g, as gcn_norm.hip: a NaN y passes its gradient.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

constexpr int kF = 32;                    // the one output width built
constexpr int kWaves = 4;                 // per block
constexpr int kThreads = 64 * kWaves;
constexpr int kFwdUnits = kThreads / 8;   // units of one block per pass of the forward sweep
constexpr int64_t kFwdBlocks = 4096;      // grid cap of the forward sweep (grid stride above it)
constexpr int kFinishRows = 128;          // partial rows the finishing launch stages per pass

// y = act(z · W + b): 8 lanes per unit, 4 adjacent columns per lane
template <int FIN>
__global__ __launch_bounds__(kThreads) void al_forward_kernel(const float *__restrict__ z,
                                                              const float *__restrict__ W,
                                                              const float *__restrict__ bias, float *__restrict__ y,
                                                              int64_t units, int relu)
{
    const int c0 = 4 * (threadIdx.x & 7);
    float w[FIN][4], b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < FIN; ++i) Run4<float>::load(W + i * kF + c0, w[i]);
    const bool has_bias = bias != nullptr;
    if (has_bias) Run4<float>::load(bias + c0, b);
    const int64_t stride = (int64_t)gridDim.x * kFwdUnits;
    for (int64_t u = (int64_t)blockIdx.x * kFwdUnits + (threadIdx.x >> 3); u < units; u += stride) {
        float x[FIN];
#pragma unroll
        for (int i = 0; i < FIN; i += 4) {
            const f32x4 v = *(const f32x4 *)(z + u * FIN + i);
            x[i] = v.x; x[i + 1] = v.y; x[i + 2] = v.z; x[i + 3] = v.w;
        }
        float acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = __builtin_fmaf(x[0], w[0][c], 0.f);
#pragma unroll
        for (int i = 1; i < FIN; ++i) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_fmaf(x[i], w[i][c], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = act(has_bias ? acc[c] + b[c] : acc[c], relu);
        Run4<float>::store_rounded(y + u * kF + c0, acc);
    }
}

// partial[block][FIN * 32 + 32]: z^T · gp and colsum(gp) over the block's units, in double
template <int FIN>
__global__ __launch_bounds__(kThreads) void al_backward_kernel(const float *__restrict__ g,
                                                               const float *__restrict__ y,
                                                               const float *__restrict__ z,
                                                               double *__restrict__ partial, int64_t units,
                                                               int64_t per_wave, int relu)
{
    constexpr int kRow = FIN * kF + kF;
    __shared__ double red[kWaves][kRow];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    const int64_t u0 = ((int64_t)blockIdx.x * kWaves + wave) * per_wave;
    const int64_t u1 = min(u0 + per_wave, units);
    double acc[FIN], accb = 0.0;
#pragma unroll
    for (int i = 0; i < FIN; ++i) acc[i] = 0.0;
    // kBatch units of the lane at a time, all their loads in flight before the first use (a lane's loads are small;
    // worth 4 % at Fin = 8); the units are still added in ascending order
    constexpr int kBatch = FIN <= 8 ? 8 : FIN <= 16 ? 4 : 2;
    int64_t u = u0 + h;
    for (; u + 2 * (kBatch - 1) < u1; u += 2 * kBatch) {
        float gv[kBatch], yv[kBatch], x[kBatch][FIN];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int64_t ub = u + 2 * b;
            gv[b] = g[ub * kF + c];
            yv[b] = relu ? y[ub * kF + c] : 1.f;
#pragma unroll
            for (int i = 0; i < FIN; i += 4) {
                const f32x4 v = *(const f32x4 *)(z + ub * FIN + i);
                x[b][i] = v.x; x[b][i + 1] = v.y; x[b][i + 2] = v.z; x[b][i + 3] = v.w;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const double gd = (double)(yv[b] <= 0.f ? 0.f : gv[b]);   // threshold_backward: a NaN y passes g
#pragma unroll
            for (int i = 0; i < FIN; ++i) acc[i] = fma((double)x[b][i], gd, acc[i]);
            accb += gd;
        }
    }
    for (; u < u1; u += 2) {                                          // the last, partial batch
        float gv = g[u * kF + c];
        if (relu) gv = y[u * kF + c] <= 0.f ? 0.f : gv;
        float x[FIN];
#pragma unroll
        for (int i = 0; i < FIN; i += 4) {
            const f32x4 v = *(const f32x4 *)(z + u * FIN + i);
            x[i] = v.x; x[i + 1] = v.y; x[i + 2] = v.z; x[i + 3] = v.w;
        }
        const double gd = (double)gv;
#pragma unroll
        for (int i = 0; i < FIN; ++i) acc[i] = fma((double)x[i], gd, acc[i]);
        accb += gd;
    }
    // the two halves of a wave hold different units of the same column: a + b = b + a, both get the same bits
#pragma unroll
    for (int i = 0; i < FIN; ++i) acc[i] += __shfl_xor(acc[i], 32, 64);
    accb += __shfl_xor(accb, 32, 64);
    if (h == 0) {
#pragma unroll
        for (int i = 0; i < FIN; ++i) red[wave][i * kF + c] = acc[i];
        red[wave][FIN * kF + c] = accb;
    }
    __syncthreads();
    double *row = partial + (int64_t)blockIdx.x * kRow;
    for (int e = threadIdx.x; e < kRow; e += kThreads) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) a += red[w][e];             // wave order
        row[e] = a;
    }
}

// grad_w, grad_b = the n_blocks partial rows added in BLOCK ORDER, rounded once.  Thread (grp, c) of a
// 1024-thread block stages the rows t·128 + grp + 32·m (m = 0 .. 3) of column blockIdx.x * 32 + c in LDS; thread
// (0, c) then adds the 128 staged rows in ascending order to its running sum, pass after pass.
__global__ __launch_bounds__(1024) void al_finish_kernel(const double *__restrict__ partial, int n_blocks,
                                                         int row_len, int n_w, float *__restrict__ grad_w,
                                                         float *__restrict__ grad_b)
{
    __shared__ double red[kFinishRows][33];
    const int c = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + c;                              // (row_len is a multiple of 32)
    double total = 0.0;
    for (int base = 0; base < n_blocks; base += kFinishRows) {
#pragma unroll
        for (int m = 0; m < kFinishRows / 32; ++m) {
            const int k = base + grp + 32 * m;
            red[grp + 32 * m][c] = k < n_blocks ? partial[(int64_t)k * row_len + e] : 0.0;
        }
        __syncthreads();
        if (grp == 0) {
            const int rows = min(kFinishRows, n_blocks - base);
            for (int k = 0; k < rows; ++k) total += red[k][c];
        }
        __syncthreads();
    }
    if (grp == 0) {
        if (e < n_w) grad_w[e] = (float)total;
        else if (grad_b != nullptr) grad_b[e - n_w] = (float)total;
    }
}

struct Geometry {                         // of the backward sweep
    int64_t units, per_wave, per_block, blocks;
    Geometry(int64_t n_rows, int64_t batch)
    {
        units = n_rows * batch;
        const int64_t p = (units + 64 * kSlabBlocks - 1) / (64 * kSlabBlocks);
        per_wave = 16 * p;
        per_block = kWaves * per_wave;
        blocks = (units + per_block - 1) / per_block;
    }
};

bool shape_ok(int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch)
{
    return n_rows >= 1 && n_rows <= ((int64_t)1 << 40) && Fin >= 4 && Fin <= 32 && Fin % 4 == 0 && Fout == kF &&
           batch >= 1 && batch <= kMaxBatch;
}

int check(const char *who, int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch, bool null_ptr,
          uintptr_t tensors, uintptr_t words)
{
    if (!shape_ok(n_rows, Fin, Fout, batch))
        return bad(who, GCN_E_BADARG, "needs n_rows >= 1, Fin in {4, 8, ..., 32}, Fout = 32 and 1 <= batch <= 65535");
    if (null_ptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if (tensors % 16 != 0 || words % 4 != 0)
        return bad(who, GCN_E_ALIGN, "16-byte alignment required (grad_w, grad_b: 4, partials: 8)");
    return 0;
}

}   // namespace

extern "C" {

int64_t gcn_agg_linear_partial_rows(int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch)
{
    if (!shape_ok(n_rows, Fin, Fout, batch)) return 0;
    return Geometry(n_rows, batch).blocks;
}

int gcn_agg_linear_forward(const float *z, const float *weight, const float *bias, float *y, int64_t n_rows,
                           int64_t Fin, int64_t Fout, int64_t batch, int relu, void *stream)
{
    const char *who = "gcn_agg_linear_forward";
    if (int rc = check(who, n_rows, Fin, Fout, batch, z == nullptr || weight == nullptr || y == nullptr,
                       (uintptr_t)z | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)y, 0))
        return rc;
    const int64_t units = n_rows * batch;
    const int64_t blocks = std::min<int64_t>((units + kFwdUnits - 1) / kFwdUnits, kFwdBlocks);
    pick_int<4, 8, 12, 16, 20, 24, 28, 32>((int)Fin, [&](auto fin) {
        hipLaunchKernelGGL(al_forward_kernel<decltype(fin)::value>, dim3((unsigned)blocks), dim3(kThreads), 0,
                           (hipStream_t)stream, z, weight, bias, y, units, relu);
    });
    return launched(who);
}

int gcn_agg_linear_backward(const float *g, const float *y, const float *z, int64_t n_rows, int64_t Fin,
                            int64_t Fout, int64_t batch, int relu, float *grad_w, float *grad_b, double *partials,
                            int64_t partial_rows, void *stream)
{
    const char *who = "gcn_agg_linear_backward";
    if (int rc = check(who, n_rows, Fin, Fout, batch,
                       g == nullptr || z == nullptr || grad_w == nullptr || (relu && y == nullptr),
                       (uintptr_t)g | (uintptr_t)z | (relu ? (uintptr_t)y : 0),
                       (uintptr_t)grad_w | (uintptr_t)grad_b))
        return rc;
    const Geometry geo(n_rows, batch);
    if (partials == nullptr || partial_rows < geo.blocks)
        return bad(who, GCN_E_WORKSPACE, "partials: fewer rows than gcn_agg_linear_partial_rows");
    if ((uintptr_t)partials % 8 != 0)
        return bad(who, GCN_E_ALIGN, "16-byte alignment required (grad_w, grad_b: 4, partials: 8)");
    hipStream_t st = (hipStream_t)stream;
    const int row_len = (int)(Fin * kF + kF);
    pick_int<4, 8, 12, 16, 20, 24, 28, 32>((int)Fin, [&](auto fin) {
        hipLaunchKernelGGL(al_backward_kernel<decltype(fin)::value>, dim3((unsigned)geo.blocks), dim3(kThreads), 0,
                           st, g, y, z, partials, geo.units, geo.per_wave, relu);
    });
    hipLaunchKernelGGL(al_finish_kernel, dim3(row_len / 32), dim3(1024), 0, st, (const double *)partials,
                       (int)geo.blocks, row_len, (int)(Fin * kF), grad_w, grad_b);
    return launched(who);
}

}   // extern "C"
