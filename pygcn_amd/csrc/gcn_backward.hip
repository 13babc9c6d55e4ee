// gcn_backward.hip — the element-wise backward sweeps of the GraphConvolution epilogues, for gfx950 (MI355X, CDNA4):
// gcn_relu_dropout_backward and the three *_backward_colsum entry points of include/gcn_spmm.h (the backward of the
// fused ReLU + dropout, of the fused log_softmax and of the NLL loss on it, each with the bias gradient's column sums).
// Streaming passes, HBM-bound; no sparse operand anywhere in this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

// ------------------------------------------------------------------------------------------
// backward of the fused ReLU + inverted-dropout epilogue: out = relu(z) * mask / (1 - p), so
// out > 0 <=> (z > 0 and kept), and grad_z = grad_out * scale * [out > 0].  One streaming pass,
// 16 B per lane, grid-stride (HBM-bound: 2 reads + 1 write per element).
// ------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(256) void relu_dropout_bwd_kernel(const T *__restrict__ grad_out,
                                                               const T *__restrict__ out,
                                                               T *__restrict__ grad_pre,
                                                               int64_t n_units, float scale)
{
    typedef typename Elem<T, VEC>::Raw Raw;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_units; i += stride) {
        float g[VEC], o[VEC];
        Elem<T, VEC>::unpack(((const Raw *)grad_out)[i], g);
        Elem<T, VEC>::unpack(((const Raw *)out)[i], o);
#pragma unroll
        for (int k = 0; k < VEC; ++k) g[k] = o[k] > 0.f ? g[k] * scale : 0.f;
        ((Raw *)grad_pre)[i] = Elem<T, VEC>::pack(g);
    }
}

// ------------------------------------------------------------------------------------------
// the same pass with the column sums of its result (grad_bias = sum over rows of grad_pre,
// autograd of `output + self.bias`, pygcn/layers.py:35-36) produced on the fly.  A 256-thread
// block owns a contiguous slab of rows; thread t owns the 4 columns 4*(t % CG) (CG = F/4 column
// groups) of every (256/CG)-th row, keeps 4 running sums, and the block writes one partial row
// [F]; a second tiny kernel adds the partial rows in block order (deterministic, no atomics).
// MODE 0 gives a plain column sum (layer without a fused ReLU), MODE 1 the ReLU / dropout mask,
// MODE 2 the backward of a fused log_softmax: grad_pre = g - exp(out) * rowsum(g), the row sum by
// xor-shuffles over the row's CG <= 64 lanes; rows of g that are entirely zero (every vertex
// outside idx_train) are written as zeros without reading `out`.
// MODE 3 is MODE 2 for the gradient of a mean NLL loss over ALL rows (F.nll_loss(output, labels),
// reference pygcn/train.py:153 without the index selection): g has one non-zero per row,
// g[r][target[r]] = coef, so it is never materialised — grad_pre = coef * (onehot(target[r]) -
// exp(out)), straight from `out` and the label vector: 2 instead of 4 full-height streams.
// ------------------------------------------------------------------------------------------
template <typename T, int VEC, int MODE>
__global__ __launch_bounds__(256) void bwd_colsum_kernel(const T *__restrict__ grad_out,
                                                         const T *__restrict__ out,
                                                         T *__restrict__ grad_pre,
                                                         float *__restrict__ partial, int64_t n_rows,
                                                         int F, float scale, int rows_per_block,
                                                         uint8_t *__restrict__ rowflag,
                                                         int32_t *__restrict__ nnz_rows, int skip,
                                                         const int64_t *__restrict__ target,
                                                         const float *__restrict__ coef)
{
    typedef typename Elem<T, VEC>::Raw Raw;
    __shared__ float red[256 * VEC];
    const float cf = MODE == 3 ? *coef : 0.f;
    const int CG = F / VEC, RL = 256 / CG;         // column groups (16 B each), row lanes
    const int cg = threadIdx.x % CG, rl = threadIdx.x / CG;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(r0 + (int64_t)rows_per_block, n_rows);
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    int nz_count = 0;
    // (measured on MI355X: unroll 2 / 4 and 8192 slabs change nothing (+-1 %): the pass already runs at
    //  the device's mixed read+write rate, 5.5 TB/s)
#pragma unroll 1
    for (int64_t r = r0 + rl; r < r1; r += RL) {
        const int64_t off = r * F + VEC * cg;
        float g[VEC];
        if (MODE != 3) Elem<T, VEC>::unpack(*(const Raw *)(grad_out + off), g);
        Raw packed = {};
        if (MODE == 3) {
            const int64_t t_row = target[r];          // (one address per row: a broadcast load)
            const int64_t t = t_row - VEC * cg;
#pragma unroll
            for (int i = 0; i < VEC; ++i) g[i] = 0.f;
            if (t_row >= 0) {   // a negative label (torch's ignore_index = -100) is an ignored row: zeros
                float o[VEC];
                Elem<T, VEC>::unpack(*(const Raw *)(out + off), o);
#pragma unroll
                for (int i = 0; i < VEC; ++i) g[i] = cf * ((t == i ? 1.f : 0.f) - expf(o[i]));
            }
            packed = Elem<T, VEC>::pack(g);
            Elem<T, VEC>::unpack(packed, g);
        }
        if (MODE == 1) {
            // lanes whose 16 bytes of grad_out are all zero produce zeros whatever `out` holds:
            // they skip its load (row-sparse gradients: most of the `out` traffic disappears)
            bool gnz = false;
#pragma unroll
            for (int i = 0; i < VEC; ++i) gnz |= (g[i] != 0.f);
            if (gnz) {
                float o[VEC];
                Elem<T, VEC>::unpack(*(const Raw *)(out + off), o);
#pragma unroll
                for (int i = 0; i < VEC; ++i) g[i] = o[i] > 0.f ? g[i] * scale : 0.f;
            }
            packed = Elem<T, VEC>::pack(g);
            Elem<T, VEC>::unpack(packed, g);   // sums and flags follow the STORED (rounded) values
        }
        if (MODE == 2) {
            float rs = 0.f;
            bool gnz = false;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                rs += g[i];
                gnz |= (g[i] != 0.f);
            }
            for (int o2 = 1; o2 < CG; o2 <<= 1) rs += __shfl_xor(rs, o2, 64);
            const unsigned long long gb = __ballot(gnz);
            const int ln = threadIdx.x & 63;
            const unsigned long long gm = CG >= 64 ? ~0ull : (((1ull << CG) - 1) << (ln & ~(CG - 1)));
            if (gb & gm) {   // uniform over the row's lanes
                float o[VEC];
                Elem<T, VEC>::unpack(*(const Raw *)(out + off), o);
#pragma unroll
                for (int i = 0; i < VEC; ++i) g[i] -= expf(o[i]) * rs;
            }
            packed = Elem<T, VEC>::pack(g);
            Elem<T, VEC>::unpack(packed, g);
        }
        bool any = false;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            acc[i] += g[i];
            any |= (g[i] != 0.f);
        }
        bool row_nz = true;
        if (rowflag != nullptr) {
            // a row lives in CG <= 64 consecutive lanes of one wave (all active or all inactive
            // together): its non-zero flag is a slice of the wave's ballot over the active lanes;
            // the row's first lane writes the byte
            const unsigned long long b = __ballot(any);
            const int lane = threadIdx.x & 63;
            const unsigned long long m = CG >= 64 ? ~0ull : (((1ull << CG) - 1) << (lane & ~(CG - 1)));
            row_nz = (b & m) != 0;
            if (cg == 0) {
                rowflag[r] = row_nz ? 1 : 0;
                nz_count += row_nz ? 1 : 0;
            }
        }
        // skip mode: all-zero rows of the result are not written (the consumer reads the flagged
        // rows only) — at the labelled share of the bench that is 84-95 % of the pass's writes
        if (MODE != 0 && (!skip || row_nz)) *(Raw *)(grad_pre + off) = packed;
    }
    if (rowflag != nullptr) {
        // one atomic per wave: lanes that own rows hold their counts
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) nz_count += __shfl_xor(nz_count, off, 64);
        if ((threadIdx.x & 63) == 0 && nz_count) atomicAdd(nnz_rows, nz_count);
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) red[threadIdx.x * VEC + i] = acc[i];
    __syncthreads();
    if (rl == 0) {
        for (int k = 1; k < RL; ++k)   // fixed order
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] += red[(k * CG + cg) * VEC + i];
#pragma unroll
        for (int i = 0; i < VEC; ++i) partial[(int64_t)blockIdx.x * F + VEC * cg + i] = acc[i];
    }
}

// per-row bytes -> bitmap words (1 bit per row; fits the XCD L2 where the byte table does not)
__global__ __launch_bounds__(256) void pack_row_flags_kernel(const uint8_t *__restrict__ bytes,
                                                             uint32_t *__restrict__ bits, int64_t n_rows)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_words = (n_rows + 31) >> 5;
    if (w >= n_words) return;
    uint32_t v = 0;
    const int64_t r0 = w << 5;
#pragma unroll 8
    for (int i = 0; i < 32; ++i)
        if (r0 + i < n_rows && bytes[r0 + i]) v |= 1u << i;
    bits[w] = v;
}

// partial[n_blocks][F] -> colsum[F].  A 1024-thread block owns 32 columns; thread (g, c) adds the
// partial rows g, g+32, g+64, ... of column c (4 loads in flight), then the 32 group sums are added
// in group order through LDS: a fixed summation order, so the result is bitwise reproducible.
__global__ __launch_bounds__(1024) void colsum_finish_kernel(const float *__restrict__ partial,
                                                             float *__restrict__ colsum, int n_blocks,
                                                             int F)
{
    __shared__ float red[32][33];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int f = blockIdx.x * 32 + c;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (f < F) {
        int b = g;
        for (; b + 96 < n_blocks; b += 128) {
            s0 += partial[(int64_t)b * F + f];
            s1 += partial[(int64_t)(b + 32) * F + f];
            s2 += partial[(int64_t)(b + 64) * F + f];
            s3 += partial[(int64_t)(b + 96) * F + f];
        }
        for (; b < n_blocks; b += 32) s0 += partial[(int64_t)b * F + f];
    }
    red[g][c] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (g == 0 && f < F) {
        float s = 0.f;
        for (int k = 0; k < 32; ++k) s += red[k][c];
        colsum[f] = s;
    }
}

}   // namespace

extern "C" {

int gcn_relu_dropout_backward(int dtype, const void *grad_out, const void *out, void *grad_pre,
                              int64_t n_elems, float scale, void *stream)
{
    const char *who = "gcn_relu_dropout_backward";
    if (dtype != GCN_DTYPE_F32 && dtype != GCN_DTYPE_BF16) return bad(who, GCN_E_BADARG, "unknown dtype");
    if (n_elems < 0) return bad(who, GCN_E_BADARG, "negative size");
    if (n_elems == 0) return 0;
    if (grad_out == nullptr || out == nullptr || grad_pre == nullptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    const int64_t per = lane_elems(dtype);
    const bool vec = (n_elems % per == 0) && (((uintptr_t)grad_out | (uintptr_t)out |
                                                (uintptr_t)grad_pre) % 16 == 0);
    const int64_t n_units = vec ? n_elems / per : n_elems;
    const unsigned blocks = (unsigned)std::min<int64_t>((n_units + 255) / 256, 256 * 8 * 4);
    hipStream_t s = (hipStream_t)stream;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        pick_int<Lane<T>::V, 1>(vec ? Lane<T>::V : 1, [&](auto v) {
            hipLaunchKernelGGL((relu_dropout_bwd_kernel<T, decltype(v)::value>), dim3(blocks), dim3(256), 0, s,
                               (const T *)grad_out, (const T *)out, (T *)grad_pre, n_units, scale);
        });
    });
    return launched("relu_dropout_backward launch");
}

size_t gcn_bwd_colsum_workspace_bytes(int64_t n_rows, int64_t F, int dtype)
{
    if (n_rows <= 0 || !lane_width_ok(F, dtype)) return 0;
    // partial column sums + one byte per row (staging for the row bitmap)
    return (size_t)RowSlabs(n_rows).blocks * (size_t)F * sizeof(float) + (((size_t)n_rows + 15) & ~(size_t)15);
}

static int bwd_colsum_impl(const char *who, int mode, int dtype, const void *grad_out, const void *out,
                           void *grad_pre, float *colsum, int64_t n_rows, int64_t F, float scale,
                           uint32_t *row_bits, int32_t *nnz_rows, int skip_zero_rows,
                           void *workspace, size_t workspace_bytes, void *stream,
                           const int64_t *target = nullptr, const float *coef = nullptr)
{
    if (dtype != GCN_DTYPE_F32 && dtype != GCN_DTYPE_BF16) return bad(who, GCN_E_BADARG, "unknown dtype");
    if ((row_bits == nullptr) != (nnz_rows == nullptr))
        return bad(who, GCN_E_BADARG, "row_bits and nnz_rows go together");
    const int64_t vec = lane_elems(dtype);
    if (n_rows < 0 || !lane_width_ok(F, dtype))
        return bad(who, GCN_E_BADARG, "F must be a multiple of the 16-byte lane width with F/width dividing 256");
    if (mode >= 2 && F / vec > 64)
        return bad(who, GCN_E_BADARG, "a row must fit one wavefront (F / lane width <= 64)");
    if (row_bits != nullptr && F / vec > 64)   // a row spans several wavefronts: no per-row ballot
        return bad(who, GCN_E_BADARG, "row_bits / nnz_rows need F / lane width <= 64 (pass NULL for wider rows)");
    if (skip_zero_rows && (row_bits == nullptr || mode == 0))
        return bad(who, GCN_E_BADARG, "skip_zero_rows needs the row bitmap outputs and a result tensor");
    if (colsum == nullptr || (grad_out == nullptr && mode != 3) || (out != nullptr && grad_pre == nullptr)
        || (mode == 3 && (target == nullptr || coef == nullptr || out == nullptr)))
        return bad(who, GCN_E_BADARG, "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    if (nnz_rows != nullptr) {
        hipError_t e = hipMemsetAsync(nnz_rows, 0, sizeof(int32_t), s);
        if (e != hipSuccess) return gcn_internal_fail_hip((int)e, who);
    }
    if (n_rows == 0) {
        hipError_t e = hipMemsetAsync(colsum, 0, (size_t)F * sizeof(float), s);
        return e == hipSuccess ? 0 : gcn_internal_fail_hip((int)e, who);
    }
    const size_t need = gcn_bwd_colsum_workspace_bytes(n_rows, F, dtype);
    if (workspace == nullptr || workspace_bytes < need) return bad(who, GCN_E_WORKSPACE, "workspace too small");
    if (((uintptr_t)grad_out | (uintptr_t)out | (uintptr_t)grad_pre | (uintptr_t)workspace) % 16 != 0)
        return bad(who, GCN_E_ALIGN, "16-byte alignment required");
    const RowSlabs sl(n_rows);
    uint8_t *row_nonzero = row_bits ? (uint8_t *)workspace + (size_t)sl.blocks * (size_t)F * sizeof(float)
                                    : nullptr;
    const dim3 grid((unsigned)sl.blocks), block(256);
    float *part = (float *)workspace;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        pick_int<0, 1, 2, 3>(mode, [&](auto m) {
            hipLaunchKernelGGL((bwd_colsum_kernel<T, Lane<T>::V, decltype(m)::value>), grid, block, 0, s,
                               (const T *)grad_out, (const T *)out, (T *)grad_pre, part, n_rows, (int)F, scale,
                               sl.rows_per_block, row_nonzero, nnz_rows, skip_zero_rows ? 1 : 0, target, coef);
        });
    });
    hipLaunchKernelGGL(colsum_finish_kernel, dim3((unsigned)((F + 31) / 32)), dim3(1024), 0, s,
                       (const float *)workspace, colsum, (int)sl.blocks, (int)F);
    if (row_bits != nullptr)
        hipLaunchKernelGGL(pack_row_flags_kernel, dim3((unsigned)((((n_rows + 31) >> 5) + 255) / 256)),
                           dim3(256), 0, s, (const uint8_t *)row_nonzero, row_bits, n_rows);
    return launched(who);
}

int gcn_relu_dropout_backward_colsum(int dtype, const void *grad_out, const void *out, void *grad_pre,
                                     float *colsum, int64_t n_rows, int64_t F, float scale,
                                     uint32_t *row_bits, int32_t *nnz_rows, int skip_zero_rows,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    return bwd_colsum_impl("gcn_relu_dropout_backward_colsum", out != nullptr ? 1 : 0, dtype, grad_out,
                           out, grad_pre, colsum, n_rows, F, scale, row_bits, nnz_rows, skip_zero_rows,
                           workspace, workspace_bytes, stream);
}

int gcn_log_softmax_backward_colsum(int dtype, const void *grad_out, const void *out, void *grad_pre,
                                    float *colsum, int64_t n_rows, int64_t F, uint32_t *row_bits,
                                    int32_t *nnz_rows, int skip_zero_rows, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    if (out == nullptr) return bad("gcn_log_softmax_backward_colsum", GCN_E_BADARG, "NULL pointer");
    return bwd_colsum_impl("gcn_log_softmax_backward_colsum", 2, dtype, grad_out, out, grad_pre, colsum,
                           n_rows, F, 1.f, row_bits, nnz_rows, skip_zero_rows, workspace,
                           workspace_bytes, stream);
}

int gcn_nll_log_softmax_backward_colsum(int dtype, const int64_t *target, const float *coef,
                                        const void *out, void *grad_pre, float *colsum, int64_t n_rows,
                                        int64_t F, void *workspace, size_t workspace_bytes, void *stream)
{
    return bwd_colsum_impl("gcn_nll_log_softmax_backward_colsum", 3, dtype, nullptr, out, grad_pre,
                           colsum, n_rows, F, 1.f, nullptr, nullptr, 0, workspace, workspace_bytes,
                           stream, target, coef);
}

}   // extern "C"
