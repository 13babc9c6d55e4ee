// gcn_pack.hip — rows of a mostly-zero activation as bitmask + non-zero values (gfx950).
//
// Used by the multi-GPU path's COMPRESSED hidden-layer exchange (pygcn_amd/sharded.py,
// ShardedGraph(compress_hidden=True)): the input of the second GraphConvolution layer is the
// output of relu + dropout (pygcn/models.py:48,50 upstream), >= 75 % zeros in training — its halo
// rows travel as 1 bit per element + the non-zero values and are expanded on arrival.  The
// reference has no multi-device code; this is part of the scaling design of SURVEY §8(e).
//
// Layout: bit j of bits[r][w] is set iff element 32·w + j of row r is non-zero (F a multiple of
// 32); vals holds the non-zero elements of the rows in row-major order, row r starting at
// offsets[r] (exclusive prefix sums of counts[]).  One wave per row; a lane owns 4 consecutive
// elements, so a 256-element slab is one wave instruction (16 B per lane at fp32).
//   pack, pass 1  gcn_rows_pack_count : bits + counts        (reads the rows once)
//   (exclusive scan of counts by the caller: offsets, total)
//   pack, pass 2  gcn_rows_pack_values: vals                  (reads the rows again; positions
//                                                              from ballots + mbcnt, no atomics)
//   unpack        gcn_rows_unpack     : dense rows from bits + offsets + vals
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

constexpr int kRowsPerBlock = 4;          // one wave per row, 4 waves per workgroup

__device__ __forceinline__ int below(unsigned long long m)      // set bits of m in lanes below this one
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// OR over each group of 8 consecutive lanes (quad xor-1, xor-2, then the half-row mirror)
__device__ __forceinline__ uint32_t or8(uint32_t v)
{
    v |= dpp_move<0xB1>(v);
    v |= dpp_move<0x4E>(v);
    v |= dpp_move<0x141>(v);
    return v;
}

template <typename T>
__global__ __launch_bounds__(kWave *kRowsPerBlock) void pack_count_kernel(
    const T *__restrict__ src, int64_t ld, const int64_t *__restrict__ rows, int64_t m, int F,
    uint32_t *__restrict__ bits, int32_t *__restrict__ counts)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (r >= m) return;
    const T *row = src + (rows ? rows[r] : r) * ld;
    const int words = F >> 5;
    int cnt = 0;
    for (int f0 = 0; f0 < F; f0 += 4 * kWave) {           // a slab of 256 elements per pass
        const int f = f0 + 4 * lane;
        uint32_t nib = 0u;
        if (f < F) {
            float x[4];
            Run4<T>::load(row + f, x);
#pragma unroll
            for (int k = 0; k < 4; ++k) nib |= (x[k] != 0.f ? 1u : 0u) << k;
        }
        cnt += __builtin_popcount(nib);
        const uint32_t w = or8(nib << (4 * (lane & 7)));   // the 8 lanes of a word hold its 8 nibbles
        if ((lane & 7) == 0 && f < F) bits[r * words + (f >> 5)] = w;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, kWave);
    if (lane == 0) counts[r] = cnt;
}

template <typename T>
__global__ __launch_bounds__(kWave *kRowsPerBlock) void pack_values_kernel(
    const T *__restrict__ src, int64_t ld, const int64_t *__restrict__ rows, int64_t m, int F,
    const int64_t *__restrict__ offsets, T *__restrict__ vals)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (r >= m) return;
    const T *row = src + (rows ? rows[r] : r) * ld;
    int64_t base = offsets[r];
    for (int f0 = 0; f0 < F; f0 += 4 * kWave) {
        const int f = f0 + 4 * lane;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (f < F) Run4<T>::load(row + f, x);
        // position of element (lane, k) among the non-zeros of the slab, in row order (4·lane + k):
        // all non-zeros of lower lanes + the non-zeros of this lane at lower k
        unsigned long long b[4];
        int pos = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = __ballot(x[k] != 0.f);
            pos += below(b[k]);
            total += __builtin_popcountll(b[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (x[k] != 0.f) {
                T out;
                if (sizeof(T) == 4) *(float *)&out = x[k];
                else *(bf16_t *)&out = (bf16_t)(__float_as_uint(x[k]) >> 16);
                vals[base + pos] = out;
                ++pos;
            }
        }
        base += total;
    }
}

template <typename T>
__global__ __launch_bounds__(kWave *kRowsPerBlock) void unpack_kernel(
    const uint32_t *__restrict__ bits, const int64_t *__restrict__ offsets, const T *__restrict__ vals,
    int64_t m, int F, T *__restrict__ dst, int64_t ldd)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (r >= m) return;
    const int words = F >> 5;
    int64_t base = offsets[r];
    for (int f0 = 0; f0 < F; f0 += 4 * kWave) {
        const int f = f0 + 4 * lane;
        uint32_t nib = 0u;
        if (f < F) nib = (bits[r * words + (f >> 5)] >> (4 * (lane & 7))) & 0xFu;
        float x[4];
        int pos = 0, total = 0;
        unsigned long long b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = __ballot(((nib >> k) & 1u) != 0u);
            pos += below(b[k]);
            total += __builtin_popcountll(b[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = 0.f;
            if ((nib >> k) & 1u) {
                const T v = vals[base + pos];
                x[k] = sizeof(T) == 4 ? *(const float *)&v : __uint_as_float((uint32_t)(*(const bf16_t *)&v) << 16);
                ++pos;
            }
        }
        if (f < F) Run4<T>::store_exact(dst + r * ldd + f, x);      // (the values ARE bf16 numbers)
        base += total;
    }
}

// counts[r] = set bits of row r of bits [m, words] (the receiver's side of the scan: the wire carries
// no counts).  8 lanes per row, 16 bytes per lane per pass.
__global__ __launch_bounds__(256) void bits_count_kernel(const uint32_t *__restrict__ bits, int64_t m, int words,
                                                         int32_t *__restrict__ counts)
{
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int sub = threadIdx.x & 7;
    int c = 0;
    if (r < m)
        for (int w = sub; w < words; w += 8) c += __builtin_popcount(bits[r * words + w]);
    c += __shfl_xor(c, 1, kWave);
    c += __shfl_xor(c, 2, kWave);
    c += __shfl_xor(c, 4, kWave);
    if (r < m && sub == 0) counts[r] = c;
}

// ------------------------------------------------------------------------------------------------
// FIXED-SLOT form for the single-GPU layer-2 gather (gcn_spmm_csr_packed): one 512-byte slot per 256-wide fp32
// row, four 128-byte sub-slots, one per column QUARTER in the lane order of the 256-wide GEMM's keep bits —
// quarter q holds columns 16 cb + 4 q + j (cb 0..15, j 0..3), bit 4 cb + j.  A sub-slot is 32 words:
//     [0] [1]   the 64-bit mask, bit set <=> the element's BIT PATTERN is non-zero (-0.0 is kept: the slot
//               reproduces the row bit for bit)
//     [2]       the number of set bits; more than GCN_PACK512_CAPACITY (29) marks the quarter — and with it the
//               row — as overflowed: its first 29 values are stored, a reader takes the dense row instead
//     [3 ..]    the non-zero values in bit order (words past the count are left unwritten)
// One wave per row, 16 lanes per quarter: lane (q, i) reads the 16 bytes of columns 16 i + 4 q .. + 3 (the wave
// reads the whole 1-KiB row), the quarter's mask is an OR over its 16 lanes (DPP), a value's place its rank.
constexpr int kPack512Cap = GCN_PACK512_CAPACITY;

__device__ __forceinline__ uint32_t or16(uint32_t v)       // OR over each row of 16 lanes
{
    v = or8(v);
    v |= dpp_move<0x140>(v);
    return v;
}

// The slot is put together in a wave-private 512-byte LDS image (header words from lanes 0..2 of the quarter, a
// value at its rank) and leaves as ONE 8-byte store per lane: 512 contiguous bytes, four whole 128-byte lines per
// wave instruction.  A wave carries kPack512RowsPerWave consecutive rows, their 16-byte loads issued first.  Words
// past a quarter's count carry whatever the image held (the format leaves them undefined; no reader uses them).
// Only the wave's own lanes touch its images, so a wavefront-scope fence orders write and read: no workgroup
// barrier (the last block's waves may have no rows and return).
#ifndef GCN_PACK512_ROWS_PER_WAVE
#define GCN_PACK512_ROWS_PER_WAVE 2
#endif
constexpr int kPack512RowsPerWave = GCN_PACK512_ROWS_PER_WAVE;
constexpr int kPack512RowsPerBlock = kRowsPerBlock * kPack512RowsPerWave;     // (kRowsPerBlock waves)

__global__ __launch_bounds__(kWave *kRowsPerBlock) void pack512_kernel(const float *__restrict__ src, int64_t ld,
                                                                       int64_t m, uint32_t *__restrict__ slots)
{
    constexpr int R = kPack512RowsPerWave;
    __shared__ __attribute__((aligned(16))) uint32_t image_all[kRowsPerBlock * R * 128];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r0 = ((int64_t)blockIdx.x * kRowsPerBlock + wave) * R;
    if (r0 >= m) return;
    const int nr = (int)(m - r0 < R ? m - r0 : R);           // wave-uniform
    const int q = lane >> 4, i = lane & 15;
    uint32_t *image = image_all + wave * (R * 128);
    uint4 v[R];
#pragma unroll
    for (int k = 0; k < R; ++k)    // (rows past m: the last row again, loaded and not stored)
        v[k] = *(const uint4 *)(src + (r0 + (k < nr ? k : nr - 1)) * ld + 16 * i + 4 * q);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t x[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        uint32_t nib = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) nib |= (x[j] != 0u ? 1u : 0u) << j;
        const uint32_t lo = or16(i < 8 ? nib << (4 * i) : 0u), hi = or16(i >= 8 ? nib << (4 * (i - 8)) : 0u);
        const unsigned long long mask = ((unsigned long long)hi << 32) | lo;
        int rank = __builtin_popcountll(mask & ((1ull << (4 * i)) - 1ull));
        uint32_t *sub = image + k * 128 + 32 * q;
        if (i < 3) sub[i] = i == 0 ? lo : i == 1 ? hi : (uint32_t)__builtin_popcountll(mask);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((nib >> j) & 1u) {
                if (rank < kPack512Cap) sub[3 + rank] = x[j];
                ++rank;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (k < nr) {
            const uint2 w = *(const uint2 *)(image + k * 128 + 2 * lane);
            *(uint2 *)(slots + (r0 + k) * 128 + 2 * lane) = w;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// POOLED 384-byte form (gcn_spmm_csr_packed384; the format: include/gcn_spmm.h): 96 words per row — the four masks
// in words 0..7, the header in word 8 (running quarter counts in bytes 0..2, min(total, 255) in byte 3), ONE pool of
// values from word 9 on, quarter after quarter.  pack512_kernel's structure: rows per wave with their 16-byte loads
// first, the masks by DPP OR, a value at its rank in a wave-private LDS image, wavefront-scope fences only.  A
// value's rank is where its quarter begins in the pool — the counts of the quarters before it, exchanged through
// v_readlane of lanes 0, 16, 32 (wave-uniform) — plus its rank inside the quarter.  The image leaves as 384
// contiguous bytes: 8 bytes per lane on lanes 0..47, three whole lines.  Ranks from 87 on are not written (the row
// is overflowed: its value words are undefined), so nothing is written past word 95.
constexpr int kPack384Cap = GCN_PACK384_CAPACITY;
constexpr int kPack384Words = 96;
static_assert(9 + kPack384Cap == kPack384Words, "masks + header + pool fill the slot");
#ifndef GCN_PACK384_ROWS_PER_WAVE
#define GCN_PACK384_ROWS_PER_WAVE 2
#endif
constexpr int kPack384RowsPerWave = GCN_PACK384_ROWS_PER_WAVE;
constexpr int kPack384RowsPerBlock = kRowsPerBlock * kPack384RowsPerWave;

__global__ __launch_bounds__(kWave *kRowsPerBlock) void pack384_kernel(const float *__restrict__ src, int64_t ld,
                                                                       int64_t m, uint32_t *__restrict__ slots)
{
    constexpr int R = kPack384RowsPerWave;
    __shared__ __attribute__((aligned(16))) uint32_t image_all[kRowsPerBlock * R * kPack384Words];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r0 = ((int64_t)blockIdx.x * kRowsPerBlock + wave) * R;
    if (r0 >= m) return;
    const int nr = (int)(m - r0 < R ? m - r0 : R);           // wave-uniform
    const int q = lane >> 4, i = lane & 15;
    uint32_t *image = image_all + wave * (R * kPack384Words);
    uint4 v[R];
#pragma unroll
    for (int k = 0; k < R; ++k)    // (rows past m: the last row again, loaded and not stored)
        v[k] = *(const uint4 *)(src + (r0 + (k < nr ? k : nr - 1)) * ld + 16 * i + 4 * q);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t x[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        uint32_t nib = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) nib |= (x[j] != 0u ? 1u : 0u) << j;
        const uint32_t lo = or16(i < 8 ? nib << (4 * i) : 0u), hi = or16(i >= 8 ? nib << (4 * (i - 8)) : 0u);
        const unsigned long long mask = ((unsigned long long)hi << 32) | lo;
        const int cq = __builtin_popcountll(mask);
        const uint32_t s1 = (uint32_t)__builtin_amdgcn_readlane(cq, 0);            // c0
        const uint32_t s2 = s1 + (uint32_t)__builtin_amdgcn_readlane(cq, 16);      // c0 + c1
        const uint32_t s3 = s2 + (uint32_t)__builtin_amdgcn_readlane(cq, 32);      // c0 + c1 + c2  (<= 192)
        const uint32_t total = s3 + (uint32_t)__builtin_amdgcn_readlane(cq, 48);
        const uint32_t header = s1 | (s2 << 8) | (s3 << 16) | ((total < 255u ? total : 255u) << 24);
        int rank = (int)(q == 0 ? 0u : q == 1 ? s1 : q == 2 ? s2 : s3)
                   + __builtin_popcountll(mask & ((1ull << (4 * i)) - 1ull));
        uint32_t *img = image + k * kPack384Words;
        if (i < 2) img[2 * q + i] = i == 0 ? lo : hi;
        if (lane == 2) img[8] = header;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((nib >> j) & 1u) {
                if (rank < kPack384Cap) img[9 + rank] = x[j];
                ++rank;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < kPack384Words / 2) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (k < nr) {
                const uint2 w = *(const uint2 *)(image + k * kPack384Words + 2 * lane);
                *(uint2 *)(slots + (r0 + k) * kPack384Words + 2 * lane) = w;
            }
        }
    }
}

int check(const char *who, int dtype, int64_t m, int64_t F, int64_t ld)
{
    if (dtype != GCN_DTYPE_F32 && dtype != GCN_DTYPE_BF16) return gcn_internal_fail(GCN_E_BADARG, who);
    if (m < 0 || F <= 0 || F % 32 != 0 || F > INT32_MAX || ld < F || ld % 4 != 0)
        return gcn_internal_fail(GCN_E_BADARG, who);
    return 0;
}

}   // namespace

extern "C" {

int gcn_rows_pack_count(int dtype, const void *src, int64_t ld, const int64_t *rows, int64_t m, int64_t F,
                        uint32_t *bits, int32_t *counts, void *stream)
{
    if (int rc = check("gcn_rows_pack_count: bad dtype / sizes (F a multiple of 32, ld a multiple of 4)", dtype, m, F, ld))
        return rc;
    if (m == 0) return 0;
    if (src == nullptr || bits == nullptr || counts == nullptr)
        return gcn_internal_fail(GCN_E_BADARG, "gcn_rows_pack_count: NULL pointer");
    if (((uintptr_t)src) % 16 != 0) return gcn_internal_fail(GCN_E_ALIGN, "gcn_rows_pack_count: 16-byte alignment required");
    const dim3 grid((unsigned)((m + kRowsPerBlock - 1) / kRowsPerBlock)), block(kWave * kRowsPerBlock);
    hipStream_t s = (hipStream_t)stream;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(pack_count_kernel<T>, grid, block, 0, s, (const T *)src, ld, rows, m, (int)F, bits, counts);
    });
    return launched("gcn_rows_pack_count launch");
}

int gcn_rows_pack_values(int dtype, const void *src, int64_t ld, const int64_t *rows, int64_t m, int64_t F,
                         const int64_t *offsets, void *vals, void *stream)
{
    if (int rc = check("gcn_rows_pack_values: bad dtype / sizes (F a multiple of 32, ld a multiple of 4)", dtype, m, F, ld))
        return rc;
    if (m == 0) return 0;
    if (src == nullptr || offsets == nullptr || vals == nullptr)
        return gcn_internal_fail(GCN_E_BADARG, "gcn_rows_pack_values: NULL pointer");
    if (((uintptr_t)src) % 16 != 0) return gcn_internal_fail(GCN_E_ALIGN, "gcn_rows_pack_values: 16-byte alignment required");
    const dim3 grid((unsigned)((m + kRowsPerBlock - 1) / kRowsPerBlock)), block(kWave * kRowsPerBlock);
    hipStream_t s = (hipStream_t)stream;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(pack_values_kernel<T>, grid, block, 0, s, (const T *)src, ld, rows, m, (int)F, offsets, (T
                           *)vals);
    });
    return launched("gcn_rows_pack_values launch");
}

int gcn_rows_unpack(int dtype, const uint32_t *bits, const int64_t *offsets, const void *vals, int64_t m,
                    int64_t F, void *dst, int64_t ldd, void *stream)
{
    if (int rc = check("gcn_rows_unpack: bad dtype / sizes (F a multiple of 32, ldd a multiple of 4)", dtype, m, F, ldd))
        return rc;
    if (m == 0) return 0;
    if (bits == nullptr || offsets == nullptr || dst == nullptr)
        return gcn_internal_fail(GCN_E_BADARG, "gcn_rows_unpack: NULL pointer");
    if (((uintptr_t)dst) % 16 != 0) return gcn_internal_fail(GCN_E_ALIGN, "gcn_rows_unpack: 16-byte alignment required");
    const dim3 grid((unsigned)((m + kRowsPerBlock - 1) / kRowsPerBlock)), block(kWave * kRowsPerBlock);
    hipStream_t s = (hipStream_t)stream;
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(unpack_kernel<T>, grid, block, 0, s, bits, offsets, (const T *)vals, m, (int)F, (T *)dst,
                           ldd);
    });
    return launched("gcn_rows_unpack launch");
}

int gcn_rows_pack512(const float *src, int64_t ld, int64_t m, uint32_t *slots, void *stream)
{
    if (m < 0 || ld < 256 || ld % 4 != 0) return gcn_internal_fail(GCN_E_BADARG, "gcn_rows_pack512: bad sizes (256 columns, ld a multiple of 4)");
    if (m == 0) return 0;
    if (src == nullptr || slots == nullptr) return gcn_internal_fail(GCN_E_BADARG, "gcn_rows_pack512: NULL pointer");
    if ((((uintptr_t)src) | ((uintptr_t)slots)) % 16 != 0)
        return gcn_internal_fail(GCN_E_ALIGN, "gcn_rows_pack512: 16-byte alignment required");
    const int64_t blocks = (m + kPack512RowsPerBlock - 1) / kPack512RowsPerBlock;
    if (blocks > INT32_MAX) return gcn_internal_fail(GCN_E_BADARG, "gcn_rows_pack512: too many rows");
    const dim3 grid((unsigned)blocks), block(kWave * kRowsPerBlock);
    hipLaunchKernelGGL(pack512_kernel, grid, block, 0, (hipStream_t)stream, src, ld, m, slots);
    return launched("gcn_rows_pack512 launch");
}

int gcn_rows_pack384(const float *src, int64_t ld, int64_t m, uint32_t *slots, void *stream)
{
    if (m < 0 || ld < 256 || ld % 4 != 0) return gcn_internal_fail(GCN_E_BADARG, "gcn_rows_pack384: bad sizes (256 columns, ld a multiple of 4)");
    if (m == 0) return 0;
    if (src == nullptr || slots == nullptr) return gcn_internal_fail(GCN_E_BADARG, "gcn_rows_pack384: NULL pointer");
    if ((((uintptr_t)src) | ((uintptr_t)slots)) % 16 != 0)
        return gcn_internal_fail(GCN_E_ALIGN, "gcn_rows_pack384: 16-byte alignment required");
    const int64_t blocks = (m + kPack384RowsPerBlock - 1) / kPack384RowsPerBlock;
    if (blocks > INT32_MAX) return gcn_internal_fail(GCN_E_BADARG, "gcn_rows_pack384: too many rows");
    const dim3 grid((unsigned)blocks), block(kWave * kRowsPerBlock);
    hipLaunchKernelGGL(pack384_kernel, grid, block, 0, (hipStream_t)stream, src, ld, m, slots);
    return launched("gcn_rows_pack384 launch");
}

int gcn_bits_row_counts(const uint32_t *bits, int64_t m, int64_t words, int32_t *counts, void *stream)
{
    if (m < 0 || words <= 0 || words > (1 << 20))
        return gcn_internal_fail(GCN_E_BADARG, "gcn_bits_row_counts: bad sizes");
    if (m == 0) return 0;
    if (bits == nullptr || counts == nullptr) return gcn_internal_fail(GCN_E_BADARG, "gcn_bits_row_counts: NULL pointer");
    const dim3 grid((unsigned)((m * 8 + 255) / 256)), block(256);
    hipLaunchKernelGGL(bits_count_kernel, grid, block, 0, (hipStream_t)stream, bits, m, (int)words, counts);
    return launched("gcn_bits_row_counts launch");
}

}   // extern "C"
