// gcn_internal.h — what two or more of the .hip files of this directory need, written once.  Internal: it is
// not installed, and every name in it has internal linkage (static, the anonymous namespace, __forceinline__),
// so the shared library's symbol table does not know that it exists.  Each .hip file includes it after
// gcn_spmm.h.  The rule: a helper that a SECOND .hip file needs moves here; what one file uses stays in it.
#ifndef GCN_INTERNAL_H
#define GCN_INTERNAL_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "gcn_spmm.h"

// ================================================================================================
// host side
// ================================================================================================
// error reporting (one gcn_last_error() for the whole library): defined in gcn_error.hip, with the thread-local
// message buffer
int gcn_internal_fail(int code, const char *msg);
int gcn_internal_fail_hip(int hip_error, const char *where);

// keep-threshold of the fused dropout: an element is kept iff its 16-bit field >= round(p * 2^16),
// clamped to [1, 65535] for p > 0 (0 = dropout off) — include/gcn_spmm.h, struct gcn_epilogue
static inline uint32_t gcn_dropout_threshold16(float p)
{
    if (!(p > 0.f)) return 0u;
    const double t = (double)p * 65536.0 + 0.5;
    return (uint32_t)std::min(65535.0, std::max(1.0, (double)(int64_t)t));
}
// the scale that goes with that threshold: the kernels keep an element with probability
// (65536 - T) / 65536, so 65536 / (65536 - T) — not 1 / (1 - p) of the unquantised p — makes
// E[dropout(x)] = x exactly (the two agree to 2^-17 away from the clamps, and exactly at p = 1/2)
static inline float gcn_dropout_scale16(uint32_t thresh)
{
    return thresh == 0u ? 1.f : 65536.f / (float)(65536u - thresh);
}

namespace {

typedef uint16_t bf16_t;                 // raw bf16 bits

constexpr int kWave = 64;                // lanes of a wavefront; the most rows a row-batch item of the plan holds

// "<who>: <what>" as the library's last error; returns code
[[maybe_unused]] int bad(const char *who, int code, const char *what)
{
    char msg[200];
    std::snprintf(msg, sizeof msg, "%s: %s", who, what);
    return gcn_internal_fail(code, msg);
}

// the end of an entry point that launched kernels: 0, or the launch error as "<who>: <hip's text>"
[[maybe_unused]] int launched(const char *who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gcn_internal_fail_hip((int)e, who);
}
// the same behind host calls that return their own status: an earlier error `e` is the one reported
[[maybe_unused]] int launched(const char *who, hipError_t e)
{
    if (e == hipSuccess) e = hipGetLastError();
    return e == hipSuccess ? 0 : gcn_internal_fail_hip((int)e, who);
}

// ------------------------------------------------------------------------------------------------
// shape rules that more than one file's sweeps share
// ------------------------------------------------------------------------------------------------
constexpr int64_t kMaxBatch = 65535;     // windows / sample groups ride on gridDim.y
constexpr int64_t kSlabBlocks = 2048;    // slabs of rows = partial rows of a full-height sweep

// elements per 16-byte lane (Lane<T>::V on the device side)
[[maybe_unused]] int64_t lane_elems(int dtype) { return dtype == GCN_DTYPE_BF16 ? 8 : 4; }

// a row of F elements as 16-byte lanes, F / width of them dividing a 256-thread block
[[maybe_unused]] bool lane_width_ok(int64_t F, int dtype)
{
    if (dtype != GCN_DTYPE_F32 && dtype != GCN_DTYPE_BF16) return false;
    const int64_t v = lane_elems(dtype);
    return F >= v && F <= 256 * v && (F % v) == 0 && (256 % (F / v)) == 0;
}

// n_rows >= 1 rows as at most kSlabBlocks contiguous slabs, of 64 rows at least, one per block
struct RowSlabs {
    int64_t blocks;
    int rows_per_block;
    explicit RowSlabs(int64_t n_rows)
    {
        blocks = std::min<int64_t>((n_rows + 63) / 64, kSlabBlocks);
        rows_per_block = (int)((n_rows + blocks - 1) / blocks);
    }
};

// the same in whole tiles of `tile` rows: `slabs` = min(tiles, kSlabBlocks) is what a workspace is sized by
struct TileSlabs {
    int64_t slabs;
    int rows_per_block;
    TileSlabs(int64_t n_rows, int64_t tile)
    {
        slabs = std::min<int64_t>((n_rows + tile - 1) / tile, kSlabBlocks);
        rows_per_block = (int)((n_rows + tile * slabs - 1) / (tile * slabs)) * (int)tile;
    }
};

// ------------------------------------------------------------------------------------------------
// THE PICKS: how an entry point turns a run-time argument into a template argument.  The callable gets the choice
// as a value whose TYPE carries it (a generic lambda reads it back with `typename decltype(t)::type` or
// `decltype(v)::value`), so a launch is written once and only the instantiations some branch names exist.
// A kernel's template-id with a comma in it goes in parentheses inside hipLaunchKernelGGL.
// ------------------------------------------------------------------------------------------------
template <typename T> struct TypeTag { typedef T type; };

// f(TypeTag<float>) for GCN_DTYPE_F32, f(TypeTag<bf16_t>) otherwise (the caller has checked dtype)
template <typename F> auto pick_dtype(int dtype, F &&f)
{
    if (dtype == GCN_DTYPE_F32) return f(TypeTag<float>{});
    return f(TypeTag<bf16_t>{});
}
// f(TypeTag<int64_t>) or f(TypeTag<int32_t>): the width of a CSR row pointer
template <typename F> auto pick_index(bool is64, F &&f)
{
    if (is64) return f(TypeTag<int64_t>{});
    return f(TypeTag<int32_t>{});
}
// f(std::integral_constant<int, V>) for the V of the list that equals v; false, and no call, when none does
template <int... Vs, typename F> bool pick_int(int v, F &&f)
{
    return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// ================================================================================================
// device side
// ================================================================================================
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi)
{
    f32x2 v = {lo, hi};
    bf16x2 b = __builtin_convertvector(v, bf16x2);   // v_cvt_pk_bf16_f32, round-to-nearest-even
    return __builtin_bit_cast(uint32_t, b);
}

// 16 bytes of a row, one lane's share of a wave-wide access, <-> V fp32 registers
template <typename T> struct Lane;
template <> struct Lane<float> {
    static constexpr int V = 4;
    typedef f32x4 Raw;
    static __device__ __forceinline__ void unpack(const Raw &r, float (&x)[4])
    {
        x[0] = r.x; x[1] = r.y; x[2] = r.z; x[3] = r.w;
    }
    static __device__ __forceinline__ Raw pack(const float (&x)[4])
    {
        Raw r = {x[0], x[1], x[2], x[3]};
        return r;
    }
};
template <> struct Lane<bf16_t> {
    static constexpr int V = 8;
    typedef u32x4 Raw;
    static __device__ __forceinline__ void unpack(const Raw &r, float (&x)[8])
    {
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = __uint_as_float(w[i] << 16);
            x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ Raw pack(const float (&x)[8])
    {
        Raw r = {pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]),
                 pack_bf16x2(x[6], x[7])};
        return r;
    }
};

// Elem<T, VEC>: how VEC elements of T travel between memory and fp32 registers.  The 16-byte forms are Lane<T>; the
// scalar forms serve the kernels that also take rows no 16-byte lane fits (gcn_spmm.hip, gcn_backward.hip)
template <typename T, int VEC> struct Elem;
template <> struct Elem<float, 4> : Lane<float> {};
template <> struct Elem<bf16_t, 8> : Lane<bf16_t> {};
template <> struct Elem<float, 1> {
    typedef float Raw;
    static __device__ __forceinline__ void unpack(const Raw &r, float (&x)[1]) { x[0] = r; }
    static __device__ __forceinline__ Raw pack(const float (&x)[1]) { return x[0]; }
};
template <> struct Elem<bf16_t, 1> {
    typedef bf16_t Raw;
    static __device__ __forceinline__ void unpack(const Raw &r, float (&x)[1])
    {
        x[0] = __uint_as_float(((uint32_t)r) << 16);
    }
    static __device__ __forceinline__ Raw pack(const float (&x)[1])
    {
        return (bf16_t)(pack_bf16x2(x[0], 0.f) & 0xffffu);
    }
};

// four consecutive elements of a row <-> four floats (8-byte aligned at bf16, 16-byte at fp32).  Two stores:
// store_rounded rounds fp32 to bf16 (nearest even); store_exact takes the upper halves, for values that ARE
// bf16 numbers already.  At fp32 the two are the same store.
template <typename T> struct Run4;
template <> struct Run4<float> {
    static __device__ __forceinline__ void load(const float *p, float (&x)[4])
    {
        const float4 v = *(const float4 *)p;
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    }
    static __device__ __forceinline__ void store_rounded(float *p, const float (&x)[4])
    {
        *(float4 *)p = make_float4(x[0], x[1], x[2], x[3]);
    }
    static __device__ __forceinline__ void store_exact(float *p, const float (&x)[4]) { store_rounded(p, x); }
};
template <> struct Run4<bf16_t> {
    static __device__ __forceinline__ void load(const bf16_t *p, float (&x)[4])
    {
        const uint2 v = *(const uint2 *)p;
        x[0] = __uint_as_float(v.x << 16); x[1] = __uint_as_float(v.x & 0xffff0000u);
        x[2] = __uint_as_float(v.y << 16); x[3] = __uint_as_float(v.y & 0xffff0000u);
    }
    static __device__ __forceinline__ void store_rounded(bf16_t *p, const float (&x)[4])
    {
        uint2 v;
        v.x = pack_bf16x2(x[0], x[1]);
        v.y = pack_bf16x2(x[2], x[3]);
        *(uint2 *)p = v;
    }
    static __device__ __forceinline__ void store_exact(bf16_t *p, const float (&x)[4])
    {
        uint2 v;
        v.x = (__float_as_uint(x[0]) >> 16) | (__float_as_uint(x[1]) & 0xffff0000u);
        v.y = (__float_as_uint(x[2]) >> 16) | (__float_as_uint(x[3]) & 0xffff0000u);
        *(uint2 *)p = v;
    }
};

// torch.relu: NaN stays NaN (fmaxf would drop it)
__device__ __forceinline__ float act(float z, int relu) { return (relu && z < 0.f) ? 0.f : z; }

// a / D for 0 <= a < 2^13 and 1 <= D <= 2^13 given r = 1.0f / D: (a + 0.5) / D is at least 1 / (2 D) away from
// an integer and the fp32 evaluation is within 2^-22 * a / D of it — the truncation is exact
__device__ __forceinline__ int fdiv(int a, float r) { return (int)(((float)a + 0.5f) * r); }

// THE SELECTION ORDER on fp32 (include/gcn_spmm.h, "Vertex selection"; gcn_select, gcn_dense): -0 is +0, every NaN is
// above +inf, otherwise numeric.  order_key() is the uint32 with that order: negatives have all bits flipped,
// non-negatives the sign bit set, NaN is 0xFFFFFFFF.
__device__ __forceinline__ uint32_t order_key(float f)
{
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;       // NaN, any sign or payload
    if (u == 0x80000000u) u = 0u;                                  // -0 is +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the canonical float of a key: NaN is 0x7FC00000, zero is +0
__device__ __forceinline__ float key_float(uint32_t t)
{
    if (t == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((t & 0x80000000u) ? (t & 0x7fffffffu) : ~t);
}

// One DPP row operation CTRL on a register: a VALU modifier, no trip through the LDS crossbar and no address
// registers.  quad_perm [1,0,3,2] = 0xB1 and [2,3,0,1] = 0x4E are the xor-1 / xor-2 exchanges; after them a quad
// is uniform, so row_half_mirror = 0x141 (lane i <-> 7 - i) and row_mirror = 0x140 (i <-> 15 - i) act as
// xor 4 / xor 8.
template <int CTRL> __device__ __forceinline__ uint32_t dpp_move(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL> __device__ __forceinline__ float dpp_move(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// ------------------------------------------------------------------------------------------------
// THE KEEP FUNCTION of the dropout, and its generator.
//
// Philox4x32-10 (Salmon et al., SC'11): counter-based, so the dropout mask of element (row, f)
// depends only on (seed, row, f) — never on which kernel variant, vector width, wave or launch
// produced the row.  One call yields 128 bits = EIGHT 16-bit keep fields (ABI 22; before: four
// 32-bit words — half the integer multiplies per element now) — or, at p = 1/2 where one bit
// decides, 128 ONE-bit fields (ABI 23).  Element (row, f), 16-bit form:
//     block = ((f >> 4) << 1) | ((f >> 2) & 1)          counter word 2
//     field = (((f >> 3) & 1) << 2) | (f & 3)           0..7: word field >> 1, half field & 1
//     w     = philox(counter = (row_lo, row_hi, block, 0), key = seed)   (row incl. drop_row_base)
//     keep  = ((w[field >> 1] >> 16 * (field & 1)) & 0xFFFF) >= round(p * 65536)
// The block groups columns {16c + 4b + (0..3), 16c + 4b + 8 + (0..3)} (b = bit 2 of f): exactly the
// eight columns one lane of the MFMA GEMMs' transposed accumulator tile stores per 16-column
// group (gcn_gemm.hip), so the GEMM epilogues need ONE call per eight stored elements too.
// One-bit form, T = 32768 (p = 1/2, the reference's default):
//     block = ((f >> 8) << 1) | ((f >> 2) & 1),   index = (((f & 255) >> 3) << 2) | (f & 3)
//     keep  = (w[index >> 5] >> (index & 31)) & 1
// the same layout rule at a 256-column span: a lane of the GEMMs' transposed accumulator tile finds
// ALL its columns of a 256-wide row in one call (16 calls per tile before).
// Every kernel that draws the mask extracts its fields in its own lane order, from THIS generator.
//
// The two 32 x 32 -> 64 products of a round are written in one of two forms, which compile to different
// code — so the form is a parameter, and which form a kernel uses is that kernel's business:
//   kPhiloxMulPair   __umulhi + a low multiply per product (gcn_spmm, gcn_rows, gcn_select)
//   kPhiloxMulWide   one 32 x 32 -> 64 multiply per product — v_mad_u64_u32 — instead of a mul_hi +
//                    mul_lo pair: integer multiplies run at a quarter of the VALU rate and dominate
//                    the GEMM epilogues (gcn_gemm)
// The bits are the same.
// ------------------------------------------------------------------------------------------------
enum PhiloxMul { kPhiloxMulPair, kPhiloxMulWide };

template <PhiloxMul MUL>
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
    constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, lo0, hi1, lo1;
        if constexpr (MUL == kPhiloxMulWide) {
            const uint64_t p0 = (uint64_t)kM0 * (uint64_t)c0, p1 = (uint64_t)kM1 * (uint64_t)c2;
            hi0 = (uint32_t)(p0 >> 32); lo0 = (uint32_t)p0;
            hi1 = (uint32_t)(p1 >> 32); lo1 = (uint32_t)p1;
        } else {
            hi0 = __umulhi(kM0, c0); lo0 = kM0 * c0;
            hi1 = __umulhi(kM1, c2); lo1 = kM1 * c2;
        }
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}   // namespace

#endif   // GCN_INTERNAL_H
