// gcn_spmm.hip — CSR SpMM for the GraphConvolution hot path, written for gfx950 (MI355X, CDNA4).
//
// The sparse kernels over a gcn_csr_plan of the C-ABI of include/gcn_spmm.h: the forward product (gcn_spmm_csr*) and,
// at the end of the file and for a reason given there, the SDDMM.  The element-wise backward sweeps are
// gcn_backward.hip, the host planner and transpose gcn_host.hip, the error state gcn_error.hip.  (bench.py stamps
// its traffic figures with this file's hash: they describe the product's kernels.)
// What it replaces in the reference:
//   torch.spmm(adj, support)          pygcn/layers.py:34      -> gcn_spmm_csr on CSR(adj)
//   adj.t() @ grad_output (autograd)  pygcn/train.py:157      -> gcn_spmm_csr on CSR(adj^T)
//   output + self.bias                pygcn/layers.py:35-36   -> fused epilogue
//
// Execution model (see DESIGN.md §3 for the numbers):
//   * HBM-bound gather: every stored entry pulls one dense row B[col,:] (F*s bytes).  A 64-lane
//     wavefront reads one such row with ONE instruction (16 B per lane -> 1 KiB for fp32 F=256),
//     so all B traffic is full-line coalesced and the column index / value are wave-uniform
//     scalars (v_readlane from a 64-entry register tile, scalar address arithmetic).
//   * Latency is hidden by keeping D row-loads in flight per wave in a register ring that is
//     refilled as soon as a slot is consumed, times 8 waves per SIMD.
//   * Load balance on power-law graphs comes from the static schedule in gcn_csr_plan: short
//     rows are packed into equal-cost row-batch items (one wave each); rows longer than
//     long_thresh are cut into chunks summed by separate waves into an fp32 slab and added in
//     chunk order by a tiny second kernel — no float atomics, bitwise reproducible.
//   * Narrow feature widths (F*s < 1 KiB) put several stored entries of one row side by side in
//     one wave instruction (lane groups) and finish with a wavefront shuffle reduction.
//
// gfx950 only.  No other architecture is supported or intended.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <type_traits>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

constexpr int kWavesPerBlock = 4;

struct KParams {
    const void *rowptr;
    const int32_t *col;
    const float *val;
    const int32_t *items;
    const int32_t *chunk_row;
    const int64_t *chunk_e0;
    const int32_t *long_row;
    const int32_t *long_chunk0;
    const void *B;
    void *C;
    const float *bias;
    float *partial;
    int64_t ldb;   // elements
    int64_t ldc;   // elements
    int32_t F;
    int32_t n_total;    // n_chunks + n_items
    int32_t n_chunks;
    int32_t n_long;
    int32_t long_thresh;
    int32_t relu;
    uint32_t drop_thresh;   // keep an element iff its 16 random bits >= drop_thresh (0: no dropout)
    float drop_scale;       // 65536 / (65536 - drop_thresh): 1 / (1 - p) of the quantised p
    uint32_t seed_lo, seed_hi;
    int64_t drop_row_base;  // added to the row index in the dropout counter (a shard's first row)
    const void *B2;          // optional second block of B: rows >= b_split live here (ldb2)
    int64_t ldb2;
    int32_t b_split;         // INT32_MAX when B is one block
    const uint32_t *bflag;   // optional bitmap [ceil(n_cols/32)]: bit c clear = row c of B is all zero
    const int32_t *bnnz;     // optional device scalar: number of non-zero rows of B
    int32_t n_cols;
    uint8_t *cflag;          // optional output [n_rows], pre-zeroed: 1 = stored row has a non-zero
    int32_t log_softmax;     // store log_softmax of the row (whole row inside one store_out call)
    const uint64_t *seed_dev;   // optional device-resident dropout seed (overrides seed_lo/hi)
    const uint32_t *csel;       // optional bitmap over output rows: clear bit = row not wanted
    int32_t cskip;              // with cflag: all-zero rows are not stored
    uint32_t *cabsmax;          // optional output: max |stored value| as BITS (atomic max; inf / NaN sort on top)
    const void *packed;         // spmm_wide_packed_kernel: the slots of the rows of B (gcn_rows_pack512 / _pack384)
};

// Row flags of a row-sparse dense operand are used only when they can pay: a device-side count
// (no host synchronisation) says fewer than num/den of the rows are non-zero.  The wide kernel
// (1-KiB rows, cheap scalar compaction) gains up to 3/4; the narrow kernel's lane compaction only
// below 1/8 (measured at C5: 16 % non-zero rows = 80 % surviving entries ran 47 ms hinted against
// 41 ms dense, 5 % ran 18 ms).
__device__ __forceinline__ bool use_row_flags(const KParams &p, int num, int den)
{
    if (p.bflag == nullptr || p.bnnz == nullptr) return false;
    const int nz = __builtin_amdgcn_readfirstlane(*p.bnnz);
    return (int64_t)nz * den < (int64_t)p.n_cols * num;
}

__device__ __forceinline__ bool row_bit(const uint32_t *__restrict__ bits, int c)
{
    return (bits[c >> 5] >> (c & 31)) & 1u;
}

__device__ __forceinline__ int readlane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float readlane_f(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// the keep function (gcn_internal.h, above philox4x32_10) of VEC consecutive columns from f on:
// VEC = 1, or VEC and f multiples of 4
template <int VEC>
__device__ __forceinline__ void apply_dropout(const KParams &p, int64_t row, int f, float (&o)[VEC])
{
    uint32_t r[4];
    uint32_t k0 = p.seed_lo, k1 = p.seed_hi;
    if (p.seed_dev != nullptr) {   // wave-uniform scalar load: the seed as of execution time
        const uint64_t sd = *p.seed_dev;
        k0 = (uint32_t)sd;
        k1 = (uint32_t)(sd >> 32);
    }
    row += p.drop_row_base;
    if (p.drop_thresh == 32768u) {
        // p = 1/2 (the reference's default): the one-bit form, 128 fields per call
#pragma unroll
        for (int q = 0; q < (VEC + 3) / 4; ++q) {
            const int fq = f + 4 * q;
            const uint32_t blk = ((uint32_t)(fq >> 8) << 1) | ((uint32_t)(fq >> 2) & 1u);
            const int idx = (((fq & 255) >> 3) << 2) | (fq & 3);          // (VEC >= 4: fq & 3 == 0)
            philox4x32_10<kPhiloxMulPair>((uint32_t)row, (uint32_t)(row >> 32), blk, 0u, k0, k1, r);
            const int ws = idx >> 5;
            const uint32_t w = (ws & 2) ? ((ws & 1) ? r[3] : r[2]) : ((ws & 1) ? r[1] : r[0]);
            const uint32_t nib = w >> (idx & 31);
#pragma unroll
            for (int j = 0; j < (VEC == 1 ? 1 : 4); ++j)
                o[4 * q + j] = ((nib >> j) & 1u) ? o[4 * q + j] * p.drop_scale : 0.f;
        }
        return;
    }
    if (VEC == 1) {
        const uint32_t blk = ((uint32_t)(f >> 4) << 1) | ((uint32_t)(f >> 2) & 1u);
        const int fld = (((f >> 3) & 1) << 2) | (f & 3);
        philox4x32_10<kPhiloxMulPair>((uint32_t)row, (uint32_t)(row >> 32), blk, 0u, k0, k1, r);
        const uint32_t w = (fld & 4) ? ((fld & 2) ? r[3] : r[2]) : ((fld & 2) ? r[1] : r[0]);
        const uint32_t bits = (fld & 1) ? (w >> 16) : (w & 0xFFFFu);
        o[0] = (bits >= p.drop_thresh) ? o[0] * p.drop_scale : 0.f;
    } else {
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {       // 4 consecutive columns = fields 4s .. 4s+3 of one block
            const int fq = f + 4 * q;
            const uint32_t blk = ((uint32_t)(fq >> 4) << 1) | ((uint32_t)(fq >> 2) & 1u);
            philox4x32_10<kPhiloxMulPair>((uint32_t)row, (uint32_t)(row >> 32), blk, 0u, k0, k1, r);
            const bool hi = ((fq >> 3) & 1) != 0;
            const uint32_t w0 = hi ? r[2] : r[0], w1 = hi ? r[3] : r[1];
            o[4 * q + 0] = ((w0 & 0xFFFFu) >= p.drop_thresh) ? o[4 * q + 0] * p.drop_scale : 0.f;
            o[4 * q + 1] = ((w0 >> 16) >= p.drop_thresh) ? o[4 * q + 1] * p.drop_scale : 0.f;
            o[4 * q + 2] = ((w1 & 0xFFFFu) >= p.drop_thresh) ? o[4 * q + 2] * p.drop_scale : 0.f;
            o[4 * q + 3] = ((w1 >> 16) >= p.drop_thresh) ? o[4 * q + 3] * p.drop_scale : 0.f;
        }
    }
}

// xor-butterfly reductions inside groups of LPR consecutive lanes (LPR a power of two).  The first
// four steps are DPP row operations (dpp_move, gcn_internal.h): xor 1, 2, 4, 8.  max and + are
// commutative, so every lane of a group ends with the same bits.
// Wider groups finish with wave shuffles (ds_bpermute).
template <int LPR>
__device__ __forceinline__ float group_max(float m)
{
    if (LPR >= 2) m = fmaxf(m, dpp_move<0xB1>(m));
    if (LPR >= 4) m = fmaxf(m, dpp_move<0x4E>(m));
    if (LPR >= 8) m = fmaxf(m, dpp_move<0x141>(m));
    if (LPR >= 16) m = fmaxf(m, dpp_move<0x140>(m));
#pragma unroll
    for (int off = 16; off < LPR; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
    return m;
}

template <int LPR>
__device__ __forceinline__ float group_sum(float s)
{
    if (LPR >= 2) s += dpp_move<0xB1>(s);
    if (LPR >= 4) s += dpp_move<0x4E>(s);
    if (LPR >= 8) s += dpp_move<0x141>(s);
    if (LPR >= 16) s += dpp_move<0x140>(s);
#pragma unroll
    for (int off = 16; off < LPR; off <<= 1) s += __shfl_xor(s, off, kWave);
    return s;
}

// bias add + ReLU + dropout + conversion + store of one output row segment (VEC floats per lane)
// (a row is held by LPR consecutive lanes, VEC elements each, starting at a multiple of LPR)
// XEPI = 0 compiles the log_softmax / output-row-flag code out, 1 keeps log_softmax only (the last
// layer of every forward pass: without the row-flag code the bf16 narrow instantiation keeps 6
// waves per SIMD), 2 keeps both: the plain instantiations keep
// the register budget they were tuned with (wide fp32: 62 VGPRs; the extras cost 8-15 more)
// Returns (XEPI >= 2 with p.cabsmax set, else 0) the largest |stored value| of this lane as its bit
// pattern: callers keep a running maximum per lane and publish it once per wave (publish_absmax).
template <typename T, int VEC, int LPR, int XEPI, bool ALLOW_SKIP = true>
__device__ __forceinline__ uint32_t store_out(const KParams &p, int64_t row, int f, bool act,
                                              const float (&acc)[VEC], const float (&bias)[VEC])
{
    float o[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        o[i] = acc[i] + bias[i];
        if (p.relu) o[i] = fmaxf(o[i], 0.f);
    }
    if (p.drop_thresh != 0u) apply_dropout<VEC>(p, row, f, o);   // wave-uniform branch
    if (XEPI >= 1 && p.log_softmax) {   // wave-uniform; the host guarantees the whole row sits in these LPR lanes
        const bool valid = f < p.F;
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < VEC; ++i) m = valid ? fmaxf(m, o[i]) : m;
        m = group_max<LPR>(m);
        float se = 0.f;
#pragma unroll
        for (int i = 0; i < VEC; ++i) se += valid ? __expf(o[i] - m) : 0.f;   // arguments <= 0
        se = group_sum<LPR>(se);
        const float lse = m + __logf(se);   // se in [1, F]: hardware exp2 / log2, ~1e-7 absolute
#pragma unroll
        for (int i = 0; i < VEC; ++i) o[i] -= lse;
    }
    bool do_store = act;
    if (XEPI >= 2 && p.cflag != nullptr) {   // wave-uniform; every lane holding a non-zero stores the same byte
        bool nz = false;
#pragma unroll
        for (int i = 0; i < VEC; ++i) nz |= (o[i] != 0.f);
        if (ALLOW_SKIP && p.cskip) {
            // an all-zero row is not written at all: the decision must be the same for the LPR
            // lanes that hold the row -> their slice of the wave's ballot
            const unsigned long long b = __ballot(act && nz);
            const int ln = (int)(threadIdx.x & (kWave - 1));
            const unsigned long long gm =
                LPR >= kWave ? ~0ull : (((1ull << LPR) - 1ull) << (ln & ~(LPR - 1)));
            do_store = act && (b & gm) != 0ull;
        }
        if (act && nz) p.cflag[row] = 1;
    }
    if (do_store) {
        T *dst = (T *)p.C + row * p.ldc + f;
        *(typename Elem<T, VEC>::Raw *)dst = Elem<T, VEC>::pack(o);
    }
    uint32_t amax = 0u;
    if (XEPI >= 2 && p.cabsmax != nullptr && do_store) {   // (uniform pointer test)
        float st[VEC];                                       // the values as STORED (bf16: rounded)
        Elem<T, VEC>::unpack(Elem<T, VEC>::pack(o), st);
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (f + i < p.F) amax = max(amax, __float_as_uint(st[i]) & 0x7fffffffu);
    }
    return amax;
}

// One atomic per wave at most, and only when the wave's maximum beats the value already published
// (a plain load at the end of the wave's work: its latency hides nothing that matters).
template <int XEPI>
__device__ __forceinline__ void publish_absmax(const KParams &p, uint32_t amax)
{
    if (XEPI >= 2 && p.cabsmax != nullptr) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, off, kWave));
        if ((threadIdx.x & (kWave - 1)) == 0 && amax != 0u &&
            amax > __atomic_load_n(p.cabsmax, __ATOMIC_RELAXED))
            atomicMax(p.cabsmax, amax);
    }
}

// ------------------------------------------------------------------------------------------
// WIDE kernel: one dense row segment (64 lanes x VEC elements) per wave instruction.
// Used when F/VEC > 32 lanes; blockIdx.y walks further 64*VEC-wide feature slabs.
// ------------------------------------------------------------------------------------------
// 16-byte load of a dense-row segment through a buffer descriptor built from wave-uniform
// scalars: base = B + col*ldb (SGPR pair), num_records = row bytes.  The hardware range check
// returns zeros for lanes past the end of the row (feature tail) and for whole slots whose
// num_records is 0 (slots past the end of an edge tile), so the gather needs no branches.
// (Default cache policy: non-temporal loads and stores were measured and dropped)
__device__ __forceinline__ u32x4 row_load16(uint64_t base, uint32_t nbytes, uint32_t voff)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    void *pb = (void *)(((uint64_t)hi << 32) | lo);
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(pb, 0, nbytes, 0x00020000);
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0);
}

template <typename T, int VEC, int D, bool ROWS, bool FLAGS, int XEPI>
__device__ __forceinline__ void wide_stream(const KParams &p, const int32_t *__restrict__ colp,
                                            const float *__restrict__ valp, int ne, int lane,
                                            unsigned ld_off_bytes, float (&acc)[VEC],
                                            int rel_end, int nr, int64_t row0, int f, bool act,
                                            const float (&bias)[VEC], uint32_t &amax)
{
    typedef typename Elem<T, VEC>::Raw Raw;
    static_assert(sizeof(Raw) == 16, "wide kernel moves 16 bytes per lane");
    const uint32_t ldb_bytes = (uint32_t)(p.ldb * (int64_t)sizeof(T));   // < 4 GiB, host-checked
    const uint32_t ldb2_bytes = (uint32_t)(p.ldb2 * (int64_t)sizeof(T));
    const uint32_t row_bytes = (uint32_t)p.F * (uint32_t)sizeof(T);
    // row c of the dense operand: in B below the split, in B2 (rebased) from the split on; all
    // scalar arithmetic (the sharded path keeps a rank's own rows and its halo rows apart)
    auto row_base = [&](int c) -> uint64_t {
        return c < p.b_split ? (uint64_t)p.B + (uint64_t)(uint32_t)c * ldb_bytes
                             : (uint64_t)p.B2 + (uint64_t)(uint32_t)(c - p.b_split) * ldb2_bytes;
    };
    int r = 0;
    int rend = ROWS ? readlane_i(rel_end, 0) : INT_MAX;
    const bool flags = FLAGS && use_row_flags(p, 3, 4);   // wave-uniform; FLAGS = false: dense operand,
                                                    // the flag code is compiled out
    const bool sel = FLAGS && ROWS && p.csel != nullptr;  // output-row selection (wave-uniform)
    // lane l < nr: is row row0 + l wanted
    const int want = (sel && lane < nr) ? (int)row_bit(p.csel, (int)row0 + lane) : 1;
    auto emit = [&](int rr) {   // store row rr of the item unless the caller does not want it
        if (!sel || readlane_i(want, rr))
            amax = max(amax, store_out<T, VEC, kWave, XEPI>(p, row0 + rr, f, act, acc, bias));
    };
    auto consume = [&](int e, const u32x4 &raw, float a) {
        if (ROWS) {
            while (e >= rend) {   // row finished (loop: rows without stored entries follow)
                emit(r);
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
                ++r;
                rend = readlane_i(rel_end, r);
            }
        }
        float x[VEC];
        Elem<T, VEC>::unpack(__builtin_bit_cast(Raw, raw), x);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = fmaf(a, x[i], acc[i]);
    };

    for (int t = 0; t < ne; t += kWave) {
        const int cnt = min(kWave, ne - t);
        int cv = 0;
        float vv = 0.f;   // lanes >= cnt keep value 0: slots past the tile add 0 * 0
        if (lane < cnt) {
            cv = colp[t + lane];
            vv = valp[t + lane];
        }
        // row-sparse operand: one byte gather per tile tells which of the 64 rows are all-zero;
        // their slots get num_records = 0 like the slots past the end of the tile (no traffic)
        if (FLAGS && (flags || sel)) {
            // row-sparse operand: one bitmap probe per lane tells which of the tile's rows of B are
            // all-zero; only the stored entries whose bit is set are visited (ascending order, so
            // the row bookkeeping of consume() is unchanged), D at a time
            int fv = (lane < cnt) ? 1 : 0;
            if (flags) fv = fv && row_bit(p.bflag, cv);
            if (sel) {
                // output-row selection: the row of entry i = t + lane is the first r with
                // rel_end[r] > i (binary search over the row ends held in lanes 0..nr-1); entries
                // of rows the caller does not want are not visited either
                const int i = t + lane;
                int lo = 0, hi = nr - 1;
#pragma unroll
                for (int s = 0; s < 6; ++s) {
                    const int mid = (lo + hi) >> 1;
                    const int v = __shfl(rel_end, mid, kWave);
                    if (v > i) hi = mid; else lo = min(mid + 1, nr - 1);
                }
                // (the shuffle must run in ALL lanes: a lane switched off by a short-circuit would
                //  supply 0 to the lanes that read it)
                const int w = __shfl(want, lo, kWave);
                fv &= w;
            }
            unsigned long long m = __ballot(fv != 0);
            while (m) {
                int kk[D];
                u32x4 x[D];
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    kk[j] = m ? (int)__builtin_ctzll(m) : -1;
                    m &= m - 1;   // (0 stays 0)
                    const int c = readlane_i(cv, kk[j] < 0 ? 0 : kk[j]);
                    x[j] = row_load16(row_base(c), kk[j] >= 0 ? row_bytes : 0u, ld_off_bytes);
                }
#pragma unroll
                for (int j = 0; j < D; ++j)
                    if (kk[j] >= 0) consume(t + kk[j], x[j], readlane_f(vv, kk[j]));
            }
            continue;
        }
        for (int k = 0; k < cnt; k += D) {
            // D row loads in flight, branch-free
            u32x4 x[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const bool ok = k + j < cnt;
                const int c = readlane_i(cv, k + j);   // k + j <= 63 always (k <= 56)
                x[j] = row_load16(row_base(c), ok ? row_bytes : 0u, ld_off_bytes);
            }
#pragma unroll
            for (int j = 0; j < D; ++j)
                consume(min(t + k + j, ne - 1), x[j], readlane_f(vv, k + j));
        }
    }
    if (ROWS) {
        while (r < nr) {   // last row of the item and any trailing empty rows
            emit(r);
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
            ++r;
        }
    }
}

template <typename T, int VEC, typename IdxT, int D, bool FLAGS, int XEPI>
__global__ __launch_bounds__(kWave *kWavesPerBlock) void spmm_wide_kernel(KParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int item =
        blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= p.n_total) return;
    const int f = blockIdx.y * (kWave * VEC) + lane * VEC;
    const bool act = f < p.F;
    // lanes past the end of the row (F not a multiple of 64*VEC) are zeroed by the range check
    const unsigned ld_off_bytes = (unsigned)f * (unsigned)sizeof(T);
    const IdxT *__restrict__ rp = (const IdxT *)p.rowptr;

    float acc[VEC], bias[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        acc[i] = 0.f;
        bias[i] = 0.f;
    }

    if (item < p.n_chunks) {
        // ---- one chunk of a long row -> fp32 partial slab
        const int row = p.chunk_row[item];
        if (FLAGS && p.csel != nullptr && !row_bit(p.csel, row)) return;   // long row not wanted
        const int64_t e0 = p.chunk_e0[item];
        const int64_t e1 = min(e0 + (int64_t)p.long_thresh, (int64_t)rp[row + 1]);
        uint32_t unused = 0u;
        wide_stream<T, VEC, D, false, FLAGS, XEPI>(p, p.col + e0, p.val + e0, (int)(e1 - e0), lane,
                                      ld_off_bytes, acc, 0, 0, 0, f, act, bias, unused);
        if (act) {
            float *dst = p.partial + (int64_t)item * p.F + f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) dst[i] = acc[i];
        }
        return;
    }

    // ---- a row-batch item: rows [ra, rb), <= 64 rows, contiguous stored entries
    const int it = item - p.n_chunks;
    const int ra = p.items[2 * it], rb = p.items[2 * it + 1];
    const int nr = rb - ra;
    const int64_t ea = (int64_t)rp[ra];
    const int rel_end = (lane < nr) ? (int)((int64_t)rp[ra + 1 + lane] - ea) : 0;
    const int ne = readlane_i(rel_end, nr - 1);
    if (p.bias != nullptr && act) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) bias[i] = p.bias[f + i];
    }
    uint32_t amax = 0u;
    wide_stream<T, VEC, D, true, FLAGS, XEPI>(p, p.col + ea, p.val + ea, ne, lane, ld_off_bytes, acc, rel_end,
                                 nr, (int64_t)ra, f, act, bias, amax);
    publish_absmax<XEPI>(p, amax);
}

// ------------------------------------------------------------------------------------------
// WIDE kernel on PACKED rows (gcn_spmm_csr_packed): the 256-wide fp32 operand is gathered from the 512-byte
// slots of gcn_rows_pack512 (gcn_pack.hip: four 128-byte sub-slots, one per column quarter: 64-bit mask,
// count, non-zero values in bit order) — half the bytes of a dense row per stored entry.
//   * per stored entry ONE 8-byte buffer load per lane at the lane-static offset 8 * lane: lane (q, i) =
//     (lane >> 4, lane & 15) holds words 2i, 2i + 1 of sub-slot q; the ladder is that of wide_stream (D loads in
//     flight, no branch, a slot past the tile has num_records 0 and reads zeros = an empty mask);
//   * lane (q, i) OWNS columns 16 i + 4 q .. + 3 = bits 4i .. 4i + 3 of its quarter.  The loaded 8 bytes per lane
//     are STAGED in a wave-private LDS copy of the slot (one ds_write_b64 per lane; D copies per wave, one per
//     load in flight): the mask is then a broadcast read of words 0, 1 of the sub-slot, and the lane's up to four
//     values are the consecutive words w0 .. w0 + 3, w0 = 3 + popcount(mask below bit 4i) — one computed address
//     and fixed offsets — handed out by the nibble (v_bfe_i32 bit masks, v_and / v_bfi: nothing goes through VCC).
//     The D copies are written; then the masks are read four entries at a time and the values two entries at a
//     time (what 72 registers leave room for): LDS latency is paid per group, never per entry.
//     Only the wave's own lanes touch its copies, so wavefront-scope fences order them: there is NO workgroup
//     barrier in this kernel (waves of a block run different trip counts and return early);
//   * LDS image of a copy (kStageWords): sub-slot q starts at word 42 q + 6 (q & 1) = 0, 48, 84, 132 — 36 words
//     each, because a lane of a full quarter reads up to word 35 (selected away), and the two quarters that share
//     a 32-lane half of a ds_read_b32 sit 16 banks apart (their value words run over the same range of ranks);
//   * the same fmaf per (entry, column) in the same order as the dense launch — a cleared bit contributes
//     fmaf(a, 0, acc) as the dense zero does — so the result is bit-identical;
//   * an entry whose slot reports an overflowed quarter (count > 29; wave-uniform test on the loaded words)
//     takes its four values from the dense row instead, in place: the order of the sum does not change.
//   * the POOLED 384-byte slots of gcn_rows_pack384 (gcn_spmm_csr_packed384) go through the same code with another
//     slot geometry (SlotGeom below): three lines per entry instead of four, one pool of values, the lane's first
//     word 9 + prefix(q) + popcount(mask below bit 4i).  The nibble queue and the fmaf order are the same;
// Row bookkeeping, long-row chunks (fp32 partial slab, spmm_long_reduce_kernel) and the store are wide_stream's;
// only the column a lane owns differs (the store is still 16 bytes per lane, one full row per wave).
// ------------------------------------------------------------------------------------------
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u32x2 slot_load8(uint64_t base, uint32_t nbytes, uint32_t voff)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    void *pb = (void *)(((uint64_t)hi << 32) | lo);
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(pb, 0, nbytes, 0x00020000);
    return __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, 0, 0);
}

// THE SLOT GEOMETRY: all that differs between the two fixed-slot formats (include/gcn_spmm.h), as the compile-time
// parameter of packed_stream and spmm_wide_packed_kernel.  Lane (q, i) = (lane >> 4, lane & 15) throughout.
//   kBytes       a slot in memory; the load is 8 bytes per lane at 8 * lane, lanes from kLanes on are past
//                num_records and read zeros without traffic
//   kStageWords  the LDS image of one staged slot; own_word: where a lane stages its 8 bytes; mask_word: the
//                quarter's 64-bit mask; pool_word: word 0 of the values the lane's ranks count from
//   kTailWords   behind the last wave's last copy: how far a DISCARDED read may reach past a copy (below)
template <int BYTES> struct SlotGeom;
// 512: four sub-slots (mask, count, 29 values).  Image: sub-slots at 0, 48, 84, 132, 36 words each (see above).  An
// OVERFLOWED quarter (its values come from the dense row) may have all 64 bits set: its lanes' discarded reads reach
// word 3 + 60 + 3 of the sub-slot, 31 words past the copy — into the wave's next copy, the next wave's, or the tail.
template <> struct SlotGeom<512> {
    static constexpr int kBytes = 512, kLanes = 64, kStageWords = 168, kTailWords = 32;
    static constexpr uint32_t kCap = GCN_PACK512_CAPACITY;
    static constexpr bool kPooled = false;
    static __device__ __forceinline__ int mask_word(int q) { return 42 * q + 6 * (q & 1); }
    static __device__ __forceinline__ int own_word(int q, int i) { return mask_word(q) + 2 * i; }
    static __device__ __forceinline__ int pool_word(int q) { return mask_word(q) + 3; }
};
// 384: masks in words 0..7, header in word 8, ONE pool of 87 values from word 9.  The image is the slot as it is in
// words 0..95; the copy is SIZED at 128 words so that lanes 48..63, which hold zeros, stage them in words 96..127 of
// their own copy and the ds_write_b64 needs no mask (a masked write compiled to a branch per staged slot).  The place
// of a lane's first value is 9 + prefix(q) + popcount(mask_q below bit 4 i), prefix(q) = byte q - 1 of the header (0
// for q = 0).  The two quarters of a 32-lane half read consecutive runs of the pool, so the 512 form's bank offset
// has no counterpart.  Discarded reads: a row that fits reads up to word 9 + 87 + 2 = 98; an OVERFLOWED row with
// all 256 bits set computes 9 + 252 and reads up to word 264 — 137 words past its copy.  The tail is SIZED for that
// (no clamp: a clamp is one more VALU per entry), and whatever is read there is selected away bit by bit (expand).
template <> struct SlotGeom<384> {
    static constexpr int kBytes = 384, kLanes = 48, kStageWords = 128, kTailWords = 9 + 252 + 4 - 128;
    static constexpr uint32_t kCap = GCN_PACK384_CAPACITY;
    static constexpr bool kPooled = true;
    static __device__ __forceinline__ int mask_word(int q) { return 2 * q; }
    static __device__ __forceinline__ int own_word(int q, int i) { return 2 * (16 * q + i); }
    static __device__ __forceinline__ int pool_word(int) { return 9; }
};
template <typename G, int D> constexpr int stage_block_words() { return kWavesPerBlock * D * G::kStageWords + G::kTailWords; }

// Orders this wave's LDS writes and reads of its own copies (no other wave touches them): compiler fences of
// wavefront scope, no instruction and no workgroup barrier.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename G, int D, bool ROWS>
__device__ __forceinline__ void packed_stream(const KParams &p, uint32_t *stage, const int32_t *__restrict__ colp,
                                              const float *__restrict__ valp, int ne, int lane, float (&acc)[4],
                                              int rel_end, int nr, int64_t row0, int f, const float (&bias)[4])
{
    const int q = lane >> 4, i = lane & 15;
    const uint32_t ldb_bytes = (uint32_t)(p.ldb * 4);                    // the dense rows (overflowed slots)
    const uint32_t voff = (uint32_t)lane * 8u;
    // lane-static: this lane's sub-slot in a staged copy and its own two words there; which mask word holds its
    // nibble and where; the bits below its nibble in either mask word
    uint32_t *const sub = stage + G::mask_word(q);        // the quarter's mask in a staged copy
    uint32_t *const mine = stage + G::own_word(q, i);
    uint32_t *const pool = stage + G::pool_word(q);       // word 0 of the values the lane's ranks count from
    const bool upper = i >= 8;
    const uint32_t sh = 4u * (uint32_t)(i & 7);
    const uint32_t below_lo = upper ? ~0u : (1u << sh) - 1u, below_hi = upper ? (1u << sh) - 1u : 0u;
    const bool cnt_lane = i == 1;                         // (512) loads words 2, 3 of its sub-slot: .x is the count
    // (384) where the lane's quarter begins in the pool: bits [pre_off, pre_off + pre_len) of the header word —
    // byte q - 1, and no bits at all (v_bfe_u32 of width 0 = 0) for quarter 0
    const uint32_t pre_off = q > 0 ? 8u * (uint32_t)(q - 1) : 0u, pre_len = q > 0 ? 8u : 0u;
    int r = 0;
    int rend = ROWS ? readlane_i(rel_end, 0) : INT_MAX;
    // store row rr of the item and start the next one
    auto emit = [&](int rr) {
        store_out<float, 4, kWave, 0>(p, row0 + rr, f, true, acc, bias);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = 0.f;
    };
    // the lane's four columns of a staged slot: `nibs` = its mask word from its nibble on, v = the words
    // w0 .. w0 + 3 of its sub-slot.  Bit by bit of the nibble, "take the head of the queue if the bit is set" — a
    // cleared bit leaves +0.0.  b[k] is all ones or zero (v_bfe_i32 of one bit), a select is v_bfi, a take v_and:
    // 15 instructions, none through VCC.  (v_bfi by name: written as and / or, the selects come back as compares,
    // v_cndmask and twice the instructions.)
    auto expand = [](uint32_t nibs, const uint32_t (&v)[4], float (&x)[4]) {
        uint32_t b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = (uint32_t)__builtin_amdgcn_sbfe((int)nibs, (uint32_t)k, 1u);
        auto sel = [](uint32_t m, uint32_t yes, uint32_t no) {
            uint32_t d;
            asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "v"(m), "v"(yes), "v"(no));
            return d;
        };
        uint32_t q0 = v[0], q1 = v[1], q2 = v[2];
        x[0] = __uint_as_float(q0 & b[0]);
        q0 = sel(b[0], q1, q0); q1 = sel(b[0], q2, q1); q2 = sel(b[0], v[3], q2);
        x[1] = __uint_as_float(q0 & b[1]);
        q0 = sel(b[1], q1, q0); q1 = sel(b[1], q2, q1);
        x[2] = __uint_as_float(q0 & b[2]);
        q0 = sel(b[2], q1, q0);
        x[3] = __uint_as_float(q0 & b[3]);
    };
    // entry e with value a and the lane's four columns x of the gathered row; `over`: the slot overflowed
    // (wave-uniform), column c's dense row stands in
    auto consume = [&](int e, float (&x)[4], bool over, float a, int c) {
        if (ROWS) {
            while (e >= rend) {   // row finished (loop: rows without stored entries follow)
                emit(r);
                ++r;
                rend = readlane_i(rel_end, r);
            }
        }
        if (over) {                                  // wave-uniform and rare: a quarter did not fit its sub-slot
            const u32x4 d = row_load16((uint64_t)p.B + (uint64_t)(uint32_t)c * ldb_bytes, 1024u, (uint32_t)f * 4u);
            Elem<float, 4>::unpack(__builtin_bit_cast(f32x4, d), x);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(a, x[k], acc[k]);
    };

    for (int t = 0; t < ne; t += kWave) {
        const int cnt = min(kWave, ne - t);
        int cv = 0;
        float vv = 0.f;   // lanes >= cnt keep value 0: slots past the tile add 0 * 0
        if (lane < cnt) {
            cv = colp[t + lane];
            vv = valp[t + lane];
        }
        for (int k = 0; k < cnt; k += D) {
            u32x2 x[D];
            int cc[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const bool ok = k + j < cnt;
                cc[j] = readlane_i(cv, k + j);   // k + j <= 63 always (k <= 56)
                x[j] = slot_load8((uint64_t)p.packed + (uint64_t)(uint32_t)cc[j] * (uint64_t)G::kBytes,
                                  ok ? (uint32_t)G::kBytes : 0u, voff);
            }
            // stage the D slots (the previous group's reads come first).  512: one test per group tells whether any of
            // them overflowed (the largest count word: .x of lane 1 of a quarter).  384: the header word is .x of lane
            // 4; v_readlane makes it wave-uniform, so "overflowed" is one scalar compare per entry (byte 3 is the
            // total: total > 87 <=> header >= 88 << 24) with no ballot and no test per group, and the prefixes below
            // are cut from the same scalar register
            wave_sync();
            uint32_t top = 0u, hdr[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                *(u32x2 *)(mine + j * G::kStageWords) = x[j];
                if constexpr (G::kPooled) hdr[j] = (uint32_t)__builtin_amdgcn_readlane((int)x[j].x, 4);
                else top = max(top, x[j].x);
            }
            bool any_over = true;
            if constexpr (!G::kPooled) any_over = __ballot(cnt_lane && top > G::kCap) != 0ull;
            wave_sync();
            // kMaskGroup masks at a time -> per entry the lane's nibble and the place of its first value; then,
            // kValueGroup entries at a time, the value words and the arithmetic.  (The group sizes are what 72
            // registers = 7 waves per SIMD leave room for: LDS latency is paid per group, not per entry.)
            constexpr int kMaskGroup = 4, kValueGroup = 2;
            static_assert(D % kMaskGroup == 0 && kMaskGroup % kValueGroup == 0, "groups");
#pragma unroll
            for (int g0 = 0; g0 < D; g0 += kMaskGroup) {
                uint32_t nibs[kMaskGroup];
                const uint32_t *first[kMaskGroup];
                u32x2 h[kMaskGroup];
                wave_sync();        // (keeps these reads behind the previous group's arithmetic)
#pragma unroll
                for (int j = 0; j < kMaskGroup; ++j) h[j] = *(const u32x2 *)(sub + (g0 + j) * G::kStageWords);
#pragma unroll
                for (int j = 0; j < kMaskGroup; ++j) {
                    nibs[j] = (upper ? h[j].y : h[j].x) >> sh;
                    int w0;
                    if constexpr (G::kPooled) {      // (the prefix rides in the first v_bcnt's addend, the first sum
                        w0 = (int)__builtin_amdgcn_ubfe(hdr[g0 + j], pre_off, pre_len);     //  in the second's)
                        asm("" : "+v"(w0));
                        w0 += __builtin_popcount(h[j].x & below_lo);
                        asm("" : "+v"(w0));
                        w0 += __builtin_popcount(h[j].y & below_hi);
                    } else {
                        w0 = __builtin_popcount(h[j].x & below_lo) + __builtin_popcount(h[j].y & below_hi);
                    }
                    asm("" : "+v"(w0));      // (keeps the sum in v_bcnt's addend: the scaling by 4 comes after)
                    first[j] = pool + (g0 + j) * G::kStageWords + w0;        // (over: see SlotGeom::kTailWords)
                }
#pragma unroll
                for (int g = 0; g < kMaskGroup; g += kValueGroup) {
                    uint32_t v[kValueGroup][4];
                    float xs[kValueGroup][4];
                    wave_sync();    // (keeps these reads behind the previous group's arithmetic)
#pragma unroll
                    for (int j = 0; j < kValueGroup; ++j)
#pragma unroll
                        for (int w = 0; w < 4; ++w) v[j][w] = first[g + j][w];
#pragma unroll
                    for (int j = 0; j < kValueGroup; ++j) expand(nibs[g + j], v[j], xs[j]);
#pragma unroll
                    for (int j = 0; j < kValueGroup; ++j) {
                        const int e = g0 + g + j;                            // the entry's place among the D
                        bool over;
                        if constexpr (G::kPooled) over = hdr[e] >= ((G::kCap + 1u) << 24);
                        else over = any_over && __ballot(sub[e * G::kStageWords + 2] > G::kCap) != 0ull;
                        consume(min(t + k + e, ne - 1), xs[j], over, readlane_f(vv, k + e), cc[e]);
                    }
                }
            }
        }
    }
    if (ROWS) {
        while (r < nr) {   // last row of the item and any trailing empty rows
            emit(r);
            ++r;
        }
    }
}

template <typename IdxT, int D, int SLOT>
__global__ __launch_bounds__(kWave *kWavesPerBlock) __attribute__((amdgpu_waves_per_eu(7, 8)))
void spmm_wide_packed_kernel(KParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int item =
        blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= p.n_total) return;
    const int f = 16 * (lane & 15) + 4 * (lane >> 4);          // (F = 256: every lane holds four columns)
    const IdxT *__restrict__ rp = (const IdxT *)p.rowptr;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, bias[4] = {0.f, 0.f, 0.f, 0.f};
    // D staged slot copies per wave, private to it (packed_stream; no __syncthreads anywhere below)
    typedef SlotGeom<SLOT> G;
    __shared__ __attribute__((aligned(16))) uint32_t stage_all[stage_block_words<G, D>()];
    uint32_t *stage = stage_all + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (D * G::kStageWords);

    if (item < p.n_chunks) {
        // ---- one chunk of a long row -> fp32 partial slab
        const int row = p.chunk_row[item];
        const int64_t e0 = p.chunk_e0[item];
        const int64_t e1 = min(e0 + (int64_t)p.long_thresh, (int64_t)rp[row + 1]);
        packed_stream<G, D, false>(p, stage, p.col + e0, p.val + e0, (int)(e1 - e0), lane, acc, 0, 0, 0, f, bias);
        float *dst = p.partial + (int64_t)item * p.F + f;
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = acc[k];
        return;
    }
    // ---- a row-batch item: rows [ra, rb), <= 64 rows, contiguous stored entries
    const int it = item - p.n_chunks;
    const int ra = p.items[2 * it], rb = p.items[2 * it + 1];
    const int nr = rb - ra;
    const int64_t ea = (int64_t)rp[ra];
    const int rel_end = (lane < nr) ? (int)((int64_t)rp[ra + 1 + lane] - ea) : 0;
    const int ne = readlane_i(rel_end, nr - 1);
    if (p.bias != nullptr) {
#pragma unroll
        for (int k = 0; k < 4; ++k) bias[k] = p.bias[f + k];
    }
    packed_stream<G, D, true>(p, stage, p.col + ea, p.val + ea, ne, lane, acc, rel_end, nr, (int64_t)ra, f, bias);
}

// ------------------------------------------------------------------------------------------
// NARROW kernel: a dense row segment needs only LPR (< 64, or 64 with scalar elements) lanes,
// so G = 64/LPR stored entries of the SAME output row travel side by side in one wave
// instruction; the G partial sums meet in a wavefront shuffle reduction.
// ------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ const char *narrow_row_ptr(const KParams &p, int c)
{
    return c < p.b_split ? (const char *)p.B + (int64_t)c * (p.ldb * (int64_t)sizeof(T))
                         : (const char *)p.B2 + (int64_t)(c - p.b_split) * (p.ldb2 * (int64_t)sizeof(T));
}

template <typename T, int VEC, int LPR, int U>
__device__ __forceinline__ void narrow_row(const KParams &p, const int32_t *__restrict__ col,
                                           const float *__restrict__ val, int64_t e0, int64_t e1,
                                           int g, unsigned ld_off, float (&acc)[VEC],
                                           bool flags = false)
{
    typedef typename Elem<T, VEC>::Raw Raw;
    constexpr int G = kWave / LPR;
    if (flags) {
        // Row-sparse dense operand: per 64-entry tile probe the row bitmap once per lane, move the
        // surviving entries to the front of the wave (a full lane permutation: survivors keep
        // their order in [0, nv), the rest go behind), then split ONLY the survivors over the G
        // lane groups.  Skipped entries cost neither a bitmap-dependent stall per entry nor a load.
        const int lane = (int)(threadIdx.x & (kWave - 1));
        for (int64_t t = e0; t < e1; t += kWave) {
            const int cnt = (int)min((int64_t)kWave, e1 - t);
            int c = 0;
            float a = 0.f;
            bool keep = false;
            if (lane < cnt) {
                c = col[t + lane];
                a = val[t + lane];
                keep = row_bit(p.bflag, c);
            }
            const unsigned long long m = __ballot(keep);
            const int nv = __builtin_popcountll(m);
            if (nv == 0) continue;   // wave-uniform
            const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            const int dest = keep ? below : nv + (lane - below);   // a permutation of 0..63
            const int cc = __builtin_amdgcn_ds_permute(dest << 2, c);
            const float aa = __int_as_float(__builtin_amdgcn_ds_permute(dest << 2, __float_as_int(a)));
            for (int k = 0; k < nv; k += G * U) {   // uniform trip count
                Raw x[U];
                float w[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int idx = k + u * G + g;
                    const bool ok = idx < nv;
                    const int ck = __shfl(cc, idx & (kWave - 1), kWave);
                    const float ak = __shfl(aa, idx & (kWave - 1), kWave);
                    w[u] = ok ? ak : 0.f;
                    Raw z = {};
                    x[u] = z;
                    if (ok) x[u] = *(const Raw *)(narrow_row_ptr<T>(p, ck) + ld_off);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {   // unloaded slots hold zeros with weight 0: exact
                    float xf[VEC];
                    Elem<T, VEC>::unpack(x[u], xf);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[i] = fmaf(w[u], xf[i], acc[i]);
                }
            }
        }
    } else
    for (int64_t e = e0; e < e1; e += (int64_t)G * U) {   // uniform trip count
        int c[U];
        float a[U];
        Raw x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t ee = e + (int64_t)u * G + g;
            const bool ok = ee < e1;
            c[u] = ok ? col[ee] : 0;
            a[u] = ok ? val[ee] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // entries past the end of the row point at row 0 (a harmless cached read); their
            // products are skipped below, so non-finite values there cannot leak in
            x[u] = *(const Raw *)(narrow_row_ptr<T>(p, c[u]) + ld_off);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t ee = e + (int64_t)u * G + g;
            if (ee < e1) {
                float xf[VEC];
                Elem<T, VEC>::unpack(x[u], xf);
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = fmaf(a[u], xf[i], acc[i]);
            }
        }
    }
    if (G > 1) {
#pragma unroll
        for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off, kWave);
        }
    }
}

template <typename T, int VEC, int LPR, typename IdxT, int XEPI>
__global__ __launch_bounds__(kWave *kWavesPerBlock) void spmm_narrow_kernel(KParams p)
{
    constexpr int U = 4;
    const int lane = threadIdx.x & (kWave - 1);
    const int item =
        blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= p.n_total) return;
    const int g = lane / LPR, l = lane % LPR;
    const int f = blockIdx.y * (LPR * VEC) + l * VEC;
    const bool act = f < p.F;
    const unsigned ld_off = act ? (unsigned)f * (unsigned)sizeof(T) : 0u;
    const IdxT *__restrict__ rp = (const IdxT *)p.rowptr;
    const bool flags = use_row_flags(p, 1, 8);   // wave-uniform

    float acc[VEC], bias[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        acc[i] = 0.f;
        bias[i] = 0.f;
    }

    const bool sel = p.csel != nullptr;   // output-row selection (wave-uniform)
    uint32_t amax = 0u;                   // running max |stored value| of this lane (see store_out)
    if (item < p.n_chunks) {
        const int row = p.chunk_row[item];
        if (sel && !row_bit(p.csel, row)) return;   // long row not wanted
        const int64_t e0 = p.chunk_e0[item];
        const int64_t e1 = min(e0 + (int64_t)p.long_thresh, (int64_t)rp[row + 1]);
        narrow_row<T, VEC, LPR, U>(p, p.col, p.val, e0, e1, g, ld_off, acc, flags);
        if (act && g == 0) {
            float *dst = p.partial + (int64_t)item * p.F + f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) dst[i] = acc[i];
        }
        return;
    }

    const int it = item - p.n_chunks;
    const int ra = p.items[2 * it], rb = p.items[2 * it + 1];
    const int nr = rb - ra;
    if (p.bias != nullptr && act) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) bias[i] = p.bias[f + i];
    }
    constexpr int G = kWave / LPR;
    const int64_t ea = (int64_t)rp[ra];
    const int rel_end = (lane < nr) ? (int)((int64_t)rp[ra + 1 + lane] - ea) : 0;
    const int ne = readlane_i(rel_end, nr - 1);

    if (G == 1 || nr == 1 || ne > kWave) {
        // one row at a time, its stored entries split over the G lane groups
        int64_t e0 = ea;
        for (int r = ra; r < rb; ++r) {
            const int64_t e1 = (int64_t)rp[r + 1];
            if (sel && !row_bit(p.csel, r)) {   // row not wanted: neither computed nor stored
                e0 = e1;
                continue;
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
            narrow_row<T, VEC, LPR, U>(p, p.col, p.val, e0, e1, g, ld_off, acc, flags);
            amax = max(amax, store_out<T, VEC, LPR, XEPI>(p, (int64_t)r, f, act && g == 0, acc, bias));
            e0 = e1;
        }
        publish_absmax<XEPI>(p, amax);
        return;
    }

    // ---- row-per-group: each lane group owns a different SHORT row of the item, so G*RU rows
    // are in flight for the accumulator cost of RU rows and no cross-lane reduction is needed.
    // Row ends and the (col, val) tile of the item (<= 64 entries) sit in lanes and are read
    // with ds_bpermute: no dependent memory round trip per row.
    typedef typename Elem<T, VEC>::Raw Raw;
    // (tuned on MI355X, C4 graph: RU 2 / UU 2 / kShort 8 beat 1,3,4 / 1,4 / 4,16,32)
    constexpr int RU = 2;                     // rounds in flight
    constexpr int UU = 2;                     // entries per row per step
    constexpr int kShort = 8;                 // rows longer than this take the edge-split path
    const int64_t ldb_bytes = p.ldb * (int64_t)sizeof(T);
    int cv = 0;
    float vv = 0.f;
    if (lane < ne) {
        cv = p.col[ea + lane];
        vv = p.val[ea + lane];
        if (flags && !row_bit(p.bflag, cv)) vv = 0.f, cv = -1;   // all-zero row of B: skip its gather
    }
    const int up = __shfl_up(rel_end, 1, kWave);
    const int rel_start = (lane == 0) ? 0 : up;
    // lane r < nr: is row ra + r wanted by the caller (c_row_select)
    const int wantn = (sel && lane < nr) ? (int)row_bit(p.csel, ra + lane) : 1;
    unsigned long long medium = __ballot(lane < nr && rel_end - rel_start > kShort && wantn != 0);

    for (int q0 = 0; q0 < nr; q0 += G * RU) {
        int e0[RU], e1[RU], row[RU];
        float a2[RU][VEC];
#pragma unroll
        for (int ru = 0; ru < RU; ++ru) {
            const int r = q0 + ru * G + g;
            const int s0 = __shfl(rel_start, r & (kWave - 1), kWave);
            const int s1 = __shfl(rel_end, r & (kWave - 1), kWave);
            const int wr = __shfl(wantn, r & (kWave - 1), kWave);   // (all lanes run the shuffle)
            const bool mine = r < nr && s1 - s0 <= kShort && wr != 0;
            row[ru] = mine ? r : -1;
            e0[ru] = s0;
            e1[ru] = mine ? s1 : s0;
#pragma unroll
            for (int i = 0; i < VEC; ++i) a2[ru][i] = 0.f;
        }
        for (int j = 0; j < kShort; j += UU) {
            bool more = false;
#pragma unroll
            for (int ru = 0; ru < RU; ++ru) more |= (e0[ru] + j < e1[ru]);
            if (!__any(more)) break;
            Raw x[RU][UU];
            float av[RU][UU];
#pragma unroll
            for (int ru = 0; ru < RU; ++ru) {
#pragma unroll
                for (int u = 0; u < UU; ++u) {
                    const int idx = e0[ru] + j + u;
                    const int c = __shfl(cv, idx & (kWave - 1), kWave);
                    const bool ok = idx < e1[ru] && c >= 0;
                    const float a = __shfl(vv, idx & (kWave - 1), kWave);
                    av[ru][u] = ok ? a : 0.f;
                    Raw z = {};
                    x[ru][u] = z;
                    if (ok)
                        x[ru][u] = *(const Raw *)(narrow_row_ptr<T>(p, c) + ld_off);
                }
            }
#pragma unroll
            for (int ru = 0; ru < RU; ++ru) {
#pragma unroll
                for (int u = 0; u < UU; ++u) {
                    // slots that were not loaded hold zeros with weight 0: adding them is exact
                    float xf[VEC];
                    Elem<T, VEC>::unpack(x[ru][u], xf);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) a2[ru][i] = fmaf(av[ru][u], xf[i], a2[ru][i]);
                }
            }
        }
#pragma unroll
        for (int ru = 0; ru < RU; ++ru) {
            if (row[ru] >= 0)
                amax = max(amax, store_out<T, VEC, LPR, XEPI>(p, (int64_t)(ra + row[ru]), f, act, a2[ru], bias));
        }
    }

    // ---- the item's medium rows (kShort < entries <= long_thresh): entries split over the
    // lane groups, wavefront shuffle reduction
    while (medium) {
        const int rr = __builtin_ctzll(medium);
        medium &= medium - 1;
        const int s0 = readlane_i(rel_start, rr), s1 = readlane_i(rel_end, rr);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
        narrow_row<T, VEC, LPR, U>(p, p.col, p.val, ea + s0, ea + s1, g, ld_off, acc, flags);
        amax = max(amax, store_out<T, VEC, LPR, XEPI>(p, (int64_t)(ra + rr), f, act && g == 0, acc, bias));
    }
    publish_absmax<XEPI>(p, amax);
}

// ------------------------------------------------------------------------------------------
// long rows: add the chunk partials in chunk order, apply the epilogue, write the row
// ------------------------------------------------------------------------------------------
// Sum of column f over the chunk partials c0 .. c1-1 of one long row: SIXTEEN independent running
// sums — sixteen loads in flight per thread — combined in a fixed order: the result depends only
// on (c0, c1), never on scheduling.  (One running sum made every load wait for the previous add:
// a hub row of config C5 has > 1 000 chunks, and the serial chain of L2 round trips of that ONE
// row set the kernel's time, 1.0-1.7 ms per launch.)
__device__ __forceinline__ float long_row_sum(const float *__restrict__ partial, int F, int f, int c0, int c1)
{
    float s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = 0.f;
    int c = c0;
    for (; c + 16 <= c1; c += 16) {
#pragma unroll
        for (int k = 0; k < 16; ++k) s[k] += partial[(int64_t)(c + k) * F + f];
    }
#pragma unroll
    for (int k = 0; k < 15; ++k)
        if (c + k < c1) s[k] += partial[(int64_t)(c + k) * F + f];
    return (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))) +
           (((s[8] + s[9]) + (s[10] + s[11])) + ((s[12] + s[13]) + (s[14] + s[15])));
}

// ONE WAVE per long row, four rows per workgroup: config C5 has 7.4e5 long rows of 4.5 chunks on
// average (long_thresh 256), and a 256-thread workgroup per row — half of its threads idle at
// F = 128 — made the launch dispatch-bound (1.1 ms for 1.7 GB of partials).  A lane owns the
// columns lane, lane + 64, ...: one chunk row is a coalesced 256-byte read per pass.
template <typename T>
__global__ __launch_bounds__(256) void spmm_long_reduce_kernel(KParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int j = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= p.n_long) return;
    const int64_t row = p.long_row[j];
    if (p.csel != nullptr && !row_bit(p.csel, (int)row)) return;   // (its chunks were skipped too)
    const int c0 = p.long_chunk0[j], c1 = p.long_chunk0[j + 1];
    uint32_t amax = 0u;
    if (p.log_softmax) {
        // F <= 512 (host check): the lane owns columns lane + 64k, k < 8; wave-wide max and sum
        // (8-byte loads of column pairs were measured: no faster — the launch is bound by its
        //  dependent index loads per row, not by the width of the partial reads)
        auto col = [&](int k) { return lane + kWave * k; };
        float z[8], m = -INFINITY;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int f = col(k);
            z[k] = -INFINITY;
            if (f < p.F) z[k] = long_row_sum(p.partial, p.F, f, c0, c1) + (p.bias ? p.bias[f] : 0.f);
            m = fmaxf(m, z[k]);
        }
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) se += (col(k) < p.F) ? expf(z[k] - m) : 0.f;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) se += __shfl_xor(se, off, kWave);
        const float lse = m + logf(se);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int f = col(k);
            if (f < p.F) {
                const float o[1] = {z[k] - lse};
                ((T *)p.C)[row * p.ldc + f] = Elem<T, 1>::pack(o);
                if (p.cflag != nullptr && o[0] != 0.f) p.cflag[row] = 1;
                float st[1];
                Elem<T, 1>::unpack(Elem<T, 1>::pack(o), st);
                amax = max(amax, __float_as_uint(st[0]) & 0x7fffffffu);
            }
        }
        publish_absmax<2>(p, amax);
        return;
    }
    for (int f = lane; f < p.F; f += kWave) {
        const float s = long_row_sum(p.partial, p.F, f, c0, c1);
        float a[1] = {s};
        float b[1] = {p.bias ? p.bias[f] : 0.f};
        amax = max(amax, store_out<T, 1, 1, 2, false>(p, row, f, true, a, b));   // long rows: always stored
    }
    publish_absmax<2>(p, amax);
}

// ------------------------------------------------------------------------------------------
// host-side dispatch
// ------------------------------------------------------------------------------------------
// XEPI, the extras of a store: 2 = row flags / maximum (log_softmax or not), 1 = log_softmax alone, 0 = none.
// LPR = lpr for the powers of two below 64, and 64 for anything else.
template <typename T, int VEC>
void launch_narrow(const KParams &kp, bool is64, int lpr, dim3 grid, hipStream_t s)
{
    const dim3 block(kWave * kWavesPerBlock);
    const int xepi = (kp.cflag != nullptr || kp.cabsmax != nullptr) ? 2 : (kp.log_softmax ? 1 : 0);
    auto go = [&](auto l) {
        pick_int<0, 1, 2>(xepi, [&](auto x) {
            pick_index(is64, [&](auto i) {
                hipLaunchKernelGGL((spmm_narrow_kernel<T, VEC, decltype(l)::value, typename decltype(i)::type,
                                                       decltype(x)::value>),
                                   grid, block, 0, s, kp);
            });
        });
    };
    if (!pick_int<1, 2, 4, 8, 16, 32>(lpr, go)) go(std::integral_constant<int, 64>{});
}

// FLAGS = operand hint / row selection.  It has no log_softmax-alone form (XEPI 1): there log_softmax takes the
// full-extras instantiation.  Without FLAGS, XEPI 1 is the last layer of every forward pass: log_softmax without
// the row-flag / maximum code.
template <typename T, int VEC>
void launch_wide(const KParams &kp, bool is64, dim3 grid, hipStream_t s)
{
    constexpr int D = 8;
    const dim3 block(kWave * kWavesPerBlock);
    const bool flags = kp.bflag != nullptr || kp.csel != nullptr;
    const bool extras = kp.cflag != nullptr || kp.cabsmax != nullptr;
    const int xepi = (extras || (flags && kp.log_softmax)) ? 2 : (kp.log_softmax ? 1 : 0);
    auto go = [&](auto fl, auto x) {
        pick_index(is64, [&](auto i) {
            hipLaunchKernelGGL((spmm_wide_kernel<T, VEC, typename decltype(i)::type, D, decltype(fl)::value,
                                                 decltype(x)::value>),
                               grid, block, 0, s, kp);
        });
    };
    if (flags) pick_int<0, 2>(xepi, [&](auto x) { go(std::true_type{}, x); });
    else pick_int<0, 1, 2>(xepi, [&](auto x) { go(std::false_type{}, x); });
}

int next_pow2(int v)
{
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

template <typename T, int VECW>
int spmm_typed(const gcn_csr_plan *plan, KParams &kp, hipStream_t s, int slot_bytes)
{
    const int F = kp.F;
    const bool is64 = plan->rowptr_is64 != 0;
    const bool vec_ok = (F % VECW == 0) && (((uintptr_t)kp.B) % 16 == 0) &&
                        (((uintptr_t)kp.B2) % 16 == 0) &&
                        ((kp.ldb2 * (int64_t)sizeof(T)) % 16 == 0) &&
                        (((uintptr_t)kp.C) % 16 == 0) &&
                        ((kp.ldb * (int64_t)sizeof(T)) % 16 == 0) &&
                        ((kp.ldc * (int64_t)sizeof(T)) % 16 == 0);
    const unsigned nblk = (unsigned)((kp.n_total + kWavesPerBlock - 1) / kWavesPerBlock);
    // skipping all-zero rows is a per-store decision: only when one store call holds the whole row
    if (kp.cskip && !(F <= kWave || (vec_ok && F / VECW <= kWave))) kp.cskip = 0;
    if (kp.log_softmax && !(F <= kWave || (vec_ok && F / VECW <= kWave)))
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "log_softmax needs the row inside one wavefront "
                                  "(F <= 64, or 16-byte aligned operands with F/lane width <= 64)");
    if (kp.n_total > 0) {
        if (kp.packed != nullptr) {
            if constexpr (sizeof(T) == 4) {      // (fp32, F = 256, aligned: gcn_spmm_csr_packed checked)
                const dim3 grid(nblk, 1), block(kWave * kWavesPerBlock);
                pick_int<512, 384>(slot_bytes, [&](auto g) {
                    pick_index(is64, [&](auto i) {
                        hipLaunchKernelGGL((spmm_wide_packed_kernel<typename decltype(i)::type, 8, decltype(g)::value>),
                                           grid, block, 0, s, kp);
                    });
                });
            }
        } else if (vec_ok) {
            const int lanes = F / VECW;
            if (lanes > 32) {
                dim3 grid(nblk, (unsigned)((lanes + kWave - 1) / kWave));
                launch_wide<T, VECW>(kp, is64, grid, s);
            } else {
                dim3 grid(nblk, 1);
                launch_narrow<T, VECW>(kp, is64, next_pow2(lanes), grid, s);
            }
        } else {
            const int lpr = std::min(kWave, next_pow2(F));
            dim3 grid(nblk, (unsigned)((F + lpr - 1) / lpr));
            launch_narrow<T, 1>(kp, is64, lpr, grid, s);
        }
        if (int rc = launched("spmm launch")) return rc;
    }
    if (kp.n_long > 0) {
        hipLaunchKernelGGL((spmm_long_reduce_kernel<T>), dim3((unsigned)((kp.n_long + 3) / 4)), dim3(256), 0,
                           s, kp);
        return launched("long-row reduce launch");
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// SDDMM: out[e] = < G[row(e), :], B[col[e], :] > for every stored entry e of the CSR pattern — the
// gradient of the adjacency VALUES when a caller sets adj.requires_grad (PyTorch's `mm` derivative
// for a sparse first operand: grad_self = (grad · mat2ᵀ) sampled on self's pattern,
// derivatives.yaml `mm` / pygcn/layers.py:34).  The reference never needs it (adj is a loaded
// constant, pygcn/train.py:80,123); SURVEY row f4 lists it as optional.
// Same work units as the product (row-batch items and long-row chunks, one per wave); a wave keeps
// the row of G it works on in registers where the row fits one wave instruction, gathers U = 4
// rows of B at a time (16 B per lane, row address wave-uniform) and reduces the 4 partial dot
// products across the wave.  Gather-bound like the product: nnz·(F·s) + n·(F·s) bytes.
//
// WHY IT LIVES IN THIS FILE, next to the product it is no part of: sddmm_kernel hands Lane<float>::unpack a reference
// straight into global memory.  As long as one kernel of the translation unit does, LLVM's argument promotion leaves
// that helper's signature alone; without one (the product's own kernels unpack registers only) it passes the 16 bytes
// by value, the helper is inlined in another form, and all 42 fp32 lane instantiations of spmm_narrow_kernel compile
// to other instructions (profiles/spmm_split_isa.md §1).  Whoever moves this kernel out has those 42
// to measure again.
// ------------------------------------------------------------------------------------------
struct SddmmParams {
    const void *rowptr;
    const int32_t *col;
    const int32_t *items;
    const int32_t *chunk_row;
    const int64_t *chunk_e0;
    const void *G;
    const void *B;
    float *out;
    int64_t ldg, ldb;      // elements
    int32_t F, n_total, n_chunks, long_thresh;
};

template <typename T, int VEC, typename IdxT>
__global__ __launch_bounds__(kWave *kWavesPerBlock) void sddmm_kernel(SddmmParams p)
{
    typedef typename Elem<T, VEC>::Raw Raw;
    constexpr int U = 4;
    const int lane = threadIdx.x & (kWave - 1);
    const int item =
        blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= p.n_total) return;
    const IdxT *__restrict__ rp = (const IdxT *)p.rowptr;
    int ra, rb;
    int64_t e_lo = -1, e_hi = -1;                   // entry window of a chunk (whole rows otherwise)
    if (item < p.n_chunks) {
        ra = p.chunk_row[item];
        rb = ra + 1;
        e_lo = p.chunk_e0[item];
        e_hi = min(e_lo + (int64_t)p.long_thresh, (int64_t)rp[ra + 1]);
    } else {
        const int it = item - p.n_chunks;
        ra = p.items[2 * it];
        rb = p.items[2 * it + 1];
    }
    const int slab = kWave * VEC;                   // elements one wave instruction covers
    for (int r = ra; r < rb; ++r) {                 // (wave-uniform loop)
        const int64_t es = e_lo >= 0 ? e_lo : (int64_t)rp[r];
        const int64_t ee = e_lo >= 0 ? e_hi : (int64_t)rp[r + 1];
        if (es >= ee) continue;
        const T *grow = (const T *)p.G + (int64_t)r * p.ldg;
        for (int64_t e = es; e < ee; e += U) {
            const int cnt = (int)min((int64_t)U, ee - e);
            float part[U];
#pragma unroll
            for (int u = 0; u < U; ++u) part[u] = 0.f;
            for (int f0 = lane * VEC; f0 < p.F; f0 += slab) {
                float g[VEC];
                Elem<T, VEC>::unpack(*(const Raw *)(grow + f0), g);      // (L1-resident across the row)
                Raw braw[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int c = p.col[e + (u < cnt ? u : 0)];          // (uniform: scalar load)
                    braw[u] = *(const Raw *)((const T *)p.B + (int64_t)c * p.ldb + f0);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float b[VEC];
                    Elem<T, VEC>::unpack(braw[u], b);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) part[u] = fmaf(g[i], b[i], part[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float s = group_sum<kWave>(part[u]);
                if (lane == u && u < cnt) p.out[e + u] = s;
            }
        }
    }
}

}   // namespace

extern "C" {

size_t gcn_spmm_workspace_bytes(const gcn_csr_plan *plan, int64_t F)
{
    if (plan == nullptr || F <= 0 || plan->n_chunks <= 0) return 0;
    return (size_t)plan->n_chunks * (size_t)F * sizeof(float);
}

// gcn_spmm_csr_ep, and (`packed` != NULL: the slots of the rows of B) gcn_spmm_csr_packed
static int spmm_csr_impl(const gcn_csr_plan *plan, int dtype, const void *B, int64_t ldb, void *C,
                         int64_t ldc, int64_t F, const gcn_epilogue *ep, void *workspace,
                         size_t workspace_bytes, void *stream, const void *packed, int slot_bytes = 512)
{
    const float *bias = ep ? ep->bias : nullptr;
    const int relu = ep ? ep->relu : 0;
    const float drop_p = ep ? ep->dropout_p : 0.f;
    if (!(drop_p >= 0.f && drop_p < 1.f))
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "dropout_p must be in [0, 1)");
    if (plan == nullptr) return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "plan is NULL");
    if (dtype != GCN_DTYPE_F32 && dtype != GCN_DTYPE_BF16)
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "unknown dtype");
    if (plan->n_rows < 0 || plan->n_cols < 0 || plan->nnz < 0 || F < 0 || F > INT32_MAX)
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "negative size");
    if (plan->n_rows == 0 || F == 0) return 0;
    if (C == nullptr || (B == nullptr && plan->nnz > 0 && !(ep && ep->b2 && ep->b_split == 0)))
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "B or C is NULL");
    if (ldb < F || ldc < F) return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "ldb/ldc smaller than F");
    if (ldb * 4 >= ((int64_t)1 << 32))
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "row stride of B must be below 4 GiB");
    if (plan->rowptr == nullptr || plan->items == nullptr ||
        (plan->nnz > 0 && (plan->col == nullptr || plan->val == nullptr)))
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "plan has NULL arrays");
    if (plan->n_chunks > 0 && (plan->chunk_row == nullptr || plan->chunk_e0 == nullptr ||
                               plan->long_row == nullptr || plan->long_chunk0 == nullptr))
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "plan has long rows but NULL chunk arrays");
    if (plan->n_items + plan->n_chunks >= INT32_MAX || plan->n_long >= INT32_MAX)
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "schedule too large");
    const size_t need = gcn_spmm_workspace_bytes(plan, F);
    if (need > 0 && (workspace == nullptr || workspace_bytes < need))
        return bad("gcn_spmm_csr_ep", GCN_E_WORKSPACE, "workspace too small");

    KParams kp;
    kp.packed = packed;
    kp.rowptr = plan->rowptr;
    kp.col = plan->col;
    kp.val = plan->val;
    kp.items = plan->items;
    kp.chunk_row = plan->chunk_row;
    kp.chunk_e0 = plan->chunk_e0;
    kp.long_row = plan->long_row;
    kp.long_chunk0 = plan->long_chunk0;
    kp.B = B;
    kp.C = C;
    kp.bias = bias;
    kp.partial = (float *)workspace;
    kp.ldb = ldb;
    kp.ldc = ldc;
    kp.F = (int32_t)F;
    kp.n_total = (int32_t)(plan->n_items + plan->n_chunks);
    kp.n_chunks = (int32_t)plan->n_chunks;
    kp.n_long = (int32_t)plan->n_long;
    kp.long_thresh = plan->long_thresh > 0 ? plan->long_thresh : GCN_DEFAULT_LONG_THRESH;
    kp.relu = relu ? 1 : 0;
    // keep iff rand16 >= round(p * 2^16)  (p = 0 -> threshold 0 -> dropout off)
    kp.drop_thresh = gcn_dropout_threshold16(drop_p);
    kp.drop_scale = gcn_dropout_scale16(kp.drop_thresh);
    kp.drop_row_base = ep ? ep->drop_row_base : 0;
    kp.seed_lo = ep ? (uint32_t)ep->seed : 0u;
    kp.seed_hi = ep ? (uint32_t)(ep->seed >> 32) : 0u;
    kp.seed_dev = ep ? ep->seed_dev : nullptr;
    kp.csel = ep ? ep->c_row_select : nullptr;
    kp.cabsmax = ep ? (uint32_t *)ep->c_absmax : nullptr;
    kp.cskip = (ep && ep->c_skip_zero_rows && ep->c_row_nonzero) ? 1 : 0;
    kp.B2 = ep ? ep->b2 : nullptr;
    kp.ldb2 = ep && ep->b2 ? ep->ldb2 : 0;
    kp.b_split = (ep && ep->b2) ? (int32_t)std::min<int64_t>(ep->b_split, INT32_MAX) : INT32_MAX;
    if (ep && ep->b2 && (ep->b_split < 0 || ep->ldb2 < F || ep->ldb2 * 4 >= ((int64_t)1 << 32)))
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "bad second block of B");
    kp.bflag = ep ? ep->b_row_nonzero : nullptr;
    kp.bnnz = ep ? ep->b_nnz_rows : nullptr;
    if (kp.bflag == nullptr || kp.bnnz == nullptr) kp.bflag = nullptr, kp.bnnz = nullptr;
    kp.cflag = ep ? ep->c_row_nonzero : nullptr;
    kp.log_softmax = (ep && ep->log_softmax) ? 1 : 0;
    if (kp.log_softmax && (relu || drop_p > 0.f))
        return bad("gcn_spmm_csr_ep", GCN_E_BADARG, "log_softmax cannot be combined with relu / dropout");
    kp.n_cols = (int32_t)std::min<int64_t>(plan->n_cols, INT32_MAX);
    hipStream_t s = (hipStream_t)stream;
    return pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        return spmm_typed<T, Lane<T>::V>(plan, kp, s, slot_bytes);
    });
}

int gcn_spmm_csr_ep(const gcn_csr_plan *plan, int dtype, const void *B, int64_t ldb, void *C,
                    int64_t ldc, int64_t F, const gcn_epilogue *ep, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    return spmm_csr_impl(plan, dtype, B, ldb, C, ldc, F, ep, workspace, workspace_bytes, stream, nullptr);
}

int gcn_spmm_csr_packed(const gcn_csr_plan *plan, const uint32_t *slots, const float *B, int64_t ldb, float *C,
                        int64_t ldc, void *workspace, size_t workspace_bytes, void *stream)
{
    if (slots == nullptr || B == nullptr) return bad("gcn_spmm_csr_packed", GCN_E_BADARG, "slots or B is NULL");
    if ((((uintptr_t)slots) | ((uintptr_t)B) | ((uintptr_t)C)) % 16 != 0 || ldb % 4 != 0 || ldc % 4 != 0)
        return bad("gcn_spmm_csr_packed", GCN_E_ALIGN, "16-byte aligned slots and rows required");
    return spmm_csr_impl(plan, GCN_DTYPE_F32, B, ldb, C, ldc, 256, nullptr, workspace, workspace_bytes, stream, slots);
}

int gcn_spmm_csr_packed384(const gcn_csr_plan *plan, const uint32_t *slots, const float *B, int64_t ldb, float *C,
                           int64_t ldc, void *workspace, size_t workspace_bytes, void *stream)
{
    if (slots == nullptr || B == nullptr) return bad("gcn_spmm_csr_packed384", GCN_E_BADARG, "slots or B is NULL");
    if ((((uintptr_t)slots) | ((uintptr_t)B) | ((uintptr_t)C)) % 16 != 0 || ldb % 4 != 0 || ldc % 4 != 0)
        return bad("gcn_spmm_csr_packed384", GCN_E_ALIGN, "16-byte aligned slots and rows required");
    return spmm_csr_impl(plan, GCN_DTYPE_F32, B, ldb, C, ldc, 256, nullptr, workspace, workspace_bytes, stream, slots,
                         384);
}

int gcn_spmm_csr(const gcn_csr_plan *plan, int dtype, const void *B, int64_t ldb, void *C,
                 int64_t ldc, int64_t F, const float *bias, int relu, void *workspace,
                 size_t workspace_bytes, void *stream)
{
    gcn_epilogue ep = {};          // (every option off; fields added later stay zero)
    ep.bias = bias;
    ep.relu = relu;
    return gcn_spmm_csr_ep(plan, dtype, B, ldb, C, ldc, F, &ep, workspace, workspace_bytes, stream);
}

int gcn_sddmm_csr(const gcn_csr_plan *plan, int dtype, const void *G, int64_t ldg, const void *B,
                  int64_t ldb, int64_t F, float *out_vals, void *stream)
{
    const char *who = "gcn_sddmm_csr";
    if (plan == nullptr) return bad(who, GCN_E_BADARG, "plan is NULL");
    if (dtype != GCN_DTYPE_F32 && dtype != GCN_DTYPE_BF16) return bad(who, GCN_E_BADARG, "unknown dtype");
    if (plan->n_rows < 0 || plan->n_cols < 0 || plan->nnz < 0 || F < 0 || F > INT32_MAX)
        return bad(who, GCN_E_BADARG, "negative size");
    if (plan->nnz == 0) return 0;
    if (G == nullptr || B == nullptr || out_vals == nullptr || plan->rowptr == nullptr ||
        plan->col == nullptr || plan->items == nullptr)
        return bad(who, GCN_E_BADARG, "NULL pointer");
    if (plan->n_chunks > 0 && (plan->chunk_row == nullptr || plan->chunk_e0 == nullptr))
        return bad(who, GCN_E_BADARG, "plan has long rows but NULL chunk arrays");
    if (ldg < F || ldb < F) return bad(who, GCN_E_BADARG, "ldg / ldb smaller than F");
    hipStream_t s = (hipStream_t)stream;
    if (F == 0) {
        hipError_t e = hipMemsetAsync(out_vals, 0, (size_t)plan->nnz * sizeof(float), s);
        return e == hipSuccess ? 0 : gcn_internal_fail_hip((int)e, who);
    }
    SddmmParams sp;
    sp.rowptr = plan->rowptr;
    sp.col = plan->col;
    sp.items = plan->items;
    sp.chunk_row = plan->chunk_row;
    sp.chunk_e0 = plan->chunk_e0;
    sp.G = G;
    sp.B = B;
    sp.out = out_vals;
    sp.ldg = ldg;
    sp.ldb = ldb;
    sp.F = (int32_t)F;
    sp.n_total = (int32_t)(plan->n_items + plan->n_chunks);
    sp.n_chunks = (int32_t)plan->n_chunks;
    sp.long_thresh = plan->long_thresh > 0 ? plan->long_thresh : GCN_DEFAULT_LONG_THRESH;
    const bool is64 = plan->rowptr_is64 != 0;
    const int64_t vw = lane_elems(dtype), es = 16 / vw;
    const bool vec_ok = (F % vw == 0) && (((uintptr_t)G | (uintptr_t)B) % 16 == 0) &&
                        ((ldg * es) % 16 == 0) && ((ldb * es) % 16 == 0);
    const dim3 grid((unsigned)((sp.n_total + kWavesPerBlock - 1) / kWavesPerBlock)), block(kWave * kWavesPerBlock);
    pick_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        pick_int<Lane<T>::V, 1>(vec_ok ? Lane<T>::V : 1, [&](auto v) {
            pick_index(is64, [&](auto i) {
                hipLaunchKernelGGL((sddmm_kernel<T, decltype(v)::value, typename decltype(i)::type>), grid, block, 0,
                                   s, sp);
            });
        });
    });
    return launched("gcn_sddmm_csr launch");
}

}   // extern "C"
