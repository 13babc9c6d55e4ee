// gcn_sample.hip — neighbour sampling (gfx950): at most K of the stored entries of every row of a CSR matrix, as
// a CSR matrix of its own (include/gcn_spmm.h, "Neighbour sampling"; CSRGraph.sample_neighbors).  A per-row
// segmented select with no sort and NO WORKSPACE: the key of an entry is a function of (seed, stream, e), e the
// entry's index in the source arrays, from the counter-based Philox stream of gcn_internal.h — so a pass that needs
// the keys again computes them again, and no launch shape can change a draw.
//
// A lane owns the QUAD of four consecutive entries 4q .. 4q + 3 (one Philox call yields their four words), masked
// to the row: consecutive lanes hold consecutive quads, so (chunk, lane, i) order IS stored order.
//
// Two kernels, both grid-striding over ALL output rows and skipping the rows of the other class (the classes are
// found on the device, from the row lengths):
//   sample_wave_kernel    rows of 1 .. kWaveRowMax = 253 entries, one wavefront per row: such a row spans at most 64
//                         quads whatever its alignment, so the row is in registers, four keys per lane.  The K-th
//                         largest key comes from an MSB-first radix select, one bit per step, by __ballot and
//                         __popcll; the output positions from prefix popcounts.
//   sample_block_kernel   longer rows, one 256-thread workgroup per row.  A workgroup reads the lengths of 256 rows,
//                         lists the long ones in LDS and takes them one after the other: four 8-bit digit passes
//                         over the row with a 256-bin LDS histogram (integer atomics: the counts do not depend on
//                         arrival order), the keys recomputed in every pass, then one ordered compaction pass — per
//                         chunk of 1024 entries the wave totals through LDS plus the popcount prefix, one barrier
//                         per chunk (as select_write_kernel of gcn_select.hip has it).
// A row of at most K entries is copied by the kernel of its class.
//
// Selection: with T the K'-th largest key of the candidates and need_eq = K' - (keys above T), an entry is kept iff
// its key is above T, or equals T with fewer than need_eq equal keys stored before it.  The diagonal entry, when it
// is kept ahead of the order, is no candidate and K' = K - 1.  An entry's output slot is (kept entries before it).
//
// rescale: the double sums S (all entries) and S' (kept ones) are carried in the same pass — a lane adds its own
// entries in stored order, the 64 lanes of a wave by an xor butterfly, the 4 waves of a workgroup in wave order: a
// fixed order, the same bytes on every run.
//
// Reads: uniform mode reads `val` of the kept entries only (all of them under rescale), `col` of the kept entries
// only (all of them while the diagonal is looked for).
//
// gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int64_t kWaveRowMax = GCN_SAMPLE_WAVE_ROW_MAX;              // 3 + 253 = 256 entries = 64 quads at the worst alignment
constexpr int64_t kWaveGrid = GCN_SAMPLE_WAVE_SWEEP_ROWS / kWaves;    // workgroups of the row-per-wave kernel
constexpr int64_t kBlockGrid = 4096;                                  // workgroups of the row-per-workgroup kernel
constexpr int64_t kMaxRows = (int64_t)1 << 40;

struct SampleParams {
    const void *rowptr;
    const int32_t *col;
    const float *val;
    const int64_t *rows;
    int64_t m, fanout;
    uint32_t seed_lo, seed_hi, draw_stream;
    int keep_diag, rescale;
    const void *rowptr_out;
    int32_t *col_out;
    float *val_out;
};

template <typename P> __device__ __forceinline__ int64_t at(const void *p, int64_t i) { return (int64_t)((const P *)p)[i]; }

// output row r: source row s with the entries [s0, s1), output slots o0 .. o0 + room
struct Row {
    int64_t s, s0, s1, o0, room;
};

template <typename PI, typename PO> __device__ __forceinline__ Row row_of(const SampleParams &P, int64_t r)
{
    Row R;
    R.s = P.rows != nullptr ? P.rows[r] : r;
    R.s0 = at<PI>(P.rowptr, R.s);
    R.s1 = at<PI>(P.rowptr, R.s + 1);
    R.o0 = at<PO>(P.rowptr_out, r);
    R.room = at<PO>(P.rowptr_out, r + 1) - R.o0;     // (nothing is written outside the row's own slots)
    return R;
}

// the keys of the quad q = entries 4q .. 4q + 3 with the values v (read in the weight and strongest modes only)
template <int MODE>
__device__ __forceinline__ void quad_keys(const SampleParams &P, int64_t q, const float (&v)[4], uint32_t (&k)[4])
{
    if constexpr (MODE == GCN_SAMPLE_STRONGEST) {
#pragma unroll
        for (int i = 0; i < 4; ++i) k[i] = order_key(v[i]);
    } else {
        uint32_t u[4];
        philox4x32_10<kPhiloxMulPair>((uint32_t)q, (uint32_t)(q >> 32), P.draw_stream, 2u, P.seed_lo, P.seed_hi, u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (MODE == GCN_SAMPLE_UNIFORM) {
                k[i] = u[i];
            } else {                                 // the race key of gcn_race_keys, in the selection order
                const double e = -log(((double)u[i] + 0.5) * 0x1p-32);
                k[i] = order_key((float)((double)v[i] / e));
            }
        }
    }
}

// which of the quad's entries are kept and where they go: g0 / q0 = the candidates above T / equal to T that are
// stored before the quad, diag_e = the entry kept ahead of the order (-1: none)
__device__ __forceinline__ void place(int64_t e0, const bool (&gt)[4], const bool (&eq)[4], int64_t g0, int64_t q0,
                                      int64_t need_eq, int64_t diag_e, bool (&sel)[4], int64_t (&pos)[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t e = e0 + i;
        sel[i] = e == diag_e || gt[i] || (eq[i] && q0 < need_eq);
        pos[i] = g0 + min(q0, need_eq) + ((diag_e >= 0 && diag_e < e) ? 1 : 0);
        g0 += gt[i] ? 1 : 0;
        q0 += eq[i] ? 1 : 0;
    }
}

// (above T, equal to T) in the lanes below this one, and in the whole wave
__device__ __forceinline__ void wave_counts(const bool (&gt)[4], const bool (&eq)[4], unsigned long long below,
                                            int &g_pre, int &q_pre, int &g_all, int &q_all)
{
    g_pre = q_pre = g_all = q_all = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned long long mg = __ballot(gt[i]), mq = __ballot(eq[i]);
        g_pre += __popcll(mg & below);
        q_pre += __popcll(mq & below);
        g_all += __popcll(mg);
        q_all += __popcll(mq);
    }
}

__device__ __forceinline__ double wave_sum(double x)
{
    for (int m = 1; m < kWave; m <<= 1) x += __shfl_xor(x, m, kWave);   // (a + b == b + a: every lane holds the same bits)
    return x;
}

// the factor of rescale = "sum", or 1 with *scale = false where it is not finite
__device__ __forceinline__ float sum_ratio(double S, double Sp, bool *scale)
{
    const float ratio = (float)(S / Sp);
    *scale = isfinite(ratio);
    return ratio;
}

template <int MODE, typename PI, typename PO> __global__ __launch_bounds__(kBlock) void sample_wave_kernel(const SampleParams P)
{
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
    const bool all_vals = MODE != GCN_SAMPLE_UNIFORM || P.rescale != GCN_SAMPLE_RESCALE_NONE;
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    for (int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < P.m; r += stride) {   // (wave-uniform)
        const Row R = row_of<PI, PO>(P, r);
        const int64_t d = R.s1 - R.s0;
        if (d < 1 || d > kWaveRowMax) continue;
        const int64_t e0 = ((R.s0 >> 2) + lane) << 2;
        bool live[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) live[i] = e0 + i >= R.s0 && e0 + i < R.s1;
        if (d <= P.fanout) {                          // the row as it is
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t e = e0 + i, pos = e - R.s0;
                if (live[i] && pos < R.room) {
                    P.col_out[R.o0 + pos] = P.col[e];
                    P.val_out[R.o0 + pos] = P.val[e];
                }
            }
            continue;
        }
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (all_vals) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (live[i]) v[i] = P.val[e0 + i];
        }
        int64_t diag_e = -1;
        if (P.keep_diag) {                            // the first stored entry of column s
            int first = 4;
#pragma unroll
            for (int i = 3; i >= 0; --i)
                if (live[i] && (int64_t)P.col[e0 + i] == R.s) first = i;
            const unsigned long long hit = __ballot(first < 4);
            if (hit != 0ull) {
                const int L = __ffsll((long long)hit) - 1;
                diag_e = (((R.s0 >> 2) + L) << 2) + __shfl(first, L, kWave);
            }
        }
        uint32_t k[4];
        quad_keys<MODE>(P, e0 >> 2, v, k);
        bool cand[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cand[i] = live[i] && e0 + i != diag_e;
        // the K'-th largest candidate key, one bit per step from the top (K' < the number of candidates: d > K)
        uint32_t rank = (uint32_t)(P.fanout - (diag_e >= 0 ? 1 : 0)), prefix = 0u, known = 0u;
        const bool any = rank > 0u;
        if (any) {
            for (int b = 31; b >= 0; --b) {
                const uint32_t bit = 1u << b;
                uint32_t ones = 0u;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    ones += (uint32_t)__popcll(__ballot(cand[i] && (k[i] & known) == prefix && (k[i] & bit) != 0u));
                if (ones >= rank) prefix |= bit; else rank -= ones;
                known |= bit;
            }
        }
        const int64_t need_eq = any ? (int64_t)rank : 0;     // of the keys equal to T = prefix: the first `rank`
        bool gt[4], eq[4], sel[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            gt[i] = any && cand[i] && k[i] > prefix;
            eq[i] = any && cand[i] && k[i] == prefix;
        }
        int g_pre, q_pre, g_all, q_all;
        wave_counts(gt, eq, below, g_pre, q_pre, g_all, q_all);
        int64_t pos[4];
        place(e0, gt, eq, g_pre, q_pre, need_eq, diag_e, sel, pos);
        if (!all_vals) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (sel[i]) v[i] = P.val[e0 + i];
        }
        bool scale = false;
        float ratio = 1.f;
        if (P.rescale == GCN_SAMPLE_RESCALE_SUM) {
            double s_all = 0.0, s_kept = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (live[i]) s_all += (double)v[i];
                if (sel[i]) s_kept += (double)v[i];
            }
            ratio = sum_ratio(wave_sum(s_all), wave_sum(s_kept), &scale);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (sel[i] && pos[i] < R.room) {
                P.col_out[R.o0 + pos[i]] = P.col[e0 + i];
                P.val_out[R.o0 + pos[i]] = scale ? v[i] * ratio : v[i];
            }
        }
    }
}

struct BlockShared {
    int64_t list[kBlock];                 // the long rows among the 256 rows of the tile
    unsigned long long diag_min;
    double sums[2][kWaves];
    uint32_t hist[256], above[256];
    uint32_t pick[2];                     // prefix, rank after a digit pass
    int wave_tot[2][2][kWaves];           // [chunk parity][above, equal][wave]
    int n_list;
};

template <int MODE, typename PI, typename PO>
__device__ __forceinline__ void sample_long_row(const SampleParams &P, int64_t r, BlockShared &sh)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
    const Row R = row_of<PI, PO>(P, r);
    const int64_t q_first = R.s0 >> 2, n_quads = ((R.s1 - 1) >> 2) - q_first + 1;
    if (R.s1 - R.s0 <= P.fanout) {                // the row as it is (workgroup-uniform)
        for (int64_t g = tid; g < n_quads; g += kBlock) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t e = ((q_first + g) << 2) + i, pos = e - R.s0;
                if (e >= R.s0 && e < R.s1 && pos < R.room) {
                    P.col_out[R.o0 + pos] = P.col[e];
                    P.val_out[R.o0 + pos] = P.val[e];
                }
            }
        }
        return;
    }
    int64_t diag_e = -1;
    if (P.keep_diag) {                            // the first stored entry of column s
        if (tid == 0) sh.diag_min = ~0ull;
        __syncthreads();
        unsigned long long mine = ~0ull;
        for (int64_t g = tid; g < n_quads && mine == ~0ull; g += kBlock) {
#pragma unroll
            for (int i = 3; i >= 0; --i) {
                const int64_t e = ((q_first + g) << 2) + i;
                if (e >= R.s0 && e < R.s1 && (int64_t)P.col[e] == R.s) mine = (unsigned long long)e;
            }
        }
        if (mine != ~0ull) atomicMin(&sh.diag_min, mine);
        __syncthreads();
        if (sh.diag_min != ~0ull) diag_e = (int64_t)sh.diag_min;
    }
    // the K'-th largest candidate key, 8 bits per pass from the top (K' < the number of candidates: d > K)
    uint32_t rank = (uint32_t)(P.fanout - (diag_e >= 0 ? 1 : 0)), prefix = 0u;
    const bool any = rank > 0u;
    if (any) {
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t known = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
            sh.hist[tid] = 0u;
            if (tid == 0) { sh.pick[0] = prefix; sh.pick[1] = rank; }
            __syncthreads();
            for (int64_t g = tid; g < n_quads; g += kBlock) {
                const int64_t e0 = (q_first + g) << 2;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                uint32_t k[4];
                if (MODE != GCN_SAMPLE_UNIFORM) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (e0 + i >= R.s0 && e0 + i < R.s1) v[i] = P.val[e0 + i];
                }
                quad_keys<MODE>(P, e0 >> 2, v, k);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t e = e0 + i;
                    if (e >= R.s0 && e < R.s1 && e != diag_e && (k[i] & known) == prefix)
                        atomicAdd(&sh.hist[(k[i] >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            // thread t owns bin t: the bin whose keys hold the rank, by an inclusive suffix scan
            const uint32_t count = sh.hist[tid];
            sh.above[tid] = count;
            __syncthreads();
            for (int s = 1; s < kBlock; s <<= 1) {
                const uint32_t add = tid + s < kBlock ? sh.above[tid + s] : 0u;
                __syncthreads();
                sh.above[tid] += add;
                __syncthreads();
            }
            const uint32_t over = sh.above[tid] - count;
            if (over < rank && rank <= over + count) {       // exactly one thread
                sh.pick[0] = prefix | ((uint32_t)tid << shift);
                sh.pick[1] = rank - over;
            }
            __syncthreads();
            prefix = sh.pick[0];
            rank = sh.pick[1];
            __syncthreads();                                 // (read by all before the next pass rewrites it)
        }
    }
    const int64_t need_eq = any ? (int64_t)rank : 0;
    const bool all_vals = MODE != GCN_SAMPLE_UNIFORM || P.rescale != GCN_SAMPLE_RESCALE_NONE;
    int64_t g_before = 0, q_before = 0;
    double s_all = 0.0, s_kept = 0.0;
    int it = 0;
    for (int64_t base = 0; base < n_quads; base += kBlock, ++it) {       // (workgroup-uniform trip count)
        const int64_t e0 = (q_first + base + tid) << 2;
        bool live[4], gt[4], eq[4], sel[4];
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t k[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            live[i] = e0 + i >= R.s0 && e0 + i < R.s1;       // (false in every lane past the row's last quad)
            if (all_vals && live[i]) v[i] = P.val[e0 + i];
        }
        quad_keys<MODE>(P, e0 >> 2, v, k);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool cand = any && live[i] && e0 + i != diag_e;
            gt[i] = cand && k[i] > prefix;
            eq[i] = cand && k[i] == prefix;
        }
        int g_pre, q_pre, g_all, q_all;
        wave_counts(gt, eq, below, g_pre, q_pre, g_all, q_all);
        if (lane == 0) {
            sh.wave_tot[it & 1][0][wave] = g_all;
            sh.wave_tot[it & 1][1][wave] = q_all;
        }
        __syncthreads();                  // (the other parity is the previous chunk's: one barrier per chunk)
        int64_t g0 = g_before + g_pre, q0 = q_before + q_pre;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int a = sh.wave_tot[it & 1][0][w], b = sh.wave_tot[it & 1][1][w];
            if (w < wave) { g0 += a; q0 += b; }
            g_before += a;
            q_before += b;
        }
        int64_t pos[4];
        place(e0, gt, eq, g0, q0, need_eq, diag_e, sel, pos);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (sel[i] && !all_vals) v[i] = P.val[e0 + i];
            if (live[i]) s_all += (double)v[i];
            if (sel[i]) {
                s_kept += (double)v[i];
                if (pos[i] < R.room) {
                    P.col_out[R.o0 + pos[i]] = P.col[e0 + i];
                    P.val_out[R.o0 + pos[i]] = v[i];
                }
            }
        }
    }
    if (P.rescale == GCN_SAMPLE_RESCALE_SUM) {
        s_all = wave_sum(s_all);
        s_kept = wave_sum(s_kept);
        if (lane == 0) {
            sh.sums[0][wave] = s_all;
            sh.sums[1][wave] = s_kept;
        }
        __syncthreads();                  // (also: the row's stores above are visible to the whole workgroup)
        double S = sh.sums[0][0], Sp = sh.sums[1][0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            S += sh.sums[0][w];
            Sp += sh.sums[1][w];
        }
        bool scale;
        const float ratio = sum_ratio(S, Sp, &scale);
        if (scale) {
            const int64_t kept = min(P.fanout, R.room);
            for (int64_t p = tid; p < kept; p += kBlock) P.val_out[R.o0 + p] *= ratio;
        }
    }
    __syncthreads();                      // (the next row reuses the shared state)
}

template <int MODE, typename PI, typename PO> __global__ __launch_bounds__(kBlock) void sample_block_kernel(const SampleParams P)
{
    __shared__ BlockShared sh;
    const int64_t tiles = (P.m + kBlock - 1) / kBlock;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (workgroup-uniform)
        if (threadIdx.x == 0) sh.n_list = 0;
        __syncthreads();
        const int64_t r = tile * kBlock + threadIdx.x;
        if (r < P.m) {
            const int64_t s = P.rows != nullptr ? P.rows[r] : r;
            if (at<PI>(P.rowptr, s + 1) - at<PI>(P.rowptr, s) > kWaveRowMax) sh.list[atomicAdd(&sh.n_list, 1)] = r;
        }
        __syncthreads();
        const int n = sh.n_list;          // (the order of the list varies from run to run; a row's bytes do not)
        for (int j = 0; j < n; ++j) sample_long_row<MODE, PI, PO>(P, sh.list[j], sh);
        __syncthreads();
    }
}

}   // namespace

extern "C" {

int gcn_csr_sample_rows(const void *rowptr, int rowptr_is64, const int32_t *col, const float *val, const int64_t *rows,
                        int64_t m, int64_t fanout, int mode, uint64_t seed, uint32_t draw_stream, int keep_diagonal,
                        int rescale, const void *rowptr_out, int out_is64, int32_t *col_out, float *val_out, void *stream)
{
    const char *who = "gcn_csr_sample_rows";
    if (fanout < 1) return bad(who, GCN_E_BADARG, "needs fanout >= 1");
    if (mode != GCN_SAMPLE_UNIFORM && mode != GCN_SAMPLE_WEIGHT && mode != GCN_SAMPLE_STRONGEST)
        return bad(who, GCN_E_BADARG, "unknown mode");
    if (rescale != GCN_SAMPLE_RESCALE_NONE && rescale != GCN_SAMPLE_RESCALE_SUM)
        return bad(who, GCN_E_BADARG, "unknown rescale");
    if (m < 0 || m > kMaxRows) return bad(who, GCN_E_BADARG, "needs 0 <= m <= 2^40");
    if (m == 0) return 0;
    if (rowptr == nullptr || col == nullptr || val == nullptr || rowptr_out == nullptr || col_out == nullptr ||
        val_out == nullptr)
        return bad(who, GCN_E_BADARG, "NULL pointer");
    if ((uintptr_t)rowptr % (rowptr_is64 ? 8 : 4) != 0 || (uintptr_t)rowptr_out % (out_is64 ? 8 : 4) != 0 ||
        (uintptr_t)rows % 8 != 0 || (uintptr_t)col % 4 != 0 || (uintptr_t)val % 4 != 0 || (uintptr_t)col_out % 4 != 0 ||
        (uintptr_t)val_out % 4 != 0)
        return bad(who, GCN_E_ALIGN, "rows and 64-bit row pointers: 8-byte, the other arrays: 4-byte alignment required");
    SampleParams P;
    P.rowptr = rowptr; P.col = col; P.val = val; P.rows = rows;
    P.m = m; P.fanout = fanout;
    P.seed_lo = (uint32_t)seed; P.seed_hi = (uint32_t)(seed >> 32); P.draw_stream = draw_stream;
    P.keep_diag = keep_diagonal != 0; P.rescale = rescale;
    P.rowptr_out = rowptr_out; P.col_out = col_out; P.val_out = val_out;
    const dim3 block(kBlock);
    const dim3 wave_grid((unsigned)std::min<int64_t>((m + kWaves - 1) / kWaves, kWaveGrid));
    const dim3 block_grid((unsigned)std::min<int64_t>((m + kBlock - 1) / kBlock, kBlockGrid));
    hipStream_t s = (hipStream_t)stream;
    pick_int<GCN_SAMPLE_UNIFORM, GCN_SAMPLE_WEIGHT, GCN_SAMPLE_STRONGEST>(mode, [&](auto mv) {
        constexpr int MODE = decltype(mv)::value;
        pick_index(rowptr_is64 != 0, [&](auto pi) {
            typedef typename decltype(pi)::type PI;
            pick_index(out_is64 != 0, [&](auto po) {
                typedef typename decltype(po)::type PO;
                hipLaunchKernelGGL((sample_wave_kernel<MODE, PI, PO>), wave_grid, block, 0, s, P);
                hipLaunchKernelGGL((sample_block_kernel<MODE, PI, PO>), block_grid, block, 0, s, P);
            });
        });
    });
    return launched(who);
}

}   // extern "C"
