// gcn_select.hip — choosing NN vertices out of N on the device (gfx950): the k-th largest of a [k, n]
// score vector by radix select, the indices above it, the fork's top-NN flag, and the keys of an
// exponential race (sampling without replacement).
//
// Every policy generator of the reference fork ends by choosing NN vertices:
//     Generator / Hierarchical_Generator      reference pygcn/models.py:373-377, :398-406
//         sorted_indices = torch.argsort(mlp_output, dim=0, descending=True)
//         topk_mask = torch.where(mlp_output > mlp_output[sorted_indices[NN]], reciprocal, zero)
//         vac_flag = mlp_output * topk_mask
//     SoftGenerator's training step           reference pygcn/rl-policy-generator.py:324-336
//         torch.multinomial(attn, NN, replacement=False).tolist()
// Neither needs a sort or the host.  Layout as the attention head's (gcn_norm.hip): every per-vertex
// vector is fp32 [batch, n_rows], one window's rows consecutive; blockIdx.y is the window.
//
// ORDER.  One total order on fp32: -0 is +0, every NaN is greater than +inf (where torch.argsort(descending)
// puts it), otherwise numeric.  order_key() maps a float to the uint32 with that order: negatives have all
// bits flipped, non-negatives the sign bit set, NaN is 0xFFFFFFFF.
//
// RADIX SELECT, 11 / 11 / 10 bits from the top, three histogram passes.  At 10^7 vertices a pass reads 40 MB
// (~10 us) and a launch boundary costs 1.5-2 us, so the launches are the design variable: 8-bit digits would
// need four read passes and four pick steps (9 launches with the zeroing); 11/11/10 needs 7, and 2048 bins
// are 8 KiB of LDS, far below what limits occupancy.
//     select_init_kernel    zeroes the three global histograms, state = (prefix 0, rank kth, count_gt 0)
//     select_hist_kernel    x3: a block counts the digit of its slab's keys THAT MATCH THE PREFIX in LDS
//                           (integer atomics), then adds its non-zero bins to the window's global histogram
//                           (integer atomics: the sum does not depend on arrival order)
//     select_pick_kernel    x3: one block per window walks the 2048 bins from the top, finds the digit that
//                           holds the rank, and carries prefix | digit, the rank inside that bin and the
//                           count above in the workspace; the last one decodes thr and writes count_gt
// Separate launches: no block waits for another inside a kernel.  A wave whose live lanes all hold the same
// bin (all keys equal; the low digits of clustered keys) adds its lane count once instead of 64 times.
//
// INDICES.  select_count_kernel counts (> thr, == thr) per block, select_scan_kernel turns the counts of a
// window's blocks into exclusive offsets, select_write_kernel re-reads the slab chunk by chunk, ranks every
// selected vertex inside the chunk by ballots, and stores it at (selected before it) — ascending vertex
// order, the ties at thr by lowest index, a pure function of the keys.  The two sweeps use the same slabs.
//
// The sweeps read 4 bytes per lane: a window starts at j * n_rows floats, which is 16-byte aligned only
// when n_rows is a multiple of 4, so the loads stay scalar and coalesced (256 B per wave instruction).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

constexpr int kBins = 2048;               // 11-bit digit (the last pass uses 1024 of them)
constexpr int kPasses = 3;
constexpr int kState = 8;                 // uint32 per window: prefix, rank, count_gt (+ padding)
constexpr int64_t kBlocks = 1024;         // slabs of rows per window
constexpr int64_t kRowsPerBlock = 1024;   // a block's slab is at least this long before a second block starts
constexpr int64_t kMaxRows = INT32_MAX;   // n_rows < 2^31: counts and ranks are int32

__host__ __device__ constexpr int pass_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__host__ __device__ constexpr int pass_bins(int pass) { return pass == 2 ? 1024 : 2048; }
// the bits the earlier passes fixed
__host__ __device__ constexpr uint32_t pass_himask(int pass)
{
    return pass == 0 ? 0u : (pass == 1 ? 0xffe00000u : 0xfffffc00u);
}

struct Slabs {
    int64_t blocks;
    int64_t rows_per_block;
    explicit Slabs(int64_t n_rows)
    {
        blocks = std::min<int64_t>((n_rows + kRowsPerBlock - 1) / kRowsPerBlock, kBlocks);
        rows_per_block = (n_rows + blocks - 1) / blocks;
    }
};

// workspace of one call, in uint32: [batch][kPasses][kBins] histograms, [batch][kState] state,
// [batch][B][2] per-block counts
struct Scratch {
    uint32_t *hist, *state;
    int32_t *counts;
    Scratch(void *ws, int64_t batch, int64_t blocks)
    {
        hist = (uint32_t *)ws;
        state = hist + batch * kPasses * kBins;
        counts = (int32_t *)(state + batch * kState);
        (void)blocks;
    }
};

__global__ __launch_bounds__(256) void select_init_kernel(uint32_t *__restrict__ hist, uint32_t *__restrict__ state,
                                                          int64_t n_hist, int batch, uint32_t kth)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = t; i < n_hist; i += (int64_t)gridDim.x * 256) hist[i] = 0u;
    if (t < batch) {
        state[t * kState] = 0u;
        state[t * kState + 1] = kth;
        state[t * kState + 2] = 0u;
    }
}

template <int PASS>
__global__ __launch_bounds__(256) void select_hist_kernel(const float *__restrict__ keys,
                                                          const uint32_t *__restrict__ state,
                                                          uint32_t *__restrict__ hist, int64_t n_rows,
                                                          int64_t rows_per_block)
{
    constexpr int NB = pass_bins(PASS), SHIFT = pass_shift(PASS);
    constexpr uint32_t HI = pass_himask(PASS);
    __shared__ uint32_t bins[NB];
    for (int b = threadIdx.x; b < NB; b += 256) bins[b] = 0u;
    __syncthreads();
    const uint32_t prefix = state[(int64_t)blockIdx.y * kState];
    const float *w = keys + (int64_t)blockIdx.y * n_rows;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(r0 + rows_per_block, n_rows);
    for (int64_t base = r0; base < r1; base += 256) {      // (block-uniform trip count)
        const int64_t r = base + threadIdx.x;
        bool live = r < r1;
        uint32_t t = 0u;
        if (live) {
            t = order_key(w[r]);
            live = (t & HI) == prefix;
        }
        const int bin = (int)((t >> SHIFT) & (uint32_t)(NB - 1));
        const unsigned long long on = __ballot(live);
        if (on == 0ull) continue;                          // (wave-uniform)
        const int first = __ffsll((long long)on) - 1;      // the lowest live lane
        const int lead = __shfl(bin, first, 64);
        if (__ballot(live && bin == lead) == on) {         // one bin for the whole wave: one add
            if ((int)(threadIdx.x & 63) == first) atomicAdd(&bins[bin], (uint32_t)__popcll(on));
        } else if (live) {
            atomicAdd(&bins[bin], 1u);
        }
    }
    __syncthreads();
    uint32_t *g = hist + ((int64_t)blockIdx.y * kPasses + PASS) * kBins;
    for (int b = threadIdx.x; b < NB; b += 256) {
        const uint32_t c = bins[b];
        if (c != 0u) atomicAdd(&g[b], c);
    }
}

// One block per window.  Thread t owns the NB / 256 consecutive bins from t * (NB / 256); a suffix scan of
// the thread sums through LDS finds the thread, which then walks its bins from the top.
template <int PASS>
__global__ __launch_bounds__(256) void select_pick_kernel(const uint32_t *__restrict__ hist,
                                                          uint32_t *__restrict__ state, float *__restrict__ thr,
                                                          int32_t *__restrict__ count_gt)
{
    constexpr int NB = pass_bins(PASS), SHIFT = pass_shift(PASS), PER = NB / 256;
    __shared__ uint32_t above[256];       // inclusive suffix sums of the thread totals
    const uint32_t *g = hist + ((int64_t)blockIdx.x * kPasses + PASS) * kBins;
    uint32_t *st = state + (int64_t)blockIdx.x * kState;
    uint32_t c[PER], total = 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        c[i] = g[threadIdx.x * PER + i];
        total += c[i];
    }
    above[threadIdx.x] = total;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        const uint32_t add = (int)threadIdx.x + s < 256 ? above[threadIdx.x + s] : 0u;
        __syncthreads();
        above[threadIdx.x] += add;
        __syncthreads();
    }
    const uint32_t rank = st[1];          // 1-based among the keys that match the prefix; 1 <= rank <= above[0]
    uint32_t over = above[threadIdx.x] - total;            // keys in the bins of the threads after this one
    __syncthreads();                      // (every thread has read the state before one rewrites it)
    if (over < rank && rank <= over + total) {             // exactly one thread
        int d = 0;
        bool found = false;
#pragma unroll
        for (int i = PER - 1; i >= 0; --i) {               // (unrolled: c[] stays in registers)
            if (!found) {
                if (over + c[i] >= rank) { d = i; found = true; }
                else over += c[i];
            }
        }
        const uint32_t prefix = st[0] | ((uint32_t)(threadIdx.x * PER + d) << SHIFT);
        const uint32_t gt = st[2] + over;
        st[0] = prefix;
        st[1] = rank - over;
        st[2] = gt;
        if (PASS == kPasses - 1) {
            thr[blockIdx.x] = key_float(prefix);
            count_gt[blockIdx.x] = (int32_t)gt;
        }
    }
}

// (greater, equal) than thr of the block's slab -> counts[window][block][2]
__global__ __launch_bounds__(256) void select_count_kernel(const float *__restrict__ keys,
                                                           const float *__restrict__ thr,
                                                           int32_t *__restrict__ counts, int64_t n_rows,
                                                           int64_t rows_per_block)
{
    __shared__ int red[2][4];
    const uint32_t T = order_key(thr[blockIdx.y]);
    const float *w = keys + (int64_t)blockIdx.y * n_rows;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(r0 + rows_per_block, n_rows);
    int gt = 0, eq = 0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
        const uint32_t t = order_key(w[r]);
        gt += t > T;
        eq += t == T;
    }
    for (int m = 1; m < 64; m <<= 1) {
        gt += __shfl_xor(gt, m, 64);
        eq += __shfl_xor(eq, m, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = gt;
        red[1][threadIdx.x >> 6] = eq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t *dst = counts + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        dst[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        dst[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

// counts[window][0 .. n_blocks)[2] -> exclusive prefix sums, in place; one block per window, n_blocks <= 1024:
// thread t owns blocks 4t .. 4t + 3
__global__ __launch_bounds__(256) void select_scan_kernel(int32_t *__restrict__ counts, int n_blocks)
{
    __shared__ int sums[2][256];
    int32_t *c = counts + (int64_t)blockIdx.x * n_blocks * 2;
    int v[4][2], tot[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = threadIdx.x * 4 + i;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            v[i][s] = b < n_blocks ? c[2 * b + s] : 0;
            tot[s] += v[i][s];
        }
    }
    sums[0][threadIdx.x] = tot[0];
    sums[1][threadIdx.x] = tot[1];
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        const int a0 = (int)threadIdx.x >= s ? sums[0][threadIdx.x - s] : 0;
        const int a1 = (int)threadIdx.x >= s ? sums[1][threadIdx.x - s] : 0;
        __syncthreads();
        sums[0][threadIdx.x] += a0;
        sums[1][threadIdx.x] += a1;
        __syncthreads();
    }
    int run[2] = {sums[0][threadIdx.x] - tot[0], sums[1][threadIdx.x] - tot[1]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = threadIdx.x * 4 + i;
        if (b < n_blocks) {
            c[2 * b] = run[0];
            c[2 * b + 1] = run[1];
        }
        run[0] += v[i][0];
        run[1] += v[i][1];
    }
}

// idx[window][selected before r] = r for every selected vertex r of the block's slab: selected = greater
// than thr, or equal with fewer than need_eq = m - count_gt equal keys before it.  offsets = the scanned counts.
__global__ __launch_bounds__(256) void select_write_kernel(const float *__restrict__ keys,
                                                           const float *__restrict__ thr,
                                                           const int32_t *__restrict__ count_gt,
                                                           const int32_t *__restrict__ offsets,
                                                           int64_t *__restrict__ idx, int64_t n_rows,
                                                           int64_t rows_per_block, int64_t m)
{
    __shared__ int wave_tot[2][2][4];     // [chunk parity][gt, eq][wave]
    const uint32_t T = order_key(thr[blockIdx.y]);
    const int64_t need_eq = m - (int64_t)count_gt[blockIdx.y];
    const int32_t *off = offsets + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    int64_t gt_before = off[0], eq_before = off[1];
    const float *w = keys + (int64_t)blockIdx.y * n_rows;
    int64_t *out = idx + (int64_t)blockIdx.y * m;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(r0 + rows_per_block, n_rows);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int it = 0;
    for (int64_t base = r0; base < r1; base += 256, ++it) {     // (block-uniform trip count)
        const int64_t r = base + threadIdx.x;
        bool gt = false, eq = false;
        if (r < r1) {
            const uint32_t t = order_key(w[r]);
            gt = t > T;
            eq = t == T;
        }
        const unsigned long long mg = __ballot(gt), me = __ballot(eq);
        if (lane == 0) {
            wave_tot[it & 1][0][wave] = __popcll(mg);
            wave_tot[it & 1][1][wave] = __popcll(me);
        }
        __syncthreads();                  // (the other parity is the previous chunk's: one barrier per chunk)
        int64_t g0 = gt_before, e0 = eq_before;
        int all_g = 0, all_e = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int a = wave_tot[it & 1][0][q], b = wave_tot[it & 1][1][q];
            if (q < wave) { g0 += a; e0 += b; }
            all_g += a;
            all_e += b;
        }
        g0 += __popcll(mg & below);
        e0 += __popcll(me & below);
        if (gt || (eq && e0 < need_eq)) {
            const int64_t pos = g0 + min(e0, max(need_eq, (int64_t)0));
            if (pos < m) out[pos] = r;    // (always, when thr / count_gt are gcn_select_kth's for kth = m)
        }
        gt_before += all_g;
        eq_before += all_e;
    }
}

__global__ __launch_bounds__(256) void topk_flag_kernel(const float *s, const float *__restrict__ thr, float *flag,
                                                        int64_t n_rows)
{
    const float t = thr[blockIdx.y];
    const int64_t w = (int64_t)blockIdx.y * n_rows;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256) {
        const float x = s[w + r];
        const float inv = 1.0f / x;       // IEEE division (no fast-math in this build), rounded once
        flag[w + r] = x > t ? x * inv : 0.0f;
    }
}

// a thread draws the four vertices 4q .. 4q + 3 of its window from one call of the dropout's generator
__global__ __launch_bounds__(256) void race_keys_kernel(const float *p, float *keys, int64_t n_rows,
                                                        uint32_t seed_lo, uint32_t seed_hi,
                                                        const uint64_t *__restrict__ seed_dev)
{
    if (seed_dev != nullptr) {     // the seed as of execution time (a captured launch), as gcn_epilogue.seed_dev
        const uint64_t sd = *seed_dev;
        seed_lo = (uint32_t)sd;
        seed_hi = (uint32_t)(sd >> 32);
    }
    const int64_t w = (int64_t)blockIdx.y * n_rows;
    const int64_t groups = (n_rows + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += (int64_t)gridDim.x * 256) {
        uint32_t u[4];
        philox4x32_10<kPhiloxMulPair>((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)blockIdx.y, 1u, seed_lo, seed_hi,
                                      u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t r = 4 * q + i;
            if (r < n_rows) {
                const double e = -log(((double)u[i] + 0.5) * 0x1p-32);
                keys[w + r] = (float)((double)p[w + r] / e);
            }
        }
    }
}

bool rows_ok(int64_t n_rows) { return n_rows >= 1 && n_rows <= kMaxRows; }
bool batch_ok(int64_t batch) { return batch >= 1 && batch <= kMaxBatch; }

int check_shape(const char *who, int64_t n_rows, int64_t batch)
{
    if (!rows_ok(n_rows)) return bad(who, GCN_E_BADARG, "needs 1 <= n_rows < 2^31");
    if (!batch_ok(batch)) return bad(who, GCN_E_BADARG, "needs 1 <= batch <= 65535");
    return 0;
}

int check_workspace(const char *who, int64_t n_rows, int64_t batch, const void *ws, size_t ws_bytes)
{
    if (ws == nullptr || ws_bytes < gcn_select_workspace_bytes(n_rows, batch))
        return bad(who, GCN_E_WORKSPACE, "workspace too small");
    if ((uintptr_t)ws % 4 != 0) return bad(who, GCN_E_ALIGN, "workspace: 4-byte alignment required");
    return 0;
}

dim3 flat_grid(int64_t items, int64_t batch)
{
    return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 4096)), (unsigned)batch);
}

}   // namespace

extern "C" {

size_t gcn_select_workspace_bytes(int64_t n_rows, int64_t batch)
{
    if (!rows_ok(n_rows) || !batch_ok(batch)) return 0;
    return (size_t)batch * (size_t)(kPasses * kBins + kState + 2 * Slabs(n_rows).blocks) * sizeof(uint32_t);
}

int gcn_select_kth(const float *keys, int64_t n_rows, int64_t batch, int64_t kth, float *thr, int32_t *count_gt,
                   void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gcn_select_kth";
    if (int rc = check_shape(who, n_rows, batch)) return rc;
    if (kth < 1 || kth > n_rows) return bad(who, GCN_E_BADARG, "needs 1 <= kth <= n_rows");
    if (keys == nullptr || thr == nullptr || count_gt == nullptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if (int rc = check_workspace(who, n_rows, batch, workspace, workspace_bytes)) return rc;
    if ((uintptr_t)keys % 4 != 0 || (uintptr_t)thr % 4 != 0 || (uintptr_t)count_gt % 4 != 0)
        return bad(who, GCN_E_ALIGN, "keys, thr, count_gt: 4-byte alignment required");
    const Slabs sl(n_rows);
    const Scratch sc(workspace, batch, sl.blocks);
    const dim3 grid((unsigned)sl.blocks, (unsigned)batch), block(256), one((unsigned)batch);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_hist = batch * kPasses * kBins;
    hipLaunchKernelGGL(select_init_kernel, flat_grid(n_hist, 1), block, 0, s, sc.hist, sc.state, n_hist, (int)batch,
                       (uint32_t)kth);
    hipLaunchKernelGGL(select_hist_kernel<0>, grid, block, 0, s, keys, (const uint32_t *)sc.state, sc.hist, n_rows,
                       sl.rows_per_block);
    hipLaunchKernelGGL(select_pick_kernel<0>, one, block, 0, s, (const uint32_t *)sc.hist, sc.state, thr, count_gt);
    hipLaunchKernelGGL(select_hist_kernel<1>, grid, block, 0, s, keys, (const uint32_t *)sc.state, sc.hist, n_rows,
                       sl.rows_per_block);
    hipLaunchKernelGGL(select_pick_kernel<1>, one, block, 0, s, (const uint32_t *)sc.hist, sc.state, thr, count_gt);
    hipLaunchKernelGGL(select_hist_kernel<2>, grid, block, 0, s, keys, (const uint32_t *)sc.state, sc.hist, n_rows,
                       sl.rows_per_block);
    hipLaunchKernelGGL(select_pick_kernel<2>, one, block, 0, s, (const uint32_t *)sc.hist, sc.state, thr, count_gt);
    return launched(who);
}

int gcn_select_indices(const float *keys, int64_t n_rows, int64_t batch, int64_t m, const float *thr,
                       const int32_t *count_gt, int64_t *idx, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gcn_select_indices";
    if (int rc = check_shape(who, n_rows, batch)) return rc;
    if (m < 1 || m > n_rows) return bad(who, GCN_E_BADARG, "needs 1 <= m <= n_rows");
    if (keys == nullptr || thr == nullptr || count_gt == nullptr || idx == nullptr)
        return bad(who, GCN_E_BADARG, "NULL pointer");
    if (int rc = check_workspace(who, n_rows, batch, workspace, workspace_bytes)) return rc;
    if ((uintptr_t)keys % 4 != 0 || (uintptr_t)thr % 4 != 0 || (uintptr_t)count_gt % 4 != 0 || (uintptr_t)idx % 8 != 0)
        return bad(who, GCN_E_ALIGN, "idx: 8-byte, keys, thr, count_gt: 4-byte alignment required");
    const Slabs sl(n_rows);
    const Scratch sc(workspace, batch, sl.blocks);
    const dim3 grid((unsigned)sl.blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(select_count_kernel, grid, block, 0, s, keys, thr, sc.counts, n_rows, sl.rows_per_block);
    hipLaunchKernelGGL(select_scan_kernel, dim3((unsigned)batch), block, 0, s, sc.counts, (int)sl.blocks);
    hipLaunchKernelGGL(select_write_kernel, grid, block, 0, s, keys, thr, count_gt, (const int32_t *)sc.counts, idx,
                       n_rows, sl.rows_per_block, m);
    return launched(who);
}

int gcn_topk_flag(const float *s, int64_t n_rows, int64_t batch, const float *thr, float *flag, void *stream)
{
    const char *who = "gcn_topk_flag";
    if (int rc = check_shape(who, n_rows, batch)) return rc;
    if (s == nullptr || thr == nullptr || flag == nullptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if ((uintptr_t)s % 4 != 0 || (uintptr_t)thr % 4 != 0 || (uintptr_t)flag % 4 != 0)
        return bad(who, GCN_E_ALIGN, "s, thr, flag: 4-byte alignment required");
    hipLaunchKernelGGL(topk_flag_kernel, flat_grid(n_rows, batch), dim3(256), 0, (hipStream_t)stream, s, thr, flag,
                       n_rows);
    return launched(who);
}

int gcn_race_keys(const float *p, int64_t n_rows, int64_t batch, uint64_t seed, float *keys, void *stream)
{
    const char *who = "gcn_race_keys";
    if (int rc = check_shape(who, n_rows, batch)) return rc;
    if (p == nullptr || keys == nullptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if ((uintptr_t)p % 4 != 0 || (uintptr_t)keys % 4 != 0)
        return bad(who, GCN_E_ALIGN, "p, keys: 4-byte alignment required");
    hipLaunchKernelGGL(race_keys_kernel, flat_grid((n_rows + 3) / 4, batch), dim3(256), 0, (hipStream_t)stream, p, keys,
                       n_rows, (uint32_t)seed, (uint32_t)(seed >> 32), (const uint64_t *)nullptr);
    return launched(who);
}

int gcn_race_keys_dev(const float *p, int64_t n_rows, int64_t batch, const uint64_t *seed_dev, float *keys,
                      void *stream)
{
    const char *who = "gcn_race_keys_dev";
    if (int rc = check_shape(who, n_rows, batch)) return rc;
    if (p == nullptr || keys == nullptr || seed_dev == nullptr) return bad(who, GCN_E_BADARG, "NULL pointer");
    if ((uintptr_t)p % 4 != 0 || (uintptr_t)keys % 4 != 0 || (uintptr_t)seed_dev % 8 != 0)
        return bad(who, GCN_E_ALIGN, "seed_dev: 8-byte, p, keys: 4-byte alignment required");
    hipLaunchKernelGGL(race_keys_kernel, flat_grid((n_rows + 3) / 4, batch), dim3(256), 0, (hipStream_t)stream, p, keys,
                       n_rows, 0u, 0u, seed_dev);
    return launched(who);
}

}   // extern "C"
