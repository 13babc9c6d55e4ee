// gcn_host.hip — the pure CPU algorithms of the C-ABI of include/gcn_spmm.h: the host planner (gcn_plan_count_host /
// gcn_plan_fill_host, the static schedule of the CSR product: row-batch items and long-row chunks) and the host
// transpose gcn_csr_transpose_host.  No kernel and no call into the HIP runtime: errors go through bad()
// (gcn_internal.h), so the file also compiles, host-only, into a stand-alone program with hooks of its own —
// tests/c_abi/host_check.cpp runs it under the address and undefined-behaviour sanitizers on arrays of exactly the
// sizes this API asks for.  The device planner (gcn_plan.hip) computes the same schedule.
#include <climits>
#include <cstdint>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

template <typename IdxT>
int plan_walk(const IdxT *rp, int64_t n_rows, int item_cost, int long_thresh, int32_t *items,
              int64_t cap_items, int32_t *chunk_row, int64_t *chunk_e0, int64_t cap_chunks,
              int32_t *long_row, int32_t *long_chunk0, int64_t cap_long, int64_t *n_items,
              int64_t *n_chunks, int64_t *n_long)
{
    const bool fill = items != nullptr;
    int64_t ni = 0, nc = 0, nl = 0;
    int64_t ra = 0, cost = 0;
    auto close = [&](int64_t rb) -> bool {
        if (rb > ra) {
            if (fill) {
                if (ni >= cap_items) return false;
                items[2 * ni] = (int32_t)ra;
                items[2 * ni + 1] = (int32_t)rb;
            }
            ++ni;
        }
        ra = rb;
        cost = 0;
        return true;
    };
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t deg = (int64_t)rp[r + 1] - (int64_t)rp[r];
        if (deg < 0) return GCN_E_BADARG;
        if (deg > long_thresh) {
            if (!close(r)) return GCN_E_CAPACITY;
            ra = r + 1;   // the long row belongs to no row-batch item
            const int64_t k = (deg + long_thresh - 1) / long_thresh;
            if (fill) {
                if (nl >= cap_long || nc + k > cap_chunks) return GCN_E_CAPACITY;
                long_row[nl] = (int32_t)r;
                long_chunk0[nl] = (int32_t)nc;
                for (int64_t c = 0; c < k; ++c) {
                    chunk_row[nc + c] = (int32_t)r;
                    chunk_e0[nc + c] = (int64_t)rp[r] + c * long_thresh;
                }
            }
            nc += k;
            ++nl;
            continue;
        }
        const int64_t c = deg + 1;
        if (r > ra && (cost + c > item_cost || r - ra >= kWave)) {
            if (!close(r)) return GCN_E_CAPACITY;
        }
        cost += c;
    }
    if (!close(n_rows)) return GCN_E_CAPACITY;
    if (fill && long_chunk0 != nullptr) {
        if (nl > cap_long) return GCN_E_CAPACITY;
        long_chunk0[nl] = (int32_t)nc;
    }
    if (n_items) *n_items = ni;
    if (n_chunks) *n_chunks = nc;
    if (n_long) *n_long = nl;
    return 0;
}

}   // namespace

extern "C" {

int gcn_plan_count_host(const void *rowptr_host, int rowptr_is64, int64_t n_rows,
                        int32_t item_cost, int32_t long_thresh, int64_t *n_items,
                        int64_t *n_chunks, int64_t *n_long)
{
    const char *who = "gcn_plan_count_host";
    if (rowptr_host == nullptr || n_rows < 0 || n_rows >= INT32_MAX)
        return bad(who, GCN_E_BADARG, "bad rowptr / n_rows");
    if (item_cost <= 0) item_cost = GCN_DEFAULT_ITEM_COST;
    if (long_thresh <= 0) long_thresh = GCN_DEFAULT_LONG_THRESH;
    int rc = pick_index(rowptr_is64 != 0, [&](auto i) {
        return plan_walk((const typename decltype(i)::type *)rowptr_host, n_rows, item_cost, long_thresh, nullptr, 0,
                         nullptr, nullptr, 0, nullptr, nullptr, 0, n_items, n_chunks, n_long);
    });
    return rc ? bad(who, rc, "rowptr is not monotone") : 0;
}

int gcn_plan_fill_host(const void *rowptr_host, int rowptr_is64, int64_t n_rows,
                       int32_t item_cost, int32_t long_thresh, int32_t *items, int64_t n_items,
                       int32_t *chunk_row, int64_t *chunk_e0, int64_t n_chunks,
                       int32_t *long_row, int32_t *long_chunk0, int64_t n_long)
{
    const char *who = "gcn_plan_fill_host";
    // (chunk_row / chunk_e0 / long_row may be NULL only when their count says that nothing is written there)
    if (rowptr_host == nullptr || n_rows < 0 || n_rows >= INT32_MAX || items == nullptr ||
        long_chunk0 == nullptr || (n_chunks > 0 && (chunk_row == nullptr || chunk_e0 == nullptr)) ||
        (n_long > 0 && long_row == nullptr))
        return bad(who, GCN_E_BADARG, "null output or bad n_rows");
    if (item_cost <= 0) item_cost = GCN_DEFAULT_ITEM_COST;
    if (long_thresh <= 0) long_thresh = GCN_DEFAULT_LONG_THRESH;
    int64_t ni = 0, nc = 0, nl = 0;
    int rc = pick_index(rowptr_is64 != 0, [&](auto i) {
        return plan_walk((const typename decltype(i)::type *)rowptr_host, n_rows, item_cost, long_thresh, items,
                         n_items, chunk_row, chunk_e0, n_chunks, long_row, long_chunk0, n_long, &ni, &nc, &nl);
    });
    if (rc) return bad(who, rc, "output arrays too small or rowptr not monotone");
    if (ni != n_items || nc != n_chunks || nl != n_long)
        return bad(who, GCN_E_CAPACITY, "sizes differ from gcn_plan_count_host");
    return 0;
}

int gcn_csr_transpose_host(const void *rowptr_host, int rowptr_is64, const int32_t *col,
                           const float *val, int64_t n_rows, int64_t n_cols, void *rowptr_t,
                           int32_t *col_t, float *val_t)
{
    const char *who = "gcn_csr_transpose_host";
    if (rowptr_host == nullptr || rowptr_t == nullptr || n_rows < 0 || n_cols < 0)
        return bad(who, GCN_E_BADARG, "bad arguments");
    int rc = pick_index(rowptr_is64 != 0, [&](auto i) -> int {
        typedef typename decltype(i)::type I;
        const I *rp = (const I *)rowptr_host;
        I *rpt = (I *)rowptr_t;
        const int64_t nnz = (int64_t)rp[n_rows];
        if (nnz > 0 && (col == nullptr || val == nullptr || col_t == nullptr || val_t == nullptr))
            return GCN_E_BADARG;
        for (int64_t k = 0; k <= n_cols; ++k) rpt[k] = 0;
        for (int64_t e = 0; e < nnz; ++e) {
            if (col[e] < 0 || col[e] >= n_cols) return GCN_E_BADARG;
            rpt[col[e] + 1]++;
        }
        for (int64_t k = 0; k < n_cols; ++k) rpt[k + 1] += rpt[k];
        for (int64_t i = 0; i < n_rows; ++i) {
            for (int64_t e = (int64_t)rp[i]; e < (int64_t)rp[i + 1]; ++e) {
                const int64_t dst = (int64_t)rpt[col[e]]++;
                col_t[dst] = (int32_t)i;
                val_t[dst] = val[e];
            }
        }
        for (int64_t k = n_cols; k > 0; --k) rpt[k] = rpt[k - 1];
        rpt[0] = (I)0;
        return 0;
    });
    return rc ? bad(who, rc, "column index out of range or NULL array") : 0;
}

}   // extern "C"
