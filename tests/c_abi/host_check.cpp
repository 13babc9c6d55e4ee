// host_check.cpp — the CPU algorithms of pygcn_amd/csrc/gcn_host.hip (host planner, host transpose), checked by a
// plain host program (its own main, no GPU, no library): tests/test_host_cpu.py compiles this file TOGETHER with
// gcn_host.hip, host-only, under the address and undefined-behaviour sanitizers and runs it.  Every array the API
// writes is heap-allocated at exactly the size the API asks for, so a write one past the end is a sanitizer report.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "gcn_spmm.h"
#include "gcn_internal.h"

// the two error hooks the header declares (gcn_error.hip defines them in the library); these keep the last message
static char last_error[256] = "";
int gcn_internal_fail(int code, const char *msg)
{
    std::snprintf(last_error, sizeof last_error, "%s", msg);
    return code;
}
int gcn_internal_fail_hip(int hip_error, const char *where)
{
    std::snprintf(last_error, sizeof last_error, "%s: hip error %d", where, hip_error);
    return hip_error;
}

static int failures = 0;
static const char *shape = "";      // the case being checked, for the report
#define CHECK(...)                                                                         \
    do {                                                                                   \
        if (!(__VA_ARGS__)) {                                                              \
            std::printf("host_check: line %d [%s]: %s\n", __LINE__, shape, #__VA_ARGS__); \
            ++failures;                                                                    \
        }                                                                                  \
    } while (0)

static bool refused(int rc, int code, const char *text)
{
    return rc == code && std::strstr(last_error, text) != nullptr;
}

// n elements on the heap, exactly (n = 0: a valid pointer to no element), optionally copied from a vector
template <typename T> std::unique_ptr<T[]> exact(int64_t n) { return std::unique_ptr<T[]>(new T[(size_t)n]()); }
template <typename T, typename S> std::unique_ptr<T[]> exact(const std::vector<S> &v)
{
    auto p = exact<T>((int64_t)v.size());
    for (size_t k = 0; k < v.size(); ++k) p[k] = (T)v[k];
    return p;
}

template <typename I> std::unique_ptr<I[]> rowptr_of(const std::vector<int64_t> &deg)
{
    auto rp = exact<I>((int64_t)deg.size() + 1);
    for (size_t r = 0; r < deg.size(); ++r) rp[r + 1] = (I)((int64_t)rp[r] + deg[r]);
    return rp;
}

// ------------------------------------------------------------------------------------------------
// planner
// ------------------------------------------------------------------------------------------------
struct Plan {
    int64_t ni = 0, nc = 0, nl = 0;
    std::unique_ptr<int32_t[]> items, chunk_row, long_row, long_chunk0;
    std::unique_ptr<int64_t[]> chunk_e0;
    // arrays of exactly the sizes gcn_plan_fill_host asks for at these counts
    void allocate()
    {
        items = exact<int32_t>(2 * ni);
        chunk_row = exact<int32_t>(nc);
        chunk_e0 = exact<int64_t>(nc);
        long_row = exact<int32_t>(nl);
        long_chunk0 = exact<int32_t>(nl + 1);
    }
    template <typename I> int fill(const I *rp, int64_t n, int item_cost, int long_thresh)
    {
        return gcn_plan_fill_host(rp, sizeof(I) == 8, n, item_cost, long_thresh, items.get(), ni, chunk_row.get(),
                                  chunk_e0.get(), nc, long_row.get(), long_chunk0.get(), nl);
    }
};

// count, fill into exact arrays, and every property of the schedule; want_* < 0: no particular count expected
template <typename I>
void check_plan(const char *name, const std::vector<int64_t> &deg, int item_cost, int long_thresh,
                int64_t want_items = -1, int64_t want_chunks = -1, int64_t want_long = -1)
{
    shape = name;
    const int64_t n = (int64_t)deg.size();
    const auto rp = rowptr_of<I>(deg);
    Plan p;
    CHECK(gcn_plan_count_host(rp.get(), sizeof(I) == 8, n, item_cost, long_thresh, &p.ni, &p.nc, &p.nl) == 0);
    CHECK(want_items < 0 || p.ni == want_items);
    CHECK(want_chunks < 0 || p.nc == want_chunks);
    CHECK(want_long < 0 || p.nl == want_long);
    p.allocate();
    CHECK(p.fill(rp.get(), n, item_cost, long_thresh) == 0);      // (the fill compares its counts with these)
    const int64_t cost_cap = item_cost > 0 ? item_cost : GCN_DEFAULT_ITEM_COST;
    const int64_t lt = long_thresh > 0 ? long_thresh : GCN_DEFAULT_LONG_THRESH;

    // items: every short row exactly once, in order, at most 64 rows each; what lies between two items is long
    std::vector<int> covered((size_t)n, 0);
    int64_t next = 0;
    for (int64_t k = 0; k < p.ni; ++k) {
        const int64_t ra = p.items[2 * k], rb = p.items[2 * k + 1];
        CHECK(ra >= next && ra < rb && rb <= n && rb - ra <= 64);
        if (!(ra >= next && ra < rb && rb <= n)) return;
        for (int64_t r = next; r < ra; ++r) CHECK(deg[(size_t)r] > lt);
        int64_t cost = 0;
        for (int64_t r = ra; r < rb; ++r) {
            CHECK(deg[(size_t)r] <= lt);
            ++covered[(size_t)r];
            cost += deg[(size_t)r] + 1;
        }
        CHECK(rb - ra == 1 || cost <= cost_cap);      // only a single row may exceed the item cost
        next = rb;
    }
    for (int64_t r = next; r < n; ++r) CHECK(deg[(size_t)r] > lt);
    for (int64_t r = 0; r < n; ++r) CHECK(covered[(size_t)r] == (deg[(size_t)r] <= lt ? 1 : 0));

    // long rows in row order; each one's chunks are consecutive windows of long_thresh entries that end with the row
    int64_t j = 0, c = 0;
    for (int64_t r = 0; r < n; ++r) {
        if (deg[(size_t)r] <= lt) continue;
        CHECK(j < p.nl);
        if (j >= p.nl) return;
        CHECK(p.long_row[j] == r && p.long_chunk0[j] == c);
        const int64_t k = (deg[(size_t)r] + lt - 1) / lt;
        CHECK(c + k <= p.nc);
        if (c + k > p.nc) return;
        for (int64_t q = 0; q < k; ++q) {
            CHECK(p.chunk_row[c + q] == r);
            CHECK(p.chunk_e0[c + q] == (int64_t)rp[r] + q * lt);
        }
        CHECK(p.chunk_e0[c + k - 1] < (int64_t)rp[r + 1] && p.chunk_e0[c + k - 1] + lt >= (int64_t)rp[r + 1]);
        c += k;
        ++j;
    }
    CHECK(j == p.nl && c == p.nc);
    CHECK(p.long_chunk0[p.nl] == p.nc);
}

template <typename I> void planner_shapes()
{
    const int64_t L = 8, big = 1000000;
    check_plan<I>("no rows", {}, 0, 0, 0, 0, 0);
    check_plan<I>("one empty row", {0}, 0, 0, 1, 0, 0);
    check_plan<I>("64 one-entry rows", std::vector<int64_t>(64, 1), (int)big, 0, 1, 0, 0);
    check_plan<I>("65 one-entry rows", std::vector<int64_t>(65, 1), (int)big, 0, 2, 0, 0);
    check_plan<I>("costs sum to item_cost", {4, 4}, 10, 0, 1, 0, 0);
    check_plan<I>("costs sum to item_cost + 1", {4, 5}, 10, 0, 2, 0, 0);
    check_plan<I>("a row of long_thresh entries", {L}, 0, (int)L, 1, 0, 0);
    check_plan<I>("a row of long_thresh + 1 entries", {L + 1}, 0, (int)L, 0, 2, 1);
    check_plan<I>("long row first", {L + 1, 1, 1}, 0, (int)L, 1, 2, 1);
    check_plan<I>("long row last", {1, 1, L + 1}, 0, (int)L, 1, 2, 1);
    check_plan<I>("long row between two short runs", {1, 0, 2 * L + 1, 1, 1}, 0, (int)L, 2, 3, 1);
    check_plan<I>("two adjacent long rows", {1, L + 1, 3 * L, 1}, 0, (int)L, 2, 5, 2);
    check_plan<I>("only long rows", {2 * L, L + 1}, 0, (int)L, 0, 4, 2);
    // item_cost <= 0 and long_thresh <= 0 select the defaults: 256 entries are short, 257 are two chunks; rows of
    // cost 32 close an item at every second row
    const int64_t D = GCN_DEFAULT_LONG_THRESH;
    check_plan<I>("defaults (0, 0)", {31, 31, 31, D, D + 1, 31}, 0, 0, 4, 2, 1);
    check_plan<I>("defaults (-5, -1)", {31, 31, 31, D, D + 1, 31}, -5, -1, 4, 2, 1);
}

template <typename I> void planner_refusals()
{
    const bool is64 = sizeof(I) == 8;
    int64_t ni = 0, nc = 0, nl = 0;
    shape = "planner refusals";
    {   // a row pointer that goes down
        const auto rp = exact<I>(std::vector<int64_t>{0, 5, 3});
        CHECK(refused(gcn_plan_count_host(rp.get(), is64, 2, 0, 0, &ni, &nc, &nl), GCN_E_BADARG, "monotone"));
        Plan p;
        p.allocate();
        CHECK(refused(p.fill(rp.get(), 2, 0, 0), GCN_E_BADARG, "gcn_plan_fill_host"));
    }
    const std::vector<int64_t> deg = {1, 1, 9, 1, 1, 17, 1};      // item cost 4: 3 items; 2 long rows, 2 + 3 chunks
    const int64_t n = (int64_t)deg.size();
    const auto rp = rowptr_of<I>(deg);
    CHECK(gcn_plan_count_host(rp.get(), is64, n, 4, 8, &ni, &nc, &nl) == 0 && ni == 3 && nc == 5 && nl == 2);
    for (int which = 0; which < 3; ++which) {
        for (int delta = -1; delta <= 1; delta += 2) {
            // one count off by one, the arrays allocated at THAT size: too small must stop before the write past
            // the end, too large is caught by the comparison of the sizes
            Plan p;
            p.ni = ni + (which == 0 ? delta : 0);
            p.nc = nc + (which == 1 ? delta : 0);
            p.nl = nl + (which == 2 ? delta : 0);
            p.allocate();
            CHECK(refused(p.fill(rp.get(), n, 4, 8), GCN_E_CAPACITY, delta < 0 ? "too small" : "sizes differ"));
        }
    }
    Plan p;
    p.ni = ni, p.nc = nc, p.nl = nl;
    p.allocate();
    CHECK(p.fill(rp.get(), n, 4, 8) == 0);
    // NULL arguments
    CHECK(refused(gcn_plan_count_host(nullptr, is64, n, 4, 8, &ni, &nc, &nl), GCN_E_BADARG, "gcn_plan_count_host"));
    CHECK(refused(gcn_plan_count_host(rp.get(), is64, -1, 4, 8, &ni, &nc, &nl), GCN_E_BADARG, "n_rows"));
    CHECK(refused(gcn_plan_fill_host(nullptr, is64, n, 4, 8, p.items.get(), ni, p.chunk_row.get(), p.chunk_e0.get(),
                                     nc, p.long_row.get(), p.long_chunk0.get(), nl),
                  GCN_E_BADARG, "null output"));
    CHECK(refused(gcn_plan_fill_host(rp.get(), is64, n, 4, 8, nullptr, ni, p.chunk_row.get(), p.chunk_e0.get(), nc,
                                     p.long_row.get(), p.long_chunk0.get(), nl),
                  GCN_E_BADARG, "null output"));
    CHECK(refused(gcn_plan_fill_host(rp.get(), is64, n, 4, 8, p.items.get(), ni, p.chunk_row.get(), p.chunk_e0.get(),
                                     nc, p.long_row.get(), nullptr, nl),
                  GCN_E_BADARG, "null output"));
    // the three arrays that may be NULL at a count of 0 are refused at a count above it
    CHECK(refused(gcn_plan_fill_host(rp.get(), is64, n, 4, 8, p.items.get(), ni, nullptr, p.chunk_e0.get(), nc,
                                     p.long_row.get(), p.long_chunk0.get(), nl),
                  GCN_E_BADARG, "null output"));
    CHECK(refused(gcn_plan_fill_host(rp.get(), is64, n, 4, 8, p.items.get(), ni, p.chunk_row.get(), nullptr, nc,
                                     p.long_row.get(), p.long_chunk0.get(), nl),
                  GCN_E_BADARG, "null output"));
    CHECK(refused(gcn_plan_fill_host(rp.get(), is64, n, 4, 8, p.items.get(), ni, p.chunk_row.get(), p.chunk_e0.get(),
                                     nc, nullptr, p.long_chunk0.get(), nl),
                  GCN_E_BADARG, "null output"));
    {   // ... and taken at 0: a graph without long rows, planned with NULL chunk and long-row arrays
        const auto rs = rowptr_of<I>({1, 2, 0});
        Plan q;
        CHECK(gcn_plan_count_host(rs.get(), is64, 3, 0, 0, &q.ni, &q.nc, &q.nl) == 0 && q.nc == 0 && q.nl == 0);
        q.allocate();
        CHECK(gcn_plan_fill_host(rs.get(), is64, 3, 0, 0, q.items.get(), q.ni, nullptr, nullptr, 0, nullptr,
                                 q.long_chunk0.get(), 0) == 0);
        CHECK(q.ni == 1 && q.items[0] == 0 && q.items[1] == 3 && q.long_chunk0[0] == 0);
    }
}

// ------------------------------------------------------------------------------------------------
// transpose
// ------------------------------------------------------------------------------------------------
struct Coo {      // a CSR matrix as plain vectors
    int64_t n_rows, n_cols;
    std::vector<int64_t> rp;
    std::vector<int32_t> col;
    std::vector<float> val;
    bool operator==(const Coo &o) const
    {
        return n_rows == o.n_rows && n_cols == o.n_cols && rp == o.rp && col == o.col && val == o.val;
    }
};

// column by column, the rows in ascending order and a row's entries in stored order
static Coo naive_transpose(const Coo &a)
{
    Coo t{a.n_cols, a.n_rows, {0}, {}, {}};
    for (int64_t c = 0; c < a.n_cols; ++c) {
        for (int64_t i = 0; i < a.n_rows; ++i)
            for (int64_t e = a.rp[(size_t)i]; e < a.rp[(size_t)i + 1]; ++e)
                if (a.col[(size_t)e] == c) {
                    t.col.push_back((int32_t)i);
                    t.val.push_back(a.val[(size_t)e]);
                }
        t.rp.push_back((int64_t)t.col.size());
    }
    return t;
}

// every row's entries sorted by column, equal columns in stored order
static Coo row_sorted(const Coo &a)
{
    Coo s = a;
    for (int64_t i = 0; i < a.n_rows; ++i) {
        std::vector<int64_t> order;
        for (int64_t e = a.rp[(size_t)i]; e < a.rp[(size_t)i + 1]; ++e) order.push_back(e);
        std::stable_sort(order.begin(), order.end(),
                         [&](int64_t x, int64_t y) { return a.col[(size_t)x] < a.col[(size_t)y]; });
        for (size_t k = 0; k < order.size(); ++k) {
            s.col[(size_t)a.rp[(size_t)i] + k] = a.col[(size_t)order[k]];
            s.val[(size_t)a.rp[(size_t)i] + k] = a.val[(size_t)order[k]];
        }
    }
    return s;
}

// gcn_csr_transpose_host on exact arrays: n_cols + 1 row pointers and nnz entries out
template <typename I> Coo transpose(const Coo &a, int *rc_out = nullptr)
{
    const int64_t nnz = a.rp.back();
    const auto rp = exact<I>(a.rp);
    const auto col = exact<int32_t>(a.col);
    const auto val = exact<float>(a.val);
    auto rpt = exact<I>(a.n_cols + 1);
    auto col_t = exact<int32_t>(nnz);
    auto val_t = exact<float>(nnz);
    for (int64_t e = 0; e < nnz; ++e) col_t[e] = -7, val_t[e] = -7.f;
    const int rc = gcn_csr_transpose_host(rp.get(), sizeof(I) == 8, col.get(), val.get(), a.n_rows, a.n_cols,
                                          rpt.get(), col_t.get(), val_t.get());
    if (rc_out) *rc_out = rc;
    else CHECK(rc == 0);
    Coo t{a.n_cols, a.n_rows, {}, {}, {}};
    for (int64_t k = 0; k <= a.n_cols; ++k) t.rp.push_back((int64_t)rpt[k]);
    for (int64_t e = 0; e < nnz; ++e) t.col.push_back(col_t[e]), t.val.push_back(val_t[e]);
    return t;
}

template <typename I> void transpose_shapes()
{
    const Coo cases[] = {
        {0, 0, {0}, {}, {}},
        {3, 0, {0, 0, 0, 0}, {}, {}},
        {1, 1, {0, 1}, {0}, {2.5f}},
        // 3 x 5: row 1 is empty, column 2 is empty, row 0 holds column 3 twice and out of order
        {3, 5, {0, 3, 3, 6}, {3, 1, 3, 4, 0, 1}, {1.f, 2.f, 3.f, 4.f, 5.f, 6.f}},
    };
    const char *names[] = {"transpose 0 x 0", "transpose 3 x 0", "transpose 1 x 1", "transpose 3 x 5"};
    for (int k = 0; k < 4; ++k) {
        shape = names[k];
        const Coo t = transpose<I>(cases[k]);
        CHECK(t == naive_transpose(cases[k]));
        CHECK(transpose<I>(t) == row_sorted(cases[k]));      // twice: the original with sorted rows
    }
}

template <typename I> void transpose_refusals()
{
    const bool is64 = sizeof(I) == 8;
    shape = "transpose refusals";
    for (int32_t wrong : {-1, 5}) {      // below the range and n_cols itself: found by the counting pass
        Coo a{3, 5, {0, 3, 3, 6}, {3, 1, 3, 4, 0, 1}, {1.f, 2.f, 3.f, 4.f, 5.f, 6.f}};
        a.col[4] = wrong;
        int rc = 0;
        const Coo t = transpose<I>(a, &rc);
        CHECK(refused(rc, GCN_E_BADARG, "column index out of range"));
        for (size_t e = 0; e < t.col.size(); ++e) CHECK(t.col[e] == -7 && t.val[e] == -7.f);   // nothing scattered
    }
    const auto rp = exact<I>(std::vector<int64_t>{0, 1});
    const auto col = exact<int32_t>(1), col_t = exact<int32_t>(1);
    const auto val = exact<float>(1), val_t = exact<float>(1);
    const auto rpt = exact<I>(2);
    const char *text = "gcn_csr_transpose_host";
    CHECK(gcn_csr_transpose_host(rp.get(), is64, col.get(), val.get(), 1, 1, rpt.get(), col_t.get(), val_t.get()) == 0);
    CHECK(refused(gcn_csr_transpose_host(rp.get(), is64, nullptr, val.get(), 1, 1, rpt.get(), col_t.get(), val_t.get()),
                  GCN_E_BADARG, text));
    CHECK(refused(gcn_csr_transpose_host(rp.get(), is64, col.get(), nullptr, 1, 1, rpt.get(), col_t.get(), val_t.get()),
                  GCN_E_BADARG, text));
    CHECK(refused(gcn_csr_transpose_host(rp.get(), is64, col.get(), val.get(), 1, 1, rpt.get(), nullptr, val_t.get()),
                  GCN_E_BADARG, text));
    CHECK(refused(gcn_csr_transpose_host(rp.get(), is64, col.get(), val.get(), 1, 1, rpt.get(), col_t.get(), nullptr),
                  GCN_E_BADARG, text));
    CHECK(refused(gcn_csr_transpose_host(nullptr, is64, col.get(), val.get(), 1, 1, rpt.get(), col_t.get(), val_t.get()),
                  GCN_E_BADARG, "bad arguments"));
    CHECK(refused(gcn_csr_transpose_host(rp.get(), is64, col.get(), val.get(), 1, 1, nullptr, col_t.get(), val_t.get()),
                  GCN_E_BADARG, "bad arguments"));
}

int main()
{
    planner_shapes<int32_t>();
    planner_shapes<int64_t>();
    planner_refusals<int32_t>();
    planner_refusals<int64_t>();
    transpose_shapes<int32_t>();
    transpose_shapes<int64_t>();
    transpose_refusals<int32_t>();
    transpose_refusals<int64_t>();
    if (failures == 0) std::printf("host_check ok\n");
    return failures == 0 ? 0 : 1;
}
