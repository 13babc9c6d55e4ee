// pick_check.cpp — the host-side picks of pygcn_amd/csrc/gcn_internal.h, checked by a plain host program (its own
// main, no GPU, no library): tests/test_host_cpu.py compiles it host-only under the address and undefined-behaviour
// sanitizers and runs it.
#include <cstdio>
#include <type_traits>

#include "gcn_spmm.h"
#include "gcn_internal.h"

// the two error hooks the header declares (gcn_error.hip defines them in the library); nothing here fails
int gcn_internal_fail(int code, const char *) { return code; }
int gcn_internal_fail_hip(int hip_error, const char *) { return -1000 - hip_error; }

static int failures = 0;
#define CHECK(...)                                                           \
    do {                                                                     \
        if (!(__VA_ARGS__)) {                                                \
            std::printf("pick_check: line %d: %s\n", __LINE__, #__VA_ARGS__); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

template <typename Want> struct Is {
    template <typename Tag> bool operator()(Tag) const { return std::is_same<typename Tag::type, Want>::value; }
};

int main()
{
    CHECK(pick_dtype(GCN_DTYPE_F32, Is<float>{}));
    CHECK(pick_dtype(GCN_DTYPE_BF16, Is<bf16_t>{}));
    CHECK(!pick_dtype(GCN_DTYPE_BF16, Is<float>{}));
    CHECK(pick_dtype(GCN_DTYPE_F32, [](auto t) { return sizeof(typename decltype(t)::type); }) == 4);
    CHECK(pick_dtype(GCN_DTYPE_BF16, [](auto t) { return sizeof(typename decltype(t)::type); }) == 2);

    CHECK(pick_index(true, Is<int64_t>{}));
    CHECK(pick_index(false, Is<int32_t>{}));
    CHECK(pick_index(1 != 0, [](auto i) { return sizeof(typename decltype(i)::type); }) == 8);
    CHECK(pick_index(0 != 0, [](auto i) { return sizeof(typename decltype(i)::type); }) == 4);

    // pick_int: exactly one call, with the matching constant; none, and false, outside the list
    for (int v : {1, 2, 4, 8, 16, 32}) {
        int calls = 0, got = -1;
        const bool found = pick_int<1, 2, 4, 8, 16, 32>(v, [&](auto c) {
            static_assert(std::is_same<typename decltype(c)::value_type, int>::value, "an integral_constant<int, V>");
            ++calls;
            got = decltype(c)::value;
        });
        CHECK(found && calls == 1 && got == v);
    }
    for (int v : {0, 3, 64, -1}) {
        int calls = 0;
        CHECK(!pick_int<1, 2, 4, 8, 16, 32>(v, [&](auto) { ++calls; }));
        CHECK(calls == 0);
    }
    {   // a value listed twice is still one call
        int calls = 0;
        CHECK((pick_int<4, 1, 4>(4, [&](auto) { ++calls; })) && calls == 1);
    }
    {   // nested picks reach one instantiation, the innermost sees all three choices
        int calls = 0;
        pick_dtype(GCN_DTYPE_BF16, [&](auto t) {
            pick_index(false, [&](auto i) {
                pick_int<0, 1, 2>(2, [&](auto x) {
                    ++calls;
                    CHECK(sizeof(typename decltype(t)::type) == 2 && sizeof(typename decltype(i)::type) == 4 &&
                          decltype(x)::value == 2);
                });
            });
        });
        CHECK(calls == 1);
    }

    // the shape rules that ride in the same host section
    CHECK(lane_width_ok(4, GCN_DTYPE_F32) && lane_width_ok(1024, GCN_DTYPE_F32) && !lane_width_ok(8, GCN_DTYPE_F32 + 7));
    CHECK(!lane_width_ok(12, GCN_DTYPE_F32) && !lane_width_ok(4, GCN_DTYPE_BF16) && lane_width_ok(2048, GCN_DTYPE_BF16));
    CHECK(RowSlabs(1).blocks == 1 && RowSlabs(64).blocks == 1 && RowSlabs(65).blocks == 2 && RowSlabs(65).rows_per_block == 33);
    CHECK(RowSlabs(64 * 2048 + 1).blocks == 2048 && RowSlabs(64 * 2048 + 1).rows_per_block == 65);
    CHECK(TileSlabs(65, 64).slabs == 2 && TileSlabs(65, 64).rows_per_block == 64);
    CHECK(TileSlabs(64 * 2048 + 1, 64).slabs == 2048 && TileSlabs(64 * 2048 + 1, 64).rows_per_block == 128);

    if (failures == 0) std::printf("pick_check ok\n");
    return failures == 0 ? 0 : 1;
}
