// The long-message plan (suruga_amd/csrc/sg_msg_plan.cpp, host only) under
// AddressSanitizer / UndefinedBehaviorSanitizer: the sweep of
// tests/test_msg_plan.py as a stand-alone program.  Built and run by
// tests/test_msg_sanitizers.py; prints "msg plan sanitizer checks passed"; a
// sanitizer report aborts the program (halt_on_error).
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/suruga_gpu.h"

static int g_failed = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            ++g_failed;                                                                    \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                                  \
    } while (0)

static void check_plan(uint64_t n, uint64_t adlen, uint32_t groups) {
    sg_msg_plan p;
    CHECK(sg_msg_plan_for(n, adlen, groups, &p) == SG_OK);
    const uint64_t B = (adlen + 16u + n + 15u) / 16u;
    CHECK(p.mac_blocks == B);
    CHECK(p.tile_blocks >= 1u && p.tile_bytes == 16u * p.tile_blocks);
    CHECK(p.zero_blocks < p.tile_blocks);
    CHECK(p.zero_blocks + B == p.tiles * p.tile_blocks);
    CHECK(p.groups >= 1u && p.tiles_per_group >= 1u);
    if (groups) CHECK(p.groups <= groups);
    // the groups' tile ranges partition [0, tiles): no group empty, none past the end
    CHECK((uint64_t)(p.groups - 1u) * p.tiles_per_group < p.tiles);
    CHECK(p.tiles <= (uint64_t)p.groups * p.tiles_per_group);
    CHECK(p.tiles * p.tile_bytes < (1ull << 62));
}

int main() {
    const uint64_t adlens[] = {0, 1, 7, 8, 13, 255, 256, 4096, 70001};
    const uint32_t groups[] = {0, 1, 2, 3, 7};
    for (uint64_t n = 0; n <= 70000; n += 997)
        for (uint64_t a : adlens)
            for (uint32_t g : groups) check_plan(n, a, g);
    for (uint32_t g : groups) check_plan(SG_MSG_MAX_LEN, SG_MSG_MAX_LEN, g);
    sg_msg_plan p;
    CHECK(sg_msg_plan_for(SG_MSG_MAX_LEN + 1u, 0, 0, &p) == SG_E_ARG);
    CHECK(sg_msg_plan_for(0, SG_MSG_MAX_LEN + 1u, 0, &p) == SG_E_ARG);
    CHECK(sg_msg_plan_for(~0ull, ~0ull, 0, &p) == SG_E_ARG);
    CHECK(sg_msg_plan_for(0, 0, 0, nullptr) == SG_E_ARG);
    // the switch: set, query, restore
    const int prev = sg_set_msg_groups(5);
    CHECK(sg_set_msg_groups(-1) == 5);
    CHECK(sg_set_msg_groups(1 << 30) == 5);
    CHECK(sg_set_msg_groups(prev) == 1024);
    if (g_failed) return 1;
    std::printf("msg plan sanitizer checks passed\n");
    return 0;
}
