// The long-message plan (suruga_amd/csrc/sg_msg_plan.cpp, host only) under
// AddressSanitizer / UndefinedBehaviorSanitizer: the sweep of
// tests/test_msg_plan.py as a stand-alone program, and the shared per-message
// argument check (msg_check_args) over the table of
// tests/test_msg_args_shared.py plus the lengths at SG_MSG_MAX_LEN and one
// either side of it.  Built and run by
// tests/test_msg_sanitizers.py; prints "msg plan sanitizer checks passed"; a
// sanitizer report aborts the program (halt_on_error).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/suruga_gpu.h"
#include "../../suruga_amd/csrc/sg_msg_plan.h"

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

// one call of msg_check_args: the text (NULL = may run), and for a message that
// may run its data length and whether it is a short open
static void check_args(const sg::MsgArgs& a, bool open, const char* text, uint64_t want_n = 0, bool want_short = false) {
    uint64_t n = ~0ull;
    bool shrt = !want_short;
    const char* got = sg::msg_check_args(a, open, &n, &shrt);
    if (!text) {
        CHECK(got == nullptr);
        CHECK(shrt == want_short);
        CHECK(n == want_n);
    } else {
        CHECK(got != nullptr && std::strstr(got, text) == got);
    }
}

static void check_msg_args() {
    // the made-up addresses of tests/test_msg_batch_abi.py: never dereferenced
    const void* key = (const void*)0x1000;
    const void* st = (const void*)0x2000;
    const void* ad = (const void*)0x101000;
    const uintptr_t in_a = 0x210000;  // (address arithmetic on the integer: the pointers are never formed from one another)
    const void* in = (const void*)in_a;
    auto at = [&](int64_t off) { return (const void*)(in_a + (uintptr_t)off); };
    const void* out = (const void*)0x410000;
    const uint64_t M = SG_MSG_MAX_LEN;
    const char* nulls = "in/out/ad must be non-NULL";
    const char* overlap = "out overlaps in (only out == in is allowed)";
    for (int o = 0; o < 2; ++o) {
        const bool open = o != 0;
        check_args({key, ad, 13, in, 100, out, st}, open, nullptr, open ? 84 : 100);
        check_args({key, ad, 13, in, 100, in, st}, open, nullptr, open ? 84 : 100);  // in place
        check_args({key, nullptr, 13, in, 100, out, st}, open, nulls);
        check_args({key, ad, 13, nullptr, 100, out, st}, open, nulls);
        check_args({key, ad, 13, in, 100, nullptr, st}, open, nulls);
        check_args({nullptr, ad, 13, in, 100, out, st}, open, "key must be non-NULL");
        check_args({key, ad, M + 1, in, 100, out, st}, open, "ad_len exceeds SG_MSG_MAX_LEN");
        check_args({key, ad, M, in, 100, out, st}, open, nullptr, open ? 84 : 100);
        check_args({key, ad, M - 1, in, 100, out, st}, open, nullptr, open ? 84 : 100);
        // n at the bound and one either side of it (open: n = in_len - 16)
        const uint64_t tag = open ? SG_MAC_LEN : 0;
        const void* far = (const void*)((uintptr_t)1 << 40);  // no overlap at any of these lengths
        check_args({key, ad, 13, in, M - 1 + tag, far, st}, open, nullptr, M - 1);
        check_args({key, ad, 13, in, M + tag, far, st}, open, nullptr, M);
        check_args({key, ad, 13, in, M + 1 + tag, far, st}, open, "message longer than SG_MSG_MAX_LEN");
        check_args({key, ad, 13, in, ~0ull, far, st}, open, "message longer than SG_MSG_MAX_LEN");
    }
    check_args({key, ad, 13, nullptr, 0, nullptr, st}, false, nulls);  // an empty seal still writes a tag
    check_args({key, nullptr, 0, nullptr, 16, nullptr, st}, true, nulls);
    check_args({key, nullptr, 0, in, 16, nullptr, st}, true, nullptr, 0);  // an empty open writes nothing
    check_args({key, ad, 13, in, 100, out, nullptr}, true, "open requires a status byte");
    check_args({key, ad, 13, in, 100, out, nullptr}, false, nullptr, 100);
    // a short open is the caller's SG_E_SHORT: nothing else is looked at
    check_args({nullptr, nullptr, ~0ull, nullptr, 15, nullptr, nullptr}, true, nullptr, 0, true);
    check_args({key, ad, 13, in, 0, out, st}, true, nullptr, 0, true);
    // the three overlap cases
    check_args({key, ad, 13, in, 100, at(1), st}, false, overlap);
    check_args({key, ad, 13, in, 100, at(-100), st}, false, overlap);  // the tag reaches into in
    check_args({key, ad, 13, in, 116, at(115), st}, true, overlap);
    check_args({key, ad, 13, in, 100, at(-116), st}, false, nullptr, 100);  // out ends where in begins
    check_args({key, ad, 13, in, 116, at(116), st}, true, nullptr, 100);
}

int main() {
    check_msg_args();
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
