// test_wg_san.cpp -- the host-only code of the WireGuard transport data batch under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_wg_sanitizers.py builds
// this file and sg_wg_host.cpp with g++ -fsanitize=address,undefined and runs the program
// directly; no GPU, no HIP header, nothing loaded into Python).
//
// The argument rules of sg_seal_batch_wg / sg_open_batch_wg (sg::wg::check_args: the struct
// is read, never what it points to, so the pointers here are small integers that a
// dereference would fault on) and sg_wg_padded_len / sg_wg_message_len over every length
// of a few MTUs, ragged caps and the ends of 32 bits, where nothing may wrap.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/suruga_gpu.h"
#include "../../suruga_amd/csrc/sg_wg.h"

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

template <class T>
static T* at(uintptr_t a) {
    return reinterpret_cast<T*>(a);
}

static sg_wg_batch good() {
    sg_wg_batch b;
    std::memset(&b, 0, sizeof b);
    b.count = 4;
    b.num_keys = 2;
    b.pad_cap = 1420;
    b.keys = at<const uint8_t>(0x1000);
    b.receiver = at<const uint32_t>(0x2000);
    b.counter = at<const uint64_t>(0x4000);
    b.counter_out = at<uint64_t>(0x5000);
    b.status = at<uint8_t>(0x6000);
    b.in = at<const uint8_t>(0x10001);  // packets lie at any address
    b.out = at<uint8_t>(0x20003);
    b.uniform_len = 1200;
    return b;
}

static void argument_rules() {
    using sg::wg::check_args;
    for (int open = 0; open < 2; ++open) {
        const uint32_t limit = SG_WG_MAX_MESSAGE_LEN - (open ? 0u : 32u);
        uint32_t max_len = 7;
        sg_wg_batch b = good();
        CHECK(check_args(&b, open, &max_len) == nullptr && max_len == 1200);
        CHECK(check_args(&b, open, nullptr) == nullptr);
        CHECK(check_args(nullptr, open, &max_len) != nullptr);
        b.flags = SG_WG_KEEP_FAILED;
        CHECK(check_args(&b, open, &max_len) == nullptr);
        b.flags = 0x2;
        CHECK(check_args(&b, open, &max_len) != nullptr);
        b.flags = 0x80000001u;
        CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.keys = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.status = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.in = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.out = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.receiver = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open == 0));
        b = good(); b.counter = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open == 0));
        b = good(); b.counter_out = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        b = good(); b.inner_len = at<uint32_t>(0x7000); b.key_index = at<const uint32_t>(0x7100);
        CHECK(check_args(&b, open, &max_len) == nullptr);
        for (uintptr_t o = 1; o < 8; ++o) {
            const bool odd4 = (o & 3) != 0;
            b = good(); b.receiver = at<const uint32_t>(0x2000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.key_index = at<const uint32_t>(0x7000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.inner_len = at<uint32_t>(0x7000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.len = at<const uint32_t>(0x7000 + o); b.max_len = 100; CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.counter = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.counter_out = at<uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.in_off = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.out_off = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
        }
        const uint32_t caps[] = {0u, 1u, 1420u, 16352u, 16353u, 0xffffffffu};
        for (uint32_t cap : caps) {
            b = good(); b.pad_cap = cap;
            CHECK((check_args(&b, open, &max_len) == nullptr) == (cap <= SG_WG_MAX_MESSAGE_LEN - 32u));
        }
        const uint32_t lens[] = {0u, limit, limit + 1u, 0xffffffffu};
        for (uint32_t l : lens) {
            b = good(); b.uniform_len = l;
            CHECK((check_args(&b, open, &max_len) == nullptr) == (l <= limit));
            if (l <= limit) CHECK(max_len == l);
            b = good(); b.len = at<const uint32_t>(0x7000); b.max_len = l; b.uniform_len = 0xffffffffu;
            CHECK((check_args(&b, open, &max_len) == nullptr) == (l <= limit));
        }
        b = good(); b.num_keys = 0; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.num_keys = 0xffffffffu; CHECK(check_args(&b, open, &max_len) == nullptr);
        b = good(); b.count = 0; b.keys = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);  // checked for an empty call too
    }
}

static void length_functions() {
    const uint32_t caps[] = {0u, 1u, 15u, 16u, 17u, 1280u, 1420u, 1500u, 9000u, 16352u, 0xfffffff0u, 0xffffffffu};
    for (uint32_t cap : caps)
        for (uint32_t len = 0; len <= 16400u; ++len) {
            const uint32_t p = sg_wg_padded_len(len, cap);
            const uint32_t up = (len + 15u) / 16u * 16u;
            CHECK(p >= len && p - len < 16u && p <= up);
            if (cap == 0u || up <= (len > cap ? len : cap)) CHECK(p == up);
            else CHECK(p == (len > cap ? len : cap));
            CHECK(p == sg::wg::padded_len(len, cap));
            CHECK(sg_wg_message_len(len, cap) == p + 32u);
        }
    const uint32_t ends[] = {0xffffffc0u, 0xffffffcfu, 0xffffffd0u, 0xffffffdfu, 0xffffffe0u, 0xffffffefu, 0xfffffff0u,
                             0xfffffff1u, 0xfffffffeu, 0xffffffffu};
    for (uint32_t cap : caps)
        for (uint32_t len : ends) {
            const uint32_t p = sg_wg_padded_len(len, cap);
            CHECK(p >= len && p - len < 16u);  // never below len, never wrapped
            const uint32_t m = sg_wg_message_len(len, cap);
            CHECK(m == (p > 0xffffffffu - 32u ? 0xffffffffu : p + 32u));
        }
    CHECK(sg_wg_padded_len(0xfffffff0u, 0) == 0xfffffff0u && sg_wg_padded_len(0xfffffff1u, 0) == 0xfffffff1u);
    CHECK(sg_wg_message_len(0, 0) == 32u && sg_wg_message_len(1, 0) == 48u && sg_wg_message_len(1419, 1420) == 1452u);
}

int main() {
    argument_rules();
    length_functions();
    std::printf("wg sanitizer checks passed\n");
    return 0;
}
