// test_esp_san.cpp -- the host-only code of the IPsec ESP batch under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_esp_sanitizers.py builds this file and
// sg_esp_host.cpp with g++ -fsanitize=address,undefined and runs the program directly; no
// GPU, no HIP header, nothing loaded into Python).
//
// The argument rules of sg_seal_batch_esp / sg_open_batch_esp (sg::esp::check_args: the
// struct is read, never what it points to, so the pointers here are small integers that a
// dereference would fault on), sg_esp_padded_len / sg_esp_packet_len over every length of a
// few MTUs, every align and the ends of 32 bits, where nothing may wrap, and sg_esp_seq_hi
// against the interval it is defined by, at the edges of both of its cases.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/suruga_gpu.h"
#include "../../suruga_amd/csrc/sg_esp.h"

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

static sg_esp_batch good() {
    sg_esp_batch b;
    std::memset(&b, 0, sizeof b);
    b.count = 4;
    b.num_sas = 2;
    b.align = 4;
    b.uniform_next_header = 4;
    b.keys = at<const uint8_t>(0x1000);
    b.salts = at<const uint8_t>(0x2000);
    b.spi = at<const uint32_t>(0x3000);
    b.seq = at<const uint64_t>(0x4000);
    b.seq_out = at<uint64_t>(0x5000);
    b.status = at<uint8_t>(0x6000);
    b.in = at<const uint8_t>(0x10001);  // packets lie at any address
    b.out = at<uint8_t>(0x20003);
    b.uniform_len = 1200;
    return b;
}

static void argument_rules() {
    using sg::esp::check_args;
    for (int open = 0; open < 2; ++open) {
        uint32_t max_len = 7;
        sg_esp_batch b = good();
        CHECK(check_args(&b, open, &max_len) == nullptr && max_len == 1200);
        CHECK(check_args(&b, open, nullptr) == nullptr);
        CHECK(check_args(nullptr, open, &max_len) != nullptr);
        b.flags = SG_ESP_KEEP_FAILED;
        CHECK(check_args(&b, open, &max_len) == nullptr);
        b.flags = 0x4;
        CHECK(check_args(&b, open, &max_len) != nullptr);
        b.flags = 0x80000001u;
        CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.keys = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.salts = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.spi = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.status = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.in = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.out = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.seq = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open == 0));
        b = good(); b.seq_out = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        // the trailer's two outputs go together (open)
        b = good(); b.payload_len = at<uint32_t>(0x7000); CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        b = good(); b.next_header_out = at<uint8_t>(0x7001); CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        b = good(); b.payload_len = at<uint32_t>(0x7000); b.next_header_out = at<uint8_t>(0x7001);
        b.sa_index = at<const uint32_t>(0x7100); b.iv = at<const uint64_t>(0x7200); b.next_header = at<const uint8_t>(0x7303);
        CHECK(check_args(&b, open, &max_len) == nullptr);
        // extended sequence numbers: open reads replay_top and window
        b = good(); b.flags = SG_ESP_ESN; CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        const uint32_t windows[] = {0u, 1u, 64u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xffffffffu};
        for (uint32_t w : windows) {
            b = good(); b.flags = SG_ESP_ESN; b.replay_top = at<const uint64_t>(0x9000); b.window = w;
            CHECK((check_args(&b, open, &max_len) == nullptr) == (open == 0 || (w >= 1u && w <= 0x80000000u)));
            b.flags = 0;  // without the flag neither is read
            CHECK(check_args(&b, open, &max_len) == nullptr);
        }
        for (uintptr_t o = 1; o < 8; ++o) {
            const bool odd4 = (o & 3) != 0;
            b = good(); b.salts = at<const uint8_t>(0x2000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.spi = at<const uint32_t>(0x3000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.sa_index = at<const uint32_t>(0x7000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.payload_len = at<uint32_t>(0x7000 + o); b.next_header_out = at<uint8_t>(0x7101);
            CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.len = at<const uint32_t>(0x7000 + o); b.max_len = 100; CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.seq = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.iv = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.seq_out = at<uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.replay_top = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.in_off = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.out_off = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.next_header = at<const uint8_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) == nullptr);  // bytes
        }
        for (uint32_t a = 0; a <= 600u; ++a) {
            b = good(); b.align = a;
            CHECK((check_args(&b, open, &max_len) == nullptr) == (a >= 4u && a <= 256u && a % 4u == 0u));
        }
        b = good(); b.align = 0xfffffffcu; CHECK(check_args(&b, open, &max_len) != nullptr);
        const uint32_t nhs[] = {0u, 59u, 255u, 256u, 0xffffffffu};
        for (uint32_t nh : nhs) {
            b = good(); b.uniform_next_header = nh;
            CHECK((check_args(&b, open, &max_len) == nullptr) == (nh <= 255u));
        }
        // the length bound: open on the packet; seal on 32 + P, for every align
        const uint32_t aligns[] = {4u, 8u, 16u, 64u, 252u, 256u};
        for (uint32_t a : aligns) {
            uint32_t limit = SG_ESP_MAX_PACKET_LEN;
            if (!open) {
                limit = 0;
                while (sg_esp_packet_len(limit + 1u, a) <= SG_ESP_MAX_PACKET_LEN) ++limit;
                CHECK(limit <= SG_ESP_MAX_PACKET_LEN - 34u && limit + 2u + a > SG_ESP_MAX_PACKET_LEN - 32u);
                if (a == 4u || a == 16u) CHECK(limit == SG_ESP_MAX_PACKET_LEN - 34u);
            }
            const uint32_t lens[] = {0u, limit, limit + 1u, 0xffffffdfu, 0xffffffffu};
            for (uint32_t l : lens) {
                b = good(); b.align = a; b.uniform_len = l;
                CHECK((check_args(&b, open, &max_len) == nullptr) == (l <= limit));
                if (l <= limit) CHECK(max_len == l);
                b = good(); b.align = a; b.len = at<const uint32_t>(0x7000); b.max_len = l; b.uniform_len = 0xffffffffu;
                CHECK((check_args(&b, open, &max_len) == nullptr) == (l <= limit));
            }
        }
        b = good(); b.num_sas = 0; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.num_sas = 0xffffffffu; CHECK(check_args(&b, open, &max_len) == nullptr);
        b = good(); b.count = 0; b.keys = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);  // checked for an empty call too
    }
}

static void length_functions() {
    for (uint32_t a = 0; a <= 260u; ++a)
        for (uint32_t len = 0; len <= 3100u; ++len) {
            const uint32_t p = sg_esp_padded_len(len, a), d = a ? a : 1u;
            CHECK(p >= len + 2u && p - len - 2u < d && p % d == 0u);
            CHECK(p == sg::esp::padded_len(len, a) && p - len - 2u == sg::esp::pad_len(len, a));
            CHECK(sg_esp_packet_len(len, a) == p + 32u);
        }
    const uint32_t aligns[] = {0u, 1u, 4u, 16u, 252u, 256u, 0x80000000u, 0xffffffffu};
    const uint32_t ends[] = {0xffffff00u, 0xffffffd9u, 0xffffffdau, 0xffffffdbu, 0xffffffdfu, 0xfffffff9u, 0xfffffffau,
                             0xfffffffbu, 0xfffffffdu, 0xfffffffeu, 0xffffffffu};
    for (uint32_t a : aligns)
        for (uint32_t len : ends) {
            const uint64_t d = a ? a : 1u;
            const uint64_t want = ((uint64_t)len + 2u + d - 1u) / d * d;
            const uint32_t p = sg_esp_padded_len(len, a);
            CHECK(p == (want > 0xffffffffull ? 0xffffffffu : (uint32_t)want));  // never below len + 2, never wrapped
            CHECK(sg_esp_packet_len(len, a) == (p > 0xffffffffu - 32u ? 0xffffffffu : p + 32u));
        }
    CHECK(sg_esp_padded_len(84, 4) == 88u && sg_esp_packet_len(0, 4) == 36u && sg_esp_packet_len(0, 256) == 288u);
}

// the one 64-bit number with the low bits lo in [T - W + 1, T - W + 1 + 2^32), mod 2^64
static uint32_t hi_by_interval(uint64_t top, uint32_t w, uint32_t lo) {
    const uint64_t start = top - w + 1u;
    return (uint32_t)((start + (uint32_t)(lo - (uint32_t)start)) >> 32);
}

static void seq_hi_edges() {
    const uint32_t ws[] = {1u, 2u, 3u, 64u, 1024u, 0x7fffffffu, 0x80000000u};
    const uint32_t ths[] = {0u, 1u, 5u, 0xfffffffeu, 0xffffffffu};
    for (uint32_t w : ws)
        for (uint32_t th : ths) {
            const uint32_t tls[] = {0u, 1u, w - 2u, w - 1u, w, w + 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
            for (uint32_t tl : tls) {
                const uint64_t top = ((uint64_t)th << 32) | tl;
                const uint32_t bl = tl - w + 1u;
                const uint32_t los[] = {0u, 1u, bl - 2u, bl - 1u, bl, bl + 1u, tl - 1u, tl, tl + 1u, 0x7fffffffu, 0x80000000u,
                                        0xfffffffeu, 0xffffffffu};
                for (uint32_t lo : los) {
                    CHECK(sg_esp_seq_hi(top, w, lo) == hi_by_interval(top, w, lo));
                    CHECK(sg_esp_seq_hi(top, w, lo) == sg::esp::seq_hi(top, w, lo));
                }
                CHECK(sg_esp_seq_hi(top, w, tl) == th);  // the top itself
            }
        }
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < 200000; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint64_t top = x;
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint32_t w = (uint32_t)(x % 0x80000000ull) + 1u, lo = (uint32_t)(x >> 32);
        CHECK(sg_esp_seq_hi(top, w, lo) == hi_by_interval(top, w, lo));
    }
    // a window of 0 or above 2^31 is rejected by the calls; the function itself still returns
    (void)sg_esp_seq_hi(0, 0, 0);
    (void)sg_esp_seq_hi(0xffffffffffffffffull, 0xffffffffu, 0xffffffffu);
}

int main() {
    argument_rules();
    length_functions();
    seq_hi_edges();
    std::printf("esp sanitizer checks passed\n");
    return 0;
}
