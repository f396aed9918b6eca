// test_dtls13_san.cpp -- the host-only code of the DTLS 1.3 record batch under AddressSanitizer
// and UndefinedBehaviorSanitizer (tests/test_dtls13_sanitizers.py builds this file and
// sg_dtls13_host.cpp with g++ -fsanitize=address,undefined and runs the program directly; no
// GPU, no HIP header, nothing loaded into Python).
//
// The argument rules of sg_seal_batch_dtls13 / sg_open_batch_dtls13 (sg::dtls13::check_args:
// the struct is read, never what it points to, so the pointers here are small integers that
// a dereference would fault on), sg_dtls13_header_len / sg_dtls13_inner_len /
// sg_dtls13_record_len over every length of a few MTUs, every pad_to and the ends of 32
// bits, where nothing may wrap, and the sequence number's reconstruction (sg_quic.h's
// decode_pn at one and two bytes) against the interval it is defined by.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/suruga_gpu.h"
#include "../../suruga_amd/csrc/sg_dtls13.h"

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

static sg_dtls13_batch good() {
    sg_dtls13_batch b;
    std::memset(&b, 0, sizeof b);
    b.count = 4;
    b.num_conns = 2;
    b.cid_len = 8;
    b.uniform_type = 23;
    b.keys = at<const uint8_t>(0x1000);
    b.ivs = at<const uint8_t>(0x2000);
    b.sn_keys = at<const uint8_t>(0x3000);
    b.cids = at<const uint8_t>(0x3801);
    b.seq = at<const uint64_t>(0x4000);
    b.expected = at<const uint64_t>(0x4800);
    b.seq_out = at<uint64_t>(0x5000);
    b.epoch_out = at<uint8_t>(0x5801);
    b.content_len = at<uint32_t>(0x5c00);
    b.type_out = at<uint8_t>(0x5e03);
    b.status = at<uint8_t>(0x6000);
    b.in = at<const uint8_t>(0x10001);  // records lie at any address
    b.out = at<uint8_t>(0x20003);
    b.uniform_len = 1200;
    return b;
}

static void argument_rules() {
    using sg::dtls13::check_args;
    for (int open = 0; open < 2; ++open) {
        uint32_t max_len = 7;
        sg_dtls13_batch b = good();
        CHECK(check_args(&b, open, &max_len) == nullptr && max_len == 1200);
        CHECK(check_args(&b, open, nullptr) == nullptr);
        CHECK(check_args(nullptr, open, &max_len) != nullptr);
        for (uint32_t f = 0; f < 16u; ++f) {
            b.flags = f;
            CHECK(check_args(&b, open, &max_len) == nullptr);
        }
        b.flags = 0x10;
        CHECK(check_args(&b, open, &max_len) != nullptr);
        b.flags = 0x80000001u;
        CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.keys = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.ivs = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.sn_keys = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.status = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.in = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.out = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        // what only one direction reads
        b = good(); b.seq = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open == 0));
        b = good(); b.cids = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open == 0));
        b = good(); b.cids = nullptr; b.cid_len = 0; CHECK(check_args(&b, open, &max_len) == nullptr);
        b = good(); b.expected = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        b = good(); b.seq_out = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        b = good(); b.epoch_out = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        b = good(); b.content_len = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        b = good(); b.type_out = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        b = good(); b.key_index = at<const uint32_t>(0x7100); b.type = at<const uint8_t>(0x7201); b.epoch = at<const uint8_t>(0x7303);
        CHECK(check_args(&b, open, &max_len) == nullptr);
        for (uintptr_t o = 1; o < 8; ++o) {
            const bool odd4 = (o & 3) != 0;
            b = good(); b.ivs = at<const uint8_t>(0x2000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.key_index = at<const uint32_t>(0x7000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.content_len = at<uint32_t>(0x7000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.len = at<const uint32_t>(0x7000 + o); b.max_len = 1200; CHECK((check_args(&b, open, &max_len) != nullptr) == odd4);
            b = good(); b.seq = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.expected = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.seq_out = at<uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.in_off = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.out_off = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            // bytes lie anywhere
            b = good(); b.keys = at<const uint8_t>(0x1000 + o); b.sn_keys = at<const uint8_t>(0x3000 + o);
            b.type = at<const uint8_t>(0x7200 + o); b.epoch_out = at<uint8_t>(0x5800 + o);
            CHECK(check_args(&b, open, &max_len) == nullptr);
        }
        b = good(); b.num_conns = 0; CHECK(check_args(&b, open, &max_len) != nullptr);
        const uint32_t cids[] = {0u, 1u, 250u, 251u, 255u, 256u, 0xffffffffu};
        for (uint32_t c : cids) {
            b = good(); b.cid_len = c;
            CHECK((check_args(&b, open, &max_len) == nullptr) == (c <= SG_DTLS13_MAX_CID_LEN));
        }
        const uint32_t pads[] = {0u, 1u, 2u, 16u, 10000u, 16384u, 16385u, 0x80000000u, 0xffffffffu};
        for (uint32_t q : pads) {
            b = good(); b.pad_to = q;
            CHECK((check_args(&b, open, &max_len) == nullptr) == (q <= 16384u));
        }
        // the bound: open on the record, seal on the content
        const uint32_t limit = open ? SG_DTLS13_MAX_RECORD_LEN : SG_DTLS13_MAX_CONTENT_LEN;
        b = good(); b.uniform_len = limit; CHECK(check_args(&b, open, &max_len) == nullptr && max_len == limit);
        b.uniform_len = limit + 1u; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.len = at<const uint32_t>(0x9000); b.uniform_len = 0xffffffffu; b.max_len = limit;
        CHECK(check_args(&b, open, &max_len) == nullptr && max_len == limit);  // with a length array uniform_len is not read
        b.max_len = limit + 1u; CHECK(check_args(&b, open, &max_len) != nullptr);
        b.max_len = 0xffffffffu; CHECK(check_args(&b, open, &max_len) != nullptr);
    }
}

static void lengths() {
    const uint32_t pads[] = {0u, 1u, 2u, 3u, 16u, 64u, 100u, 256u, 4096u, 10000u, 16384u};
    for (uint32_t pad_to : pads) {
        for (uint32_t n = 0; n <= 17000u; ++n) {
            const uint32_t inner = sg_dtls13_inner_len(n, pad_to);
            CHECK(inner >= n + 1u);  // the type byte always fits
            if (pad_to <= 1u || n >= 16384u) {
                CHECK(inner == n + 1u);
            } else {
                CHECK(inner <= 16385u && inner < n + 1u + pad_to);
                CHECK(inner % pad_to == 0u || inner == 16385u);
            }
            CHECK(sg_dtls13_record_len(n, pad_to, 0u, 0u) == 2u + inner + 16u);
            CHECK(sg_dtls13_record_len(n, pad_to, SG_DTLS13_SEQ16 | SG_DTLS13_LENGTH, 250u) == 255u + inner + 16u);
        }
    }
    for (uint32_t f = 0; f < 16u; ++f)
        for (uint32_t c = 0; c <= 250u; ++c)
            CHECK(sg_dtls13_header_len(f, c) == 1u + c + ((f & SG_DTLS13_SEQ16) ? 2u : 1u) + ((f & SG_DTLS13_LENGTH) ? 2u : 0u));
    CHECK(sg_dtls13_header_len(3u, 0xffffffffu) == 0xffffffffu && sg_dtls13_header_len(0u, 0xfffffffdu) == 0xffffffffu);
    CHECK(sg_dtls13_record_len(16384u, 0u, 3u, 250u) == SG_DTLS13_MAX_RECORD_LEN);
    // the ends of 32 bits: nothing wraps
    const uint32_t ends[] = {0xfffffff0u, 0xfffffffdu, 0xfffffffeu, 0xffffffffu};
    for (uint32_t n : ends) {
        for (uint32_t pad_to : pads) {
            CHECK(sg_dtls13_inner_len(n, pad_to) == (n == 0xffffffffu ? 0xffffffffu : n + 1u));
            CHECK(sg_dtls13_record_len(n, pad_to, 3u, 250u) == 0xffffffffu);
        }
    }
}

static void reconstruction() {
    using sg::quic::decode_pn;
    for (uint32_t nbytes = 1; nbytes <= 2u; ++nbytes) {
        const uint64_t win = 1ull << (8u * nbytes), h = win / 2u;
        const uint64_t expected[] = {0ull, 1ull, h - 1u, h, h + 1u, win, 5u * win + 77u, (1ull << 48) - 1u, (1ull << 48), (1ull << 60) + 3u};
        for (uint64_t e : expected) {
            for (uint64_t t = 0; t < win; ++t) {
                const uint64_t s = decode_pn(e, (uint32_t)t, nbytes);
                CHECK((s & (win - 1u)) == t);
                // in (e - h, e + h], or the nearest there is above zero
                const bool in_window = s + h > e && s <= e + h;
                CHECK(in_window || (s < win && s > e + h));
            }
            // every number of the window comes back from its low bits
            for (uint64_t d = 0; d < win; ++d) {
                if (e + h < d) continue;
                const uint64_t s = e + h - d;  // e + h down to e - h + 1
                CHECK(decode_pn(e, (uint32_t)(s & (win - 1u)), nbytes) == s);
            }
        }
    }
}

int main() {
    argument_rules();
    lengths();
    reconstruction();
    std::puts("dtls13 sanitizer checks passed");
    return 0;
}
