// test_quic_san.cpp -- the host-only code of the QUIC packet protection batch under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_quic_sanitizers.py builds
// this file, sg_quic_host.cpp and sg_keysched.cpp with g++ -fsanitize=address,undefined and
// runs the program directly; no GPU, no HIP header, nothing loaded into Python).
//
// The argument rules of sg_seal_batch_quic / sg_open_batch_quic (sg::quic::check_args: the
// struct is read, never what it points to, so the pointers here are small integers that a
// dereference would fault on), sg_quic_decode_pn over the edges of its arithmetic (shifts by
// 8 * pn_len, the comparisons next to 0 and to 2^62, any 64-bit expected_pn), and
// sg_quic_packet_keys over exact-size heap tables of `count` rows on several threads, its
// values against RFC 9001 appendix A.5 and against sg_hkdf_expand_label.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/suruga_gpu.h"
#include "../../suruga_amd/csrc/sg_err.h"
#include "../../suruga_amd/csrc/sg_quic.h"

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

static int g_fails = 0;
int sg::fail(int code, const char* fmt, const char*) {
    if (!fmt || !*fmt) std::exit(2);  // every failure carries a message
    ++g_fails;
    return code;
}

static std::unique_ptr<uint8_t[]> exact(size_t n, uint8_t fill) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
    std::memset(p.get(), fill, n ? n : 1);
    return p;
}

template <class T>
static T* at(uintptr_t a) {
    return reinterpret_cast<T*>(a);
}

static sg_quic_batch good() {
    sg_quic_batch b;
    std::memset(&b, 0, sizeof b);
    b.count = 4;
    b.num_keys = 2;
    b.keys = at<const uint8_t>(0x1000);
    b.ivs = at<const uint8_t>(0x2000);
    b.hp_keys = at<const uint8_t>(0x3000);
    b.pn = at<const uint64_t>(0x4000);
    b.pn_out = at<uint64_t>(0x5000);
    b.status = at<uint8_t>(0x6000);
    b.in = at<const uint8_t>(0x10001);  // packets lie at any address
    b.out = at<uint8_t>(0x20003);
    b.uniform_pn_off = 9;
    b.uniform_len = 1200;
    return b;
}

static void argument_rules() {
    using sg::quic::check_args;
    for (int open = 0; open < 2; ++open) {
        const uint32_t limit = SG_QUIC_MAX_PACKET_LEN - (open ? 0u : 16u);
        uint32_t max_len = 7;
        sg_quic_batch b = good();
        CHECK(check_args(&b, open, &max_len) == nullptr && max_len == 1200);
        CHECK(check_args(&b, open, nullptr) == nullptr);
        CHECK(check_args(nullptr, open, &max_len) != nullptr);
        b.flags = SG_QUIC_KEY_PHASE | SG_QUIC_KEEP_FAILED;
        CHECK(check_args(&b, open, &max_len) == nullptr);
        b.flags = 0x4;
        CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.keys = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.ivs = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.hp_keys = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.status = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.in = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.out = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.pn = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);
        b = good(); b.pn_out = nullptr; CHECK((check_args(&b, open, &max_len) != nullptr) == (open != 0));
        for (uintptr_t o = 1; o < 8; ++o) {
            b = good(); b.ivs = at<const uint8_t>(0x2000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == ((o & 3) != 0));
            b = good(); b.key_index = at<const uint32_t>(0x7000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == ((o & 3) != 0));
            b = good(); b.pn_off = at<const uint32_t>(0x7000 + o); CHECK((check_args(&b, open, &max_len) != nullptr) == ((o & 3) != 0));
            b = good(); b.len = at<const uint32_t>(0x7000 + o); b.max_len = 100; CHECK((check_args(&b, open, &max_len) != nullptr) == ((o & 3) != 0));
            b = good(); b.pn = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.pn_out = at<uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.in_off = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
            b = good(); b.out_off = at<const uint64_t>(0x8000 + o); CHECK(check_args(&b, open, &max_len) != nullptr);
        }
        const uint32_t offs[] = {0u, 1u, 251u, 252u, 0xffffffffu};
        for (uint32_t off : offs) {
            b = good(); b.uniform_pn_off = off;
            CHECK((check_args(&b, open, &max_len) == nullptr) == (off >= 1u && off <= SG_QUIC_MAX_PN_OFF));
            b.pn_off = at<const uint32_t>(0x7000);  // per-packet offsets: the uniform one is not read
            CHECK(check_args(&b, open, &max_len) == nullptr);
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
        b = good(); b.flags = SG_QUIC_KEY_PHASE; b.num_keys = 3; CHECK(check_args(&b, open, &max_len) != nullptr);
        b.num_keys = 0xfffffffeu; CHECK(check_args(&b, open, &max_len) == nullptr);
        b = good(); b.count = 0; b.keys = nullptr; CHECK(check_args(&b, open, &max_len) != nullptr);  // checked for an empty call too
    }
}

static void decode_pn_edges() {
    CHECK(sg_quic_decode_pn(0xa82f30eaull + 1, 0x9b32u, 2) == 0xa82f9b32ull);
    const uint64_t top = 1ull << 62;
    const uint64_t exps[] = {0, 1, 0x7f, 0x80, 0x81, 0xff, 0x100, 0x7fffffffull, 0x80000000ull, 0xffffffffull, 0x100000000ull,
                             top - 0x100000001ull, top - 0x100000000ull, top - 0x80000000ull, top - 257, top - 256, top - 128,
                             top - 1, top, (1ull << 63) - 1, 1ull << 63, ~0ull - 0x80000000ull, ~0ull};
    const uint32_t truncs[] = {0u, 1u, 0x7fu, 0x80u, 0xffu, 0x7fffu, 0x8000u, 0xffffu, 0x7fffffu, 0x800000u, 0xffffffu,
                               0x7fffffffu, 0x80000000u, 0xffffffffu};
    for (uint64_t e : exps)
        for (uint32_t t : truncs)
            for (uint32_t pn_len = 0; pn_len <= 6; ++pn_len) {
                const uint32_t nb = pn_len < 1 ? 1 : pn_len > 4 ? 4 : pn_len;
                const uint64_t win = 1ull << (8 * nb), got = sg_quic_decode_pn(e, t, pn_len);
                CHECK((got & (win - 1)) == (t & (win - 1)));  // the low bytes are the packet's
                CHECK(got == sg::quic::decode_pn(e, t, pn_len));
                if (e < top) {
                    CHECK(got < top);
                    const uint64_t d = got > e ? got - e : e - got;
                    // within half a window of the expected number, unless 0 or 2^62 is in the way
                    CHECK(d <= win / 2 || got < win || got >= top - win);
                }
            }
}

static void packet_keys() {
    const uint8_t secret[32] = {0x9a, 0xc3, 0x12, 0xa7, 0xf8, 0x77, 0x46, 0x8e, 0xbe, 0x69, 0x42, 0x27, 0x48, 0xad, 0x00, 0xa1,
                                0x54, 0x43, 0xf1, 0x82, 0x03, 0xa0, 0x7d, 0x60, 0x60, 0xf6, 0x88, 0xf3, 0x0f, 0x21, 0x63, 0x2b};
    const uint8_t key0[4] = {0xc6, 0xd9, 0x8f, 0xf3}, iv0[4] = {0xe0, 0x45, 0x9b, 0x34}, hp0[4] = {0x25, 0xa2, 0x82, 0xb9},
                  ku0[4] = {0x12, 0x23, 0x50, 0x47};  // RFC 9001 appendix A.5, the first bytes of each
    {
        auto s = exact(32, 0), k = exact(32, 0), v = exact(12, 0), h = exact(32, 0);
        std::memcpy(s.get(), secret, 32);
        CHECK(sg_quic_packet_keys(1, s.get(), k.get(), v.get(), h.get(), 0, 1) == SG_OK);
        CHECK(!std::memcmp(k.get(), key0, 4) && !std::memcmp(v.get(), iv0, 4) && !std::memcmp(h.get(), hp0, 4));
        CHECK(!std::memcmp(s.get(), secret, 32));
        CHECK(sg_quic_packet_keys(1, s.get(), nullptr, nullptr, nullptr, 1, 1) == SG_OK && !std::memcmp(s.get(), ku0, 4));
    }
    const uint32_t counts[] = {1, 2, 7, 64, 129};
    for (uint32_t count : counts)
        for (int update = 0; update < 2; ++update)
            for (int nt : {1, 3, 16, 1000}) {
                auto s = exact(32 * count, 0), k = exact(32 * count, 0xee), v = exact(12 * count, 0xee), h = exact(32 * count, 0xee);
                for (uint32_t i = 0; i < 32 * count; ++i) s[i] = (uint8_t)(i * 131u + count);
                std::vector<uint8_t> before(s.get(), s.get() + 32 * count);
                CHECK(sg_quic_packet_keys(count, s.get(), k.get(), v.get(), h.get(), update, nt) == SG_OK);
                for (uint32_t i = 0; i < count; ++i) {
                    uint8_t x[32], y[32];
                    std::memcpy(x, before.data() + 32u * i, 32);
                    if (update) {
                        CHECK(sg_hkdf_expand_label(before.data() + 32u * i, "quic ku", 7, nullptr, 0, x, 32) == SG_OK);
                    }
                    CHECK(!std::memcmp(x, s.get() + 32u * i, 32));
                    CHECK(sg_hkdf_expand_label(x, "quic key", 8, nullptr, 0, y, 32) == SG_OK && !std::memcmp(y, k.get() + 32u * i, 32));
                    CHECK(sg_hkdf_expand_label(x, "quic iv", 7, nullptr, 0, y, 12) == SG_OK && !std::memcmp(y, v.get() + 12u * i, 12));
                    CHECK(sg_hkdf_expand_label(x, "quic hp", 7, nullptr, 0, y, 32) == SG_OK && !std::memcmp(y, h.get() + 32u * i, 32));
                }
                // one table at a time: the others are not touched (NULL)
                auto s2 = exact(32 * count, 0), one = exact(32 * count, 0);
                std::memcpy(s2.get(), before.data(), 32 * count);
                CHECK(sg_quic_packet_keys(count, s2.get(), nullptr, nullptr, one.get(), 0, nt) == SG_OK);
                if (!update) CHECK(!std::memcmp(one.get(), h.get(), 32 * count));
                auto v2 = exact(12 * count, 0);
                CHECK(sg_quic_packet_keys(count, s2.get(), nullptr, v2.get(), nullptr, 0, nt) == SG_OK);
                if (!update) CHECK(!std::memcmp(v2.get(), v.get(), 12 * count));
            }
    auto s = exact(32, 1);
    const int fails = g_fails;
    CHECK(sg_quic_packet_keys(0, nullptr, nullptr, nullptr, nullptr, 0, 1) == SG_OK);
    CHECK(sg_quic_packet_keys(1, s.get(), nullptr, nullptr, nullptr, 0, 1) == SG_E_ARG);
    CHECK(sg_quic_packet_keys(1, nullptr, s.get(), nullptr, nullptr, 0, 1) == SG_E_ARG);
    CHECK(g_fails == fails + 2);
    CHECK(sg_quic_packet_keys(1, s.get(), nullptr, nullptr, nullptr, 1, 0) == SG_OK);  // threads below 1 run as one
}

int main() {
    argument_rules();
    decode_pn_edges();
    packet_keys();
    std::printf("quic sanitizer checks passed\n");
    return 0;
}
