// test_hkdf_san.cpp -- the host HKDF calls of sg_keysched.cpp under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_hkdf_sanitizers.py
// builds this file and sg_keysched.cpp with g++ -fsanitize=address,undefined and
// runs the program directly; no GPU, no HIP header, nothing loaded into Python).
//
// Every buffer is a heap allocation of exactly the size the call may touch, so
// one byte read or written outside it is a report: the bounds of
// sg_hkdf_expand_label (label 249, context 255, output 255 * 32 bytes and one
// more of each), outputs of exactly out_len bytes, sg_hkdf_extract's salts, and
// sg_tls13_traffic_keys over exact-size tables of `count` rows on several
// threads.  Values are checked where a known answer exists (RFC 5869 A.1, and
// the three ways one row can be computed agreeing with each other).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/suruga_gpu.h"
#include "../../suruga_amd/csrc/sg_err.h"

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

// n bytes on the heap, exactly (n == 0: a one-byte allocation that is never to be touched, passed as is)
static std::unique_ptr<uint8_t[]> exact(size_t n, uint8_t fill) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
    std::memset(p.get(), fill, n ? n : 1);
    return p;
}

static void expand_label_bounds() {
    auto secret = exact(32, 0x11);
    const size_t labels[] = {0, 1, 11, 249}, contexts[] = {0, 32, 255}, outs[] = {0, 1, 31, 32, 33, 64, 8160};
    for (size_t ll : labels)
        for (size_t cl : contexts)
            for (size_t ol : outs) {
                auto label = exact(ll, 'a'), context = exact(cl, 0xc7), out = exact(ol, 0xee);
                CHECK(sg_hkdf_expand_label(secret.get(), ll ? (const char*)label.get() : nullptr, ll,
                                           cl ? context.get() : nullptr, cl, ol ? out.get() : nullptr, ol) == SG_OK);
                if (ol >= 32) {  // nothing depends on what the output buffer held before
                    auto again = exact(ol, 0);
                    CHECK(sg_hkdf_expand_label(secret.get(), (const char*)label.get(), ll, context.get(), cl, again.get(),
                                               ol) == SG_OK);
                    CHECK(std::memcmp(out.get(), again.get(), ol) == 0);
                }
            }
    auto label = exact(250, 'a'), context = exact(256, 1), out = exact(8161, 0);
    const int before = g_fails;
    CHECK(sg_hkdf_expand_label(secret.get(), (const char*)label.get(), 250, context.get(), 0, out.get(), 32) == SG_E_ARG);
    CHECK(sg_hkdf_expand_label(secret.get(), (const char*)label.get(), 3, context.get(), 256, out.get(), 32) == SG_E_ARG);
    CHECK(sg_hkdf_expand_label(secret.get(), (const char*)label.get(), 3, context.get(), 0, out.get(), 8161) == SG_E_ARG);
    CHECK(sg_hkdf_expand_label(nullptr, (const char*)label.get(), 3, nullptr, 0, out.get(), 32) == SG_E_ARG);
    CHECK(sg_hkdf_expand_label(secret.get(), nullptr, 3, nullptr, 0, out.get(), 32) == SG_E_ARG);
    CHECK(sg_hkdf_expand_label(secret.get(), (const char*)label.get(), 3, nullptr, 4, out.get(), 32) == SG_E_ARG);
    CHECK(sg_hkdf_expand_label(secret.get(), (const char*)label.get(), 3, nullptr, 0, nullptr, 32) == SG_E_ARG);
    CHECK(g_fails == before + 7);
    CHECK(out[0] == 0 && out[8160] == 0);
}

static void extract_salts() {
    // RFC 5869 appendix A.1
    uint8_t ikm[22], salt[13];
    std::memset(ikm, 0x0b, sizeof ikm);
    for (int i = 0; i < 13; ++i) salt[i] = (uint8_t)i;
    const uint8_t want[32] = {0x07, 0x77, 0x09, 0x36, 0x2c, 0x2e, 0x32, 0xdf, 0x0d, 0xdc, 0x3f, 0x0d, 0xc4, 0x7b, 0xba, 0x63,
                              0x90, 0xb6, 0xc7, 0x3b, 0xb5, 0x0f, 0x9c, 0x31, 0x22, 0xec, 0x84, 0x4a, 0xd7, 0xc2, 0xb3, 0xe5};
    auto prk = exact(32, 0);
    CHECK(sg_hkdf_extract(salt, 13, ikm, 22, prk.get()) == SG_OK && std::memcmp(prk.get(), want, 32) == 0);
    auto none = exact(32, 0xff), zeros = exact(32, 0), z32 = exact(32, 0);
    CHECK(sg_hkdf_extract(nullptr, 0, ikm, 22, none.get()) == SG_OK);
    CHECK(sg_hkdf_extract(z32.get(), 32, ikm, 22, zeros.get()) == SG_OK);
    CHECK(std::memcmp(none.get(), zeros.get(), 32) == 0);  // no salt = 32 zero bytes
    auto s64 = exact(64, 0x5a), s65 = exact(65, 0x5a);
    CHECK(sg_hkdf_extract(s64.get(), 64, nullptr, 0, prk.get()) == SG_OK);  // empty ikm
    CHECK(sg_hkdf_extract(s65.get(), 65, ikm, 22, prk.get()) == SG_E_ARG);
    CHECK(sg_hkdf_extract(nullptr, 4, ikm, 22, prk.get()) == SG_E_ARG);
    CHECK(sg_hkdf_extract(nullptr, 0, nullptr, 22, prk.get()) == SG_E_ARG);
    CHECK(sg_hkdf_extract(nullptr, 0, ikm, 22, nullptr) == SG_E_ARG);
}

static void traffic_tables() {
    const uint32_t counts[] = {1, 5, 64, 257};
    const int threads[] = {1, 3, 16};
    for (uint32_t count : counts)
        for (int nt : threads)
            for (int update = 0; update < 2; ++update) {
                auto secrets = exact(32u * count, 0), keys = exact(32u * count, 0xa5), ivs = exact(12u * count, 0xa5);
                for (uint32_t i = 0; i < 32u * count; ++i) secrets[i] = (uint8_t)(i * 0x9d + (i >> 8) + count);
                std::memset(secrets.get(), 0, 32);
                if (count > 1) std::memset(secrets.get() + 32, 0xff, 32);
                std::vector<uint8_t> before(secrets.get(), secrets.get() + 32u * count);
                CHECK(sg_tls13_traffic_keys(count, secrets.get(), keys.get(), ivs.get(), update, nt) == SG_OK);
                for (uint32_t i = 0; i < count; ++i) {
                    // the same row through the general Expand-Label
                    uint8_t s[32], k[32], v[12];
                    std::memcpy(s, before.data() + 32u * i, 32);
                    if (update) CHECK(sg_hkdf_expand_label(before.data() + 32u * i, "traffic upd", 11, nullptr, 0, s, 32) == SG_OK);
                    CHECK(std::memcmp(s, secrets.get() + 32u * i, 32) == 0);
                    CHECK(sg_hkdf_expand_label(s, "key", 3, nullptr, 0, k, 32) == SG_OK && std::memcmp(k, keys.get() + 32u * i, 32) == 0);
                    CHECK(sg_hkdf_expand_label(s, "iv", 2, nullptr, 0, v, 12) == SG_OK && std::memcmp(v, ivs.get() + 12u * i, 12) == 0);
                }
                // either table alone
                auto s2 = exact(32u * count, 0), k2 = exact(32u * count, 0), v2 = exact(12u * count, 0);
                std::memcpy(s2.get(), before.data(), 32u * count);
                CHECK(sg_tls13_traffic_keys(count, s2.get(), k2.get(), nullptr, update, nt) == SG_OK);
                CHECK(std::memcmp(k2.get(), keys.get(), 32u * count) == 0);
                std::memcpy(s2.get(), before.data(), 32u * count);
                CHECK(sg_tls13_traffic_keys(count, s2.get(), nullptr, v2.get(), update, nt) == SG_OK);
                CHECK(std::memcmp(v2.get(), ivs.get(), 12u * count) == 0);
            }
    auto s = exact(32, 1);
    CHECK(sg_tls13_traffic_keys(0, nullptr, nullptr, nullptr, 0, 1) == SG_OK);
    CHECK(sg_tls13_traffic_keys(1, s.get(), nullptr, nullptr, 0, 1) == SG_E_ARG);
    CHECK(sg_tls13_traffic_keys(1, nullptr, s.get(), nullptr, 0, 1) == SG_E_ARG);
    CHECK(sg_tls13_traffic_keys(1, s.get(), nullptr, nullptr, 1, 0) == SG_OK);  // threads below 1 run as one
}

int main() {
    expand_label_bounds();
    extract_salts();
    traffic_tables();
    std::printf("hkdf sanitizer checks passed\n");
    return 0;
}
