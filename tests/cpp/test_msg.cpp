// The long-message dispatch of include/suruga/cipher.hpp: Encryptor::encrypt /
// Decryptor::decrypt above the single-record bounds (data > 32 KiB, AD > 255
// bytes; cipher/mod.rs:22-32 takes any length) go through sg_seal_msg /
// sg_open_msg, checked byte for byte against the CPU parity checker
// (oracle/suruga_oracle.c).  Needs an MI355X.
//
// Driven by tests/test_gpu_msg.py.  Exit status = number of failed checks.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/suruga/cipher.hpp"
#include "../../oracle/suruga_oracle.h"

using namespace suruga;

static int g_failed = 0, g_run = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_run;                                                                           \
        if (!(cond)) {                                                                     \
            ++g_failed;                                                                    \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                                  \
    } while (0)

static Bytes pattern(size_t n, uint32_t seed) {
    Bytes v(n);
    uint32_t x = seed;
    for (size_t i = 0; i < n; ++i) {
        x = x * 1664525u + 1013904223u;
        v[i] = (uint8_t)(x >> 24);
    }
    return v;
}

int main() {
    const Bytes key = pattern(32, 1), nonce = pattern(8, 2);
    const Bytes pt = pattern(40000, 3), ad = pattern(300, 4);  // both above the single-record bounds
    ChaCha20Poly1305 aead(0);
    auto enc = aead.new_encryptor(key);
    auto dec = aead.new_decryptor(key);

    Bytes want(pt.size() + 16);
    so_seal(key.data(), nonce.data(), pt.data(), pt.size(), ad.data(), ad.size(), want.data());
    const Bytes sealed = enc->encrypt(nonce, pt, ad);
    CHECK(sealed == want);
    CHECK(dec->decrypt(nonce, sealed, ad) == pt);

    // each bound alone
    const Bytes short_ad = pattern(13, 5);
    Bytes want2(pt.size() + 16);
    so_seal(key.data(), nonce.data(), pt.data(), pt.size(), short_ad.data(), short_ad.size(), want2.data());
    CHECK(enc->encrypt(nonce, pt, short_ad) == want2);
    const Bytes small = pattern(100, 6);
    Bytes want3(small.size() + 16);
    so_seal(key.data(), nonce.data(), small.data(), small.size(), ad.data(), ad.size(), want3.data());
    CHECK(enc->encrypt(nonce, small, ad) == want3);
    CHECK(dec->decrypt(nonce, want3, ad) == small);

    // a tampered long message is BadRecordMac "wrong mac" (chacha20_poly1305.rs:89-90)
    Bytes bad = sealed;
    bad[20000] ^= 1;
    bool threw = false;
    try {
        (void)dec->decrypt(nonce, bad, ad);
    } catch (const TlsError& e) {
        threw = e.kind == TlsErrorKind::BadRecordMac && e.desc == "wrong mac";
    }
    CHECK(threw);

    std::printf("%d checks, %d failed\n", g_run, g_failed);
    return g_failed;
}
