// sg_hkdf.h -- what the host key schedule (sg_keysched.cpp) and the device key
// table kernel (sg_hkdf.hip) share of the TLS 1.3 traffic-key derivation
// (RFC 8446 section 7.1 - 7.3 over RFC 5869 with SHA-256): the SHA-256
// compression, the HkdfLabel bytes, the message blocks built from the label
// strings at compile time, and the derivation of one row.  No HIP header: the
// host file builds with a plain host compiler (tests/cpp/test_hkdf_san.cpp).
//
// One row, with S the 32-byte traffic secret and L(label, n) the HkdfLabel
//   be16(n) || u8(6 + |label|) || "tls13 " || label || u8(0)       (empty context)
// is T(1) of HKDF-Expand: HMAC(S, L || 01), cut to n bytes (n <= 32).  HMAC with
// a 32-byte key hashes two fixed 64-byte prefix blocks, S ^ ipad and S ^ opad:
// their two midstates are computed once per secret (hmac_mid, 2 compressions)
// and every label of that secret costs 2 more (expand1): the inner hash's second
// block L || 01 || 80 || 0.. || be64(bits), which is the same for every row and
// is built here from the label string (inner_block), and the outer hash's second
// block, the inner digest with its padding.  Without a ratchet that is
// 2 + 2 * 2 = 6 compressions per row, with one 2 + 2 + 2 + 4 = 10.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_HKDF_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define SG_HKDF_FN inline
#endif
// the 64 rounds are written as one loop and unrolled in full, so that every
// index of the 16-word rolling schedule is a constant (no private memory)
#if defined(__clang__)
#define SG_HKDF_UNROLL _Pragma("unroll")
#else
#define SG_HKDF_UNROLL _Pragma("GCC unroll 64")
#endif

namespace sg {
namespace hkdf {

// ---- SHA-256 (FIPS 180-4) ---------------------------------------------------
constexpr uint32_t kK[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
constexpr uint32_t kH0[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                             0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};

SG_HKDF_FN uint32_t rotr(uint32_t x, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(x, x, n);  // v_alignbit_b32
#else
    return (x >> n) | (x << (32u - n));
#endif
}

// st <- compress(st, w): w holds the block's 16 big-endian words and is used up
// as the rolling message schedule.
SG_HKDF_FN void compress(uint32_t st[8], uint32_t w[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    SG_HKDF_UNROLL
    for (int i = 0; i < 64; ++i) {
        if (i >= 16) {
            const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
            w[i & 15] += (rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3)) + w[(i + 9) & 15] +
                         (rotr(y, 17) ^ rotr(y, 19) ^ (y >> 10));
        }
        const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kK[i] + w[i & 15];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// ---- HkdfLabel (RFC 8446 section 7.1) -----------------------------------------
constexpr size_t kMaxLabel = 249;    // u8(6 + label_len)
constexpr size_t kMaxContext = 255;  // u8(context_len)
constexpr size_t kMaxInfo = 2 + 1 + 6 + kMaxLabel + 1 + kMaxContext;
constexpr size_t kMaxOut = 255 * 32;  // RFC 5869 section 2.3

// The label prefix, six bytes in either protocol: TLS 1.3's (RFC 8446 section 7.1) and
// DTLS 1.3's (RFC 9147 section 5.9, no trailing space).
constexpr char kPrefixTls13[7] = "tls13 ";
constexpr char kPrefixDtls13[7] = "dtls13";

// out <- be16(out_len) || u8(6 + label_len) || prefix || label || u8(context_len) || context;
// returns its length (at most kMaxInfo; the bounds are the caller's to check)
constexpr size_t hkdf_label(uint8_t* out, size_t out_len, const char* label, size_t label_len,
                            const uint8_t* context, size_t context_len, const char (&prefix)[7] = kPrefixTls13) {
    size_t n = 0;
    out[n++] = (uint8_t)(out_len >> 8);
    out[n++] = (uint8_t)out_len;
    out[n++] = (uint8_t)(6 + label_len);
    for (size_t i = 0; i < 6; ++i) out[n++] = (uint8_t)prefix[i];
    for (size_t i = 0; i < label_len; ++i) out[n++] = (uint8_t)label[i];
    out[n++] = (uint8_t)context_len;
    for (size_t i = 0; i < context_len; ++i) out[n++] = context[i];
    return n;
}

struct Block {
    uint32_t w[16];
};

// The second block of the inner hash of T(1) = HMAC(S, L(label, out_len) || 01):
// the label, the counter byte, SHA-256's padding and the bit length of the 64
// prefix bytes and the message.  The label must leave room for the padding in
// this one block (the three below do: static_assert).
constexpr size_t inner_message_len(size_t label_len) { return 2 + 1 + 6 + label_len + 1 + 1; }
template <size_t N>
constexpr Block inner_block(const char (&label)[N], size_t out_len) {
    static_assert(inner_message_len(N - 1) + 1 + 8 <= 64, "label too long for one block");
    uint8_t b[64] = {};
    size_t n = hkdf_label(b, out_len, label, N - 1, nullptr, 0);
    b[n++] = 0x01;
    const size_t bits = 8 * (64 + n);
    b[n] = 0x80;
    b[62] = (uint8_t)(bits >> 8);
    b[63] = (uint8_t)bits;
    Block r = {};
    for (size_t i = 0; i < 16; ++i)
        r.w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
    return r;
}

constexpr size_t kTrafficKeyLen = 32, kTrafficIvLen = 12;
enum Label { kLabelKey = 0, kLabelIv = 1, kLabelUpdate = 2 };
constexpr Block label_block(int which) {
    return which == kLabelKey ? inner_block("key", kTrafficKeyLen)
           : which == kLabelIv ? inner_block("iv", kTrafficIvLen)
                               : inner_block("traffic upd", 32);
}

// ---- one secret -------------------------------------------------------------
// Midstates of HMAC under the 32-byte key s (8 big-endian words): the states
// after the blocks s ^ ipad and s ^ opad.
SG_HKDF_FN void hmac_mid(const uint32_t s[8], uint32_t ist[8], uint32_t ost[8]) {
    uint32_t w[16];
    SG_HKDF_UNROLL
    for (int i = 0; i < 16; ++i) w[i] = (i < 8 ? s[i] : 0u) ^ 0x36363636u;
    SG_HKDF_UNROLL
    for (int i = 0; i < 8; ++i) ist[i] = kH0[i];
    compress(ist, w);
    SG_HKDF_UNROLL
    for (int i = 0; i < 16; ++i) w[i] = (i < 8 ? s[i] : 0u) ^ 0x5c5c5c5cu;
    SG_HKDF_UNROLL
    for (int i = 0; i < 8; ++i) ost[i] = kH0[i];
    compress(ost, w);
}

// out <- the 32 bytes of T(1) for label W under the key whose midstates are ist / ost
template <int W>
SG_HKDF_FN void expand1(const uint32_t ist[8], const uint32_t ost[8], uint32_t out[8]) {
    constexpr Block blk = label_block(W);
    uint32_t w[16], h[8];
    SG_HKDF_UNROLL
    for (int i = 0; i < 16; ++i) w[i] = blk.w[i];
    SG_HKDF_UNROLL
    for (int i = 0; i < 8; ++i) h[i] = ist[i];
    compress(h, w);
    SG_HKDF_UNROLL
    for (int i = 0; i < 16; ++i) w[i] = i < 8 ? h[i] : 0u;
    w[8] = 0x80000000u;
    w[15] = 8u * (64u + 32u);
    SG_HKDF_UNROLL
    for (int i = 0; i < 8; ++i) out[i] = ost[i];
    compress(out, w);
}

// RFC 8446 section 7.2 / 7.3 for one connection, everything in big-endian words:
//   update:    s <- Expand-Label(s, "traffic upd", "", 32)   (first)
//   want_key:  key    <- Expand-Label(s, "key", "", 32)
//   want_iv:   iv[0..3) <- Expand-Label(s, "iv", "", 12)     (iv[3..8) is not part of it)
SG_HKDF_FN void traffic_row(uint32_t s[8], bool update, bool want_key, bool want_iv, uint32_t key[8],
                            uint32_t iv[8]) {
    uint32_t ist[8], ost[8];
    hmac_mid(s, ist, ost);
    if (update) {
        expand1<kLabelUpdate>(ist, ost, s);
        hmac_mid(s, ist, ost);
    }
    if (want_key) expand1<kLabelKey>(ist, ost, key);
    if (want_iv) expand1<kLabelIv>(ist, ost, iv);
}

}  // namespace hkdf
}  // namespace sg
