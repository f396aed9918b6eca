// sg_device.h -- device-side building blocks shared by the gfx950 kernels
// (sg_kernels.hip: size-class kernels, keying, bucketing; sg_wpr.hip and
// sg_wpr_keying.hip: the wave-per-record kernel for 4-16 KiB records and its keying; sg_pack.hip: the packed small
// records of mixed batches; sg_msg.hip: long messages; sg_plumb.hip: scrub).
// Not part of the public ABI.
//
//   ChaCha20 block function        klutzy/suruga src/crypto/chacha20.rs:25-135
//   Poly1305 field arithmetic      src/crypto/poly1305.rs:25-192 (exact mod 2^130-5)
//   tag = (h mod 2^128) + s        poly1305.rs:230-312
//   TLS nonce / additional data    src/tls.rs:103-112, 250-265
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sg_internal.h"

namespace sg {
namespace dev {

constexpr uint32_t M26 = (1u << 26) - 1;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }
__device__ __forceinline__ uint32_t uniform(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint32_t addc(uint32_t a, uint32_t b, uint32_t cin, uint32_t* cout) {
    return __builtin_addc(a, b, cin, cout);  // v_add_co / v_addc_co chain
}

// 16-byte accesses: aligned (global / LDS) and unaligned (LDS: one ds_read_b128)
__device__ __forceinline__ u32x4 ld16(const void* p) {
    return *reinterpret_cast<const u32x4*>(__builtin_assume_aligned(p, 16));
}
__device__ __forceinline__ void st16(void* p, u32x4 v) {
    *reinterpret_cast<u32x4*>(__builtin_assume_aligned(p, 16)) = v;
}
// Record bytes are read once and written once: the wave-per-record kernel
// moves them with the non-temporal policy (SG_STREAM_NT, default on): its
// LDS-DMA loads carry `nt` (SG_DMA_POL) and its lane-contiguous stores are
// nontemporal.  Same-box A/B on C1 (round 3): +1.5-1.7 % (seal 7.52 -> 7.42 ms,
// open 7.57 -> 7.44 ms).  The kernels whose lanes each move a 64-byte block
// (packed, size classes) keep the default policy (nt measured -1.3 % on C2).
#ifndef SG_STREAM_NT
#define SG_STREAM_NT 1
#endif
#if SG_STREAM_NT
#define SG_DMA_POL " nt"
#else
#define SG_DMA_POL ""
#endif
__device__ __forceinline__ u32x4 gld16(const void* p) {
    const u32x4* q = reinterpret_cast<const u32x4*>(__builtin_assume_aligned(p, 16));
    if constexpr (SG_STREAM_NT) return __builtin_nontemporal_load(q);
    return *q;
}
__device__ __forceinline__ void gst16(void* p, u32x4 v) {
    u32x4* q = reinterpret_cast<u32x4*>(__builtin_assume_aligned(p, 16));
    if constexpr (SG_STREAM_NT) {
        __builtin_nontemporal_store(v, q);
    } else {
        *q = v;
    }
}

typedef u32x4 u32x4_u __attribute__((aligned(1)));
__device__ __forceinline__ u32x4 ldu16(const void* p) { return *reinterpret_cast<const u32x4_u*>(p); }

// four bytes at any alignment -> little-endian word (chacha20.rs:37-39, 45-46)
__host__ __device__ __forceinline__ uint32_t le32(const uint8_t* b) {
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

// LDS writes of one lane visible to the other lanes of its wave, and no
// compiler reordering of LDS accesses across this point
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- ChaCha20 (chacha20.rs) ------------------------------------------------
// quarter round, chacha20.rs:63-81
#define SG_QR(a, b, c, d)                   \
    a += b; d ^= a; d = rotl32(d, 16);      \
    c += d; b ^= c; b = rotl32(b, 12);      \
    a += b; d ^= a; d = rotl32(d, 8);       \
    c += d; b ^= c; b = rotl32(b, 7);

// Wave-uniform variants for the scalar unit.  The SALU has no rotate and no
// byte swap: the opaque asm keeps the shift-or from being matched to
// v_alignbit / v_perm (which would move the whole uniform chain to the VALU).
__device__ __forceinline__ uint32_t srotl32(uint32_t x, int n) {
    uint32_t hi = x << n, lo = x >> (32 - n);
    asm volatile("" : "+s"(hi));
    return hi | lo;
}
__device__ __forceinline__ uint32_t sbswap32(uint32_t x) {
    uint32_t a = x << 24, b = (x << 8) & 0x00ff0000u;
    asm volatile("" : "+s"(a), "+s"(b));
    return a | b | ((x >> 8) & 0x0000ff00u) | (x >> 24);
}
#define SG_QR_S(a, b, c, d)                  \
    a += b; d ^= a; d = srotl32(d, 16);      \
    c += d; b ^= c; b = srotl32(b, 12);      \
    a += b; d ^= a; d = srotl32(d, 8);       \
    c += d; b ^= c; b = srotl32(b, 7);

constexpr uint32_t kSigma0 = 0x61707865u, kSigma1 = 0x3320646eu, kSigma2 = 0x79622d32u, kSigma3 = 0x6b206574u;

// One keystream block (chacha20.rs:25-51 state, :53-109 round20).  k[8] key
// words, ctr = state word 12, n13 = state word 13, n14/n15 = nonce words.
// ks[i] = round20(state)[i] (little-endian words).  Word 13 is 0 in the draft
// construction (chacha20.rs:114-121) and the first nonce word in RFC 8439
// (section 2.3): the Construction::kRfc8439 kernels.
__device__ __forceinline__ void chacha_block(uint32_t ks[16], const uint32_t k[8], uint32_t ctr, uint32_t n13,
                                             uint32_t n14, uint32_t n15) {
    uint32_t x0 = kSigma0, x1 = kSigma1, x2 = kSigma2, x3 = kSigma3;
    uint32_t x4 = k[0], x5 = k[1], x6 = k[2], x7 = k[3];
    uint32_t x8 = k[4], x9 = k[5], x10 = k[6], x11 = k[7];
    uint32_t x12 = ctr, x13 = n13, x14 = n14, x15 = n15;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        SG_QR(x0, x4, x8, x12) SG_QR(x1, x5, x9, x13) SG_QR(x2, x6, x10, x14) SG_QR(x3, x7, x11, x15)
        SG_QR(x0, x5, x10, x15) SG_QR(x1, x6, x11, x12) SG_QR(x2, x7, x8, x13) SG_QR(x3, x4, x9, x14)
    }
    ks[0] = x0 + kSigma0; ks[1] = x1 + kSigma1; ks[2] = x2 + kSigma2; ks[3] = x3 + kSigma3;
    ks[4] = x4 + k[0]; ks[5] = x5 + k[1]; ks[6] = x6 + k[2]; ks[7] = x7 + k[3];
    ks[8] = x8 + k[4]; ks[9] = x9 + k[5]; ks[10] = x10 + k[6]; ks[11] = x11 + k[7];
    ks[12] = x12 + ctr; ks[13] = x13 + n13; ks[14] = x14 + n14; ks[15] = x15 + n15;
}

// ---- uniform-record variant: the counter-free part of round 1 on the SALU ----
// Within one record only state word 12 (the block counter) differs between
// blocks.  The column quarter-rounds on words (1,5,9,13), (2,6,10,14),
// (3,7,11,15) and the first add of (0,4,8,12) are therefore the same for
// every block; when the record is wave-uniform (key and nonce in SGPRs) they
// are computed once on the scalar unit, which otherwise idles, instead of
// costing ~37 VALU per block (srotl32 / SG_QR_S).  Used by the size-class
// kernels (sg_kernels.hip) and the message kernels (sg_msg.hip).

struct ChaChaPre {
    uint32_t x[16];  // state after the counter-free part of round 1 (x12 unused)
};

// k, n13, n14, n15 must be wave-uniform.
__device__ __forceinline__ ChaChaPre chacha_pre(const uint32_t k[8], uint32_t n13, uint32_t n14, uint32_t n15) {
    uint32_t x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
    uint32_t x5 = k[1], x6 = k[2], x7 = k[3], x9 = k[5], x10 = k[6], x11 = k[7];
    uint32_t x13 = n13, x14 = n14, x15 = n15;
    SG_QR_S(x1, x5, x9, x13) SG_QR_S(x2, x6, x10, x14) SG_QR_S(x3, x7, x11, x15)
    return ChaChaPre{{0x61707865u + k[0], x1, x2, x3, k[0], x5, x6, x7, k[4], x9, x10, x11, 0u, x13, x14, x15}};
}

// Same result as chacha_block(ks, k, ctr, n13, n14, n15), starting from
// chacha_pre(k, n13, n14, n15).
__device__ __forceinline__ void chacha_block_pre(uint32_t ks[16], const ChaChaPre& P, const uint32_t k[8],
                                                 uint32_t ctr, uint32_t n13, uint32_t n14, uint32_t n15) {
    uint32_t x0 = P.x[0], x1 = P.x[1], x2 = P.x[2], x3 = P.x[3];
    uint32_t x4 = P.x[4], x5 = P.x[5], x6 = P.x[6], x7 = P.x[7];
    uint32_t x8 = P.x[8], x9 = P.x[9], x10 = P.x[10], x11 = P.x[11];
    uint32_t x12 = ctr, x13 = P.x[13], x14 = P.x[14], x15 = P.x[15];
    // rest of round 1, column (0,4,8,12): its first add is in x0 already
    x12 ^= x0; x12 = rotl32(x12, 16);
    x8 += x12; x4 ^= x8; x4 = rotl32(x4, 12);
    x0 += x4; x12 ^= x0; x12 = rotl32(x12, 8);
    x8 += x12; x4 ^= x8; x4 = rotl32(x4, 7);
    SG_QR(x0, x5, x10, x15) SG_QR(x1, x6, x11, x12) SG_QR(x2, x7, x8, x13) SG_QR(x3, x4, x9, x14)
#pragma unroll
    for (int r = 1; r < 10; ++r) {
        SG_QR(x0, x4, x8, x12) SG_QR(x1, x5, x9, x13) SG_QR(x2, x6, x10, x14) SG_QR(x3, x7, x11, x15)
        SG_QR(x0, x5, x10, x15) SG_QR(x1, x6, x11, x12) SG_QR(x2, x7, x8, x13) SG_QR(x3, x4, x9, x14)
    }
    ks[0] = x0 + 0x61707865u; ks[1] = x1 + 0x3320646eu; ks[2] = x2 + 0x79622d32u; ks[3] = x3 + 0x6b206574u;
    ks[4] = x4 + k[0]; ks[5] = x5 + k[1]; ks[6] = x6 + k[2]; ks[7] = x7 + k[3];
    ks[8] = x8 + k[4]; ks[9] = x9 + k[5]; ks[10] = x10 + k[6]; ks[11] = x11 + k[7];
    ks[12] = x12 + ctr; ks[13] = x13 + n13; ks[14] = x14 + n14; ks[15] = x15 + n15;
}

// ---- Poly1305 field arithmetic, radix 2^26 ---------------------------------
// Invariant of a "reduced" element: limbs 0,2,3,4 < 2^26, limb 1 < 2^26 + 2^8.
struct F26 {
    uint32_t v0, v1, v2, v3, v4;
};

__device__ __forceinline__ F26 f26_zero() { return F26{0u, 0u, 0u, 0u, 0u}; }
__device__ __forceinline__ F26 f26_one() { return F26{1u, 0u, 0u, 0u, 0u}; }
__device__ __forceinline__ F26 f26_add(const F26& a, const F26& b) {
    return F26{a.v0 + b.v0, a.v1 + b.v1, a.v2 + b.v2, a.v3 + b.v3, a.v4 + b.v4};
}
__device__ __forceinline__ void store_f26(uint32_t* p, const F26& x) {
    p[0] = x.v0; p[1] = x.v1; p[2] = x.v2; p[3] = x.v3; p[4] = x.v4;
}
__device__ __forceinline__ F26 load_f26(const uint32_t* p) { return F26{p[0], p[1], p[2], p[3], p[4]}; }

// a * b + c (mod p, reduced) -- the Int1305::mult of poly1305.rs:51-128 in
// one carry pass.  b reduced; a and c limbs < 2^27.
__device__ __forceinline__ F26 mul_add(const F26 a, const uint32_t b0, const uint32_t b1, const uint32_t b2,
                                       const uint32_t b3, const uint32_t b4, const F26 c) {
    const uint32_t s1 = b1 * 5u, s2 = b2 * 5u, s3 = b3 * 5u, s4 = b4 * 5u;
    F26 h;
    uint64_t d = (uint64_t)c.v0 + (uint64_t)a.v0 * b0 + (uint64_t)a.v1 * s4 + (uint64_t)a.v2 * s3 +
                 (uint64_t)a.v3 * s2 + (uint64_t)a.v4 * s1;
    h.v0 = (uint32_t)d & M26;
    uint32_t cy = (uint32_t)(d >> 26);
    d = (uint64_t)(c.v1 + cy) + (uint64_t)a.v0 * b1 + (uint64_t)a.v1 * b0 + (uint64_t)a.v2 * s4 +
        (uint64_t)a.v3 * s3 + (uint64_t)a.v4 * s2;
    h.v1 = (uint32_t)d & M26;
    cy = (uint32_t)(d >> 26);
    d = (uint64_t)(c.v2 + cy) + (uint64_t)a.v0 * b2 + (uint64_t)a.v1 * b1 + (uint64_t)a.v2 * b0 +
        (uint64_t)a.v3 * s4 + (uint64_t)a.v4 * s3;
    h.v2 = (uint32_t)d & M26;
    cy = (uint32_t)(d >> 26);
    d = (uint64_t)(c.v3 + cy) + (uint64_t)a.v0 * b3 + (uint64_t)a.v1 * b2 + (uint64_t)a.v2 * b1 +
        (uint64_t)a.v3 * b0 + (uint64_t)a.v4 * s4;
    h.v3 = (uint32_t)d & M26;
    cy = (uint32_t)(d >> 26);
    d = (uint64_t)(c.v4 + cy) + (uint64_t)a.v0 * b4 + (uint64_t)a.v1 * b3 + (uint64_t)a.v2 * b2 +
        (uint64_t)a.v3 * b1 + (uint64_t)a.v4 * b0;
    h.v4 = (uint32_t)d & M26;
    cy = (uint32_t)(d >> 26);
    const uint64_t e = (uint64_t)h.v0 + (uint64_t)cy * 5u;  // 2^130 == 5 (mod p)
    h.v0 = (uint32_t)e & M26;
    h.v1 += (uint32_t)(e >> 26);
    return h;
}
__device__ __forceinline__ F26 fmul(const F26 a, const F26 b) { return mul_add(a, b.v0, b.v1, b.v2, b.v3, b.v4, f26_zero()); }
__device__ __forceinline__ F26 fmul_add(const F26 a, const F26 b, const F26 c) {
    return mul_add(a, b.v0, b.v1, b.v2, b.v3, b.v4, c);
}

// One radix-2^26 pass, limb 0 up to limb 4 and limb 4's carry times 5 back into limb 0
// (2^130 == 5 mod p): value unchanged mod p, limbs 1..4 < 2^26.
__device__ __forceinline__ void carry_pass(F26& f) {
    uint32_t c;
    c = f.v0 >> 26; f.v0 &= M26; f.v1 += c;
    c = f.v1 >> 26; f.v1 &= M26; f.v2 += c;
    c = f.v2 >> 26; f.v2 &= M26; f.v3 += c;
    c = f.v3 >> 26; f.v3 &= M26; f.v4 += c;
    c = f.v4 >> 26; f.v4 &= M26; f.v0 += c * 5u;
}

// One carry pass over limbs < 2^32 (value unchanged mod p): limbs < 2^26 + 2^8.
__device__ __forceinline__ F26 carry1(F26 f) {
    carry_pass(f);
    const uint32_t c = f.v0 >> 26;
    f.v0 &= M26;
    f.v1 += c;
    return f;
}

// Strict normal form: every limb < 2^26 (value < 2^130), for limbs < 2^32.
__device__ __forceinline__ F26 ripple_full(F26 h) {
    carry_pass(h);
    carry_pass(h);
    // a second-pass fold implies v1..v4 wrapped to 0, so this cannot overflow v1
    const uint32_t c = h.v0 >> 26;
    h.v0 &= M26;
    h.v1 += c;
    return h;
}

// Canonical representative in [0, p): subtract p when h >= p, branch-free
// (the role of Int1305::normalize, poly1305.rs:165-192).
__device__ __forceinline__ F26 canonical(F26 h) {
    h = ripple_full(h);
    uint32_t g0 = h.v0 + 5u, c = g0 >> 26; g0 &= M26;
    uint32_t g1 = h.v1 + c; c = g1 >> 26; g1 &= M26;
    uint32_t g2 = h.v2 + c; c = g2 >> 26; g2 &= M26;
    uint32_t g3 = h.v3 + c; c = g3 >> 26; g3 &= M26;
    uint32_t g4 = h.v4 + c;
    const uint32_t ge = 0u - (g4 >> 26);  // all ones when h + 5 >= 2^130, i.e. h >= p
    g4 &= M26;
    h.v0 = (g0 & ge) | (h.v0 & ~ge);
    h.v1 = (g1 & ge) | (h.v1 & ~ge);
    h.v2 = (g2 & ge) | (h.v2 & ~ge);
    h.v3 = (g3 & ge) | (h.v3 & ~ge);
    h.v4 = (g4 & ge) | (h.v4 & ~ge);
    return h;
}

// tag = (h mod 2^128) + s mod 2^128, little-endian words (poly1305.rs:231-312)
__device__ __forceinline__ void tag_words(F26 h, const uint32_t s[4], uint32_t t[4]) {
    h = canonical(h);
    const uint32_t w0 = h.v0 | (h.v1 << 26);
    const uint32_t w1 = (h.v1 >> 6) | (h.v2 << 20);
    const uint32_t w2 = (h.v2 >> 12) | (h.v3 << 14);
    const uint32_t w3 = (h.v3 >> 18) | (h.v4 << 8);
    uint64_t acc = (uint64_t)w0 + s[0];
    t[0] = (uint32_t)acc;
    acc = (acc >> 32) + w1 + s[1];
    t[1] = (uint32_t)acc;
    acc = (acc >> 32) + w2 + s[2];
    t[2] = (uint32_t)acc;
    acc = (acc >> 32) + w3 + s[3];
    t[3] = (uint32_t)acc;
}

// 128-bit little-endian value (4 words) + extra high bits -> radix 2^26
__device__ __forceinline__ F26 words_to_f26(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t hi) {
    F26 c;
    c.v0 = w0 & M26;
    c.v1 = __builtin_amdgcn_alignbit(w1, w0, 26) & M26;
    c.v2 = __builtin_amdgcn_alignbit(w2, w1, 20) & M26;
    c.v3 = __builtin_amdgcn_alignbit(w3, w2, 14) & M26;
    c.v4 = (w3 >> 8) | (hi << 24);
    return c;
}

// x^e by square-and-multiply (mul_add outputs are valid multipliers as they stand)
__device__ __forceinline__ F26 fpow(const F26 x, const uint32_t e) {
    F26 acc = f26_one();
    if (e == 0u) return acc;
    for (int bit = 31 - __builtin_clz(e); bit >= 0; --bit) {
        acc = fmul(acc, acc);
        if ((e >> bit) & 1u) acc = fmul(acc, x);
    }
    return acc;
}

// f += f of the lane that DPP control word CTRL names (0 where there is none),
// limb by limb: one level of a wave's sum.  row_shr:n = 0x110 + n; after the
// row broadcasts only lane 31 / 63 holds the sum of the rows before it.
constexpr int kDppShr1 = 0x111, kDppShr2 = 0x112, kDppShr4 = 0x114, kDppShr8 = 0x118;
constexpr int kDppBcast15 = 0x142, kDppBcast31 = 0x143;
template <int CTRL>
__device__ __forceinline__ void dpp_add(F26& f) {
    auto dpp = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true); };
    f.v0 += dpp(f.v0); f.v1 += dpp(f.v1); f.v2 += dpp(f.v2); f.v3 += dpp(f.v3); f.v4 += dpp(f.v4);
}

// sum_{e=1..m} x^e by binary doubling (G(2a) = G(a) + x^a G(a), G(a+1) = G(a) + x^(a+1))
__device__ __forceinline__ F26 geo_sum(const F26 x, const uint32_t m) {
    F26 g = f26_zero(), pw = f26_one();
    if (m == 0u) return g;
    for (int bit = 31 - __builtin_clz(m); bit >= 0; --bit) {
        g = mul_add(g, pw.v0, pw.v1, pw.v2, pw.v3, pw.v4, g);
        pw = fmul(pw, pw);
        if ((m >> bit) & 1u) {
            pw = fmul(pw, x);
            g = f26_add(g, pw);
        }
    }
    return g;
}

// ---- Poly1305 Horner step with the clamped r, radix 2^32 ------------------
// h = h0 + h1 2^32 + h2 2^64 + h3 2^96 + h4 2^128 (h4 small).  r0..r3 are the
// clamped key words: r0 < 2^28, r1..r3 < 2^28 and divisible by 4, so
// r_j 2^128 == (r_j / 4) * 5 (mod p) and s_j = r_j + (r_j >> 2) stays exact.
struct H32 {
    uint32_t h0, h1, h2, h3, h4;
};

// h = (h + m + pad * 2^128) * r  (partially reduced: h4 <= 4)
__device__ __forceinline__ void horner_step(H32& h, uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3,
                                            uint32_t pad, uint32_t r0, uint32_t r1, uint32_t r2,
                                            uint32_t r3, uint32_t s1, uint32_t s2, uint32_t s3) {
    // h += m (poly1305.rs:227 c.add(&h))
    uint32_t c;
    const uint32_t a0 = addc(h.h0, m0, 0u, &c);
    const uint32_t a1 = addc(h.h1, m1, c, &c);
    const uint32_t a2 = addc(h.h2, m2, c, &c);
    const uint32_t a3 = addc(h.h3, m3, c, &c);
    const uint32_t a4 = h.h4 + pad + c;
    // * r (poly1305.rs:227 .mult(&r)): column sums < 2^63, then one carry ripple
    const uint64_t d0 = (uint64_t)a0 * r0 + (uint64_t)a1 * s3 + (uint64_t)a2 * s2 + (uint64_t)a3 * s1;
    const uint64_t d1 = (uint64_t)a0 * r1 + (uint64_t)a1 * r0 + (uint64_t)a2 * s3 + (uint64_t)a3 * s2 +
                        (uint64_t)a4 * s1;
    const uint64_t d2 = (uint64_t)a0 * r2 + (uint64_t)a1 * r1 + (uint64_t)a2 * r0 + (uint64_t)a3 * s3 +
                        (uint64_t)a4 * s2;
    const uint64_t d3 = (uint64_t)a0 * r3 + (uint64_t)a1 * r2 + (uint64_t)a2 * r1 + (uint64_t)a3 * r0 +
                        (uint64_t)a4 * s3;
    const uint32_t e1 = addc((uint32_t)d1, (uint32_t)(d0 >> 32), 0u, &c);
    const uint32_t e2 = addc((uint32_t)d2, (uint32_t)(d1 >> 32), c, &c);
    const uint32_t e3 = addc((uint32_t)d3, (uint32_t)(d2 >> 32), c, &c);
    uint32_t e4 = a4 * r0 + (uint32_t)(d3 >> 32) + c;
    // fold bits >= 2^130: (e4 >> 2) * 2^130 == (e4 >> 2) * 5
    const uint32_t f = (e4 >> 2) * 5u;
    e4 &= 3u;
    h.h0 = addc((uint32_t)d0, f, 0u, &c);
    h.h1 = addc(e1, 0u, c, &c);
    h.h2 = addc(e2, 0u, c, &c);
    h.h3 = addc(e3, 0u, c, &c);
    h.h4 = e4 + c;
}

// radix 2^32 -> 2^26 (h < 2^131: the bits from 2^130 up fold in as 5)
__device__ __forceinline__ F26 h32_to_f26(const H32& h) {
    F26 f = words_to_f26(h.h0, h.h1, h.h2, h.h3, 0u);
    f.v4 += h.h4 << 24;
    const uint32_t c = f.v4 >> 26;
    f.v4 &= M26;
    f.v0 += c * 5u;
    return f;
}

// Poly1305 key of a record: keystream block 0 (chacha20_poly1305.rs:50,75),
// r = clamp(pk[0..16]) (poly1305.rs:197-203) as radix-2^32 words, s = pk[16..32]
// (chacha20_poly1305.rs:32-39)
struct PolyKey {
    uint32_t r0, r1, r2, r3;
    uint32_t s[4];
};
__device__ __forceinline__ PolyKey poly_key(const uint32_t ks[16]) {
    return PolyKey{ks[0] & 0x0fffffffu, ks[1] & 0x0ffffffcu, ks[2] & 0x0ffffffcu, ks[3] & 0x0ffffffcu,
                   {ks[4], ks[5], ks[6], ks[7]}};
}

// Constant-time tag compare: diff |= a ^ b over all 16 bytes
// (chacha20_poly1305.rs:84-87), the received and the computed tag as four
// words each; the record's status byte, 1 = wrong mac.
template <class A, class B>
__device__ __forceinline__ uint8_t tag_mismatch(const A& rx, const B& tw) {
    const uint32_t diff = (rx[0] ^ tw[0]) | (rx[1] ^ tw[1]) | (rx[2] ^ tw[2]) | (rx[3] ^ tw[3]);
    return diff != 0u ? 1u : 0u;
}

// ---- per-record parameters ---------------------------------------------------
// Key and nonce of a record: the key words and state words 13-15 (n13 = 0 in
// the draft, whose 8-byte nonce fills words 14-15; RFC 8439 section 2.3 puts a
// 12-byte nonce in words 13-15), and the TLS sequence number (0 in explicit mode).
struct RecKey {
    uint32_t k[8];
    uint32_t n13, n14, n15;
    uint64_t seq;
};

// Row of the key table (and of the RFC 7905 write-IV table, which has num_keys
// rows too) for a key index: out-of-range indices stay inside the table.
__device__ __forceinline__ uint32_t key_slot_of(const KParams& p, uint32_t ki) {
    return ki < p.num_keys ? ki : p.num_keys - 1u;
}
__device__ __forceinline__ uint32_t key_slot(const KParams& p, uint32_t rec) {
    return key_slot_of(p, p.key_index ? p.key_index[rec] : 0u);
}

template <Construction C>
__device__ __forceinline__ RecKey record_key(const KParams& p, uint32_t rec) {
    constexpr bool RFC = C == Construction::kRfc8439;
    RecKey rk;
    const uint32_t ki = key_slot(p, rec);
    const uint32_t* kw = reinterpret_cast<const uint32_t*>(p.keys + 32u * ki);
#pragma unroll
    for (int i = 0; i < 8; ++i) rk.k[i] = kw[i];  // keys are little-endian words (chacha20.rs:37-39)
    if (p.tls) {
        // draft: nonce = u64_be_array(seq) (tls.rs:103, util.rs:43-45) loaded as
        // two little-endian words (chacha20.rs:45-46); RFC 7905 section 2: the
        // key's 12-byte write IV XOR (00 00 00 00 || be64(seq))
        rk.seq = p.seq ? p.seq[rec] : p.seq0 + rec;
        if constexpr (RFC) {
            const uint32_t* iv = reinterpret_cast<const uint32_t*>(p.ivs + 12u * ki);
            rk.n13 = iv[0];
            rk.n14 = iv[1] ^ bswap32((uint32_t)(rk.seq >> 32));
            rk.n15 = iv[2] ^ bswap32((uint32_t)rk.seq);
        } else {
            rk.n13 = 0u;
            rk.n14 = bswap32((uint32_t)(rk.seq >> 32));
            rk.n15 = bswap32((uint32_t)rk.seq);
        }
    } else {  // explicit mode: nonce_len<C>() bytes per record, little-endian words
        const uint8_t* nb = p.nonces + (uint64_t)nonce_len<C>() * rec;
        rk.seq = 0;
        rk.n13 = RFC ? le32(nb) : 0u;
        rk.n14 = le32(nb + (RFC ? 4 : 0));
        rk.n15 = le32(nb + (RFC ? 8 : 4));
    }
    return rk;
}

__device__ __forceinline__ uint32_t record_len(const KParams& p, uint32_t rec) {
    return p.len ? p.len[rec] : p.uniform_len;
}
// The AEAD's input length of a record of len bytes: an open's ciphertext without its tag (0
// for a record too short to hold one), a TLS 1.3 seal's inner plaintext, otherwise the record.
template <bool OPEN, bool T13>
__device__ __forceinline__ uint32_t aead_len(const KParams& p, uint32_t len) {
    return OPEN ? (len >= 16u ? len - 16u : 0u) : T13 ? tls13_inner_len(len, p.pad_to) : len;
}
// The AD's length: the TLS 1.3 record header, the TLS 1.2 record-layer AD, or the call's.
template <bool T13>
__device__ __forceinline__ uint32_t ad_len(const KParams& p) {
    return T13 ? 5u : p.tls ? 13u : p.ad_len;
}
// byte offset of record rec in the batch's input / output
__device__ __forceinline__ uint64_t rec_in_off(const KParams& p, uint32_t rec) {
    return p.in_off ? p.in_off[rec] : p.in_stride * rec;
}
__device__ __forceinline__ uint64_t rec_out_off(const KParams& p, uint32_t rec) {
    return p.out_off ? p.out_off[rec] : p.out_stride * rec;
}

// AD byte i of the TLS record-layer additional data (tls.rs:103-112, 250-265):
// be64(seq) || type || major || minor || be16(n)
__device__ __forceinline__ uint8_t tls_ad_byte(uint64_t seq, uint32_t hdr, uint32_t n, uint32_t i) {
    if (i < 8) return (uint8_t)(seq >> (56 - 8 * i));
    if (i < 11) return (uint8_t)(hdr >> (8 * (i - 8)));
    if (i == 11) return (uint8_t)(n >> 8);
    return (uint8_t)n;
}

// AD byte i (< 5) of a TLS 1.3 record (RFC 8446 section 5.2): the record header
// opaque_type 23 || legacy_record_version 03 03 || be16(L), L the fragment length
__device__ __forceinline__ uint8_t tls13_ad_byte(uint32_t L, uint32_t i) {
    if (i == 0) return 0x17u;
    if (i < 3) return 0x03u;
    if (i == 3) return (uint8_t)(L >> 8);
    return (uint8_t)L;
}

// The inner type byte that a TLS 1.3 seal puts behind record rec's content: the record's
// own (sg_tls13_seal_opts.inner_types) or the call's content_type
__device__ __forceinline__ uint8_t tls13_inner_type(const KParams& p, uint32_t rec) {
    return p.inner_types ? p.inner_types[rec] : (uint8_t)p.tls_hdr;
}

// AD byte i (< ad_len<T13>(p)) of a record of n AEAD input bytes: the TLS 1.3 record header
// (fragment length n + 16), the TLS 1.2 record-layer AD, or the call's own AD bytes
template <bool T13>
__device__ __forceinline__ uint8_t ad_byte(const KParams& p, uint32_t rec, uint64_t seq, uint32_t n, uint32_t i) {
    if constexpr (T13) return tls13_ad_byte(n + 16u, i);
    else return p.tls ? tls_ad_byte(seq, p.tls_hdr, n, i) : p.ads[(uint64_t)p.ad_stride * rec + i];
}

// Byte i (< ct_offset<C>(adlen)) of the MAC stream in front of the ciphertext:
// ad || le64(|ad|) in the draft (chacha20_poly1305.rs:24-26), ad and its zero
// padding in RFC 8439.
template <Construction C, bool T13 = false>
__device__ __forceinline__ uint8_t prefix_byte(const KParams& p, uint32_t rec, uint64_t seq, uint32_t n, uint32_t adlen,
                                               uint32_t i) {
    if (i < adlen) return ad_byte<T13>(p, rec, seq, n, i);
    if constexpr (C == Construction::kRfc8439) return 0u;
    else return (uint8_t)((uint64_t)adlen >> (8u * (i - adlen)));
}

}  // namespace dev
}  // namespace sg
