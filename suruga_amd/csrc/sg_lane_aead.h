// sg_lane_aead.h -- the steps of an RFC 8439 AEAD over the G lanes of a packet's group, as
// sg_quic.h lays a packet out (Geom): device code shared by the datagram kernels that keep
// this geometry.  sg_dtls13.hip is written on it; sg_quic.hip, sg_wg.hip and sg_esp.hip
// each still carry their own statement of the same steps and can move here one at a time
// (DESIGN.md section 10).  What differs between the protocols stays with the kernel: where
// the key, the nonce and the additional data come from, which bytes of the plaintext are
// input and which are made by rule, and what is parsed behind the tag.
//
//   Keying        key and nonce words of a packet; block(ks, ctr) is a keystream block
//   slot          one slot v of a lane's loop: a whole chunk, or in slot 0 the tail and the
//                 length block.  The plaintext comes through a Src: src.byte(i) is byte i of
//                 the AEAD's input, src.loadable(c) says that chunk c lies in memory as it
//                 is and src.ptr(c) where, so that it takes the four 16-byte loads; any
//                 other chunk, and the tail, is put together byte by byte
//   ad_block      one 16-byte block of additional data into a lane's sum
//   fold          the lanes' sums into the last lane (Hillis-Steele, log2 G multiply-adds)
//   finish        the tail's sum behind it and the tag's four words
//   tag_bad       open: the last lane's compare with the received tag, given to the group
//   group_sync    the group's stores visible to the group's loads
#pragma once

#include "sg_device.h"
#include "sg_quic.h"

namespace sg {
namespace lane {

using namespace dev;

typedef uint32_t u32_u __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t ldu32(const uint8_t* p) { return *reinterpret_cast<const u32_u*>(p); }
__device__ __forceinline__ void stu16(uint8_t* p, u32x4 v) { *reinterpret_cast<u32x4_u*>(p) = v; }

// h = (h + m + 2^128) r: one full 16-byte block of the RFC 8439 MAC stream
__device__ __forceinline__ F26 mac_block(const F26& h, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, const F26& r) {
    return fmul(f26_add(h, words_to_f26(w0, w1, w2, w3, 1u)), r);
}

// the group's stores visible to the group's loads (one wave: no barrier to wait at)
__device__ __forceinline__ void group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// word w of the 16-byte block j of a keystream block, j not known when compiling: the
// rolled loops over a packet's last bytes pick it with selects, so ks stays in registers
__device__ __forceinline__ uint32_t ks_word(const uint32_t (&ks)[16], uint32_t j, uint32_t w) {
    return j == 0u ? ks[w] : j == 1u ? ks[4u + w] : j == 2u ? ks[8u + w] : ks[12u + w];
}

struct Keying {
    uint32_t k[8], n13, n14, n15;
    __device__ __forceinline__ void load_key(const uint8_t* key) {
#pragma unroll
        for (int i = 0; i < 8; ++i) k[i] = ldu32(key + 4 * i);
    }
    __device__ __forceinline__ void block(uint32_t (&ks)[16], uint32_t ctr) const { chacha_block(ks, k, ctr, n13, n14, n15); }
};

// a plaintext (seal) or ciphertext (open) that lies in memory whole: every chunk is loadable
struct Wire {
    const uint8_t* p;
    __device__ __forceinline__ uint32_t byte(uint32_t i) const { return p[i]; }
    __device__ __forceinline__ bool loadable(uint32_t) const { return true; }
    __device__ __forceinline__ const uint8_t* ptr(uint32_t c) const { return p + 64ull * c; }
};

// bytes at .. at + 4 of a source as a little-endian word
template <class Src>
__device__ __forceinline__ uint32_t src_word(const Src& src, uint32_t at) {
    uint32_t x = 0u;
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) x |= src.byte(at + b) << (8u * b);
    return x;
}

// Slot v of a lane: chunk v - zc where v >= zc, the tail and the length block where v == 0,
// nothing otherwise.  dst is where byte 0 of the AEAD's output goes; the MAC runs over the
// ciphertext, which is the input on open and the output on seal.  h is the lane's sum, ts
// slot 0's.
template <bool OPEN, class Src>
__device__ __forceinline__ void slot(const quic::Geom& g, uint32_t v, const Keying& key, const Src& src, uint8_t* dst,
                                     uint32_t ad_len, uint32_t n, const F26& r, uint32_t (&ks)[16], F26& h, F26& ts) {
    const bool full = v >= g.zc;
    if (!full && v != 0u) return;
    const uint32_t c = full ? v - g.zc : g.nf;  // the chunk; slot 0 takes the tail
    key.block(ks, c + 1u);
    uint8_t* const d = dst + 64ull * c;
    if (full) {
        if (src.loadable(c)) {
            const uint8_t* const s = src.ptr(c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u32x4 a = ldu16(s + 16 * j);
                const u32x4 x = {a[0] ^ ks[4 * j], a[1] ^ ks[4 * j + 1], a[2] ^ ks[4 * j + 2], a[3] ^ ks[4 * j + 3]};
                stu16(d + 16 * j, x);
                const u32x4 m = OPEN ? a : x;
                h = mac_block(h, m[0], m[1], m[2], m[3], r);
            }
        } else {
#pragma unroll 1
            for (uint32_t j = 0; j < 4u; ++j) {  // rolled: few chunks of a packet come here
                const uint32_t at = 64u * c + 16u * j;
                const u32x4 a = {src_word(src, at), src_word(src, at + 4u), src_word(src, at + 8u), src_word(src, at + 12u)};
                const u32x4 x = {a[0] ^ ks_word(ks, j, 0), a[1] ^ ks_word(ks, j, 1), a[2] ^ ks_word(ks, j, 2), a[3] ^ ks_word(ks, j, 3)};
                stu16(d + 16u * j, x);
                const u32x4 m = OPEN ? a : x;
                h = mac_block(h, m[0], m[1], m[2], m[3], r);
            }
        }
    } else {
        // the tail's g.tail < 64 bytes, zero-padded to whole MAC blocks, then the length block
        const uint32_t base = 64u * g.nf;
#pragma unroll 1
        for (uint32_t j = 0; j < g.kt; ++j) {
            uint32_t m[4];
#pragma unroll
            for (uint32_t w = 0; w < 4u; ++w) {
                uint32_t a = 0u, keep = 0u;
#pragma unroll
                for (uint32_t b = 0; b < 4u; ++b) {
                    const uint32_t i = 16u * j + 4u * w + b;
                    if (i < g.tail) {
                        a |= src.byte(base + i) << (8u * b);
                        keep |= 0xffu << (8u * b);
                    }
                }
                const uint32_t x = (a ^ ks_word(ks, j, w)) & keep;
#pragma unroll
                for (uint32_t b = 0; b < 4u; ++b) {
                    const uint32_t i = 16u * j + 4u * w + b;
                    if (i < g.tail) d[i] = (uint8_t)(x >> (8u * b));
                }
                m[w] = OPEN ? a : x;
            }
            ts = mac_block(ts, m[0], m[1], m[2], m[3], r);
        }
        ts = mac_block(ts, ad_len, 0u, n, 0u, r);  // le64(|ad|) || le64(|ct|)
    }
}

// block a of the zero-padded additional data, ad.byte(i) for i < ad_len, into h
template <class Ad>
__device__ __forceinline__ F26 ad_block(const F26& h, const Ad& ad, uint32_t ad_len, uint32_t a, const F26& r) {
    uint32_t m[4];
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
        m[w] = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint32_t i = 16u * a + 4u * w + b;
            if (i < ad_len) m[w] |= ad.byte(i) << (8u * b);
        }
    }
    return mac_block(h, m[0], m[1], m[2], m[3], r);
}

// sum_t H_t P^(G - 1 - t) into the last lane, P = r^(4 Q)
template <uint32_t G>
__device__ __forceinline__ F26 fold(F26 h, const F26& r, uint32_t q, uint32_t t) {
    const F26 r2 = fmul(r, r);
    F26 pw = fpow(fmul(r2, r2), q);
#pragma unroll
    for (uint32_t s = 1; s < G; s <<= 1) {
        F26 up;
        up.v0 = __shfl_up(h.v0, s, G); up.v1 = __shfl_up(h.v1, s, G); up.v2 = __shfl_up(h.v2, s, G);
        up.v3 = __shfl_up(h.v3, s, G); up.v4 = __shfl_up(h.v4, s, G);
        if (t < s) up = f26_zero();
        h = fmul_add(up, pw, h);
        pw = fmul(pw, pw);
    }
    return h;
}

// ... behind it the tail's blocks and the length block: S r^(kt + 1) + TS, and the tag
template <uint32_t G>
__device__ __forceinline__ void finish(F26 h, F26 ts, const F26& r, uint32_t kt, const uint32_t (&s)[4], uint32_t (&tw)[4]) {
    ts.v0 = __shfl(ts.v0, 0, G); ts.v1 = __shfl(ts.v1, 0, G); ts.v2 = __shfl(ts.v2, 0, G);
    ts.v3 = __shfl(ts.v3, 0, G); ts.v4 = __shfl(ts.v4, 0, G);
    for (uint32_t j = 0; j <= kt; ++j) h = fmul(h, r);
    tag_words(f26_add(h, ts), s, tw);
}

// open: the last lane, which holds the tag, compares it with the 16 bytes at tp
template <uint32_t G>
__device__ __forceinline__ uint32_t tag_bad(const uint8_t* tp, const uint32_t (&tw)[4], uint32_t t) {
    uint32_t bad = 0u;
    if (t == G - 1u) {
        const uint32_t rx[4] = {ldu32(tp), ldu32(tp + 4), ldu32(tp + 8), ldu32(tp + 12)};
        bad = tag_mismatch(rx, tw);
    }
    return __shfl(bad, G - 1u, G);
}

}  // namespace lane
}  // namespace sg
