// sg_msg_device.h -- device code the two long-message kernel files share
// (sg_msg.hip: one message over the grid; sg_msg_batch.hip: many messages on
// one grid): keying from block 0, the tile body (keystream XOR, framing bytes,
// lane Horner), the workgroup sum, the tag finish and the scrub loop.  One
// copy of each; the decomposition is described in sg_msg.hip.
#pragma once

#include "sg_internal.h"
#include "sg_msg_plan.h"

#include "sg_device.h"

namespace sg {
namespace {

using namespace dev;

// The construction (Construction, sg_layout.h) is a compile-time parameter of
// the tile body and of the kernels built on it: the ciphertext starts at stream
// offset P = ct_offset<C>(adlen) and the stream is L = stream_bytes<C>(adlen, n)
// bytes long, counted in int64_t here.

// tile bytes at [kLdsFront + A, + kMsgTileBytes), A = (s0 - P) & 63 < 64; the
// 16-byte chunks the tile's edges cut are stored whole: up to 15 bytes before
// and behind the tile.  RFC 8439: P and s0 are multiples of 16, so A is 0, 16,
// 32 or 48 and no chunk is cut by a tile's edge: the same room bounds it.
constexpr uint32_t kLdsFront = 64;
constexpr uint32_t kLdsBytes = kLdsFront + 64u + kMsgTileBytes + 16u;
static_assert(kLdsBytes >= 5u * 4u * (256u + 16u), "reduction space");

struct MsgKey {
    uint32_t k[8];
    uint32_t r0, r1, r2, r3;  // clamped r (poly1305.rs:197-203)
    uint32_t s[4];
};

// key bytes at any alignment -> little-endian words (chacha20.rs:37-39), block
// 0 -> Poly1305 key (chacha20_poly1305.rs:50; RFC 8439 section 2.6, with the
// nonce's first word n13 in state word 13); everything wave-uniform
__device__ __forceinline__ MsgKey msg_key(const uint8_t* key, uint32_t n13, uint32_t n14, uint32_t n15) {
    MsgKey mk;
#pragma unroll
    for (int i = 0; i < 8; ++i) mk.k[i] = uniform(le32(key + 4 * i));
    uint32_t ks[16];
    chacha_block(ks, mk.k, 0u, n13, n14, n15);
    const PolyKey pk = poly_key(ks);
    mk.r0 = uniform(pk.r0);
    mk.r1 = uniform(pk.r1);
    mk.r2 = uniform(pk.r2);
    mk.r3 = uniform(pk.r3);
#pragma unroll
    for (int i = 0; i < 4; ++i) mk.s[i] = uniform(pk.s[i]);
    return mk;
}

// Sum of the 256 lanes' reduced elements, valid in lane 0 (limbs < 2^26 + 2^8).
// red: 5 * (256 + 16) words of LDS nobody else touches until the next barrier.
__device__ __forceinline__ F26 block_sum(const F26 x, uint32_t* red, const uint32_t lane) {
    store_f26(red + 5u * lane, x);  // odd stride: no bank conflicts
    __syncthreads();
    if (lane < 16u) {
        F26 a = f26_zero();
        for (uint32_t i = 0; i < 16u; ++i) a = f26_add(a, load_f26(red + 5u * (16u * lane + i)));  // < 2^31
        store_f26(red + 5u * (256u + lane), carry1(a));
    }
    __syncthreads();
    F26 a = f26_zero();
    if (lane == 0u) {
        for (uint32_t i = 0; i < 16u; ++i) a = f26_add(a, load_f26(red + 5u * (256u + i)));
        a = carry1(a);
    }
    return a;
}

// One message as the tile body sees it, all wave-uniform: the buffers, the
// lengths and where the MAC stream's blocks lie on the tile grid.
struct MsgStream {
    const uint8_t* ad;
    const uint8_t* in;
    uint8_t* out;
    uint32_t n13, n14, n15;
    int64_t n, adlen;
    int64_t P;       // stream offset of the ciphertext
    int64_t L;       // stream length
    int64_t TB;      // tile bytes
    uint32_t tile_blocks;
    uint64_t z;      // virtual blocks in front
    uint64_t last;   // the stream's final block (virtual index)
    uint32_t rem;    // its bytes, 1..16
};

template <Construction C>
__device__ __forceinline__ MsgStream msg_stream(const uint8_t* ad, const uint8_t* in, uint8_t* out, uint32_t n13,
                                                uint32_t n14, uint32_t n15, uint64_t n, uint64_t adlen,
                                                uint64_t mac_blocks, uint64_t zero_blocks, uint32_t tile_blocks,
                                                uint32_t tile_bytes) {
    MsgStream m;
    m.ad = ad;
    m.in = in;
    m.out = out;
    m.n13 = n13;
    m.n14 = n14;
    m.n15 = n15;
    m.n = (int64_t)n;
    m.adlen = (int64_t)adlen;
    m.P = ct_offset<C>(m.adlen);
    m.L = stream_bytes<C>(m.adlen, m.n);
    m.TB = (int64_t)tile_bytes;
    m.tile_blocks = tile_blocks;
    m.z = zero_blocks;
    m.last = m.z + mac_blocks - 1u;
    m.rem = (uint32_t)(m.L - 16 * ((int64_t)mac_blocks - 1));  // RFC 8439: always 16
    return m;
}

// r with the multiples the Horner step wants
struct MsgR {
    uint32_t r0, r1, r2, r3, s1, s2, s3;
};

__device__ __forceinline__ MsgR msg_r(const MsgKey& mk) {
    return MsgR{mk.r0, mk.r1, mk.r2, mk.r3, mk.r1 + (mk.r1 >> 2), mk.r2 + (mk.r2 >> 2), mk.r3 + (mk.r3 >> 2)};
}

// Tile t of message m: XOR its data bytes with the keystream, lay the tile's
// MAC stream out in LDS and step the lane's four blocks from h = 0 into the
// lane's chain acc = acc R + f.  Ends behind a barrier: the next tile's stores
// follow this tile's loads.
template <bool OPEN, Construction C>
__device__ __forceinline__ void msg_tile(uint8_t* lds, const uint32_t lane, const MsgStream& p, const MsgKey& mk,
                                         const ChaChaPre& pre, const MsgR& rr, const F26& R, const uint64_t t,
                                         F26& acc) {
    const int64_t n = p.n, adlen = p.adlen, P = p.P, TB = p.TB;
    const uint64_t z = p.z;
    // the tile covers stream bytes [s0, s0 + TB); s0 < 0 only in tile 0 (virtual blocks)
    const int64_t s0 = (int64_t)t * TB - 16 * (int64_t)z;
    const int64_t s1e = s0 + TB;
    const int64_t d0 = s0 - P > 0 ? s0 - P : 0;  // its data bytes [d0, d1)
    const int64_t d1 = s1e - P < n ? s1e - P : n;
    // stream byte s lives at tl[s - s0]; A keeps data byte d at d mod 64
    const uint32_t A = (uint32_t)((s0 - P) & 63);
    uint8_t* tl = lds + kLdsFront + A;

    // ---- keystream XOR: lane b owns ChaCha20 block d0 / 64 + b, clipped to [d0, d1)
    if (d1 > d0) {
        const int64_t cb = (d0 >> 6) + (int64_t)lane;
        const int64_t boff = cb << 6;
        if (boff < d1) {
            const uint8_t* ip = p.in + boff;
            uint8_t* op = p.out + boff;
            uint8_t* lp = tl + (P + boff - s0);  // 64-byte aligned, >= lds
            const bool al = ((((uintptr_t)ip) | ((uintptr_t)op)) & 15u) == 0u;
            // The block's 16-byte chunks are fetched ahead of the rounds, whose
            // ~1,400 instructions hide the latency.  A chunk cut by the tile's
            // edge is fetched whole when it lies inside the message: its other
            // bytes are the neighbour's (read, never used; they land in LDS
            // outside the tile's range) and only this tile's are written.
            // full: the block lies inside the tile (all but the one or two at
            // its edges) -- straight-line loads and stores
            const bool full = al && boff >= d0 && boff + 64 <= d1;
            u32x4 dv[4] = {};
            bool vec[4] = {full, full, full, full};
            if (full) {
#pragma unroll
                for (int c = 0; c < 4; ++c) dv[c] = gld16(ip + 16 * c);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int64_t co = boff + 16 * c;
                    vec[c] = al && co + 16 > d0 && co < d1 && co + 16 <= n;
                    if (vec[c]) dv[c] = gld16(ip + 16 * c);
                }
            }
            uint32_t ks[16];
            chacha_block_pre(ks, pre, mk.k, (uint32_t)cb + 1u, p.n13, p.n14, p.n15);  // data uses blocks 1.. (:52)
            if (full) {
                // every fetched chunk is consumed ahead of the first store: one
                // wait for the loads, none between the stores
                u32x4 xv[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    xv[c] = dv[c] ^ u32x4{ks[4 * c], ks[4 * c + 1], ks[4 * c + 2], ks[4 * c + 3]};
                    // (opaque: the compiler would sink each XOR to its store, behind the store before it)
                    asm volatile("" : "+v"(xv[c].x), "+v"(xv[c].y), "+v"(xv[c].z), "+v"(xv[c].w));
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) st16(lp + 16 * c, OPEN ? dv[c] : xv[c]);
#pragma unroll
                for (int c = 0; c < 4; ++c) gst16(op + 16 * c, xv[c]);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int64_t co = boff + 16 * c;
                    if (co + 16 <= d0 || co >= d1) continue;  // a neighbour's bytes
                    if (vec[c]) {
                        const u32x4 d = dv[c];
                        const u32x4 x = d ^ u32x4{ks[4 * c], ks[4 * c + 1], ks[4 * c + 2], ks[4 * c + 3]};
                        st16(lp + 16 * c, OPEN ? d : x);
                        if (co >= d0 && co + 16 <= d1) {
                            gst16(op + 16 * c, x);
                        } else {
                            const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                            for (int b = 0; b < 16; ++b)
                                if (co + b >= d0 && co + b < d1) op[16 * c + b] = (uint8_t)(xw[b >> 2] >> (8 * (b & 3)));
                        }
                    } else {
                        // unaligned buffers or the message's last bytes: byte
                        // granular, the loads issued together ahead of the stores
                        uint8_t xb[16];
#pragma unroll
                        for (int b = 0; b < 16; ++b) xb[b] = co + b >= d0 && co + b < d1 ? ip[16 * c + b] : (uint8_t)0;
#pragma unroll
                        for (int b = 0; b < 16; ++b) {
                            if (co + b >= d0 && co + b < d1) {
                                const uint8_t y = xb[b] ^ (uint8_t)(ks[4 * c + (b >> 2)] >> (8 * (b & 3)));
                                op[16 * c + b] = y;
                                lp[16 * c + b] = OPEN ? xb[b] : y;
                            }
                        }
                    }
                }
            }
        }
    }
    // ---- framing bytes of the tile: ad || le64(adlen) in front, le64(n) and
    // the zeros that fill the final block behind (chacha20_poly1305.rs:24-30)
    // (the block lanes above store nothing into these bytes, so no order is needed)
    // RFC 8439 (section 2.8): ad || zeros [adlen, P) in front; behind the data
    // the zeros [P + n, P + 16 ceil(n / 16)), then le64(adlen), then le64(n)
    if (s0 < P || s1e > P + n) {  // uniform
        int64_t a = s0 > 0 ? s0 : 0, b = s1e < P ? s1e : P;
        for (int64_t s = a + lane; s < b; s += kMsgThreads) {
            if constexpr (C == Construction::kRfc8439)
                tl[s - s0] = s < adlen ? p.ad[s] : (uint8_t)0;
            else
                tl[s - s0] = s < adlen ? p.ad[s] : (uint8_t)((uint64_t)adlen >> (8 * (s - adlen)));
        }
        a = s0 > P + n ? s0 : P + n;
        for (int64_t s = a + lane; s < s1e; s += kMsgThreads) {
            const int64_t i = s - (P + n);
            if constexpr (C == Construction::kRfc8439) {
                const int64_t q = i - ((16 - (n & 15)) & 15);  // place in the length block
                tl[s - s0] = q < 0 || q >= 16 ? (uint8_t)0
                             : q < 8 ? (uint8_t)((uint64_t)adlen >> (8 * q))
                                     : (uint8_t)((uint64_t)n >> (8 * (q - 8)));
            } else {
                tl[s - s0] = i < 8 ? (uint8_t)((uint64_t)n >> (8 * i)) : (uint8_t)0;
            }
        }
    }
    __syncthreads();

    // ---- Poly1305: lane l steps blocks 4 l .. 4 l + 3 of the tile from h = 0
    if (lane < kMsgMacLanes) {
        const uint64_t vb0 = t * p.tile_blocks + kMsgLaneBlocks * lane;
        const uint8_t* bp = tl + 16u * kMsgLaneBlocks * lane;
        H32 h = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < kMsgLaneBlocks; ++j) {
            u32x4 m = ldu16(bp + 16u * j);
            const uint64_t vb = vb0 + j;
            uint32_t pad = 1u;
            if (vb < z) {  // virtual: value 0, no pad bit
                m = u32x4{0u, 0u, 0u, 0u};
                pad = 0u;
            } else if (C == Construction::kDraft && vb == p.last && p.rem < 16u) {
                // a short final block carries its pad bit at its own length
                // (poly1305.rs:216-225; the bytes behind the stream are zero)
                const uint32_t fb = 1u << (8u * (p.rem & 3u));
                const uint32_t fw = p.rem >> 2;
                m.x |= fw == 0u ? fb : 0u;
                m.y |= fw == 1u ? fb : 0u;
                m.z |= fw == 2u ? fb : 0u;
                m.w |= fw == 3u ? fb : 0u;
                pad = 0u;
            }
            horner_step(h, m.x, m.y, m.z, m.w, pad, rr.r0, rr.r1, rr.r2, rr.r3, rr.s1, rr.s2, rr.s3);
        }
        acc = fmul_add(acc, R, h32_to_f26(h));  // the lane's Horner chain over the run's tiles
    }
    __syncthreads();  // the next tile's stores follow this tile's loads
}

// The power of r that puts lane l's chain at its place in a tile
__device__ __forceinline__ F26 msg_lane_power(const F26& r, const uint32_t lane) {
    return fpow(r, lane < kMsgMacLanes ? kMsgLaneBlocks * (kMsgMacLanes - 1u - lane) : 0u);
}

// The finish both ways from the accumulator before s (lane 0 only): seal
// writes ct || tag (chacha20_poly1305.rs:55); open compares in constant time,
// diff |= a ^ b over all 16 bytes (:84-87), and returns whether they differ.
template <bool OPEN>
__device__ __forceinline__ uint32_t msg_tag_finish(const F26& total, const uint32_t s[4], const uint8_t* in,
                                                   uint8_t* out, const uint64_t n) {
    uint32_t tw[4];
    tag_words(total, s, tw);
    uint32_t diff = 0u;
    if constexpr (!OPEN) {
        uint8_t* tp = out + n;
#pragma unroll
        for (int i = 0; i < 16; ++i) tp[i] = (uint8_t)(tw[i >> 2] >> (8 * (i & 3)));
    } else {
        const uint8_t* ep = in + n;
#pragma unroll
        for (int i = 0; i < 16; ++i) diff |= (uint32_t)ep[i] ^ ((tw[i >> 2] >> (8 * (i & 3))) & 0xffu);
    }
    return diff;
}

// out[0, n) = 0 by the threads i, i + stride, ...: 16-byte stores over the
// aligned middle, bytes at the two ends, and not one byte more
__device__ __forceinline__ void msg_zero(uint8_t* out, const uint64_t n, const uint64_t i, const uint64_t stride) {
    uint64_t head = (16u - ((uintptr_t)out & 15u)) & 15u;
    if (head > n) head = n;
    const uint64_t nvec = (n - head) >> 4;
    const uint64_t tail0 = head + (nvec << 4);
    for (uint64_t v = i; v < nvec; v += stride) st16(out + head + (v << 4), u32x4{0u, 0u, 0u, 0u});
    if (i < head) out[i] = 0;
    if (i < n - tail0) out[tail0 + i] = 0;
}

}  // namespace
}  // namespace sg
