// sg_msg.hip -- gfx950 kernels of the long-message path: one message (one key,
// one 8-byte nonce, n data bytes, adlen AD bytes, any lengths up to
// SG_MSG_MAX_LEN) sealed or opened by a persistent grid over the whole chip.
// Same construction as every other path of the library
// (chacha20_poly1305.rs:19-94): Poly1305 key = keystream block 0, data byte i
// XORed with keystream block 1 + i / 64, counter in state word 12 only, MAC
// over ad || le64(adlen) || ct || le64(n) without padding.
//
// ChaCha20 is position-addressable.  Poly1305 is one Horner chain
// (poly1305.rs:213-228); it is cut into independent pieces and put back
// together exactly:
//
//   * The B = ceil((adlen + 16 + n) / 16) blocks of the MAC stream are
//     preceded by z virtual blocks (value 0, no 2^128 pad bit; leading zeros do
//     not change a Horner polynomial) so that z + B = T K: T tiles of K = 1020
//     blocks (sg_msg_plan.cpp; the geometry arrives as a kernel argument).
//   * Within a tile, lane l of 255 runs the reference's step h = (h + c) r from
//     h = 0 over its 4 contiguous blocks: f = sum_j c_(4l+j) r^(4-j).  The
//     tile's hash from zero is h_t = sum_l f_(t,l) r^(4 (254 - l)).
//   * A group owns a contiguous run of tiles; its partial is
//     H_g = sum_t h_t R^(t_end - 1 - t), R = r^K.  The two sums commute, so
//     every lane keeps its own accumulator a_l = a_l R + f_(t,l) over the
//     group's tiles and the lanes meet only once, at the end of the group:
//     H_g = sum_l a_l r^(4 (254 - l)).  No per-tile reduction.
//   * sg_msg_finish_kernel adds H_g R^(tiles after group g), reduces mod
//     2^130 - 5, adds s (poly1305.rs:230-312) and writes the tag, or compares
//     it in constant time (chacha20_poly1305.rs:84-93).
//
// Everything is exact mod p = 2^130 - 5, so the tag is the sequential one bit
// for bit.
//
// Tiles are cut on the MAC-stream grid, so a tile's data bytes are an exact
// byte range [d0, d1) of the message, not aligned to ChaCha20's 64-byte blocks
// unless (adlen + 8) % 16 == 0: lane b computes keystream block d0 / 64 + b
// (at most 256 of them touch a tile) and the one or two blocks a tile shares
// with its neighbours are computed by both.  A tile uses and writes only its
// own byte range, each byte read by the lane that writes it (a 16-byte load at
// a tile's edge also fetches a neighbour's bytes, which are dropped), so no
// group ever depends on what another writes and out == in is safe.
//
// LDS per workgroup: the tile's stream bytes, placed so that the data bytes
// keep their alignment inside a ChaCha20 block (aligned 16-byte stores by the
// block lanes, unaligned 16-byte loads by the MAC lanes), 16,464 bytes: nine
// workgroups fit a CU's 160 KiB, the VGPR budget decides the occupancy.
#include "sg_internal.h"
#include "sg_msg_plan.h"

#include "sg_device.h"

namespace sg {
namespace {

using namespace dev;

// tile bytes at [kLdsFront + A, + kMsgTileBytes), A < 64; the 16-byte chunks the
// tile's edges cut are stored whole: up to 15 bytes before and behind the tile
constexpr uint32_t kLdsFront = 64;
constexpr uint32_t kLdsBytes = kLdsFront + 64u + kMsgTileBytes + 16u;

struct MsgKey {
    uint32_t k[8];
    uint32_t r0, r1, r2, r3;  // clamped r (poly1305.rs:197-203)
    uint32_t s[4];
};

// key bytes at any alignment -> little-endian words (chacha20.rs:37-39), block
// 0 -> Poly1305 key (chacha20_poly1305.rs:50); everything wave-uniform
__device__ __forceinline__ MsgKey msg_key(const uint8_t* key, uint32_t n14, uint32_t n15) {
    MsgKey mk;
#pragma unroll
    for (int i = 0; i < 8; ++i) mk.k[i] = uniform(le32(key + 4 * i));
    uint32_t ks[16];
    chacha_block(ks, mk.k, 0u, n14, n15);
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

}  // namespace

struct MsgParams {
    const uint8_t* key;
    const uint8_t* ad;
    const uint8_t* in;
    uint8_t* out;
    uint8_t* status;
    uint32_t* ws;  // plan.groups partials of kMsgPartialWords words
    uint64_t n, adlen;
    uint32_t n14, n15;
    sg_msg_plan plan;
};

namespace {

template <bool OPEN>
__global__ __launch_bounds__(256) void sg_msg_kernel(const MsgParams p) {
    __shared__ __attribute__((aligned(64))) uint8_t lds[kLdsBytes];
    static_assert(kLdsBytes >= 5u * 4u * (256u + 16u), "reduction space");
    const uint32_t lane = threadIdx.x;
    const MsgKey mk = msg_key(p.key, p.n14, p.n15);
    const uint32_t r0 = mk.r0, r1 = mk.r1, r2 = mk.r2, r3 = mk.r3;
    const uint32_t s1 = r1 + (r1 >> 2), s2 = r2 + (r2 >> 2), s3 = r3 + (r3 >> 2);
    const F26 r = words_to_f26(r0, r1, r2, r3, 0u);
    const F26 R = fpow(r, p.plan.tile_blocks);
    const F26 Pl = fpow(r, lane < kMsgMacLanes ? kMsgLaneBlocks * (kMsgMacLanes - 1u - lane) : 0u);
    const ChaChaPre pre = chacha_pre(mk.k, p.n14, p.n15);

    const int64_t n = (int64_t)p.n;
    const int64_t adlen = (int64_t)p.adlen;
    const int64_t P = adlen + 8;      // stream offset of the ciphertext
    const int64_t L = P + n + 8;      // stream length
    const int64_t TB = (int64_t)p.plan.tile_bytes;
    const uint64_t z = p.plan.zero_blocks;
    const uint64_t last = z + p.plan.mac_blocks - 1u;                       // the stream's final block
    const uint32_t rem = (uint32_t)(L - 16 * ((int64_t)p.plan.mac_blocks - 1));  // its bytes, 1..16

    const uint64_t t0 = (uint64_t)blockIdx.x * p.plan.tiles_per_group;
    uint64_t t1 = t0 + p.plan.tiles_per_group;
    if (t1 > p.plan.tiles) t1 = p.plan.tiles;

    F26 acc = f26_zero();
    for (uint64_t t = t0; t < t1; ++t) {
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
                chacha_block_pre(ks, pre, mk.k, (uint32_t)cb + 1u, p.n14, p.n15);  // data uses blocks 1.. (:52)
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
        if (s0 < P || s1e > P + n) {  // uniform
            int64_t a = s0 > 0 ? s0 : 0, b = s1e < P ? s1e : P;
            for (int64_t s = a + lane; s < b; s += kMsgThreads)
                tl[s - s0] = s < adlen ? p.ad[s] : (uint8_t)((uint64_t)adlen >> (8 * (s - adlen)));
            a = s0 > P + n ? s0 : P + n;
            for (int64_t s = a + lane; s < s1e; s += kMsgThreads) {
                const int64_t i = s - (P + n);
                tl[s - s0] = i < 8 ? (uint8_t)((uint64_t)n >> (8 * i)) : (uint8_t)0;
            }
        }
        __syncthreads();

        // ---- Poly1305: lane l steps blocks 4 l .. 4 l + 3 of the tile from h = 0
        if (lane < kMsgMacLanes) {
            const uint64_t vb0 = t * p.plan.tile_blocks + kMsgLaneBlocks * lane;
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
                } else if (vb == last && rem < 16u) {
                    // a short final block carries its pad bit at its own length
                    // (poly1305.rs:216-225; the bytes behind the stream are zero)
                    const uint32_t fb = 1u << (8u * (rem & 3u));
                    const uint32_t fw = rem >> 2;
                    m.x |= fw == 0u ? fb : 0u;
                    m.y |= fw == 1u ? fb : 0u;
                    m.z |= fw == 2u ? fb : 0u;
                    m.w |= fw == 3u ? fb : 0u;
                    pad = 0u;
                }
                horner_step(h, m.x, m.y, m.z, m.w, pad, r0, r1, r2, r3, s1, s2, s3);
            }
            acc = fmul_add(acc, R, h32_to_f26(h));  // the lane's Horner chain over the group's tiles
        }
        __syncthreads();  // the next tile's stores follow this tile's loads
    }
    // ---- the group's partial: sum of the lanes' chains, each at its place in a tile
    const F26 Hg = block_sum(fmul(acc, Pl), reinterpret_cast<uint32_t*>(lds), lane);
    if (lane == 0u) store_f26(p.ws + (uint64_t)blockIdx.x * kMsgPartialWords, Hg);
}

template <bool OPEN>
__global__ __launch_bounds__(256) void sg_msg_finish_kernel(const MsgParams p) {
    __shared__ uint32_t red[5u * (256u + 16u)];
    const uint32_t lane = threadIdx.x;
    const MsgKey mk = msg_key(p.key, p.n14, p.n15);
    const F26 R = fpow(words_to_f26(mk.r0, mk.r1, mk.r2, mk.r3, 0u), p.plan.tile_blocks);
    F26 sum = f26_zero();
    for (uint32_t g = lane; g < p.plan.groups; g += 256u) {  // <= 4 terms per lane
        const uint64_t done = (uint64_t)(g + 1u) * p.plan.tiles_per_group;
        const uint32_t after = done >= p.plan.tiles ? 0u : (uint32_t)(p.plan.tiles - done);  // < 2^20
        sum = f26_add(sum, fmul(load_f26(p.ws + (uint64_t)g * kMsgPartialWords), fpow(R, after)));
    }
    const F26 total = block_sum(carry1(sum), red, lane);
    if (lane != 0u) return;
    uint32_t tw[4];
    tag_words(total, mk.s, tw);
    if constexpr (!OPEN) {
        uint8_t* tp = p.out + p.n;  // ct || tag (chacha20_poly1305.rs:55)
#pragma unroll
        for (int i = 0; i < 16; ++i) tp[i] = (uint8_t)(tw[i >> 2] >> (8 * (i & 3)));
    } else {
        // constant-time compare: diff |= a ^ b over all 16 bytes (:84-87)
        const uint8_t* ep = p.in + p.n;
        uint32_t diff = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) diff |= (uint32_t)ep[i] ^ ((tw[i >> 2] >> (8 * (i & 3))) & 0xffu);
        *p.status = diff != 0u ? 1u : 0u;
    }
}

// A failed open hands out no plaintext (chacha20_poly1305.rs:89-93): zero
// out[0, n) when the status on the device says so.
__global__ __launch_bounds__(256) void sg_msg_scrub_kernel(uint8_t* out, const uint64_t n, const uint8_t* status) {
    if (*status == 0u) return;
    uint64_t head = (16u - ((uintptr_t)out & 15u)) & 15u;
    if (head > n) head = n;
    const uint64_t nvec = (n - head) >> 4;
    const uint64_t tail0 = head + (nvec << 4);
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t v = i; v < nvec; v += stride) st16(out + head + (v << 4), u32x4{0u, 0u, 0u, 0u});
    if (i < head) out[i] = 0;
    if (i < n - tail0) out[tail0 + i] = 0;
}

}  // namespace

hipError_t launch_msg(const uint8_t* key, const uint8_t nonce[8], const uint8_t* ad, uint64_t adlen, const uint8_t* in,
                      uint8_t* out, uint64_t n, uint8_t* status, uint32_t* ws, const sg_msg_plan& plan, bool open,
                      bool scrub, hipStream_t s) {
    if (plan.tile_blocks != kMsgTileBlocks || plan.groups == 0u || plan.groups > kMsgMaxGroups)
        return hipErrorInvalidValue;
    MsgParams p;
    p.key = key;
    p.ad = ad;
    p.in = in;
    p.out = out;
    p.status = status;
    p.ws = ws;
    p.n = n;
    p.adlen = adlen;
    // the nonce as two little-endian words (chacha20.rs:45-46)
    p.n14 = dev::le32(nonce);
    p.n15 = dev::le32(nonce + 4);
    p.plan = plan;
    if (open) {
        hipLaunchKernelGGL((sg_msg_kernel<true>), dim3(plan.groups), dim3(kMsgThreads), 0, s, p);
        hipLaunchKernelGGL((sg_msg_finish_kernel<true>), dim3(1), dim3(256), 0, s, p);
        if (scrub && n) {
            const uint64_t blocks = (n / 16u + 1023u) / 1024u;
            const uint32_t grid = blocks < 1u ? 1u : (blocks > 4096u ? 4096u : (uint32_t)blocks);
            hipLaunchKernelGGL(sg_msg_scrub_kernel, dim3(grid), dim3(256), 0, s, out, n, (const uint8_t*)status);
        }
    } else {
        hipLaunchKernelGGL((sg_msg_kernel<false>), dim3(plan.groups), dim3(kMsgThreads), 0, s, p);
        hipLaunchKernelGGL((sg_msg_finish_kernel<false>), dim3(1), dim3(256), 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace sg
