// sg_msg.hip -- gfx950 kernels of the long-message path: one message (one key,
// one nonce, n data bytes, adlen AD bytes, any lengths up to SG_MSG_MAX_LEN)
// sealed or opened by a persistent grid over the whole chip.  Two
// constructions, chosen at compile time by the Construction parameter:
//   * the draft, as every other path of the library
//     (chacha20_poly1305.rs:19-94): 8-byte nonce, Poly1305 key = keystream
//     block 0, data byte i XORed with keystream block 1 + i / 64, counter in
//     state word 12 only, MAC over ad || le64(adlen) || ct || le64(n) without
//     padding;
//   * RFC 8439 (SG_MSG_RFC8439): 12-byte nonce whose first word is state word
//     13, the same counters, MAC over ad || zeros to 16 || ct || zeros to 16 ||
//     le64(adlen) || le64(n).
// The text below describes the draft's stream; DESIGN.md section 4.8 says what
// the RFC layout changes (where the bytes lie; every block is a full block).
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
#include "sg_msg_device.h"

namespace sg {

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
    uint32_t n13;  // RFC 8439 only (behind the plan: the draft's argument offsets stay)
};

namespace {

template <bool OPEN, Construction C>
__global__ __launch_bounds__(256) void sg_msg_kernel(const MsgParams p) {
    __shared__ __attribute__((aligned(64))) uint8_t lds[kLdsBytes];
    const uint32_t lane = threadIdx.x;
    const uint32_t n13 = C == Construction::kRfc8439 ? p.n13 : 0u;
    const MsgKey mk = msg_key(p.key, n13, p.n14, p.n15);
    const MsgR rr = msg_r(mk);
    const F26 r = words_to_f26(mk.r0, mk.r1, mk.r2, mk.r3, 0u);
    const F26 R = fpow(r, p.plan.tile_blocks);
    const F26 Pl = msg_lane_power(r, lane);
    const ChaChaPre pre = chacha_pre(mk.k, n13, p.n14, p.n15);
    const MsgStream m = msg_stream<C>(p.ad, p.in, p.out, n13, p.n14, p.n15, p.n, p.adlen, p.plan.mac_blocks,
                                      p.plan.zero_blocks, p.plan.tile_blocks, p.plan.tile_bytes);

    const uint64_t t0 = (uint64_t)blockIdx.x * p.plan.tiles_per_group;
    uint64_t t1 = t0 + p.plan.tiles_per_group;
    if (t1 > p.plan.tiles) t1 = p.plan.tiles;

    F26 acc = f26_zero();
    for (uint64_t t = t0; t < t1; ++t) msg_tile<OPEN, C>(lds, lane, m, mk, pre, rr, R, t, acc);
    // ---- the group's partial: sum of the lanes' chains, each at its place in a tile
    const F26 Hg = block_sum(fmul(acc, Pl), reinterpret_cast<uint32_t*>(lds), lane);
    if (lane == 0u) store_f26(p.ws + (uint64_t)blockIdx.x * kMsgPartialWords, Hg);
}

template <bool OPEN, Construction C>
__global__ __launch_bounds__(256) void sg_msg_finish_kernel(const MsgParams p) {
    __shared__ uint32_t red[5u * (256u + 16u)];
    const uint32_t lane = threadIdx.x;
    const MsgKey mk = msg_key(p.key, C == Construction::kRfc8439 ? p.n13 : 0u, p.n14, p.n15);
    const F26 R = fpow(words_to_f26(mk.r0, mk.r1, mk.r2, mk.r3, 0u), p.plan.tile_blocks);
    F26 sum = f26_zero();
    for (uint32_t g = lane; g < p.plan.groups; g += 256u) {  // <= 4 terms per lane
        const uint64_t done = (uint64_t)(g + 1u) * p.plan.tiles_per_group;
        const uint32_t after = done >= p.plan.tiles ? 0u : (uint32_t)(p.plan.tiles - done);  // < 2^20
        sum = f26_add(sum, fmul(load_f26(p.ws + (uint64_t)g * kMsgPartialWords), fpow(R, after)));
    }
    const F26 total = block_sum(carry1(sum), red, lane);
    if (lane != 0u) return;
    const uint32_t diff = msg_tag_finish<OPEN>(total, mk.s, p.in, p.out, p.n);
    if constexpr (OPEN) *p.status = diff != 0u ? 1u : 0u;
}

// A failed open hands out no plaintext (chacha20_poly1305.rs:89-93): zero
// out[0, n) when the status on the device says so.
__global__ __launch_bounds__(256) void sg_msg_scrub_kernel(uint8_t* out, const uint64_t n, const uint8_t* status) {
    if (*status == 0u) return;
    msg_zero(out, n, (uint64_t)blockIdx.x * 256u + threadIdx.x, (uint64_t)gridDim.x * 256u);
}

}  // namespace

// nonce_hi: NULL = the draft (word 13 is 0), else the first four bytes of the
// RFC 8439 nonce; the plan is the one of that layout (sg_msg_plan_for_flags)
hipError_t launch_msg(const uint8_t* key, const uint8_t nonce[8], const uint8_t* nonce_hi, const uint8_t* ad,
                      uint64_t adlen, const uint8_t* in, uint8_t* out, uint64_t n, uint8_t* status, uint32_t* ws,
                      const sg_msg_plan& plan, bool open, bool scrub, hipStream_t s) {
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
    // the nonce as little-endian words (chacha20.rs:45-46; RFC 8439 section 2.3)
    p.n13 = nonce_hi ? dev::le32(nonce_hi) : 0u;
    p.n14 = dev::le32(nonce);
    p.n15 = dev::le32(nonce + 4);
    p.plan = plan;
    with_form(nonce_hi != nullptr, open, [&](auto OPEN, auto C) {
        hipLaunchKernelGGL((sg_msg_kernel<OPEN.value, C.value>), dim3(plan.groups), dim3(kMsgThreads), 0, s, p);
        hipLaunchKernelGGL((sg_msg_finish_kernel<OPEN.value, C.value>), dim3(1), dim3(256), 0, s, p);
    });
    if (open && scrub && n) {
        const uint64_t blocks = (n / 16u + 1023u) / 1024u;
        const uint32_t grid = blocks < 1u ? 1u : (blocks > 4096u ? 4096u : (uint32_t)blocks);
        hipLaunchKernelGGL(sg_msg_scrub_kernel, dim3(grid), dim3(256), 0, s, out, n, (const uint8_t*)status);
    }
    return hipGetLastError();
}

}  // namespace sg
