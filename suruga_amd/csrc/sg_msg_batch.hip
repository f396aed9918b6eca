// sg_msg_batch.hip -- gfx950 kernels of the message batch: many messages, each
// with its own key, nonce, AD and lengths (any, up to SG_MSG_MAX_LEN), sealed
// or opened by one persistent grid, the whole call in the draft construction or
// (SG_MSG_RFC8439) in RFC 8439.  The decomposition of one message is that
// of sg_msg.hip, tile for tile (the tile body, the keying and the finish are
// the shared code of sg_msg_device.h); here it is applied across messages:
//
//   * Every message m keeps its own tile geometry: z_m virtual blocks in
//     front, T_m tiles of K = 1020 MAC blocks.  The tiles of all messages, in
//     order, form one sequence; workgroup g owns a contiguous run of it, cut
//     at message boundaries into segments (message m, tiles [a, b) of m)
//     (sg_msg_batch_plan_for; the tables arrive in the workspace).
//   * At a segment's start the group keys from the message's descriptor (block
//     0 -> r, s; R = r^K; the lane's power of r; the ChaCha20 state), runs the
//     tile body over [a, b) with the per-lane chain a_l = a_l R + f_(t,l) from
//     zero, and stores the segment's partial
//     H_seg = sum_t h_t R^(b - 1 - t) = sum_l a_l r^(4 (254 - l)).
//   * sg_msg_batch_finish_kernel, one wave per message, adds
//     H_seg R^(T_m - b) over the message's segments -- the message's Horner
//     polynomial, split at tile boundaries, every piece at its own power --
//     reduces, adds s and writes the tag or compares it in constant time.
//   * sg_msg_batch_scrub_kernel zeroes out[0, n) of every message whose status
//     says SG_E_BAD_MAC, segment by segment on the same grid.
//
// Everything is exact mod p = 2^130 - 5.  No group waits for another: there
// are no counters, flags or spin loops; the stream orders the finish behind
// the grid and the scrub behind the finish.
#include "sg_msg_device.h"

namespace sg {

struct MsgBatchParams {
    const MsgBatchItem* items;
    const sg_msg_plan* plans;
    const sg_msg_span* msg_segs;
    const sg_msg_seg* segs;
    const sg_msg_span* group_segs;
    uint32_t* partials;  // one per segment, kMsgPartialWords words
    uint8_t* status;
    uint32_t count;
};

namespace {

// wave-uniform loads of the tables: every lane reads the same address, the
// value moves to SGPRs
__device__ __forceinline__ uint32_t uload(const uint32_t* p) { return uniform(*p); }
__device__ __forceinline__ uint64_t uload(const uint64_t* p) {
    const uint64_t v = *p;
    return (uint64_t)uniform((uint32_t)v) | ((uint64_t)uniform((uint32_t)(v >> 32)) << 32);
}
template <class T>
__device__ __forceinline__ T* uload(T* const* p) {
    return (T*)(uintptr_t)uload((const uint64_t*)p);
}

// data bytes [d0, d1) of tiles [a, b) of a message: the tile body's own cut
template <Construction C>
__device__ __forceinline__ void seg_data_range(const uint64_t zero_blocks, const uint64_t n, const uint64_t adlen,
                                               const uint32_t a, const uint32_t b, int64_t* d0, int64_t* d1) {
    const int64_t P = ct_offset<C>((int64_t)adlen);
    const int64_t s0 = (int64_t)a * (int64_t)kMsgTileBytes - 16 * (int64_t)zero_blocks;
    const int64_t s1 = (int64_t)b * (int64_t)kMsgTileBytes - 16 * (int64_t)zero_blocks;
    *d0 = s0 - P > 0 ? s0 - P : 0;
    *d1 = s1 - P < (int64_t)n ? s1 - P : (int64_t)n;
}

template <bool OPEN, Construction C>
__global__ __launch_bounds__(256) void sg_msg_batch_kernel(const MsgBatchParams p) {
    __shared__ __attribute__((aligned(64))) uint8_t lds[kLdsBytes];
    const uint32_t lane = threadIdx.x;
    const uint32_t first = uload(&p.group_segs[blockIdx.x].first);
    const uint32_t end = first + uload(&p.group_segs[blockIdx.x].count);
    for (uint32_t sgi = first; sgi < end; ++sgi) {
        const sg_msg_seg* sg = p.segs + sgi;
        const uint32_t mi = uload(&sg->msg);
        const uint32_t ta = uload(&sg->tile_begin), tb = uload(&sg->tile_end);
        const MsgBatchItem* it = p.items + mi;
        if (uload(&it->skip) != 0u) continue;  // an open of fewer than 16 bytes: nothing is touched
        const uint32_t n14 = uload(&it->n14), n15 = uload(&it->n15);
        const uint32_t n13 = C == Construction::kRfc8439 ? uload(&it->n13) : 0u;
        // ---- the message's keying, as sg_msg_kernel's
        const MsgKey mk = msg_key(uload(&it->key), n13, n14, n15);
        const MsgR rr = msg_r(mk);
        const F26 r = words_to_f26(mk.r0, mk.r1, mk.r2, mk.r3, 0u);
        const F26 R = fpow(r, kMsgTileBlocks);
        const F26 Pl = msg_lane_power(r, lane);
        const ChaChaPre pre = chacha_pre(mk.k, n13, n14, n15);
        const sg_msg_plan* pl = p.plans + mi;
        const MsgStream m = msg_stream<C>(uload(&it->ad), uload(&it->in), uload(&it->out), n13, n14, n15,
                                          uload(&it->n), uload(&it->adlen), uload(&pl->mac_blocks),
                                          uload(&pl->zero_blocks), kMsgTileBlocks, kMsgTileBytes);
        F26 acc = f26_zero();
        for (uint64_t t = ta; t < tb; ++t) msg_tile<OPEN, C>(lds, lane, m, mk, pre, rr, R, t, acc);
        // ---- the segment's partial: sum of the lanes' chains, each at its place in a tile
        const F26 Hs = block_sum(fmul(acc, Pl), reinterpret_cast<uint32_t*>(lds), lane);
        if (lane == 0u) store_f26(p.partials + (uint64_t)sgi * kMsgPartialWords, Hs);
        __syncthreads();  // the next segment's tile stores follow lane 0's loads of the sum
    }
}

// Sum over one wave's 64 lanes of reduced elements, valid in its lane 0.
// red: the wave's own 5 * (64 + 4) words of LDS.
__device__ __forceinline__ F26 wave_sum(const F26 x, uint32_t* red, const uint32_t wl) {
    store_f26(red + 5u * wl, x);
    wave_lds_sync();
    if (wl < 4u) {
        F26 a = f26_zero();
        for (uint32_t i = 0; i < 16u; ++i) a = f26_add(a, load_f26(red + 5u * (16u * wl + i)));  // < 2^31
        store_f26(red + 5u * (64u + wl), carry1(a));
    }
    wave_lds_sync();
    F26 a = f26_zero();
    if (wl == 0u) {
        for (uint32_t i = 0; i < 4u; ++i) a = f26_add(a, load_f26(red + 5u * (64u + i)));
        a = carry1(a);
    }
    return a;
}

constexpr uint32_t kFinishWaves = 4;  // messages per workgroup of the finish kernel

template <bool OPEN, Construction C>
__global__ __launch_bounds__(256) void sg_msg_batch_finish_kernel(const MsgBatchParams p) {
    __shared__ uint32_t red[kFinishWaves][5u * (64u + 4u)];
    const uint32_t wave = threadIdx.x >> 6, wl = threadIdx.x & 63u;
    const uint32_t mi = uniform(blockIdx.x * kFinishWaves + wave);
    if (mi >= p.count) return;  // the whole wave; the waves of a workgroup never meet
    const MsgBatchItem* it = p.items + mi;
    if (uload(&it->skip) != 0u) {
        if constexpr (OPEN)
            if (wl == 0u) p.status[mi] = (uint8_t)SG_E_SHORT;  // chacha20_poly1305.rs:68-70
        return;
    }
    const MsgKey mk = msg_key(uload(&it->key), C == Construction::kRfc8439 ? uload(&it->n13) : 0u, uload(&it->n14),
                              uload(&it->n15));
    const F26 R = fpow(words_to_f26(mk.r0, mk.r1, mk.r2, mk.r3, 0u), kMsgTileBlocks);
    const uint32_t tiles = (uint32_t)uload(&p.plans[mi].tiles);  // < 2^30
    const uint32_t first = uload(&p.msg_segs[mi].first), cnt = uload(&p.msg_segs[mi].count);
    F26 sum = f26_zero();
    for (uint32_t i = wl; i < cnt; i += 64u) {  // a message may have up to kMsgMaxGroups segments
        const uint32_t after = tiles - p.segs[first + i].tile_end;
        sum = fmul_add(load_f26(p.partials + (uint64_t)(first + i) * kMsgPartialWords), fpow(R, after), sum);
    }
    const F26 total = wave_sum(sum, red[wave], wl);
    if (wl != 0u) return;
    const uint64_t n = uload(&it->n);
    const uint32_t diff = msg_tag_finish<OPEN>(total, mk.s, uload(&it->in), uload(&it->out), n);
    if constexpr (OPEN) p.status[mi] = diff != 0u ? (uint8_t)SG_E_BAD_MAC : (uint8_t)SG_OK;
}

// A failed open hands out no plaintext (chacha20_poly1305.rs:89-93): the grid
// of the batch kernel again, every segment zeroing its own data bytes of a
// message whose status says SG_E_BAD_MAC.
template <Construction C>
__global__ __launch_bounds__(256) void sg_msg_batch_scrub_kernel(const MsgBatchParams p) {
    const uint32_t first = uload(&p.group_segs[blockIdx.x].first);
    const uint32_t end = first + uload(&p.group_segs[blockIdx.x].count);
    for (uint32_t sgi = first; sgi < end; ++sgi) {
        const sg_msg_seg* sg = p.segs + sgi;
        const uint32_t mi = uload(&sg->msg);
        if (uniform(p.status[mi]) != (uint32_t)SG_E_BAD_MAC) continue;
        const MsgBatchItem* it = p.items + mi;
        const uint64_t n = uload(&it->n);
        int64_t d0, d1;
        seg_data_range<C>(uload(&p.plans[mi].zero_blocks), n, uload(&it->adlen), uload(&sg->tile_begin),
                          uload(&sg->tile_end), &d0, &d1);
        if (d1 > d0) msg_zero(uload(&it->out) + d0, (uint64_t)(d1 - d0), threadIdx.x, 256u);
    }
}

}  // namespace

// rfc8439: the whole call speaks RFC 8439 (the items carry n13, the plans are
// those of that layout); else the draft
hipError_t launch_msg_batch(const MsgBatchLayout& l, void* ws, uint32_t count, uint32_t groups, uint8_t* status,
                            bool open, bool scrub, bool rfc8439, hipStream_t s) {
    if (count == 0u || groups == 0u || groups > kMsgMaxGroups) return hipErrorInvalidValue;
    uint8_t* w = (uint8_t*)ws;
    MsgBatchParams p;
    p.items = (const MsgBatchItem*)(w + l.items);
    p.plans = (const sg_msg_plan*)(w + l.plans);
    p.msg_segs = (const sg_msg_span*)(w + l.msg_segs);
    p.segs = (const sg_msg_seg*)(w + l.segs);
    p.group_segs = (const sg_msg_span*)(w + l.group_segs);
    p.partials = (uint32_t*)(w + l.partials);
    p.status = status;
    p.count = count;
    const dim3 fin((count + kFinishWaves - 1u) / kFinishWaves);
    with_form(rfc8439, open, [&](auto OPEN, auto C) {
        hipLaunchKernelGGL((sg_msg_batch_kernel<OPEN.value, C.value>), dim3(groups), dim3(kMsgThreads), 0, s, p);
        hipLaunchKernelGGL((sg_msg_batch_finish_kernel<OPEN.value, C.value>), fin, dim3(256), 0, s, p);
        if (OPEN.value && scrub)
            hipLaunchKernelGGL(sg_msg_batch_scrub_kernel<C.value>, dim3(groups), dim3(256), 0, s, p);
    });
    return hipGetLastError();
}

}  // namespace sg
