// sg_quic.hip -- QUIC packet protection of a batch in one launch (RFC 9001 section 5.3,
// 5.4; sg_seal_batch_quic / sg_open_batch_quic, suruga_gpu.h): per packet the header
// protection mask, the keying (keystream block 0), the payload XOR, the RFC 8439 MAC over
// header || payload, and on open the packet number decoding of RFC 9000 appendix A.3, the
// tag compare and the scrub of a failed packet.
//
// G lanes per packet (8 where the call's max_len is at most 2 KiB, else 16), 256 / G
// packets per workgroup, an exact grid; no LDS, no atomics, no workspace.  A lane owns
// whole 64-byte payload chunks: it loads one with four unaligned 16-byte loads (packets lie
// at any byte address: there is no aligned fast path to fall from), XORs its keystream
// block, stores it the same way and runs Poly1305 over the four ciphertext blocks from the
// registers they are in.  Only the header, the tail of n % 64 bytes and the length block go
// byte by byte.  sg_quic.h (Geom) says which lane owns which chunk and how the lanes' sums
// add up to the sequential accumulator, exactly mod 2^130 - 5: right-aligned slots, so that
// lane t's sum weighs P^(G - 1 - t), P = r^(4 Q), and a Hillis-Steele pass over the group
// (log2 G multiply-adds) leaves the whole in the last lane; tests/quic_model.py restates it.
//
// What every lane of a group needs alike -- the header protection mask on open, the packet
// number, keystream block 0 -- each lane computes for itself: a lane that waited for
// another's result would idle for the same time.
//
// Seal applies header protection last.  Its sample is ciphertext (and, under a short
// payload, tag) that other lanes of the group have just stored, so the group's stores are
// made visible within the workgroup and the sample is read back from `out`; open's scrub of
// a failed packet follows the same fence.
#include "sg_device.h"
#include "sg_quic.h"

namespace sg {
namespace {

using namespace dev;

constexpr uint32_t kQuicThreads = 256;

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

// The header as the AEAD sees it: the unprotected first byte, the input's bytes up to the
// packet number field, the packet number's low pn_len bytes big-endian.
struct Header {
    const uint8_t* in;
    uint64_t pn;
    uint32_t pn_off, pn_len, hdr_len, b0;
    __device__ __forceinline__ uint32_t byte(uint32_t i) const {
        if (i == 0u) return b0;
        if (i >= pn_off) return (uint32_t)(pn >> (8u * (hdr_len - 1u - i))) & 0xffu;
        return in[i];
    }
    // 16-byte block a of the zero-padded header, as a little-endian word each
    __device__ __forceinline__ uint32_t word(uint32_t a, uint32_t j) const {
        uint32_t w = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint32_t i = 16u * a + 4u * j + b;
            if (i < hdr_len) w |= byte(i) << (8u * b);
        }
        return w;
    }
};

// the five mask bytes of RFC 9001 section 5.4.4 under the header protection key `hk`
__device__ __forceinline__ uint64_t hp_mask(const uint8_t* hk, const uint8_t* sample) {
    uint32_t k[8], ks[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = ldu32(hk + 4 * i);
    chacha_block(ks, k, ldu32(sample), ldu32(sample + 4), ldu32(sample + 8), ldu32(sample + 12));
    return (uint64_t)ks[0] | ((uint64_t)(ks[1] & 0xffu) << 32);
}
__device__ __forceinline__ uint32_t first_byte_mask(uint32_t b0, uint64_t mask) {
    return (uint32_t)mask & ((b0 & 0x80u) ? 0x0fu : 0x1fu);
}

template <bool OPEN, uint32_t G>
__global__ __launch_bounds__(kQuicThreads) void sg_quic_kernel(const quic::Params p) {
    static_assert(G == 8u || G == 16u, "a group is a power of two and lies inside one wave");
    const uint32_t t = threadIdx.x % G;
    const uint64_t pkt64 = (uint64_t)blockIdx.x * (kQuicThreads / G) + threadIdx.x / G;
    if (pkt64 >= p.count) return;  // whole groups leave together, here and below
    const uint32_t pkt = (uint32_t)pkt64;
    const uint32_t len = p.len ? p.len[pkt] : p.uniform_len;
    uint8_t* const stp = p.status + pkt;
    if (len > p.max_len) {
        if (t == 0u) *stp = SG_STATUS_SKIPPED;
        return;
    }
    const uint32_t pn_off = p.pn_off ? p.pn_off[pkt] : p.uniform_pn_off;
    // seal reads the first byte, open the sample that ends at pn_off + 20
    if (pn_off < quic::kMinPnOff || pn_off > SG_QUIC_MAX_PN_OFF || (OPEN ? len < pn_off + quic::kSampleEnd : len <= pn_off)) {
        if (t == 0u) *stp = SG_E_SHORT;
        return;
    }
    const uint8_t* const in = p.in + (p.in_off ? p.in_off[pkt] : p.in_stride * pkt);
    uint8_t* const out = p.out + (p.out_off ? p.out_off[pkt] : p.out_stride * pkt);
    const uint32_t ki = p.key_index ? p.key_index[pkt] : 0u;
    const uint32_t conn = ki < p.rows ? ki : p.rows - 1u;
    const uint8_t* const hk = p.hp_keys + 32ull * conn;

    Header hd;
    hd.in = in;
    hd.pn_off = pn_off;
    uint64_t mask = 0;
    if constexpr (OPEN) {
        mask = hp_mask(hk, in + pn_off + 4u);
        const uint32_t b0p = in[0];
        hd.b0 = b0p ^ first_byte_mask(b0p, mask);
        hd.pn_len = (hd.b0 & 3u) + 1u;
        uint32_t trunc = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
            if (j < hd.pn_len) trunc = (trunc << 8) | (in[pn_off + j] ^ ((uint32_t)(mask >> (8u * (j + 1u))) & 0xffu));
        hd.pn = quic::decode_pn(p.pn[pkt], trunc, hd.pn_len);
    } else {
        hd.b0 = in[0];
        hd.pn_len = (hd.b0 & 3u) + 1u;
        hd.pn = p.pn[pkt];
    }
    hd.hdr_len = pn_off + hd.pn_len;
    if constexpr (!OPEN) {
        if (len < hd.hdr_len || hd.pn_len + (len - hd.hdr_len) < 4u) {  // no full sample (section 5.4.2)
            if (t == 0u) *stp = SG_E_SHORT;
            return;
        }
    }
    const uint32_t hdr_len = hd.hdr_len;
    const uint32_t n = len - hdr_len - (OPEN ? SG_MAC_LEN : 0u);  // open: len >= pn_off + 20 >= hdr_len + 16

    // key and IV row: the connection's, or under KEY_PHASE the generation the packet names
    const uint32_t phase = (hd.b0 & 0x80u) ? 0u : (hd.b0 >> 2) & 1u;
    const uint32_t row = p.key_phase ? 2u * conn + phase : conn;
    uint32_t k[8], ks[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = ldu32(p.keys + 32ull * row + 4 * i);
    const uint32_t* const iv = reinterpret_cast<const uint32_t*>(p.ivs + 12ull * row);
    const uint32_t n13 = iv[0];
    const uint32_t n14 = iv[1] ^ bswap32((uint32_t)(hd.pn >> 32));
    const uint32_t n15 = iv[2] ^ bswap32((uint32_t)hd.pn);

    chacha_block(ks, k, 0u, n13, n14, n15);
    const PolyKey pk = poly_key(ks);
    const F26 r = words_to_f26(pk.r0, pk.r1, pk.r2, pk.r3, 0u);

    const quic::Geom g = quic::geom(n, G);
    const uint8_t* const src = in + hdr_len;
    uint8_t* const dst = out + hdr_len;
    F26 h = f26_zero(), ts = f26_zero();
    for (uint32_t q = 0; q < g.q; ++q) {
        const uint32_t v = t * g.q + q;
        const bool full = v >= g.zc;
        if (full || v == 0u) {
            const uint32_t c = full ? v - g.zc : g.nf;  // the chunk; slot 0 takes the tail
            chacha_block(ks, k, c + 1u, n13, n14, n15);
            const uint8_t* const s = src + 64ull * c;
            uint8_t* const d = dst + 64ull * c;
            if (full) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u32x4 a = ldu16(s + 16 * j);
                    const u32x4 x = {a[0] ^ ks[4 * j], a[1] ^ ks[4 * j + 1], a[2] ^ ks[4 * j + 2], a[3] ^ ks[4 * j + 3]};
                    stu16(d + 16 * j, x);
                    const u32x4 m = OPEN ? a : x;  // the MAC runs over the ciphertext
                    h = mac_block(h, m[0], m[1], m[2], m[3], r);
                }
            } else {
                // the tail's g.tail < 64 bytes, zero-padded to whole MAC blocks, then the length block
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    uint32_t m[4];
#pragma unroll
                    for (uint32_t w = 0; w < 4u; ++w) {
                        uint32_t a = 0u, keep = 0u;
#pragma unroll
                        for (uint32_t b = 0; b < 4u; ++b) {
                            const uint32_t i = 16u * j + 4u * w + b;
                            if (i < g.tail) {
                                a |= (uint32_t)s[i] << (8u * b);
                                keep |= 0xffu << (8u * b);
                            }
                        }
                        const uint32_t x = (a ^ ks[4u * j + w]) & keep;
#pragma unroll
                        for (uint32_t b = 0; b < 4u; ++b) {
                            const uint32_t i = 16u * j + 4u * w + b;
                            if (i < g.tail) d[i] = (uint8_t)(x >> (8u * b));
                        }
                        m[w] = OPEN ? a : x;
                    }
                    if (j < g.kt) ts = mac_block(ts, m[0], m[1], m[2], m[3], r);
                }
                ts = mac_block(ts, hdr_len, 0u, n, 0u, r);  // le64(|ad|) || le64(|ct|)
            }
        }
        if (v + 1u == g.zc) {  // the slot in front of chunk 0: the additional data's blocks, h is 0 so far
            const uint32_t na = (hdr_len + 15u) / 16u;
            for (uint32_t a = 0; a < na; ++a) h = mac_block(h, hd.word(a, 0), hd.word(a, 1), hd.word(a, 2), hd.word(a, 3), r);
        }
    }

    // sum_t H_t P^(G - 1 - t) into the last lane, P = r^(4 Q)
    const F26 r2 = fmul(r, r);
    F26 pw = fpow(fmul(r2, r2), g.q);
#pragma unroll
    for (uint32_t s = 1; s < G; s <<= 1) {
        F26 up;
        up.v0 = __shfl_up(h.v0, s, G); up.v1 = __shfl_up(h.v1, s, G); up.v2 = __shfl_up(h.v2, s, G);
        up.v3 = __shfl_up(h.v3, s, G); up.v4 = __shfl_up(h.v4, s, G);
        if (t < s) up = f26_zero();
        h = fmul_add(up, pw, h);
        pw = fmul(pw, pw);
    }
    // ... behind it the tail's blocks and the length block: S r^(kt + 1) + TS
    ts.v0 = __shfl(ts.v0, 0, G); ts.v1 = __shfl(ts.v1, 0, G); ts.v2 = __shfl(ts.v2, 0, G);
    ts.v3 = __shfl(ts.v3, 0, G); ts.v4 = __shfl(ts.v4, 0, G);
    for (uint32_t j = 0; j <= g.kt; ++j) h = fmul(h, r);
    uint32_t tw[4];
    tag_words(f26_add(h, ts), pk.s, tw);

    if constexpr (OPEN) {
        uint32_t bad = 0u;
        if (t == G - 1u) {
            const uint8_t* const tp = src + n;
            const uint32_t rx[4] = {ldu32(tp), ldu32(tp + 4), ldu32(tp + 8), ldu32(tp + 12)};
            bad = tag_mismatch(rx, tw);
        }
        bad = __shfl(bad, G - 1u, G);
        const bool scrub = bad && !p.keep_failed;
        if (!scrub) {
            for (uint32_t i = t; i < hdr_len; i += G) out[i] = (uint8_t)hd.byte(i);
        } else {
            group_sync();  // behind the other lanes' plaintext
            for (uint32_t i = t; i < hdr_len + n; i += G) out[i] = 0u;
        }
        if (t == 0u) {
            p.pn_out[pkt] = scrub ? 0ull : hd.pn;
            *stp = bad ? SG_E_BAD_MAC : SG_OK;
        }
    } else {
        if (t == G - 1u) stu16(dst + n, u32x4{tw[0], tw[1], tw[2], tw[3]});
        group_sync();  // the sample is what the group has just stored
        mask = hp_mask(hk, out + pn_off + 4u);
        for (uint32_t i = t; i < hdr_len; i += G) {
            uint32_t m = 0u;
            if (i == 0u) m = first_byte_mask(hd.b0, mask);
            else if (i >= pn_off) m = (uint32_t)(mask >> (8u * (i - pn_off + 1u))) & 0xffu;
            out[i] = (uint8_t)(hd.byte(i) ^ m);
        }
        if (t == 0u) *stp = SG_OK;
    }
}

}  // namespace

namespace quic {

int launch(const Params& p, bool open, void* stream) {
    const uint32_t G = lanes_for(p.max_len);
    const uint32_t per = kQuicThreads / G;
    const uint32_t grid = (uint32_t)(((uint64_t)p.count + per - 1u) / per);
    hipStream_t s = (hipStream_t)stream;
    if (G == 8u) {
        if (open) hipLaunchKernelGGL((sg_quic_kernel<true, 8u>), dim3(grid), dim3(kQuicThreads), 0, s, p);
        else hipLaunchKernelGGL((sg_quic_kernel<false, 8u>), dim3(grid), dim3(kQuicThreads), 0, s, p);
    } else {
        if (open) hipLaunchKernelGGL((sg_quic_kernel<true, 16u>), dim3(grid), dim3(kQuicThreads), 0, s, p);
        else hipLaunchKernelGGL((sg_quic_kernel<false, 16u>), dim3(grid), dim3(kQuicThreads), 0, s, p);
    }
    return (int)hipGetLastError();
}

}  // namespace quic
}  // namespace sg
