// sg_wg.hip -- WireGuard transport data messages of a batch in one launch (whitepaper
// section 5.4.6; sg_seal_batch_wg / sg_open_batch_wg, suruga_gpu.h): per packet the keying
// (keystream block 0), the payload XOR, the RFC 8439 MAC over the ciphertext with an empty
// AD, on seal the 16-byte header and the zero padding of the inner packet, on open the
// header check, the counter off the wire, the tag compare, the scrub of a failed packet
// and the inner packet's length from its IP header.
//
// The geometry is sg_quic.hip's: G lanes per packet (8 where the call's max_len is at most
// 2 KiB, else 16), 256 / G packets per workgroup, an exact grid; no LDS, no atomics, no
// workspace.  A lane owns whole 64-byte chunks of the AEAD's P bytes, moved with unaligned
// 16-byte loads and stores, and runs Poly1305 over the four ciphertext blocks from the
// registers they are in; the tail of P % 64 bytes and the length block go byte by byte in
// slot 0.  sg_quic.h (Geom) says which lane owns which chunk and how the lanes' sums add
// up; the slot in front of chunk 0, which holds a QUIC packet's header, holds nothing here.
//
// Chunks are laid over the padded length P, so on seal the chunk that holds byte len is
// part content and part zeros.  P - len < 16, so of a whole chunk only its last 16-byte
// block can be cut: that block is loaded byte by byte up to len, never beyond it, and the
// whole chunk is stored, the ciphertext of a zero byte being the keystream byte.  In the
// tail the loads stop at len and the stores at P.
//
// In place (seal out + 16 == in, open out == in + 16) the payload stays at its address: a
// lane stores a chunk over the bytes it has itself just loaded, no lane loads another's
// chunk, and what every lane reads for itself -- open's type word and counter, in front of
// the stored range -- or reads late -- the received tag, behind it -- is never stored to.
// The header, the padding and the tag of a seal lie outside its len input bytes.  Open's
// inner-length parse takes the first plaintext words from the registers of the lane that
// decrypted them, not from `out`.
#include "sg_device.h"
#include "sg_wg.h"

namespace sg {
namespace {

using namespace dev;

constexpr uint32_t kWgThreads = 256;

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

// the first `have` (< 16) bytes at s as a 16-byte block, zeros behind them; s[have] on is not read
__device__ __forceinline__ u32x4 ld_cut16(const uint8_t* s, uint32_t have) {
    u32x4 a = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
        uint32_t x = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint32_t i = 4u * w + b;
            if (i < have) x |= (uint32_t)s[i] << (8u * b);
        }
        a[w] = x;
    }
    return a;
}

// The inner packet's length from the first two words of its IP header (n bytes decrypted),
// 0 where it does not fit: IPv4's total length, 20 <= L <= n; IPv6's payload length + 40 <= n.
__device__ __forceinline__ uint32_t inner_len_of(uint32_t w0, uint32_t w1, uint32_t n) {
    const uint32_t ver = (w0 >> 4) & 0xfu;
    if (ver == 4u && n >= 20u) {
        const uint32_t L = ((w0 >> 8) & 0xff00u) | (w0 >> 24);
        return (L >= 20u && L <= n) ? L : 0u;
    }
    if (ver == 6u && n >= 40u) {
        const uint32_t L = 40u + (((w1 << 8) & 0xff00u) | ((w1 >> 8) & 0xffu));
        return L <= n ? L : 0u;
    }
    return 0u;
}

template <bool OPEN, uint32_t G>
__global__ __launch_bounds__(kWgThreads) void sg_wg_kernel(const wg::Params p) {
    static_assert(G == 8u || G == 16u, "a group is a power of two and lies inside one wave");
    const uint32_t t = threadIdx.x % G;
    const uint64_t pkt64 = (uint64_t)blockIdx.x * (kWgThreads / G) + threadIdx.x / G;
    if (pkt64 >= p.count) return;  // whole groups leave together, here and below
    const uint32_t pkt = (uint32_t)pkt64;
    const uint32_t len = p.len ? p.len[pkt] : p.uniform_len;
    uint8_t* const stp = p.status + pkt;
    if (len > p.max_len) {
        if (t == 0u) *stp = SG_STATUS_SKIPPED;
        return;
    }
    if (OPEN && len < wg::kOverhead) {
        if (t == 0u) *stp = SG_E_SHORT;
        return;
    }
    const uint8_t* const in = p.in + (p.in_off ? p.in_off[pkt] : p.in_stride * pkt);
    uint8_t* const out = p.out + (p.out_off ? p.out_off[pkt] : p.out_stride * pkt);
    // open: the type word and the counter, every lane for itself
    uint64_t ctr;
    if constexpr (OPEN) {
        if (ldu32(in) != 4u) {
            if (t == 0u) *stp = SG_STATUS_BAD_HEADER;
            return;
        }
        ctr = (uint64_t)ldu32(in + 8) | ((uint64_t)ldu32(in + 12) << 32);
    } else {
        ctr = p.counter[pkt];
    }
    const uint32_t ki = p.key_index ? p.key_index[pkt] : 0u;
    const uint32_t row = ki < p.num_keys ? ki : p.num_keys - 1u;
    // n bytes through the AEAD, of which the first `have` come from the input (seal: the rest are zeros)
    const uint32_t n = OPEN ? len - wg::kOverhead : wg::padded_len(len, p.pad_cap);
    const uint32_t have = OPEN ? n : len;
    const uint8_t* const src = OPEN ? in + SG_WG_HEADER_LEN : in;
    uint8_t* const dst = OPEN ? out : out + SG_WG_HEADER_LEN;

    uint32_t k[8], ks[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = ldu32(p.keys + 32ull * row + 4 * i);
    const uint32_t n14 = (uint32_t)ctr, n15 = (uint32_t)(ctr >> 32);  // nonce 00 00 00 00 || le64(counter)

    chacha_block(ks, k, 0u, 0u, n14, n15);
    const PolyKey pk = poly_key(ks);
    const F26 r = words_to_f26(pk.r0, pk.r1, pk.r2, pk.r3, 0u);

    const quic::Geom g = quic::geom(n, G);
    F26 h = f26_zero(), ts = f26_zero();
    uint32_t pw0 = 0u, pw1 = 0u;  // open: the first two plaintext words, in the lane that decrypts them
    for (uint32_t q = 0; q < g.q; ++q) {
        const uint32_t v = t * g.q + q;
        const bool full = v >= g.zc;
        if (full || v == 0u) {
            const uint32_t c = full ? v - g.zc : g.nf;  // the chunk; slot 0 takes the tail
            chacha_block(ks, k, c + 1u, 0u, n14, n15);
            const uint8_t* const s = src + 64ull * c;
            uint8_t* const d = dst + 64ull * c;
            if (full) {
                // seal: the chunk that holds byte `have` has 49..63 input bytes, its last block is cut
                const bool whole = OPEN || 64u * c + 64u <= have;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u32x4 a = (j < 3 || whole) ? ldu16(s + 16 * j) : ld_cut16(s + 48, have - 64u * c - 48u);
                    const u32x4 x = {a[0] ^ ks[4 * j], a[1] ^ ks[4 * j + 1], a[2] ^ ks[4 * j + 2], a[3] ^ ks[4 * j + 3]};
                    stu16(d + 16 * j, x);
                    const u32x4 m = OPEN ? a : x;  // the MAC runs over the ciphertext
                    h = mac_block(h, m[0], m[1], m[2], m[3], r);
                    if (OPEN && j == 0 && c == 0u) { pw0 = x[0]; pw1 = x[1]; }
                }
            } else {
                // the tail's g.tail < 64 bytes, zero-padded to whole MAC blocks, then the length block;
                // seal: the input ends `lim` bytes into it
                const uint32_t base = 64u * g.nf;
                const uint32_t lim = OPEN ? g.tail : (have > base ? have - base : 0u);
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    uint32_t m[4];
#pragma unroll
                    for (uint32_t w = 0; w < 4u; ++w) {
                        uint32_t a = 0u, keep = 0u;
#pragma unroll
                        for (uint32_t b = 0; b < 4u; ++b) {
                            const uint32_t i = 16u * j + 4u * w + b;
                            if (i < lim) a |= (uint32_t)s[i] << (8u * b);
                            if (i < g.tail) keep |= 0xffu << (8u * b);
                        }
                        const uint32_t x = (a ^ ks[4u * j + w]) & keep;
#pragma unroll
                        for (uint32_t b = 0; b < 4u; ++b) {
                            const uint32_t i = 16u * j + 4u * w + b;
                            if (i < g.tail) d[i] = (uint8_t)(x >> (8u * b));
                        }
                        m[w] = OPEN ? a : x;
                        if (OPEN && j == 0u && w == 0u && g.nf == 0u) pw0 = x;
                        if (OPEN && j == 0u && w == 1u && g.nf == 0u) pw1 = x;
                    }
                    if (j < g.kt) ts = mac_block(ts, m[0], m[1], m[2], m[3], r);
                }
                ts = mac_block(ts, 0u, 0u, n, 0u, r);  // le64(|ad| = 0) || le64(|ct|)
            }
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
        if (scrub) {
            group_sync();  // behind the other lanes' plaintext
            for (uint32_t i = t; i < n; i += G) out[i] = 0u;
        }
        // the IP header's first words from the lane of chunk 0, or of the tail where there is no chunk
        const uint32_t owner = g.nf ? g.zc / g.q : 0u;
        const uint32_t w0 = __shfl(pw0, owner, G), w1 = __shfl(pw1, owner, G);
        if (t == 0u) {
            uint32_t st = bad ? SG_E_BAD_MAC : SG_OK, L = 0u;
            if (!bad && p.inner_len && n != 0u) {  // on a failed tag nothing is parsed
                L = inner_len_of(w0, w1, n);
                if (L == 0u) st = SG_STATUS_BAD_INNER;
            }
            p.counter_out[pkt] = scrub ? 0ull : ctr;
            if (p.inner_len) p.inner_len[pkt] = L;
            *stp = (uint8_t)st;
        }
    } else {
        if (t == G - 1u) stu16(dst + n, u32x4{tw[0], tw[1], tw[2], tw[3]});
        if (t == 0u) {
            stu16(out, u32x4{4u, p.receiver[row], n14, n15});  // le32(4) || le32(receiver) || le64(counter)
            *stp = SG_OK;
        }
    }
}

}  // namespace

namespace wg {

int launch(const Params& p, bool open, void* stream) {
    const uint32_t G = quic::lanes_for(p.max_len);
    const uint32_t per = kWgThreads / G;
    const uint32_t grid = (uint32_t)(((uint64_t)p.count + per - 1u) / per);
    hipStream_t s = (hipStream_t)stream;
    if (G == 8u) {
        if (open) hipLaunchKernelGGL((sg_wg_kernel<true, 8u>), dim3(grid), dim3(kWgThreads), 0, s, p);
        else hipLaunchKernelGGL((sg_wg_kernel<false, 8u>), dim3(grid), dim3(kWgThreads), 0, s, p);
    } else {
        if (open) hipLaunchKernelGGL((sg_wg_kernel<true, 16u>), dim3(grid), dim3(kWgThreads), 0, s, p);
        else hipLaunchKernelGGL((sg_wg_kernel<false, 16u>), dim3(grid), dim3(kWgThreads), 0, s, p);
    }
    return (int)hipGetLastError();
}

}  // namespace wg
}  // namespace sg
