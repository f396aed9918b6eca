// sg_esp.hip -- IPsec ESP packets of a batch in one launch (ChaCha20-Poly1305, RFC 7634
// over RFC 4303; sg_seal_batch_esp / sg_open_batch_esp, suruga_gpu.h): per packet the nonce
// from salt and IV, the keying (keystream block 0), the payload XOR, the RFC 8439 MAC over
// the 8- or 12-byte additional data and the ciphertext, on seal the 16-byte header, the
// padding 1, 2, 3 .. and the trailer, on open the SPI check, the sequence number off the
// wire with its inferred high half (RFC 4303 appendix A2.1), the ICV compare, the scrub of
// a failed packet and the trailer's parse.
//
// The geometry is sg_quic.hip's: G lanes per packet (8 where the call's max_len is at most
// 2 KiB, else 16), 256 / G packets per workgroup, an exact grid; no LDS, no atomics, no
// workspace.  A lane owns whole 64-byte chunks of the AEAD's P bytes, moved with unaligned
// 16-byte loads and stores, and runs Poly1305 over the four ciphertext blocks from the
// registers they are in; the tail of P % 64 bytes and the length block go byte by byte in
// slot 0.  sg_quic.h (Geom) says which lane owns which chunk and how the lanes' sums add
// up; the one block of additional data is the value of the slot in front of chunk 0.
//
// Chunks are laid over P = len + pad + 2, so on seal up to 257 bytes at the end are not
// input but made here: the cut can fall anywhere in a chunk and whole chunks can be made.
// A chunk that lies inside the payload takes the four 16-byte loads; any other is put
// together byte by byte, from the input below len and from the trailer's rule at and
// beyond it, so no input byte at or beyond len is read.  The tail does the same.
//
// In place (seal out + 16 == in, open out == in + 16) the payload stays at its address: a
// lane stores a chunk over the bytes it has itself just loaded, no lane loads another's
// chunk, and what every lane reads for itself -- open's SPI, sequence number and IV, in
// front of the stored range -- or reads late -- the received ICV, behind it -- is never
// stored to.  The header, the padding, the trailer and the ICV of a seal lie outside its
// len input bytes.  Open's trailer parse reads the padding back from `out` behind the
// group's fence, as the scrub of a failed packet writes behind it: every lane of the group
// has stored its plaintext by then, and in place those are the addresses it loaded from.
#include "sg_device.h"
#include "sg_esp.h"

namespace sg {
namespace {

using namespace dev;

constexpr uint32_t kEspThreads = 256;

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

// What a seal encrypts: the payload's `len` input bytes, then 1, 2 .. pad, then pad, then
// the next header (RFC 4303 section 2.4).  Nothing at or beyond in[len] is read.
struct Plain {
    const uint8_t* in;
    uint32_t len, pad, nh;
    __device__ __forceinline__ uint32_t byte(uint32_t i) const {
        if (i < len) return in[i];
        const uint32_t j = i - len;
        return j < pad ? j + 1u : (j == pad ? pad : nh);
    }
    // plaintext bytes at .. at + 4 as a little-endian word
    __device__ __forceinline__ uint32_t word(uint32_t at) const {
        uint32_t x = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) x |= byte(at + b) << (8u * b);
        return x;
    }
};

// word w of the 16-byte block j of a keystream block, j not known when compiling: the
// rolled loops over a packet's last bytes pick it with selects, so ks stays in registers
__device__ __forceinline__ uint32_t ks_word(const uint32_t (&ks)[16], uint32_t j, uint32_t w) {
    return j == 0u ? ks[w] : j == 1u ? ks[4u + w] : j == 2u ? ks[8u + w] : ks[12u + w];
}

template <bool OPEN, uint32_t G>
__global__ __launch_bounds__(kEspThreads) void sg_esp_kernel(const esp::Params p) {
    static_assert(G == 8u || G == 16u, "a group is a power of two and lies inside one wave");
    const uint32_t t = threadIdx.x % G;
    const uint64_t pkt64 = (uint64_t)blockIdx.x * (kEspThreads / G) + threadIdx.x / G;
    if (pkt64 >= p.count) return;  // whole groups leave together, here and below
    const uint32_t pkt = (uint32_t)pkt64;
    const uint32_t len = p.len ? p.len[pkt] : p.uniform_len;
    uint8_t* const stp = p.status + pkt;
    if (len > p.max_len) {
        if (t == 0u) *stp = SG_STATUS_SKIPPED;
        return;
    }
    if (OPEN && len < esp::kMinPacket) {
        if (t == 0u) *stp = SG_E_SHORT;
        return;
    }
    const uint8_t* const in = p.in + (p.in_off ? p.in_off[pkt] : p.in_stride * pkt);
    uint8_t* const out = p.out + (p.out_off ? p.out_off[pkt] : p.out_stride * pkt);
    const uint32_t si = p.sa_index ? p.sa_index[pkt] : 0u;
    const uint32_t row = si < p.num_sas ? si : p.num_sas - 1u;
    const uint32_t spi_be = bswap32(p.spi[row]);  // as the wire's first word reads little-endian

    // the sequence number and the IV's two words as they lie on the wire, every lane for itself
    uint64_t seq;
    uint32_t n14, n15;
    if constexpr (OPEN) {
        if (ldu32(in) != spi_be) {
            if (t == 0u) *stp = SG_STATUS_BAD_HEADER;
            return;
        }
        const uint32_t lo = bswap32(ldu32(in + 4));
        const uint32_t hi = p.esn ? esp::seq_hi(p.replay_top[row], p.window, lo) : 0u;
        seq = ((uint64_t)hi << 32) | lo;
        n14 = ldu32(in + 8);
        n15 = ldu32(in + 12);
    } else {
        seq = p.esn ? p.seq[pkt] : (uint64_t)(uint32_t)p.seq[pkt];
        const uint64_t iv = p.iv ? p.iv[pkt] : seq;
        n14 = bswap32((uint32_t)(iv >> 32));
        n15 = bswap32((uint32_t)iv);
    }
    const uint32_t lo_be = bswap32((uint32_t)seq), hi_be = bswap32((uint32_t)(seq >> 32));

    // n bytes through the AEAD, of which a seal takes the first len from the input
    Plain pl;
    pl.in = in;
    pl.len = len;
    pl.pad = OPEN ? 0u : esp::pad_len(len, p.align);
    pl.nh = OPEN ? 0u : (p.next_header ? (uint32_t)p.next_header[pkt] : p.uniform_next_header);
    const uint32_t n = OPEN ? len - esp::kOverhead : len + pl.pad + esp::kTrailer;
    const uint8_t* const src = OPEN ? in + SG_ESP_HEADER_LEN : in;
    uint8_t* const dst = OPEN ? out : out + SG_ESP_HEADER_LEN;

    uint32_t k[8], ks[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = ldu32(p.keys + 32ull * row + 4 * i);
    const uint32_t n13 = p.salts[row];  // nonce salt(4) || iv(8)

    chacha_block(ks, k, 0u, n13, n14, n15);
    const PolyKey pk = poly_key(ks);
    const F26 r = words_to_f26(pk.r0, pk.r1, pk.r2, pk.r3, 0u);

    const quic::Geom g = quic::geom(n, G);
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
                // seal: a chunk that reaches beyond the payload is put together byte by byte
                if (OPEN || 64u * c + 64u <= len) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const u32x4 a = ldu16(s + 16 * j);
                        const u32x4 x = {a[0] ^ ks[4 * j], a[1] ^ ks[4 * j + 1], a[2] ^ ks[4 * j + 2], a[3] ^ ks[4 * j + 3]};
                        stu16(d + 16 * j, x);
                        const u32x4 m = OPEN ? a : x;  // the MAC runs over the ciphertext
                        h = mac_block(h, m[0], m[1], m[2], m[3], r);
                    }
                } else {
#pragma unroll 1
                    for (uint32_t j = 0; j < 4u; ++j) {  // rolled: at most five chunks of a packet come here
                        const uint32_t at = 64u * c + 16u * j;
                        const u32x4 x = {pl.word(at) ^ ks_word(ks, j, 0), pl.word(at + 4u) ^ ks_word(ks, j, 1),
                                         pl.word(at + 8u) ^ ks_word(ks, j, 2), pl.word(at + 12u) ^ ks_word(ks, j, 3)};
                        stu16(d + 16u * j, x);
                        h = mac_block(h, x[0], x[1], x[2], x[3], r);
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
                                a |= (OPEN ? (uint32_t)s[i] : pl.byte(base + i)) << (8u * b);
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
                ts = mac_block(ts, p.esn ? 12u : 8u, 0u, n, 0u, r);  // le64(|ad|) || le64(|ct|)
            }
        }
        if (v + 1u == g.zc) {  // the slot in front of chunk 0: the additional data's one block, h is 0 so far
            // be32(spi) || be32(seq_lo), or be32(spi) || be32(seq_hi) || be32(seq_lo), zeros behind
            h = mac_block(h, spi_be, p.esn ? hi_be : lo_be, p.esn ? lo_be : 0u, 0u, r);
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
        const bool parse = !bad && p.payload_len;  // on a failed ICV nothing is parsed
        if (scrub || parse) group_sync();          // behind the other lanes' plaintext
        if (scrub)
            for (uint32_t i = t; i < n; i += G) out[i] = 0u;
        // the trailer: pad + 2 <= n and the pad bytes 1 .. pad, each lane its share of them
        uint32_t pad = 0u, nh = 0u, ok = 1u;
        if (parse) {
            pad = out[n - 2u];
            nh = out[n - 1u];
            ok = pad + esp::kTrailer <= n ? 1u : 0u;
            if (ok) {
                const uint8_t* const pp = out + (n - esp::kTrailer - pad);
                for (uint32_t i = t; i < pad; i += G) ok &= pp[i] == i + 1u ? 1u : 0u;
            }
        }
#pragma unroll
        for (uint32_t s = 1; s < G; s <<= 1) ok &= __shfl_xor(ok, s, G);
        if (t == 0u) {
            uint32_t st = bad ? SG_E_BAD_MAC : SG_OK;
            if (parse && !ok) st = SG_STATUS_BAD_INNER;
            p.seq_out[pkt] = scrub ? 0ull : seq;
            if (p.payload_len) {
                const bool valid = parse && ok;
                p.payload_len[pkt] = valid ? n - esp::kTrailer - pad : 0u;
                p.next_header_out[pkt] = valid ? (uint8_t)nh : (uint8_t)0u;
            }
            *stp = (uint8_t)st;
        }
    } else {
        if (t == G - 1u) stu16(dst + n, u32x4{tw[0], tw[1], tw[2], tw[3]});
        if (t == 0u) {
            stu16(out, u32x4{spi_be, lo_be, n14, n15});  // be32(spi) || be32(seq_lo) || be64(iv)
            *stp = SG_OK;
        }
    }
}

}  // namespace

namespace esp {

int launch(const Params& p, bool open, void* stream) {
    const uint32_t G = quic::lanes_for(p.max_len);
    const uint32_t per = kEspThreads / G;
    const uint32_t grid = (uint32_t)(((uint64_t)p.count + per - 1u) / per);
    hipStream_t s = (hipStream_t)stream;
    if (G == 8u) {
        if (open) hipLaunchKernelGGL((sg_esp_kernel<true, 8u>), dim3(grid), dim3(kEspThreads), 0, s, p);
        else hipLaunchKernelGGL((sg_esp_kernel<false, 8u>), dim3(grid), dim3(kEspThreads), 0, s, p);
    } else {
        if (open) hipLaunchKernelGGL((sg_esp_kernel<true, 16u>), dim3(grid), dim3(kEspThreads), 0, s, p);
        else hipLaunchKernelGGL((sg_esp_kernel<false, 16u>), dim3(grid), dim3(kEspThreads), 0, s, p);
    }
    return (int)hipGetLastError();
}

}  // namespace esp
}  // namespace sg
