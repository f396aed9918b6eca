// sg_dtls13.hip -- DTLS 1.3 records of a batch in one launch (TLS_CHACHA20_POLY1305_SHA256,
// RFC 9147 section 4; sg_seal_batch_dtls13 / sg_open_batch_dtls13, suruga_gpu.h): per record
// the unified header, the nonce from IV and sequence number, the keying (keystream block
// 0), the XOR of the inner plaintext, the RFC 8439 MAC over header and ciphertext and the
// record number encryption of section 4.2.3; on seal the type byte and the zero padding,
// on open the header's checks, the key row from the wire's epoch bits, the sequence number
// rebuilt from its one or two bytes, the tag compare, the scrub of a failed record and the
// strip that finds the type byte.
//
// The geometry is sg_quic.hip's: G lanes per record (8 where the call's max_len is at most
// 2 KiB, else 16), 256 / G records per workgroup, an exact grid; no LDS, no atomics, no
// workspace.  A lane owns whole 64-byte chunks of the inner plaintext, moved with unaligned
// 16-byte loads and stores, and runs Poly1305 over the four ciphertext blocks from the
// registers they are in; the tail and the length block go byte by byte in slot 0.  These
// steps, the fold of the lanes' sums and the finish are sg_lane_aead.h's.  The header, 2 to
// 255 bytes and most often one MAC block, is the additional data: the value of the slot in
// front of chunk 0, byte by byte.
//
// On seal the inner plaintext is len content bytes from the input, the type byte, and
// zeros: a chunk that lies inside the content takes the four 16-byte loads, any other is
// put together by that rule, so no input byte at or beyond len is read.
//
// What every lane of a group needs alike -- open's mask and sequence number, keystream
// block 0 -- each lane computes for itself.  Seal's sample is ciphertext (under an inner
// plaintext below 16 bytes, tag) that other lanes have just stored: the group's stores are
// made visible within the workgroup and the sample is read back from `out`.  Open's strip
// reads the plaintext back from `out`, and its scrub writes there, behind the same fence.
#include "sg_dtls13.h"
#include "sg_lane_aead.h"

namespace sg {
namespace {

using namespace dev;
using namespace lane;

constexpr uint32_t kDtlsThreads = 256;

// The unified header as the AEAD sees it: first byte, connection ID, the sequence number's
// low sn_len bytes big-endian, and where L is set be16 of the encrypted record's length.
struct Header {
    const uint8_t* cid;  // seal: the connection's row of cids; open: the wire's bytes behind the first
    uint64_t seq;
    uint32_t b0, cid_len, n;  // n: the inner plaintext's length; the encrypted record has the tag behind it
    __device__ __forceinline__ uint32_t sn_off() const { return 1u + cid_len; }
    __device__ __forceinline__ uint32_t sn_len() const { return (b0 & dtls13::kS) ? 2u : 1u; }
    __device__ __forceinline__ uint32_t hdr_len() const { return dtls13::header_len_bits(b0, cid_len); }
    __device__ __forceinline__ uint32_t byte(uint32_t i) const {
        if (i == 0u) return b0;
        if (i <= cid_len) return cid[i - 1u];
        const uint32_t j = i - 1u - cid_len;
        const uint32_t sn = sn_len();
        if (j < sn) return (uint32_t)(seq >> (8u * (sn - 1u - j))) & 0xffu;
        return ((n + SG_MAC_LEN) >> (8u * (1u + sn - j))) & 0xffu;  // j - sn is 0 or 1
    }
};

// What a seal encrypts: the content's `len` input bytes, the type byte, zeros (RFC 9147
// section 4, DTLSInnerPlaintext).  Nothing at or beyond in[len] is read.
struct Inner {
    const uint8_t* in;
    uint32_t len, type;
    __device__ __forceinline__ uint32_t byte(uint32_t i) const { return i < len ? in[i] : (i == len ? type : 0u); }
    __device__ __forceinline__ bool loadable(uint32_t c) const { return 64u * c + 64u <= len; }
    __device__ __forceinline__ const uint8_t* ptr(uint32_t c) const { return in + 64ull * c; }
};

// the first two mask bytes of section 4.2.3 under the record number key `sk`: mask[0] in
// bits 0..8, mask[1] in bits 8..16
__device__ __forceinline__ uint32_t sn_mask(const uint8_t* sk, const uint8_t* sample) {
    Keying m;
    m.load_key(sk);
    m.n13 = ldu32(sample + 4);
    m.n14 = ldu32(sample + 8);
    m.n15 = ldu32(sample + 12);
    uint32_t ks[16];
    m.block(ks, ldu32(sample));
    return ks[0] & 0xffffu;
}
// sequence number byte j on the wire and in the clear differ by this
__device__ __forceinline__ uint32_t sn_mask_byte(uint32_t mask, uint32_t j) { return (mask >> (8u * j)) & 0xffu; }

template <bool OPEN, uint32_t G>
__global__ __launch_bounds__(kDtlsThreads) void sg_dtls13_kernel(const dtls13::Params p) {
    static_assert(G == 8u || G == 16u, "a group is a power of two and lies inside one wave");
    const uint32_t t = threadIdx.x % G;
    const uint64_t rec64 = (uint64_t)blockIdx.x * (kDtlsThreads / G) + threadIdx.x / G;
    if (rec64 >= p.count) return;  // whole groups leave together, here and below
    const uint32_t rec = (uint32_t)rec64;
    const uint32_t len = p.len ? p.len[rec] : p.uniform_len;
    uint8_t* const stp = p.status + rec;
    if (len > p.max_len) {
        if (t == 0u) *stp = SG_STATUS_SKIPPED;
        return;
    }
    if (OPEN && len == 0u) {
        if (t == 0u) *stp = SG_E_SHORT;
        return;
    }
    const uint8_t* const in = p.in + (p.in_off ? p.in_off[rec] : p.in_stride * rec);
    uint8_t* const out = p.out + (p.out_off ? p.out_off[rec] : p.out_stride * rec);
    const uint32_t ki = p.key_index ? p.key_index[rec] : 0u;
    const uint32_t conn = ki < p.num_conns ? ki : p.num_conns - 1u;

    // the first byte, the header's shape and the key row
    Header hd;
    hd.cid_len = p.cid_len;
    if constexpr (OPEN) {
        hd.b0 = in[0];
        if ((hd.b0 & dtls13::kFixedMask) != dtls13::kFixed || ((hd.b0 & dtls13::kC) != 0u) != (p.cid_len != 0u)) {
            if (t == 0u) *stp = SG_STATUS_BAD_HEADER;
            return;
        }
        hd.cid = in + 1;
    } else {
        const uint32_t ep = p.epoch ? (uint32_t)p.epoch[rec] : p.uniform_epoch;
        hd.b0 = dtls13::kFixed | (p.cid_len ? dtls13::kC : 0u) | p.seal_bits | (ep & dtls13::kEpochMask);
        hd.cid = p.cids + (uint64_t)p.cid_len * conn;
    }
    const uint32_t hdr_len = hd.hdr_len();
    const uint32_t ee = hd.b0 & dtls13::kEpochMask;
    const uint32_t row = p.epoch_rows ? 4u * conn + ee : conn;

    // n bytes through the AEAD: the inner plaintext
    Inner pl;
    pl.in = in;
    pl.len = len;
    pl.type = OPEN ? 0u : (p.type ? (uint32_t)p.type[rec] : p.uniform_type);
    uint32_t n;
    if constexpr (OPEN) {
        if (len < hdr_len + SG_MAC_LEN) {
            if (t == 0u) *stp = SG_E_SHORT;
            return;
        }
        n = len - hdr_len - SG_MAC_LEN;
        if (hd.b0 & dtls13::kL) {
            const uint32_t lp = hdr_len - 2u;
            if ((((uint32_t)in[lp] << 8) | in[lp + 1u]) != n + SG_MAC_LEN) {
                if (t == 0u) *stp = SG_STATUS_BAD_HEADER;
                return;
            }
        }
        // the sequence number: its bytes unmasked, the rest from the row's expected number
        const uint32_t mask = sn_mask(p.sn_keys + 32ull * row, in + hdr_len);
        uint32_t trunc = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j)
            if (j < hd.sn_len()) trunc = (trunc << 8) | (in[hd.sn_off() + j] ^ sn_mask_byte(mask, j));
        hd.seq = quic::decode_pn(p.expected[row], trunc, hd.sn_len());
    } else {
        n = dtls13::inner_len(len, p.pad_to);
        hd.seq = p.seq[rec];
    }
    hd.n = n;
    const uint8_t* const src = OPEN ? in + hdr_len : in;
    uint8_t* const dst = OPEN ? out : out + hdr_len;

    Keying key;
    key.load_key(p.keys + 32ull * row);
    const uint32_t* const iv = reinterpret_cast<const uint32_t*>(p.ivs + 12ull * row);
    key.n13 = iv[0];
    key.n14 = iv[1] ^ bswap32((uint32_t)(hd.seq >> 32));
    key.n15 = iv[2] ^ bswap32((uint32_t)hd.seq);

    uint32_t ks[16];
    key.block(ks, 0u);
    const PolyKey pk = poly_key(ks);
    const F26 r = words_to_f26(pk.r0, pk.r1, pk.r2, pk.r3, 0u);

    const quic::Geom g = quic::geom(n, G);
    F26 h = f26_zero(), ts = f26_zero();
    // The slot in front of chunk 0 is worth the header's blocks.  The slots before it in its
    // lane add nothing to h (they are empty, or slot 0, whose sum is ts), so the lane that
    // owns it takes the header first: no keystream block is live meanwhile.
    if (t == (g.zc - 1u) / g.q) {
        const uint32_t na = (hdr_len + 15u) / 16u;
        for (uint32_t a = 0; a < na; ++a) h = ad_block(h, hd, hdr_len, a, r);
    }
    for (uint32_t q = 0; q < g.q; ++q) {
        const uint32_t v = t * g.q + q;
        if constexpr (OPEN) slot<true>(g, v, key, Wire{src}, dst, hdr_len, n, r, ks, h, ts);
        else slot<false>(g, v, key, pl, dst, hdr_len, n, r, ks, h, ts);
    }
    h = fold<G>(h, r, g.q, t);
    uint32_t tw[4];
    finish<G>(h, ts, r, g.kt, pk.s, tw);

    if constexpr (OPEN) {
        const uint32_t bad = tag_bad<G>(src + n, tw, t);
        const bool scrub = bad && !p.keep_failed;
        group_sync();  // behind the other lanes' plaintext
        if (scrub)
            for (uint32_t i = t; i < n; i += G) out[i] = 0u;
        // the strip: the last non-zero byte of the inner plaintext, G * 8 bytes a round from the end
        uint32_t found = 0u;  // its index + 1
        if (!bad) {
            for (uint32_t end = n; end != 0u && found == 0u; end = end > 8u * G ? end - 8u * G : 0u) {
#pragma unroll
                for (uint32_t e = 0; e < 8u; ++e) {
                    const uint32_t back = e * G + t;  // this lane's byte, counted from the end
                    if (back < end && out[end - 1u - back] != 0u && found == 0u) found = end - back;
                }
#pragma unroll
                for (uint32_t s = 1; s < G; s <<= 1) {
                    const uint32_t o = __shfl_xor(found, s, G);
                    found = o > found ? o : found;
                }
            }
        }
        if (t == 0u) {
            p.seq_out[rec] = scrub ? 0ull : hd.seq;
            p.epoch_out[rec] = (uint8_t)ee;
            p.content_len[rec] = found ? found - 1u : 0u;
            p.type_out[rec] = found ? out[found - 1u] : (uint8_t)0u;
            *stp = (uint8_t)(bad ? SG_E_BAD_MAC : (found ? SG_OK : SG_STATUS_NO_TYPE));
        }
    } else {
        if (t == G - 1u) stu16(dst + n, u32x4{tw[0], tw[1], tw[2], tw[3]});
        group_sync();  // the sample is what the group has just stored
        const uint32_t mask = sn_mask(p.sn_keys + 32ull * row, dst);
        for (uint32_t i = t; i < hdr_len; i += G) {
            const uint32_t j = i - hd.sn_off();  // wraps below the sequence number's bytes
            out[i] = (uint8_t)(hd.byte(i) ^ (j < hd.sn_len() ? sn_mask_byte(mask, j) : 0u));
        }
        if (t == 0u) *stp = SG_OK;
    }
}

}  // namespace

namespace dtls13 {

int launch(const Params& p, bool open, void* stream) {
    const uint32_t G = quic::lanes_for(p.max_len);
    const uint32_t per = kDtlsThreads / G;
    const uint32_t grid = (uint32_t)(((uint64_t)p.count + per - 1u) / per);
    hipStream_t s = (hipStream_t)stream;
    if (G == 8u) {
        if (open) hipLaunchKernelGGL((sg_dtls13_kernel<true, 8u>), dim3(grid), dim3(kDtlsThreads), 0, s, p);
        else hipLaunchKernelGGL((sg_dtls13_kernel<false, 8u>), dim3(grid), dim3(kDtlsThreads), 0, s, p);
    } else {
        if (open) hipLaunchKernelGGL((sg_dtls13_kernel<true, 16u>), dim3(grid), dim3(kDtlsThreads), 0, s, p);
        else hipLaunchKernelGGL((sg_dtls13_kernel<false, 16u>), dim3(grid), dim3(kDtlsThreads), 0, s, p);
    }
    return (int)hipGetLastError();
}

}  // namespace dtls13
}  // namespace sg
