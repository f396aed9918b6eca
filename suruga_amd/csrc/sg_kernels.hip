// sg_kernels.hip -- gfx950 (CDNA4) size-class kernels for suruga's
// ChaCha20-Poly1305 record AEAD (draft-agl-tls-chacha20poly1305-04 as in
// klutzy/suruga), used for every batch the wave-per-record kernel of
// sg_wpr.hip does not take (mixed sizes, records other than 16 KiB,
// unaligned or offset-table layouts).
//
// Work decomposition (records of one size class per 256-thread workgroup):
//
//   sg_keying_kernel   one lane per record: ChaCha20 block 0 -> Poly1305 key
//                      (r clamped, s; chacha20_poly1305.rs:50,75,32-39,
//                      poly1305.rs:197-203) and the 16 powers of r^k
//                      that combine the MAC lanes.
//   sg_aead_kernel<OPEN, L>   L lanes per record:
//     phase 1, all lanes: lane t owns 64-byte data blocks t, t+L, ...;
//       computes keystream block b+1 in registers (chacha20.rs:53-135),
//       XORs the record bytes (chacha20.rs:143-153), writes the result to HBM
//       and the ciphertext into LDS.
//     phase 2, PL = min(L, 64) lanes: Poly1305 over ad || le64(|ad|) || ct ||
//       le64(|ct|) (chacha20_poly1305.rs:19-42), read from LDS.  The B MAC
//       blocks are preceded by z zero "virtual" blocks (leading zeros do not
//       change a Horner polynomial) so that B + z = PL k; lane t runs the
//       reference's Horner step h = (h + c) * r (poly1305.rs:213-228) over its
//       k contiguous blocks in radix 2^32 with the clamped r; each lane then
//       scales its sum by r^(k (PL-1-t)) (radix 2^26, powers from the keying
//       record) and a DPP reduction adds the PL terms.  The last lane reduces
//       mod 2^130-5, adds s (poly1305.rs:230-312) and seals
//       (chacha20_poly1305.rs:55) or compares in constant time (:84-93) after
//       decrypting unconditionally (:80-82).
//   sg_classify_kernel   buckets a mixed-size batch into per-class lists.
//
// All Poly1305 arithmetic is exact mod p = 2^130 - 5, so the tag equals the
// reference's sequential Horner result bit for bit.
//
// The keying and AEAD kernels take the construction as a template parameter
// (Construction, sg_layout.h).  Construction::kRfc8439 (sg_*_batch_rfc8439)
// differs in three places: the 12-byte nonce fills state words 13-15
// (record_key, sg_device.h: explicit, or the RFC 7905 write IV XOR the sequence
// number), the MAC stream is framed in LDS as ad || 0.. || ct || 0.. ||
// le64(|ad|) || le64(|ct|), and mac_geom's stream length counts the padding
// (every block is full).  The draft instantiations compile to what they were
// before the parameter.
//
// T13 (KParams.tls13, sg_*_batch_tls13; with Construction::kRfc8439 only) is the
// TLS 1.3 record form of RFC 8446 section 5.2: the AD is the 5-byte record header
// 17 03 03 be16(fragment length) (tls13_ad_byte, sg_device.h), and on seal the
// AEAD input is the inner plaintext: the record's content, the inner type byte
// behind it (the call's, or the record's own: tls13_inner_type) and zeros up to
// tls13_inner_len(len, pad_to) bytes (sg_layout.h).  The keying and classify
// kernels count that length; the block that holds the type byte takes the byte
// path, a block of padding alone reads nothing, and no byte of the input at or
// beyond len is read.  The instantiations without T13 compile to what they were
// before the parameter.
//
// A record's body is aead_record: record_lens, the LDS layout, phase 1 (class_keystream per
// block), the MAC stream framing (ad_byte), load_tag, the lane's Horner run, its weight, the DPP
// sum, finish_tag, store_tag or the compare.  The comment in front of it says which
// of these are functions and which stay in its body.
//
// The launchers at the end are what the rest of the library sees of this file
// (sg_internal.h); the dispatcher of a batch is sg_dispatch.cpp.
#include "sg_internal.h"

#include "sg_device.h"

#include <stdint.h>

namespace sg {
namespace {

using namespace dev;

// (chacha_pre / chacha_block_pre, the uniform-record ChaCha20 variant with the
// counter-free part of round 1 on the scalar unit, live in sg_device.h: the
// message kernels of sg_msg.hip share them.)

// MAC geometry: stream length L, blocks B, lane chunk k (odd: spreads the
// lanes' LDS reads over banks), leading virtual zero blocks z = PL*k - B, for
// PL MAC lanes per record.
struct MacGeom {
    uint32_t L, B, k, z;
};
// (the stream length is stream_bytes<C>, sg_layout.h; RFC 8439: every block is
// full.  Its RFC form stays spelt with masks here: from the header's divisions
// the compiler folds the block count below differently and the RFC kernels'
// instructions change.)
template <Construction C>
__device__ __forceinline__ MacGeom mac_geom(uint32_t adlen, uint32_t n, uint32_t PL) {
    MacGeom g;
    static_assert(stream_bytes<Construction::kRfc8439>(13u, 100u) == ((13u + 15u) & ~15u) + ((100u + 15u) & ~15u) + 16u,
                  "the same length");
    if constexpr (C == Construction::kRfc8439) g.L = ((adlen + 15u) & ~15u) + ((n + 15u) & ~15u) + 16u;
    else g.L = stream_bytes<C>(adlen, n);
    g.B = (g.L + 15u) >> 4;
    g.k = (g.B + PL - 1u) / PL;
    g.k |= 1u;
    g.z = PL * g.k - g.B;
    return g;
}

// MAC lanes per record, a function of the payload length only so that the
// keying kernel and every AEAD size class agree on k (see size_class).
__device__ __forceinline__ uint32_t mac_lanes(uint32_t n) { return class_mac_lanes(size_class(n)); }

// ---------------------------------------------------------------------------
// Keying pre-pass: one lane per record.
// ---------------------------------------------------------------------------
// The 64 records of a wave are staged in LDS (row stride kKeyRecWords + 1
// words: no bank conflicts) and leave as one contiguous run of 16-byte stores
// (skipping the powers a record's class never reads); one lane writing its own
// record would touch a cache line per store.  (kKeyingThreads: sg_internal.h)

// The wave-per-record bucket of record rec of a mixed batch (0: a size class);
// n is the plaintext length.  The classify and keying kernels agree on it.
__device__ __forceinline__ uint32_t rec_wpr_bucket(const KParams& p, uint32_t rec, uint32_t n) {
    if (!p.wpr_mix) return 0u;
    const uint64_t ia = (uint64_t)(uintptr_t)p.in + rec_in_off(p, rec);
    const uint64_t oa = (uint64_t)(uintptr_t)p.out + rec_out_off(p, rec);
    return wpr_bucket_of(n, ia, oa);
}
// ... and for the packed small-record kernel (sg_pack.hip)
__device__ __forceinline__ bool rec_pack(const KParams& p, uint32_t rec, uint32_t n) {
    if (!p.pack_mix) return false;
    const uint64_t ia = (uint64_t)(uintptr_t)p.in + rec_in_off(p, rec);
    const uint64_t oa = (uint64_t)(uintptr_t)p.out + rec_out_off(p, rec);
    return pack_ok(n, ia, oa);
}


// Keying pre-pass of the size-class kernels: ChaCha20 block 0 -> Poly1305 key
// (chacha20_poly1305.rs:50,75,32-39; r clamped as poly1305.rs:197-203), and
// with R = r^k (k = MAC blocks per lane, mac_geom) the tables R^0..R^7 and
// R^0, R^8, .., R^56 that scale the MAC lanes' partial sums.
// KeyJobs (sg_internal.h): njobs == 0 keys every record of the batch by
// index; otherwise the records of up to kNumClasses lists (mixed batches key
// only their size-class records here), job i on blocks [blk0[i], blk0[i+1]).
// T13 (KParams.tls13, RFC 8446 section 5.2): the MAC runs over the inner
// plaintext, one byte longer than the content on seal, behind a 5-byte AD.
template <bool OPEN, Construction C, bool T13>
__global__ __launch_bounds__(64) void sg_keying_kernel(const KParams p, const KeyJobs jobs) {
    static_assert(!T13 || C == Construction::kRfc8439, "TLS 1.3 records are RFC 8439");
    constexpr uint32_t kKeyLdsStride = kKeyRecWords + 1;
    __shared__ uint32_t stage[kKeyingThreads * kKeyLdsStride];
    __shared__ uint32_t recs[kKeyingThreads];
    const uint32_t lane = threadIdx.x;
    const uint32_t* list = nullptr;
    uint32_t cnt = p.count, b0 = 0;
#pragma unroll
    for (uint32_t i = 0; i < kNumClasses; ++i)  // (constant indices: the kernarg table stays in SGPRs)
        if (i < jobs.njobs && blockIdx.x >= jobs.blk0[i]) {
            list = jobs.list[i];
            cnt = jobs.count[i];
            b0 = jobs.blk0[i];
        }
    const uint32_t slot0 = (blockIdx.x - b0) * kKeyingThreads;
    const uint32_t slot = slot0 + lane;
    const bool act = slot < cnt;
    const uint32_t rec = act ? (list ? list[slot] : slot) : 0u;
    recs[lane] = rec;
    uint32_t* out = stage + lane * kKeyLdsStride;
    const uint32_t len = act ? record_len(p, rec) : 0u;
    const uint32_t n = aead_len<OPEN, T13>(p, len);
    out[kKeyRecWords] = 0u;  // nothing to write unless keyed below
    if (act) {
        const RecKey rk = record_key<C>(p, rec);
        uint32_t ks[16];
        chacha_block(ks, rk.k, 0u, rk.n13, rk.n14, rk.n15);  // block 0 -> poly key (chacha20_poly1305.rs:50)
        const PolyKey pk = poly_key(ks);
        out[kR32Off + 0] = pk.r0;
        out[kR32Off + 1] = pk.r1;
        out[kR32Off + 2] = pk.r2;
        out[kR32Off + 3] = pk.r3;
        out[kSOff + 0] = pk.s[0];
        out[kSOff + 1] = pk.s[1];
        out[kSOff + 2] = pk.s[2];
        out[kSOff + 3] = pk.s[3];
        const uint32_t adlen = ad_len<T13>(p);
        const MacGeom g = mac_geom<C>(adlen, n, mac_lanes(n));
        const F26 r = words_to_f26(pk.r0, pk.r1, pk.r2, pk.r3, 0u);
        // R = r^k by square-and-multiply; then R^0..R^7 and R^0, R^8, .., R^56.
        // mul_add outputs are valid multipliers as they stand (limb 1 may exceed
        // 2^26 by < 2^8), so no extra carry passes are needed here.
        // (fpow starts from 1 and takes e = 0: other instructions, so not used here)
        F26 R = r;
        for (int bit = 30 - __builtin_clz(g.k); bit >= 0; --bit) {
            R = fmul(R, R);
            if ((g.k >> bit) & 1u) R = fmul(R, r);
        }
        // only the powers the record's PL MAC lanes read (a prefix of the layout)
        const uint32_t PL = mac_lanes(n);
        store_f26(out + key_hi_off(0u), f26_one());
        F26 x = f26_one();
        const uint32_t nlo = PL < 8u ? PL : 8u;
        for (uint32_t j = 0; j < nlo; ++j) {  // lo[j] = R^j
            store_f26(out + key_lo_off(j), x);
            x = fmul(x, R);
        }
        if (PL > 8u) {
            const F26 R8 = x;
            for (uint32_t i = 1; i < PL / 8u; ++i) {  // hi[i] = R^(8 i)
                store_f26(out + key_hi_off(i), x);
                if (i + 1u < PL / 8u) x = fmul(x, R8);
            }
        }
        out[kKeyRecWords] = key_used_words(PL);  // the stage row's pad word
    }
    __syncthreads();
    // coalesced flush: 16-byte stores of consecutive words of a record
    // (records by index are contiguous in the workspace; listed ones are not)
    const uint32_t nrec = cnt - slot0 < kKeyingThreads ? cnt - slot0 : kKeyingThreads;
    const uint32_t nvec = nrec * (kKeyRecWords / 4u);
    for (uint32_t v = lane; v < nvec; v += kKeyingThreads) {
        const uint32_t w = 4u * v;
        const uint32_t rr = w / kKeyRecWords, c = w - rr * kKeyRecWords;
        const uint32_t* src = stage + rr * kKeyLdsStride + c;
        if (c < stage[rr * kKeyLdsStride + kKeyRecWords])  // unread powers are not written
            *reinterpret_cast<u32x4*>(p.ws + (uint64_t)recs[rr] * kKeyRecWords + c) = u32x4{src[0], src[1], src[2], src[3]};
    }
}

// ---------------------------------------------------------------------------
// Fused seal / open.  A 256-thread workgroup serves RPW = 256 / L records with
// L lanes each (size classes: L = 16 for n <= 1 KiB, 64 for n <= 4 KiB, 256
// otherwise); PL = min(L, 64) of them run the MAC.  Per record, in LDS:
//   [0, S) virtual-block space | S: ad | le64(adlen) | A: ct (n) | le64(n) | zeros
// ---------------------------------------------------------------------------
// T13 (TLS 1.3, RFC 8446 section 5.2): n is the inner plaintext length; seal
// reads len content bytes, appends the inner type byte and pads with zeros to n,
// so the block that holds the type takes the byte path; the AD is the 5-byte
// record header.
//
// The steps of aead_record that stand as functions in front of it: record_lens, class_keystream,
// load_tag / store_tag, finish_tag (and ad_byte, tag_mismatch of sg_device.h).  The
// LDS layout, the two phase-1 block forms, the MAC stream framing, the lane's Horner run, its
// weight and the DPP sum stay in the body under their phase comments: as functions each of them
// changed registers or the order of memory operations of some instantiations (end of
// section 4.3).

// The record's length len, the AEAD's input length n (open: without the tag; TLS 1.3 seal: the
// inner plaintext) and whether the group works on the record: a slot without one does not, and an
// open too short for a tag is flagged (chacha20_poly1305.rs:68-70 "message too short").
struct RecLens {
    uint32_t len, n;
    bool work;
};
template <bool OPEN, bool T13>
__device__ __forceinline__ RecLens record_lens(const KParams& p, const uint32_t rec, const bool active,
                                               const uint32_t t) {
    RecLens q = {active ? record_len(p, rec) : 0u, 0u, active};
    if (active) {
        q.n = aead_len<false, T13 && !OPEN>(p, q.len);
        if constexpr (OPEN) {
            if (q.len < 16u) {
                if (t == 0) p.status[rec] = 2u;
                q.work = false;
            }
            q.n = q.len - 16u;  // (unguarded: n is not used when len < 16)
        }
    }
    return q;
}

// Keystream block ctr of the record: a class whose groups are whole waves (L >= 64) starts from
// the counter-free part of round 1 (pre = chacha_pre of the record, sg_device.h)
template <uint32_t L>
__device__ __forceinline__ void class_keystream(uint32_t ks[16], const ChaChaPre& pre, const RecKey& rk,
                                                const uint32_t ctr) {
    if constexpr (L >= 64u) chacha_block_pre(ks, pre, rk.k, ctr, rk.n13, rk.n14, rk.n15);
    else chacha_block(ks, rk.k, ctr, rk.n13, rk.n14, rk.n15);
}

// The 16 tag bytes at any alignment as four little-endian words: aligned words, or bytes.
// (load_tag: rx is zero on entry)
__device__ __forceinline__ void load_tag(const uint8_t* ep, uint32_t rx[4]) {
    if ((((uintptr_t)ep) & 3u) == 0u) {
        const uint32_t* e32 = reinterpret_cast<const uint32_t*>(ep);
        rx[0] = e32[0]; rx[1] = e32[1]; rx[2] = e32[2]; rx[3] = e32[3];
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) rx[i >> 2] |= (uint32_t)ep[i] << (8 * (i & 3));
    }
}
__device__ __forceinline__ void store_tag(uint8_t* tp, const uint32_t tw[4]) {
    if ((((uintptr_t)tp) & 3u) == 0u) {
        uint32_t* t32 = reinterpret_cast<uint32_t*>(tp);
        t32[0] = tw[0]; t32[1] = tw[1]; t32[2] = tw[2]; t32[3] = tw[3];
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) tp[i] = (uint8_t)(tw[i >> 2] >> (8 * (i & 3)));
    }
}

// The finish: the tag words tw of the group's sum f (held by its last lane) and the keying
// record's s; true in the lane that holds them, PL - 1.
template <uint32_t PL>
__device__ __forceinline__ bool finish_tag(const F26& f, const uint32_t* kr, const uint32_t t, uint32_t tw[4]) {
    if constexpr (PL == 64u) {
        // one record per wave: lift the sum out of lane 63 into SGPRs so the
        // final reduction and s addition run on the scalar unit instead of
        // occupying the whole wave's VALU for one lane's arithmetic
        auto lane63 = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)x, 63); };
        const F26 fs = {lane63(f.v0), lane63(f.v1), lane63(f.v2), lane63(f.v3), lane63(f.v4)};
        uint32_t s[4] = {uniform(kr[kSOff + 0]), uniform(kr[kSOff + 1]), uniform(kr[kSOff + 2]),
                         uniform(kr[kSOff + 3])};
        tag_words(fs, s, tw);
        return t == PL - 1u;
    } else {
        if (t != PL - 1u) return false;
        uint32_t s[4] = {kr[kSOff + 0], kr[kSOff + 1], kr[kSOff + 2], kr[kSOff + 3]};
        tag_words(f, s, tw);
        return true;
    }
}

template <bool OPEN, uint32_t L, Construction C, bool T13>
__device__ __forceinline__ void aead_record(const KParams& p, const uint32_t rec, const bool active,
                                            uint8_t* lds, const uint32_t t) {
    constexpr uint32_t PL = L < 64u ? L : 64u;
    constexpr bool SEAL13 = T13 && !OPEN;
    constexpr uint32_t Z = 32u * PL;  // space for the virtual blocks in front: 16 * max z
    constexpr bool RFC = C == Construction::kRfc8439;
    const RecLens q = record_lens<OPEN, T13>(p, rec, active, t);
    const uint32_t len = q.len, n = q.n;
    const bool work = q.work;
    const uint8_t* in = nullptr;
    uint8_t* out = nullptr;
    const uint32_t adlen = ad_len<T13>(p);
    // RFC 8439: [Z, A) ad and its zero padding | A: ct (n) | zeros to 16 | le64(adlen) le64(n)
    // A = Z + 16 ceil(ct_offset<C>(adlen) / 16) and S = A - ct_offset<C>(adlen) (sg_layout.h), spelt by
    // hand: taken from the header, 76 of this file's 102 kernels came out with other instructions
    static_assert(ct_offset<Construction::kRfc8439>(13u) == ((13u + 15u) & ~15u) &&
                      ct_offset<Construction::kRfc8439>(32u) == 32u && ct_offset<Construction::kDraft>(13u) == 13u + 8u,
                  "the offsets below are the header's");
    const uint32_t A = Z + (RFC ? (adlen + 15u) & ~15u : (adlen + 8u + 15u) & ~15u);
    const uint32_t S = RFC ? Z : A - adlen - 8u;  // stream start, >= Z
    uint8_t* ct_lds = lds + A;
    if (work) {
        in = p.in + rec_in_off(p, rec);
        out = p.out + rec_out_off(p, rec);
        const RecKey rk = record_key<C>(p, rec);
        uint8_t type = 0u;  // T13 seal: the inner type byte behind the content
        if constexpr (SEAL13) type = tls13_inner_type(p, rec);

        // ---- phase 1: keystream XOR, 64 bytes per lane-block ----------------
        const bool vec_ok = (((uintptr_t)in | (uintptr_t)out) & 15u) == 0u;
        const uint32_t nblocks = (n + 63u) >> 6;
        ChaChaPre pre;
        if constexpr (L >= 64u) pre = chacha_pre(rk.k, rk.n13, rk.n14, rk.n15);
        for (uint32_t b = t; b < nblocks; b += L) {
            const uint32_t off = b << 6;
            // (T13 seal: a block of content alone; or one of padding alone, which reads nothing)
            const bool zeros = SEAL13 && off > len;
            if (vec_ok && (off + 64u <= (SEAL13 ? len : n) || (zeros && off + 64u <= n))) {
                u32x4 d0 = {}, d1 = {}, d2 = {}, d3 = {};
                if (!zeros) {
                    d0 = ld16(in + off);
                    d1 = ld16(in + off + 16);
                    d2 = ld16(in + off + 32);
                    d3 = ld16(in + off + 48);
                }
                uint32_t ks[16];
                class_keystream<L>(ks, pre, rk, b + 1u);  // data uses blocks 1.. (chacha20_poly1305.rs:52)
                const u32x4 r0 = d0 ^ u32x4{ks[0], ks[1], ks[2], ks[3]};
                const u32x4 r1 = d1 ^ u32x4{ks[4], ks[5], ks[6], ks[7]};
                const u32x4 r2 = d2 ^ u32x4{ks[8], ks[9], ks[10], ks[11]};
                const u32x4 r3 = d3 ^ u32x4{ks[12], ks[13], ks[14], ks[15]};
                st16(out + off, r0);
                st16(out + off + 16, r1);
                st16(out + off + 32, r2);
                st16(out + off + 48, r3);
                if constexpr (OPEN) {
                    st16(ct_lds + off, d0);
                    st16(ct_lds + off + 16, d1);
                    st16(ct_lds + off + 32, d2);
                    st16(ct_lds + off + 48, d3);
                } else {
                    st16(ct_lds + off, r0);
                    st16(ct_lds + off + 16, r1);
                    st16(ct_lds + off + 32, r2);
                    st16(ct_lds + off + 48, r3);
                }
            } else {
                // partial last block or misaligned record: byte granular
                uint32_t ks[16];
                class_keystream<L>(ks, pre, rk, b + 1u);
#pragma unroll
                for (uint32_t w = 0; w < 16; ++w) {
#pragma unroll
                    for (uint32_t k = 0; k < 4; ++k) {
                        const uint32_t idx = off + 4u * w + k;
                        if (idx < n) {
                            uint8_t x;
                            if constexpr (SEAL13) x = idx < len ? in[idx] : idx == len ? type : (uint8_t)0u;  // content || type || zeros
                            else x = in[idx];
                            const uint8_t y = x ^ (uint8_t)(ks[w] >> (8u * k));
                            out[idx] = y;
                            ct_lds[idx] = OPEN ? x : y;
                        }
                    }
                }
            }
        }

        // ---- MAC stream framing: ad || le64(|ad|) || ct || le64(|ct|) --------
        if (RFC && t < PL) {
            // ad || 0.. (to 16) || ct || 0.. (to 16) || le64(|ad|) || le64(|ct|)  (RFC 8439 section 2.8)
            for (uint32_t i = t; i < A - Z; i += PL) {
                uint8_t v = 0u;
                if (i < adlen) v = ad_byte<T13>(p, rec, rk.seq, n, i);
                lds[S + i] = v;
            }
            const uint32_t zp = (0u - n) & 15u;  // zeros to the end of the last ciphertext block
            for (uint32_t i = t; i < zp + 16u; i += PL) {
                const uint32_t e = i - zp;  // byte of the length block
                uint8_t v = 0u;
                if (i >= zp) v = e < 8u ? (uint8_t)((uint64_t)adlen >> (8u * e)) : (uint8_t)((uint64_t)n >> (8u * (e - 8u)));
                ct_lds[n + i] = v;
            }
        }
        if (!RFC && t < PL) {
            for (uint32_t i = t; i < adlen + 8u; i += PL) {
                uint8_t v;
                if (i < adlen)
                    v = ad_byte<T13>(p, rec, rk.seq, n, i);
                else
                    v = (uint8_t)((uint64_t)adlen >> (8u * (i - adlen)));
                lds[S + i] = v;
            }
            // suffix le64(n), then zeros to the end of the last block
            for (uint32_t i = t; i < 28u; i += PL) ct_lds[n + i] = i < 8u ? (uint8_t)((uint64_t)n >> (8u * i)) : 0;
        }
    }
    __syncthreads();
    if (!work || t >= PL) return;

    // ---- phase 2: Poly1305 on PL lanes -----------------------------------------
    const MacGeom g = mac_geom<C>(adlen, n, PL);
    const uint32_t* kr = p.ws + (uint64_t)rec * kKeyRecWords;
    uint32_t r0 = kr[kR32Off + 0], r1 = kr[kR32Off + 1], r2 = kr[kR32Off + 2], r3 = kr[kR32Off + 3];
    if constexpr (PL == 64u) {  // one record per wave: keep the key in SGPRs
        r0 = uniform(r0); r1 = uniform(r1); r2 = uniform(r2); r3 = uniform(r3);
    }
    const uint32_t s1 = r1 + (r1 >> 2), s2 = r2 + (r2 >> 2), s3 = r3 + (r3 >> 2);
    // open: the finishing lane fetches the received tag after the keying record's r
    // words (loads retire in order: waiting for r must not wait for the tag), so
    // that its latency hides behind the Horner loop
    uint32_t rx[4] = {0u, 0u, 0u, 0u};
    if constexpr (OPEN) {
        if (t == PL - 1u) load_tag(in + n, rx);  // the lane that finishes the tag
    }

    // lane t: virtual blocks [t*k, t*k + k); virtual block v is real iff v >= z
    const uint32_t v0 = t * g.k;
    const uint32_t rem = g.L - 16u * (g.B - 1u);  // bytes in the final block, 1..16 (RFC 8439: always 16)
    H32 h = {0u, 0u, 0u, 0u, 0u};
    // Every block is stepped with the 2^128 pad bit; the virtual blocks (the
    // first z of the record, all in lanes t <= tp = z / k) are then discarded
    // instead of being masked block by block: lanes t < tp hold only virtual
    // blocks and drop their sum at the end, lane tp restarts from h = 0 after
    // its first nv = z mod k blocks.  Dropping a prefix of a Horner chain is
    // exact (h = 0 is the state after leading zero blocks), so the tag is the
    // reference's (poly1305.rs:213-228).  Blocks are read as one unaligned
    // 16-byte LDS load each, one block ahead of the multiply.
    {
        const uint8_t* blk = lds + (S - 16u * g.z + 16u * v0);
        const uint32_t tp = g.z / g.k, nv = g.z - tp * g.k;
        // m holds block j; run(e) steps blocks j .. e-1 (e <= k - 1), each
        // load issued one block ahead; unrolled by two so that the
        // prefetched block needs no register copy
        u32x4 m = ldu16(blk);
        uint32_t j = 0;
        auto run = [&](const uint32_t e) {
            for (; j + 2u <= e; j += 2u) {
                const u32x4 ma = ldu16(blk + 16u * (j + 1u));
                __builtin_amdgcn_sched_barrier(0);
                horner_step(h, m.x, m.y, m.z, m.w, 1u, r0, r1, r2, r3, s1, s2, s3);
                m = ldu16(blk + 16u * (j + 2u));
                __builtin_amdgcn_sched_barrier(0);
                horner_step(h, ma.x, ma.y, ma.z, ma.w, 1u, r0, r1, r2, r3, s1, s2, s3);
            }
            if (j < e) {
                const u32x4 mn = ldu16(blk + 16u * (j + 1u));
                __builtin_amdgcn_sched_barrier(0);
                horner_step(h, m.x, m.y, m.z, m.w, 1u, r0, r1, r2, r3, s1, s2, s3);
                m = mn;
                ++j;
            }
        };
        run(nv);
        if (t == tp) h = H32{0u, 0u, 0u, 0u, 0u};
        run(g.k - 1u);
        // final block: a partial one carries its pad bit at 8 * rem
        // (poly1305.rs:216-225; the bytes after the stream are zero)
        uint32_t pad = 1u;
        if (rem < 16u && t == PL - 1u) {
            const uint32_t fb = 1u << (8u * (rem & 3u));
            const uint32_t fw = rem >> 2;
            m.x |= fw == 0u ? fb : 0u;
            m.y |= fw == 1u ? fb : 0u;
            m.z |= fw == 2u ? fb : 0u;
            m.w |= fw == 3u ? fb : 0u;
            pad = 0u;
        }
        horner_step(h, m.x, m.y, m.z, m.w, pad, r0, r1, r2, r3, s1, s2, s3);
        if (t < tp) h = H32{0u, 0u, 0u, 0u, 0u};
    }
    F26 f = h32_to_f26(h);
    // combine lanes: total = sum_t h_t R^(PL-1-t), R = r^k; R^e = hi[e >> 3] * lo[e & 7]
    {
        const uint32_t e = PL - 1u - t;
        const F26 plo = load_f26(kr + key_lo_off(e & 7u));
        const F26 phi = load_f26(kr + key_hi_off(e >> 3));
        const F26 P = mul_add(phi, plo.v0, plo.v1, plo.v2, plo.v3, plo.v4, f26_zero());
        f = mul_add(f, P.v0, P.v1, P.v2, P.v3, P.v4, f26_zero());
    }
    // Sum the PL lane terms into the group's last lane with DPP row shifts
    // (groups of PL <= 16 lanes lie inside one 16-lane row) and the row
    // broadcasts for 32 and 64.  mul_add leaves limbs < 2^27, so 32 terms sum
    // below 2^32; one carry pass precedes the last doubling.
    {
        // (carry_pass of sg_device.h, spelt out: called from here, or the whole sum as a function
        // group_sum<PL>, 5 AEAD kernels order their memory operations differently and 100 change length)
        auto carry = [&]() {
            uint32_t c;
            c = f.v0 >> 26; f.v0 &= M26; f.v1 += c;
            c = f.v1 >> 26; f.v1 &= M26; f.v2 += c;
            c = f.v2 >> 26; f.v2 &= M26; f.v3 += c;
            c = f.v3 >> 26; f.v3 &= M26; f.v4 += c;
            c = f.v4 >> 26; f.v4 &= M26; f.v0 += c * 5u;
        };
        // only the group's last lane (31 or 63 for the broadcasts) is read afterwards
        if constexpr (PL == 2u) carry();
        dpp_add<kDppShr1>(f);
        if constexpr (PL == 4u) carry();
        if constexpr (PL >= 4u) dpp_add<kDppShr2>(f);
        if constexpr (PL == 8u) carry();
        if constexpr (PL >= 8u) dpp_add<kDppShr4>(f);
        if constexpr (PL == 16u) carry();
        if constexpr (PL >= 16u) dpp_add<kDppShr8>(f);
        if constexpr (PL == 32u) carry();
        if constexpr (PL >= 32u) dpp_add<kDppBcast15>(f);
        if constexpr (PL == 64u) {
            carry();
            dpp_add<kDppBcast31>(f);
        }
    }
    uint32_t tw[4];
    if (!finish_tag<PL>(f, kr, t, tw)) return;
    if constexpr (OPEN) p.status[rec] = tag_mismatch(rx, tw);
    else store_tag(out + n, tw);  // ct || tag (chacha20_poly1305.rs:55)
}

// Record slot of this lane's group.  For L >= 64 a group is a whole wave (or
// the workgroup), so the slot is made provably uniform: the record's key,
// nonce and lengths then live in SGPRs and the uniform first-round
// quarter-rounds are hoisted to scalar code.
template <uint32_t L>
__device__ __forceinline__ uint32_t group_of_thread() {
    if constexpr (L == 256u) return 0u;
    else if constexpr (L >= 64u) return __builtin_amdgcn_readfirstlane(threadIdx.x / L);
    else return threadIdx.x / L;
}

// Direct launch: workgroup w serves records w*RPW .. w*RPW + RPW - 1.
template <bool OPEN, uint32_t L, Construction C, bool T13>
__global__ __launch_bounds__(256) void sg_aead_kernel(const KParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr uint32_t RPW = 256u / L;
    const uint32_t g = group_of_thread<L>(), t = threadIdx.x % L;
    const uint32_t rec = blockIdx.x * RPW + g;
    aead_record<OPEN, L, C, T13>(p, rec, rec < p.count, lds + g * p.lds_rec_bytes, t);
}

// Bucketed launch: records listed by sg_classify_kernel for this size class.
// PERSIST = false: the host read the class population back and sized the grid
// exactly (one record group per workgroup, like the direct kernel: waves that
// finish their ChaCha20 share exit and free their slots while wave 0 runs the
// MAC).  PERSIST = true (stream capture, where the host cannot wait): a fixed
// grid walks the list; the barrier closing each iteration makes waves 1-3
// wait for wave 0's MAC, ~30 % slower per byte (tools/exp_list.py).
template <bool OPEN, uint32_t L, bool PERSIST, Construction C, bool T13>
__global__ __launch_bounds__(256) void sg_aead_list_kernel(const KParams p, const uint32_t* __restrict__ list,
                                                           const uint32_t* __restrict__ list_count) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr uint32_t RPW = 256u / L;
    const uint32_t g = group_of_thread<L>(), t = threadIdx.x % L;
    const uint32_t cnt = *list_count;
    const uint32_t stride = PERSIST ? gridDim.x * RPW : 0xffffffffu;
    // XCD-aware order: workgroup b runs on XCD b % 8, and each XCD takes one
    // contiguous run of the list, so neighbouring records (which share cache
    // lines: records are packed byte-tight) are fetched by the same L2.
    const uint32_t nb = gridDim.x, x = blockIdx.x & 7u, q = nb >> 3, r = nb & 7u;
    const uint32_t wg = x * q + (x < r ? x : r) + (blockIdx.x >> 3);
    for (uint32_t base = wg * RPW; base < cnt; base += stride) {
        const uint32_t slot = base + g;
        const bool active = slot < cnt;
        uint32_t rec = active ? list[slot] : 0u;
        if constexpr (L >= 64u) rec = __builtin_amdgcn_readfirstlane(rec);
        aead_record<OPEN, L, C, T13>(p, rec, active, lds + g * p.lds_rec_bytes, t);
        if constexpr (!PERSIST) break;
        __syncthreads();  // LDS is reused by the next iteration
    }
}

// Size-class bucketing.  A 1024-thread workgroup classifies 4096 records:
// per-wave ballots, then one device atomic per class per workgroup (a single
// counter word takes only ~88 atomics/us, so per-wave atomics cost ~0.5 ms
// for 1M records).
constexpr uint32_t kClassifyThreads = 1024;
constexpr uint32_t kClassifyPerThread = 4;

// (T13: a TLS 1.3 seal's class and routes are those of its inner length, tls13_inner_len)
template <bool OPEN, bool T13>
__global__ __launch_bounds__(1024) void sg_classify_kernel(const KParams p, uint32_t* __restrict__ lists,
                                                           uint32_t* __restrict__ counts, const uint32_t max_n) {
    // counts: the kNumLists populations, then the over-long count
    __shared__ uint32_t wave_cnt[kNumLists][kClassifyThreads / 64];
    __shared__ uint32_t wg_base[kNumLists];
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    const uint32_t rec0 = blockIdx.x * (kClassifyThreads * kClassifyPerThread);
    uint32_t cls[kClassifyPerThread];
    uint32_t mine[kNumLists] = {};  // this wave's records per list
#pragma unroll
    for (uint32_t i = 0; i < kClassifyPerThread; ++i) {
        const uint32_t rec = rec0 + i * kClassifyThreads + threadIdx.x;
        cls[i] = kNumLists;
        if (rec < p.count) {
            const uint32_t len = record_len(p, rec);
            const uint32_t n = aead_len<OPEN, T13>(p, len);
            if (n <= max_n) {
                const uint32_t J = rec_wpr_bucket(p, rec, n);
                cls[i] = J ? kNumClasses + J - kWprMinJ : rec_pack(p, rec, n) ? kPackList : size_class(n);
            } else {  // longer than the batch's max_len: no class (its LDS slot would overflow), flagged
                atomicAdd(&counts[kNumLists], 1u);
                if constexpr (OPEN) p.status[rec] = 3u;
            }
        }
#pragma unroll
        for (uint32_t c = 0; c < kNumLists; ++c) mine[c] += (uint32_t)__popcll(__ballot(cls[i] == c));
    }
    if (lane == 0)
        for (uint32_t c = 0; c < kNumLists; ++c) wave_cnt[c][wave] = mine[c];
    __syncthreads();
    if (threadIdx.x < kNumLists) {
        uint32_t tot = 0;
        for (uint32_t w = 0; w < kClassifyThreads / 64; ++w) {
            const uint32_t x = wave_cnt[threadIdx.x][w];
            wave_cnt[threadIdx.x][w] = tot;  // exclusive prefix over waves
            tot += x;
        }
        wg_base[threadIdx.x] = tot ? atomicAdd(&counts[threadIdx.x], tot) : 0u;
    }
    __syncthreads();
    uint32_t off[kNumLists];
#pragma unroll
    for (uint32_t c = 0; c < kNumLists; ++c) off[c] = wg_base[c] + wave_cnt[c][wave];
#pragma unroll
    for (uint32_t i = 0; i < kClassifyPerThread; ++i) {
        const uint32_t rec = rec0 + i * kClassifyThreads + threadIdx.x;
#pragma unroll
        for (uint32_t c = 0; c < kNumLists; ++c) {
            const uint64_t mask = __ballot(cls[i] == c);
            if (cls[i] == c) lists[(uint64_t)c * p.count + off[c] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = rec;
            off[c] += (uint32_t)__popcll(mask);
        }
    }
}

}  // namespace

hipError_t launch_keying(const KParams& p, bool open, const KeyJobs& jobs, uint32_t grid, hipStream_t s) {
    if (grid == 0) return hipSuccess;
    with_form(p, open, [&](auto OPEN, auto C, auto T13) {
        hipLaunchKernelGGL((sg_keying_kernel<OPEN.value, C.value, T13.value>), dim3(grid), dim3(kKeyingThreads), 0, s, p,
                           jobs);
    });
    return hipGetLastError();
}

// every record of the batch, by index
hipError_t launch_keying_all(const KParams& p, bool open, hipStream_t s) {
    KeyJobs jobs = {};
    return launch_keying(p, open, jobs, (p.count + kKeyingThreads - 1u) / kKeyingThreads, s);
}

hipError_t launch_classify(const KParams& p, bool open, uint32_t* lists, uint32_t* counts, uint32_t max_n,
                           hipStream_t s) {
    const uint32_t per_wg = kClassifyThreads * kClassifyPerThread;
    const dim3 grid((p.count + per_wg - 1u) / per_wg);
    if (open)  // (an open's length is the fragment's in either record form)
        hipLaunchKernelGGL((sg_classify_kernel<true, false>), grid, dim3(kClassifyThreads), 0, s, p, lists, counts, max_n);
    else if (p.tls13)
        hipLaunchKernelGGL((sg_classify_kernel<false, true>), grid, dim3(kClassifyThreads), 0, s, p, lists, counts, max_n);
    else
        hipLaunchKernelGGL((sg_classify_kernel<false, false>), grid, dim3(kClassifyThreads), 0, s, p, lists, counts, max_n);
    return hipGetLastError();
}

template <uint32_t L>
static hipError_t launch_direct(const KParams& p, bool open, hipStream_t s) {
    constexpr uint32_t RPW = 256u / L;
    const uint32_t grid = (p.count + RPW - 1u) / RPW;
    with_form(p, open, [&](auto OPEN, auto C, auto T13) {
        const size_t lds = RPW * p.lds_rec_bytes;
        hipLaunchKernelGGL((sg_aead_kernel<OPEN.value, L, C.value, T13.value>), dim3(grid), dim3(kThreads), lds, s, p);
    });
    return hipGetLastError();
}

// n_exact: the class population when the host knows it (exact grid), or
// UINT32_MAX for a persistent grid capped at kListGridPerCU workgroups per CU.
template <uint32_t L>
static hipError_t launch_list(const KParams& p, bool open, const uint32_t* list, const uint32_t* cnt, uint32_t n_exact,
                              hipStream_t s) {
    constexpr uint32_t RPW = 256u / L;
    const size_t lds = RPW * p.lds_rec_bytes;
    if (n_exact == 0) return hipSuccess;
    const bool persist = n_exact == 0xffffffffu;
    uint32_t grid = ((persist ? p.count : n_exact) + RPW - 1u) / RPW;
    const uint32_t cap = kListGridPerCU * 256u;
    if (persist && grid > cap) grid = cap;
    with_form(p, open, [&](auto OPEN, auto C, auto T13) {
        const dim3 g(grid), b(kThreads);
        constexpr bool O = OPEN.value, T = T13.value;
        if (persist) hipLaunchKernelGGL((sg_aead_list_kernel<O, L, true, C.value, T>), g, b, lds, s, p, list, cnt);
        else hipLaunchKernelGGL((sg_aead_list_kernel<O, L, false, C.value, T>), g, b, lds, s, p, list, cnt);
    });
    return hipGetLastError();
}

hipError_t launch_class(uint32_t c, const KParams& q, bool open, const uint32_t* list, const uint32_t* cnt,
                        uint32_t n_exact, hipStream_t s) {
#define SG_CLASS_CASE(C)                                                                  \
    case C:                                                                               \
        return list ? launch_list<class_lanes(C)>(q, open, list, cnt, n_exact, s)         \
                    : launch_direct<class_lanes(C)>(q, open, s);
    switch (c) {
        SG_CLASS_CASE(0) SG_CLASS_CASE(1) SG_CLASS_CASE(2) SG_CLASS_CASE(3)
        SG_CLASS_CASE(4) SG_CLASS_CASE(5) SG_CLASS_CASE(6)
        default: return list ? launch_list<class_lanes(7)>(q, open, list, cnt, n_exact, s)
                             : launch_direct<class_lanes(7)>(q, open, s);
    }
#undef SG_CLASS_CASE
}

const char* class_kernel_config() {
    return "sg_aead_kernel v9 8 size classes (2..256 lanes per record, one 64-B block per lane, device bucketing, exact class grids), "
           "lane=64B ChaCha block (counter-free round-1 QRs on SALU for wave-uniform records), Poly1305 contiguous-chunk "
           "Horner radix-2^32 (clamped r, unaligned 16-B LDS block loads, folded pad bit) on min(L,64) lanes + per-lane "
           "r^(k(PL-1-t)) scale + DPP sum, tag finalised on the SALU for one-record waves, keying pre-pass";
}

}  // namespace sg
