// sg_wpr_keying.hip -- the keying pre-pass of the gfx950 wave-per-record kernel
// (sg_wpr.hip): per record the Poly1305 key, the power tables of r that the
// record kernel's MFMA MAC reads, and the record's constant term ctot.
//
// MAC.  The reference evaluates h = sum_b v_b r^(B - b) over the 16-byte
// blocks of ad || le64(|ad|) || ct || le64(|ct|) (chacha20_poly1305.rs:19-42,
// poly1305.rs:207-228).  Ciphertext chunk m (bytes 16 m .. 16 m + 15) starts
// at stream offset o + 16 m, o = |ad| + 8 = 16 beta + sigma, so its byte a' has
// weight 2^(8 (sigma + a')) r^(E(m) + 1) when sigma + a' < 16 and
// 2^(8 (sigma + a' - 16)) r^E(m) otherwise, with E(m) = B - beta - 1 - m.
// Chunk m = 256 j + 128 h + 4 q + i (iteration j, lane 32 h + q, chunk i of
// the lane's block) factors as E(m) = 4 (31 - q) + e(j, h, i),
// e = 128 (1 - h) + 256 (3 - j) + (4 - i) + delta.  Each MFMA step (j, i) then
// computes D[c][q] += sum_{h, a'} T[c][(h, a')] (byte - 128), where column q
// is the lane's chunk and row c a base-256 digit position: T holds the signed
// digits of r^(e + 1) and r^e, shifted by sigma + a' (a Toeplitz band).  The
// eight powers per step, r^(128 k + 1 + delta + u) (k = 0..7, u = 0..4), are
// built once per record as 48-byte digit lines in LDS; a lane reads its
// 16-byte T fragment as two windows of two adjacent lines (aligned dwords
// shifted with v_alignbyte).  |D| <
// 2^23; the record's first MFMA starts from a zero accumulator and the
// assembly adds a seed of 2^24 per entry (v_mad_i64_i32 on the signed
// entries), so every 64-bit word is positive.  At the end each lane assembles
// its 16 entries exactly, X = sum_r (D[c_r][q] + 2^24) 2^(8 c_r), reduces it
// mod 2^130 - 5, multiplies by
// W = r^(4 (31 - q)) (times 2^32 for the upper half-wave) and a DPP sum adds
// the 64 terms.  This kernel supplies the per-record constant ctot:
// the AD / length blocks, the pad bits, the i8 bias and the seed.  Every step
// is exact arithmetic mod p, so tags equal the reference's bit for bit
// (tests/test_wpr_mac_model.py pins this decomposition against the CPU
// restatement of poly1305.rs).
//
// Construction::kRfc8439 (the uniform launch and the J = 2..4 buckets; sg_*_batch_rfc8439): in the RFC
// 8439 stream ad || 0.. || ct || 0.. || le64(|ad|) || le64(n) the ciphertext
// starts on a block boundary, which is the sigma = 0 case above for every AD
// length, so the MFMA body is the draft's.  The constant term
// changes (wpr_geom: o = 16 ceil(|ad| / 16), B = beta + m + 1, rem = 16,
// delta = 0; the prefix is ad and its zero padding, the suffix the one full
// length block at weight r).  tests/test_wpr_mac_model_rfc8439.py pins the constant term.
// The constant term of a bucket record (LIST) is wpr_geom<kRfc8439>(13, n) of the
// right-aligned record, with
// the S(c) pieces of the draft's bucket keying (they depend on n / 64 alone) and
// the same single length block (tests/test_wpr_bucket_model_rfc8439.py).
//
// TLS 1.3 buckets (LIST with T13): the MAC stream AD(5) || 0^11 || ct || le64(5) || le64(n)
// of a padded record of n = 64 k' inner bytes is
// the RFC bucket record's all-full-block stream behind a 5-byte AD, and
// wpr_geom<kRfc8439>(5, n) is the 13-byte AD's, so the keying differs in the prefix
// block 17 03 03 be16(n + 16) and the length block alone
// (tests/test_wpr_bucket_model_tls13.py); the descriptor's words 10 and 11 carry the
// content length and the inner type.
#include "sg_wpr_layout.h"
#include "sg_device.h"

#include <stdint.h>

namespace sg {
namespace {

using namespace dev;

constexpr uint32_t kWprKeyThreads = 64;

// units [U0, U1) of a lane's record (rec: the record's 160 words, registers), stored
// straight from registers in the grouped table layout (wpr_tab_unit, sg_wpr_layout.h)
template <uint32_t U0, uint32_t U1>
__device__ __forceinline__ void wpr_store_units(const WprList& wl, uint32_t slot, bool act, const uint32_t* rec) {
    if (!act) return;
#pragma unroll
    for (uint32_t u = U0; u < U1; ++u) {
        const u32x4 val = {rec[4u * u], rec[4u * u + 1u], rec[4u * u + 2u], rec[4u * u + 3u]};
        __builtin_nontemporal_store(val, reinterpret_cast<u32x4*>(wpr_tab_unit(wl, slot, u)));
    }
}

// One launch keys every bucket: job b on blocks [blk0[b], blk0[b + 1]).
struct WprKeyJobs {
    WprList b[kWprBuckets];
    uint32_t blk0[kWprBuckets];
    uint32_t njobs;
};

// ---- the terms of ctot (tests/wpr_model.py keying, same names) ----

// pads (poly1305.rs:224-225): 2^128 sum_{b < B-1} r^(B-b) + 2^(8 rem) r
//   = 2^128 G(B) + (2^(8 rem) + p - 2^128) r,  GB = G(B) = sum_{i=1..B} r^i
__device__ __forceinline__ F26 wpr_pads(const F26& r, const F26& GB, uint32_t rem) {
    const F26 pads = mul_add(GB, 0u, 0u, 0u, 0u, 1u << 24, f26_zero());
    F26 cf = F26{0x3fffffbu, 0x3ffffffu, 0x3ffffffu, 0x3ffffffu, 0x2ffffffu};  // p - 2^128
    const uint32_t bit = 8u * rem, li = bit / 26u, v = 1u << (bit - 26u * li);
    cf.v0 += li == 0u ? v : 0u;
    cf.v1 += li == 1u ? v : 0u;
    cf.v2 += li == 2u ? v : 0u;
    cf.v3 += li == 3u ? v : 0u;
    cf.v4 += li == 4u ? v : 0u;
    return fmul_add(cf, r, pads);
}

// i8 bias: 128 sum over the ciphertext bytes of their weights
//   = r^delta G(m) (A1 r + A2),  A1 = sum_{k=sigma}^{15} 128 2^(8k),  A2 = sum_{k<sigma} 128 2^(8k)
// (g = G(m), rdel = r^delta)
__device__ __forceinline__ F26 wpr_bias(const F26& r, const F26& g, const F26& rdel, uint32_t sigma) {
    uint32_t a1[4], a2[4];
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t mk = bytes_from(w, sigma);
        a1[w] = 0x80808080u & mk;
        a2[w] = 0x80808080u & ~mk;
    }
    const F26 A1 = words_to_f26(a1[0], a1[1], a1[2], a1[3], 0u);
    const F26 A2 = words_to_f26(a2[0], a2[1], a2[2], a2[3], 0u);
    return fmul(fmul(g, fmul_add(A1, r, A2)), rdel);
}

// accumulator seed: -(2^24 sum_c 2^(8c)) SW (every column, the idle lanes' too)
__device__ __forceinline__ F26 wpr_seed(const F26& SW) { return mul_add(SW, kCJ0, kCJ1, kCJ2, kCJ3, kCJ4, f26_zero()); }

// suffix le64(n) at stream offset o + n = 16 (beta + m) + sigma: n 2^(8 sigma) split at 2^128
// (RFC 8439: the single full block le64(adlen) || le64(n), the stream's last, at weight r)
// (rd0 = r^(1 + delta), rdel = r^delta; tail: TAIL13's ciphertext byte 2^14)
template <Construction C, bool TAIL13>
__device__ __forceinline__ F26 wpr_suffix(const F26& r, const F26& r2, const F26& rd0, const F26& rdel, uint32_t adlen,
                                          uint32_t n, uint32_t sigma, uint32_t tail) {
    if constexpr (TAIL13) {  // the tail block at r^2 (its 2^128 is in pads), then the length block
        return fmul_add(F26{tail, 0u, 0u, 0u, 0u}, r2, fmul(words_to_f26(adlen, 0u, n + 1u, 0u, 0u), r));
    } else if constexpr (C == Construction::kRfc8439) {
        return fmul(words_to_f26(adlen, 0u, n, 0u, 0u), r);
    } else {
        const uint32_t wi = sigma >> 2, bs = 8u * (sigma & 3u);
        const uint64_t v = (uint64_t)n << bs;
        uint32_t w[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            if (i == wi) {
                w[i] = (uint32_t)v;
                w[i + 1] = (uint32_t)(v >> 32);
            }
        }
        return fmul_add(words_to_f26(w[0], w[1], w[2], w[3], 0u), rd0, fmul(F26{w[4], 0u, 0u, 0u, 0u}, rdel));
    }
}

// ---------------------------------------------------------------------------
// Keying pre-pass: one lane per record, 64 records per wave, the 160-word
// record (sg_internal.h, kW*) stored unit by unit from registers (grouped layout,
// sg_wpr_layout.h).
// LIST: lane = slot of a bucket list (record wl.list[slot], any n of the
// bucket), which also writes the slot's descriptor; otherwise slot = record
// and n = 2^14.
// ---------------------------------------------------------------------------
// T13 (KParams.tls13; uniform launches of Construction::kRfc8439 only): a TLS 1.3
// record of 2^14 content bytes and the inner type byte, n = 2^14 + 1 (RFC 8446
// section 5.2).  The MAC stream is AD(5) || 11 zeros || 1024 ciphertext blocks ||
// [ct byte 2^14 || 15 zeros] || le64(5) || le64(n): the record kernel's 1024 blocks
// with one block more behind them, i.e. wpr_geom's B + 1 and delta = 1.  The
// record kernel runs the 2^14 bytes; this kernel takes the tail over: keystream
// block 257 beside block 0, the tail byte (seal: type ^ ks into out[2^14]; open:
// in[2^14] ^ ks into out[2^14]) and its block (byte + 2^128) r^2 in ctot
// (tests/test_wpr_mac_model_tls13.py).
// T13 with LIST (bucket records, n the inner length, a multiple of 64): no tail; the
// RFC bucket keying with adlen = 5, the header 17 03 03 be16(n + 16) as the prefix
// block and le64(5) || le64(n) as the length block; seal: n = tls13_inner_len(len,
// pad_to), and the descriptor carries the content length and the inner type.
// (compiled for two waves per SIMD: four and more spill to scratch)
template <bool OPEN, bool LIST, Construction C, bool T13>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void sg_wpr_keying_kernel(
    const KParams p, const WprKeyJobs jobs) {
    constexpr bool RFC = C == Construction::kRfc8439;
    static_assert(!T13 || RFC, "TLS 1.3 records are RFC 8439");
    constexpr bool TAIL13 = T13 && !LIST;  // the uniform launch: this kernel takes the tail byte and its block
    const uint32_t lane = threadIdx.x;
    WprList wl = jobs.b[0];
    uint32_t b0 = 0;
#pragma unroll
    for (uint32_t i = 1; i < kWprBuckets; ++i)  // (constant indices: the kernarg table stays in SGPRs)
        if (i < jobs.njobs && blockIdx.x >= jobs.blk0[i]) {
            wl = jobs.b[i];
            b0 = jobs.blk0[i];
        }
    const uint32_t slot0 = (blockIdx.x - b0) * kWprKeyThreads;
    const uint32_t slot = slot0 + lane;
    uint32_t rbuf[kWprRecWords];  // the lane's record (registers once unrolled)
#pragma unroll
    for (uint32_t i = 0; i < kWprRecWords; ++i) rbuf[i] = 0u;
    uint32_t* st = rbuf + 80;  // the second half first (offsets below are half-relative)
    const uint32_t adlen = ad_len<T13>(p);
    if (blockIdx.x == b0 && lane == 0u) *wl.ctr = 0u;  // the record kernel's group counter

    const bool act = slot < wl.count;
    const uint32_t rec = LIST ? (act ? wl.list[slot] : 0u) : slot;
    uint32_t n = kWprN;
    // (T13 buckets: the inner length, content || type || zeros on seal, as classified)
    if constexpr (LIST && T13 && !OPEN) n = act ? tls13_inner_len(p.len[rec], p.pad_to) : kWprN;
    else if constexpr (LIST) n = act ? p.len[rec] - (OPEN ? 16u : 0u) : kWprN;
    WprGeom G = wpr_geom<C>(adlen, n);
    if constexpr (TAIL13) {  // the tail block behind the 1024 of the record kernel
        G.B += 1u;
        G.delta = 1u;
    }

    // ---- the Poly1305 key, the tail byte (TAIL13) and the slot's descriptor (LIST) ----
    F26 r = f26_zero();
    uint32_t s[4] = {0u, 0u, 0u, 0u};
    RecKey rk = {};
    uint32_t tail = 0u;  // T13: ciphertext byte 2^14
    if (act) {
        rk = record_key<C>(p, rec);
        uint32_t ks[16];
        chacha_block(ks, rk.k, 0u, rk.n13, rk.n14, rk.n15);  // block 0 -> poly key (chacha20_poly1305.rs:50,75)
        const PolyKey pk = poly_key(ks);
        r = words_to_f26(pk.r0, pk.r1, pk.r2, pk.r3, 0u);
        s[0] = pk.s[0]; s[1] = pk.s[1]; s[2] = pk.s[2]; s[3] = pk.s[3];
        if constexpr (TAIL13) {
            chacha_block(ks, rk.k, kWprTailBlock, rk.n13, rk.n14, rk.n15);  // byte 2^14 is its first
            uint8_t* ob = p.out + p.out_stride * rec + kWprN;
            if constexpr (OPEN) {
                tail = p.in[p.in_stride * rec + kWprN];
                *ob = (uint8_t)(tail ^ ks[0]);
            } else {
                tail = (p.tls_hdr ^ ks[0]) & 0xffu;  // the inner type (content_type)
                *ob = (uint8_t)tail;
            }
        }
        if constexpr (LIST) {  // the slot's descriptor: where the record lives, its length and nonce
            const uint64_t io = rec_in_off(p, rec);
            const uint64_t oo = rec_out_off(p, rec);
            const uint32_t ki = key_slot(p, rec);
            uint32_t* d = wl.desc + (uint64_t)slot * kWprDescWords;
            st16(d, u32x4{(uint32_t)io, (uint32_t)(io >> 32), (uint32_t)oo, (uint32_t)(oo >> 32)});
            st16(d + 4, u32x4{n, rec, ki, rk.n14});
            // (T13 seal: the content length and the inner type, for the record kernel's loads and patch)
            uint32_t clen = 0u, type = 0u;
            if constexpr (T13 && !OPEN) {
                clen = p.len[rec];
                type = tls13_inner_type(p, rec);
            }
            st16(d + 8, u32x4{rk.n15, RFC ? rk.n13 : 0u, clen, type});
        }
    }

    // ---- power tables, second half: lo[b] = R^b, hi[h][a] = 2^(32 h) R^(8 a) (R = r^4) ----
    // (LIST: also the pieces of S(c) = sum_{u<c} R^u, c = (n / 64) & 31, see below)
    const uint32_t kq = n >> 6, ca = kq >> 5, cl = kq & 7u, ch = (kq >> 3) & 3u;
    auto sel = [](bool c, const F26& a, const F26& b) {
        return F26{c ? a.v0 : b.v0, c ? a.v1 : b.v1, c ? a.v2 : b.v2, c ? a.v3 : b.v3, c ? a.v4 : b.v4};
    };
    const F26 r2 = fmul(r, r), R = fmul(r2, r2);
    F26 x = f26_one(), sum_lo = f26_zero(), plo = f26_zero(), xlo = f26_one();
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        store_f26(st + (kWLo - 80u) + 5u * b, x);
        sum_lo = f26_add(sum_lo, x);
        if constexpr (LIST) {
            plo = sel((uint32_t)b < cl, f26_add(plo, x), plo);  // sum_{b' < c & 7} R^b'
            xlo = sel((uint32_t)b == cl, x, xlo);               // R^(c & 7)
        }
        x = fmul(x, R);
    }
    const F26 R8 = x;
    F26 y = f26_one(), sum_hi = f26_zero(), phi = f26_zero(), yc = f26_one();
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        store_f26(st + (kWHi - 80u) + 5u * a, y);
        store_f26(st + (kWHi - 80u) + 20u + 5u * a, mul_add(y, 0u, 64u, 0u, 0u, 0u, f26_zero()));  // * 2^32
        sum_hi = f26_add(sum_hi, y);
        if constexpr (LIST) {
            phi = sel((uint32_t)a < ch, f26_add(phi, y), phi);  // sum_{a' < c >> 3} R^(8 a')
            yc = sel((uint32_t)a == ch, y, yc);                 // R^(8 (c >> 3))
        }
        y = fmul(y, R8);
    }
    const F26 T = y;  // R^32 = r^128
    wpr_store_units<20, 40>(wl, slot, act, rbuf);
    st = rbuf;

    // ---- power tables, first half: s, rd[u] = r^(1 + delta + u), tk[k] = T^k (ctot at the end) ----
    st[kWS + 0] = s[0]; st[kWS + 1] = s[1]; st[kWS + 2] = s[2]; st[kWS + 3] = s[3];
    const F26 r3 = fmul(r2, r), r5 = fmul(R, r), r6 = fmul(R, r2);
    const bool d1 = G.delta != 0u;
    const F26 pw[6] = {r, r2, r3, R, r5, r6};
#pragma unroll
    for (int u = 0; u < 5; ++u) store_f26(st + kWRd + 5u * u, d1 ? pw[u + 1] : pw[u]);
    const F26 rd0 = d1 ? r2 : r;        // r^(1 + delta)
    const F26 rdel = d1 ? r : f26_one();  // r^delta
    F26 t = f26_one(), sum_t = f26_zero(), pta = f26_zero(), ta = f26_one();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        store_f26(st + kWTk + 5u * k, t);
        sum_t = f26_add(sum_t, t);
        if constexpr (LIST) pta = sel((uint32_t)k < ca, f26_add(pta, t), pta);  // sum_{k' < a} T^k'
        t = fmul(t, T);
        if constexpr (LIST) ta = sel((uint32_t)k + 1u == ca, t, ta);            // T^a
    }
    wpr_store_units<3, 20>(wl, slot, act, rbuf);  // rd and tk now; s and ctot (units 0-2) at the end

    // ---- geometric sums: SW = sum_{u<32} R^u; g = G(m) = sum_{i=1..m} r^i and rm = r^m
    // (m = n / 16: for n = 2^14, G(1024) = (r + r^2 + r^3 + r^4) SW sum_k T^k, r^1024 = T^8).
    // Bucket records (LIST) have n = 64 k', k' = 32 a + c (a = 2..8, c < 32), so from the
    // tables: G(4 k') = G4 S(k'), S(k') = sum_{u<k'} R^u = SW sum_{k<a} T^k + T^a S(c),
    // S(c) = sum_{a'<c>>3} R^(8 a') sum_lo + R^(8 (c>>3)) sum_{b<c&7} R^b, r^m = T^a R^(8 (c>>3)) R^(c&7)
    // (7 products instead of the ~25 of a square-and-multiply geometric sum)
    const F26 SW = fmul(carry1(sum_hi), carry1(sum_lo));
    const F26 G4 = carry1(f26_add(f26_add(r, r2), f26_add(r3, R)));
    F26 g, rm;
    if constexpr (LIST) {
        const F26 Sc = fmul_add(yc, carry1(plo), fmul(carry1(phi), carry1(sum_lo)));
        const F26 Sk = fmul_add(SW, carry1(pta), fmul(ta, Sc));
        g = fmul(G4, Sk);
        rm = fmul(ta, fmul(yc, xlo));
    } else {
        g = fmul(fmul(G4, SW), carry1(sum_t));
        rm = t;
    }

    // ---- ctot = pads + bias + seed + prefix + suffix ----
    const F26 GB = fmul_add(rm, geo_sum(r, G.B - G.m), g);  // G(B) = G(m) + r^m G(B - m)
    const F26 pads = wpr_pads(r, GB, G.rem);
    const F26 bias = wpr_bias(r, g, rdel, G.sigma);
    const F26 seed = wpr_seed(SW);
    // prefix ad || le64(|ad|) (stream bytes < o) as blocks 0..beta: Horner, then r^(B - beta) = r^m r^(1 + delta)
    // (the one term that reads the record's memory; it stays in the kernel body, where it costs no register)
    F26 hp = f26_zero();
    if (act) {
        for (uint32_t b = 0; b <= G.beta; ++b) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            for (uint32_t i = 0; i < 16u; ++i) {
                const uint32_t pos = 16u * b + i;
                // (RFC 8439: ad and its zero padding; block beta is empty, sigma = 0)
                if constexpr (T13) {  // the record header; L = n + 1 + 16 (buckets: n the inner length, L = n + 16)
                    if (pos < adlen) w[i >> 2] |= (uint32_t)tls13_ad_byte(LIST ? n + 16u : kWprN + 17u, pos) << (8u * (i & 3u));
                } else if (pos < G.o)
                    w[i >> 2] |= (uint32_t)prefix_byte<C>(p, rec, rk.seq, n, adlen, pos) << (8u * (i & 3u));
            }
            hp = fmul_add(hp, r, words_to_f26(w[0], w[1], w[2], w[3], 0u));
        }
    }
    const F26 prefix = fmul(fmul(hp, rm), rd0);
    const F26 suffix = wpr_suffix<C, TAIL13>(r, r2, rd0, rdel, adlen, n, G.sigma, tail);
    const F26 ctot = carry1(f26_add(f26_add(f26_add(pads, bias), f26_add(seed, prefix)), suffix));
    store_f26(st + kWCtot, ctot);
    wpr_store_units<0, 3>(wl, slot, act, rbuf);
}

}  // namespace

// `grid` blocks of kWprKeyThreads slots over `jobs`
template <bool LIST>
static hipError_t launch_keying_jobs(const KParams& p, bool open, const WprKeyJobs& jobs, uint32_t grid, hipStream_t s) {
    with_form(p, open, [&](auto OPEN, auto C, auto T13) {
        const dim3 g(grid), b(kWprKeyThreads);
        hipLaunchKernelGGL((sg_wpr_keying_kernel<OPEN.value, LIST, C.value, T13.value>), g, b, 0, s, p, jobs);
    });
    return hipGetLastError();
}

hipError_t launch_wpr_keying(const KParams& p, bool open, const WprList& wl, hipStream_t s) {
    WprKeyJobs jobs = {};
    jobs.b[0] = wl;
    jobs.njobs = 1;
    return launch_keying_jobs<false>(p, open, jobs, (wl.count + kWprKeyThreads - 1u) / kWprKeyThreads, s);
}

hipError_t launch_wpr_keying_lists(const KParams& p, bool open, const WprList* wl, hipStream_t s) {
    if (!p.tls) return hipErrorInvalidValue;  // buckets are TLS records: 1.2 of either construction, padded 1.3
    WprKeyJobs jobs = {};
    uint32_t grid = 0;
    for (uint32_t b = 0; b < kWprBuckets; ++b) {
        if (wl[b].count == 0) continue;
        jobs.b[jobs.njobs] = wl[b];
        jobs.blk0[jobs.njobs] = grid;
        grid += (wl[b].count + kWprKeyThreads - 1u) / kWprKeyThreads;
        ++jobs.njobs;
    }
    if (grid == 0) return hipSuccess;
    return launch_keying_jobs<true>(p, open, jobs, grid, s);
}

}  // namespace sg
