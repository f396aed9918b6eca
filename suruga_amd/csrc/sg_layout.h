// sg_layout.h -- the two AEAD constructions of the library, the geometry of
// their MAC streams and the three record forms, in one place for the record kernels (sg_kernels.hip,
// sg_wpr.hip, sg_pack.hip), the message kernels (sg_msg_device.h) and the
// host-side plan (sg_msg_plan.h).  No HIP: plain constexpr functions, which
// hipcc takes as host and device code, so the host-only programs include it too.
// Not part of the public ABI.
#pragma once

#include <stdint.h>

namespace sg {

// The construction, a compile-time parameter of every kernel that differs:
//   kDraft    draft-agl-tls-chacha20poly1305-04 as in klutzy/suruga
//             (chacha20_poly1305.rs:19-42): 8-byte nonce in state words 14-15,
//             word 13 = 0; MAC stream ad || le64(adlen) || ct || le64(n), no padding
//   kRfc8439  RFC 8439 section 2.8: 12-byte nonce in state words 13-15; MAC
//             stream ad || zeros to 16 || ct || zeros to 16 || le64(adlen) ||
//             le64(n), every block full
// KParams.rfc, SG_MSG_RFC8439 and the *_rfc8439 calls select it at run time;
// with_form (sg_internal.h) turns that into the template argument.
enum class Construction { kDraft, kRfc8439 };

template <Construction C>
constexpr uint32_t nonce_len() {
    return C == Construction::kRfc8439 ? 12u : 8u;
}

// Stream offset of the ciphertext and length of the stream for adlen AD bytes
// and n data bytes, in the caller's integer type (the record kernels count in
// uint32_t, the message kernels in int64_t, the plan in uint64_t).
template <Construction C, class T>
constexpr T ct_offset(T adlen) {
    return C == Construction::kRfc8439 ? (adlen + 15) / 16 * 16 : adlen + 8;
}
template <Construction C, class T>
constexpr T stream_bytes(T adlen, T n) {
    return C == Construction::kRfc8439 ? ct_offset<C>(adlen) + (n + 15) / 16 * 16 + 16 : ct_offset<C>(adlen) + n + 8;
}

// chacha20_poly1305.rs:19-42: the TLS record's 13 AD bytes and its le64, then
// the data and its le64 -- nothing rounded
static_assert(nonce_len<Construction::kDraft>() == 8u, "draft nonce");
static_assert(ct_offset<Construction::kDraft>(13u) == 21u && ct_offset<Construction::kDraft>(0u) == 8u, "draft");
static_assert(stream_bytes<Construction::kDraft>(13u, 16384u) == 16413u, "draft: 13 + 8 + n + 8");
static_assert(stream_bytes<Construction::kDraft>(0u, 0u) == 16u, "draft: the two lengths alone");
static_assert(stream_bytes<Construction::kDraft, int64_t>(12, 114) == 142, "draft, signed");
// RFC 8439 section 2.8.2: 12 AD bytes (padded to 16), 114 data bytes (padded
// to 128), one length block: the 160 bytes of its "Poly1305 message"
static_assert(nonce_len<Construction::kRfc8439>() == 12u, "RFC 8439 nonce");
static_assert(ct_offset<Construction::kRfc8439>(12u) == 16u && ct_offset<Construction::kRfc8439>(0u) == 0u, "RFC 8439");
static_assert(ct_offset<Construction::kRfc8439>(13u) == 16u && ct_offset<Construction::kRfc8439>(17u) == 32u, "RFC 8439");
static_assert(stream_bytes<Construction::kRfc8439>(12u, 114u) == 160u, "RFC 8439 section 2.8.2");
static_assert(stream_bytes<Construction::kRfc8439>(0u, 0u) == 16u, "RFC 8439: the length block alone");
static_assert(stream_bytes<Construction::kRfc8439, int64_t>(13, 16384) == 16416, "RFC 7905 record, signed");

// The record form of a batch call, on top of its construction: kDraft (sg_*_batch:
// the draft, TLS 1.2 records), kRfc8439 (sg_*_batch_rfc8439: RFC 8439, in TLS mode
// RFC 7905's nonce) and kTls13 (sg_*_batch_tls13: RFC 8439 over the inner plaintext
// content || type of RFC 8446 section 5.2, the 5-byte record header as AD).  The host
// layer (sg_capi.cpp) carries one such value from the entry point to KParams.rfc /
// KParams.tls13; with_form (sg_internal.h) makes those the kernels' template arguments.
enum class RecordForm { kDraft, kRfc8439, kTls13 };
constexpr uint32_t kWprN = 16384;  // a full record of the wave-per-record kernel (sg_internal.h)

constexpr Construction construction_of(RecordForm f) { return f == RecordForm::kDraft ? Construction::kDraft : Construction::kRfc8439; }
// AD bytes of a TLS-mode record, and the bytes a seal adds in front of the tag
constexpr uint32_t tls_ad_len(RecordForm f) { return f == RecordForm::kTls13 ? 5u : 13u; }
constexpr uint32_t seal_extra(RecordForm f) { return f == RecordForm::kTls13 ? 1u : 0u; }
// a full wave-per-record record: its content (seal), its fragment with the tag (open)
constexpr uint32_t wpr_len(RecordForm f, bool open) { return open ? kWprN + seal_extra(f) + 16u : kWprN; }
// One row per form: construction, TLS AD bytes, bytes in front of the tag, a full record's fragment.
constexpr bool form_is(RecordForm f, Construction c, uint32_t ad, uint32_t extra, uint32_t fragment) {
    return construction_of(f) == c && tls_ad_len(f) == ad && seal_extra(f) == extra && wpr_len(f, false) == 16384u &&
           wpr_len(f, true) == fragment;
}
// RFC 5246 section 6.2.3.3: AD = seq_num || type || version || length, 8 + 1 + 2 + 2 bytes; records of 2^14
// bytes (section 6.2.1) and a tag; RFC 7905 section 2: the same record under RFC 8439's AEAD
static_assert(form_is(RecordForm::kDraft, Construction::kDraft, 13u, 0u, 16384u + 16u), "the draft's TLS 1.2 record");
static_assert(form_is(RecordForm::kRfc8439, Construction::kRfc8439, 13u, 0u, 16384u + 16u), "RFC 7905");
// RFC 8446 section 5.2: AD = opaque_type || legacy_record_version || length, 1 + 2 + 2 bytes, over
// TLSInnerPlaintext = content || ContentType || zeros (tls13_inner_len below), content of 2^14 bytes (section 5.1);
// seal_extra is the one byte of a seal without padding, which a full record's fragment always is
static_assert(form_is(RecordForm::kTls13, Construction::kRfc8439, 5u, 1u, 16384u + 17u), "RFC 8446 section 5.2");

// Length of the TLSInnerPlaintext that a TLS 1.3 seal builds of `len` content bytes under
// the padding policy pad_to (sg_tls13_seal_opts, RFC 8446 section 5.4): content, the type
// byte, then zeros up to the next multiple of pad_to, but never beyond the 2^14 + 1 bytes
// of section 5.2.  pad_to 0 and 1 pad nothing.  The host (max_n, sg_tls13_inner_len), the
// keying and classify kernels, the size classes and the packed kernel all take it from
// here.  (A length above 2^14, which no call accepts, stays len + 1: over-long, as it was.)
constexpr uint32_t kTls13MaxInner = 16384u + 1u;
constexpr uint32_t tls13_inner_len(uint32_t len, uint32_t pad_to) {
    if (pad_to <= 1u || len >= kTls13MaxInner - 1u) return len + 1u;
    const uint32_t up = (len + pad_to) / pad_to * pad_to;  // len + 1 rounded up
    return up < kTls13MaxInner ? up : kTls13MaxInner;
}
static_assert(tls13_inner_len(0u, 0u) == 1u && tls13_inner_len(16384u, 1u) == 16385u, "no padding: content || type");
static_assert(tls13_inner_len(0u, 64u) == 64u && tls13_inner_len(63u, 64u) == 64u, "type byte in the content's last block");
static_assert(tls13_inner_len(64u, 64u) == 128u, "the type byte opens a block of its own");
static_assert(tls13_inner_len(16384u, 64u) == 16385u && tls13_inner_len(16383u, 16384u) == 16384u, "section 5.2's bound");
static_assert(tls13_inner_len(16320u, 4096u) == 16384u && tls13_inner_len(16383u, 100u) == 16385u, "capped, not rounded");
static_assert(tls13_inner_len(100u, 100u) == 200u && tls13_inner_len(99u, 100u) == 100u, "any pad_to, no power-of-two rule");

}  // namespace sg
