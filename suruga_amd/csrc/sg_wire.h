// sg_wire.h -- the record layer's wire format (host only, no HIP): the parser
// of a peer's bytes and the framing arithmetic of sg_write_records /
// sg_read_records.  tests/cpp/test_host_san.cpp runs all of it on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/suruga_gpu.h"
#include "sg_layout.h"

namespace sg {

constexpr uint32_t kChunk = 256;  // records per pipeline chunk
// The record layer carries one RecordForm (sg_layout.h) from its entry point
// down: kDraft (sg_write_records / sg_read_records), kRfc8439 (the *_rfc7905
// calls: the draft's wire, RFC 8439 under it) and kTls13 (the *_tls13 calls).
// Per form: the bytes a record's fragment adds to its content (the tag, and
// under TLS 1.3 the inner type byte in front of it) ...
constexpr uint32_t frag_extra(RecordForm f) { return seal_extra(f) + SG_MAC_LEN; }
// ... a full record on the wire: every record of a write but the last is full
constexpr size_t wire_rec(RecordForm f) { return SG_HEADER_LEN + SG_RECORD_MAX_LEN + frag_extra(f); }
constexpr size_t kWireRec = wire_rec(RecordForm::kDraft);
static_assert(kWireRec == 16405 && wire_rec(RecordForm::kRfc8439) == 16405 && wire_rec(RecordForm::kTls13) == 16406,
              "wire pitch of a full record");
// ... the parser's largest fragment: tls.rs:35 for the TLS 1.2 forms, RFC 8446
// section 5.2 (2^14 + 256) for TLS 1.3
constexpr uint32_t max_fragment(RecordForm f) {
    return f == RecordForm::kTls13 ? SG_RECORD_MAX_LEN + 256u : SG_ENC_RECORD_MAX_LEN;
}
// ... and the most plaintext a parsed fragment can deliver: everything but the
// tag, and under TLS 1.3 but the inner type byte (a fragment of 16 bytes has
// no inner byte and delivers nothing)
constexpr uint32_t frag_capacity(RecordForm f, uint32_t flen) {
    return flen >= frag_extra(f) ? flen - frag_extra(f) : 0u;
}

struct WireRec {
    size_t off;      // wire offset of the fragment (after the 5-byte header)
    uint32_t flen;   // fragment length (ct || tag)
    uint8_t type, major, minor;
};

// The complete records at the start of `wire` (at most max_records), header
// checks in TlsReader::read_record's order (tls.rs:217-238, 258-262, 269-272).
// Returns SG_OK when parsing stopped at the end of the complete records (or at
// max_records), else the error of the first bad header; `recs` holds the
// records before it.  Reads no byte outside [wire, wire + wire_len).
int32_t parse_wire(const uint8_t* wire, size_t wire_len, size_t max_records, std::vector<WireRec>& recs);
// The same for TLS 1.3 (RFC 8446 section 5.1, 5.2), checks in this order: outer
// type other than 23 -> SG_E_UNEXPECTED_MESSAGE, length above 2^14 + 256 ->
// SG_E_RECORD_OVERFLOW, length below 16 -> SG_E_SHORT.  The version bytes are
// recorded, not checked (the AD is built as 17 03 03, so others fail the tag).
int32_t parse_wire_tls13(const uint8_t* wire, size_t wire_len, size_t max_records, std::vector<WireRec>& recs);
inline int32_t parse_wire(RecordForm f, const uint8_t* wire, size_t wire_len, size_t max_records,
                          std::vector<WireRec>& recs) {
    return f == RecordForm::kTls13 ? parse_wire_tls13(wire, wire_len, max_records, recs)
                                   : parse_wire(wire, wire_len, max_records, recs);
}

inline void put_be16(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
}
// four bytes at any alignment -> little-endian word
inline uint32_t get_le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
inline void put_be64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (56 - 8 * i));
}
// the 5-byte record header (tls.rs:126-130): type, version, be16(fragment length)
inline void put_header(uint8_t* h, uint8_t type, uint8_t major, uint8_t minor, uint32_t flen) {
    h[0] = type;
    h[1] = major;
    h[2] = minor;
    put_be16(h + 3, flen);
}

// The writer's plan for `len` plaintext bytes (tls.rs:137-147: 2^14-byte
// fragments, the last one short).
struct WritePlan {
    size_t len;
    uint64_t nrec;
    RecordForm form;
    explicit WritePlan(size_t n, RecordForm f = RecordForm::kDraft)
        : len(n), nrec((n + SG_RECORD_MAX_LEN - 1) / SG_RECORD_MAX_LEN), form(f) {}
    uint32_t rec_len(uint64_t r) const {  // plaintext bytes of record r
        const size_t left = len - (size_t)r * SG_RECORD_MAX_LEN;
        return (uint32_t)(left < SG_RECORD_MAX_LEN ? left : SG_RECORD_MAX_LEN);
    }
    uint32_t frag_len(uint64_t r) const { return rec_len(r) + frag_extra(form); }  // its fragment on the wire
    size_t wire_off(uint64_t r) const { return (size_t)r * wire_rec(form); }       // of record r's header
    size_t wire_need() const {  // exact wire bytes (== sg_wire_bound(len) / sg_wire_bound_tls13(len))
        return nrec ? wire_off(nrec - 1) + SG_HEADER_LEN + frag_len(nrec - 1) : 0;
    }
};

// Explicit-mode nonce and AD of record i of a chunk, for chunks whose records
// do not share type and version: nonce = be64(seq) (tls.rs:250); AD = seq ||
// type || major || minor || be16(len - 16) (tls.rs:252-265).  Layout of `meta`:
// nonces[kChunk][8], then ads[kChunk][13].
// RFC 7905 (form kRfc8439): nonces[kChunk][12], nonce = iv XOR (0^4 || be64(seq)),
// then the same ads.
constexpr uint32_t kNonceLen = 8, kAdLen = 13;
constexpr uint32_t explicit_nonce_len(RecordForm f) { return f == RecordForm::kDraft ? kNonceLen : 12u; }
constexpr uint32_t kMetaBytes = kNonceLen + kAdLen;  // per record, the draft
constexpr uint32_t kMetaBytesMax = 12u + kAdLen;     // per record, the larger form: what a slot pins
inline void put_explicit_meta(uint8_t* meta, uint32_t i, uint64_t seq, const WireRec& R,
                              RecordForm f = RecordForm::kDraft, const uint8_t* iv = nullptr) {
    const uint32_t nl = explicit_nonce_len(f);
    if (f == RecordForm::kDraft) {
        put_be64(meta + nl * i, seq);
    } else {
        uint8_t* n = meta + nl * i;
        for (int k = 0; k < 4; ++k) n[k] = iv[k];
        put_be64(n + 4, seq);
        for (int k = 4; k < 12; ++k) n[k] ^= iv[k];
    }
    uint8_t* ad = meta + nl * kChunk + kAdLen * i;
    put_be64(ad, seq);
    ad[8] = R.type;
    ad[9] = R.major;
    ad[10] = R.minor;
    put_be16(ad + 11, R.flen - SG_MAC_LEN);
}

// The shape of a chunk of k <= kChunk parsed records (k >= 1).
struct ChunkShape {
    bool same;      // every fragment has the first one's length
    bool tls;       // every record has the first one's type and version
    bool dense;     // the records lie back to back at the first one's pitch
    uint32_t flen;  // the first fragment's length (the uniform one when `same`)
    uint32_t pre[kChunk + 1];  // plaintext bytes before record i of the chunk; pre[k]: all of them
                               // (TLS 1.3: the most there can be, frag_capacity -- the content
                               // lengths exist only after the open)
};
void chunk_shape(const WireRec* r, uint32_t k, ChunkShape* out, RecordForm f = RecordForm::kDraft);

}  // namespace sg
