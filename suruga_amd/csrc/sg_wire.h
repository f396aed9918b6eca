// sg_wire.h -- the record layer's wire format (host only, no HIP): the parser
// of a peer's bytes and the framing arithmetic of sg_write_records /
// sg_read_records.  tests/cpp/test_host_san.cpp runs all of it on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/suruga_gpu.h"

namespace sg {

constexpr uint32_t kChunk = 256;  // records per pipeline chunk
// a full record on the wire: every record of a write but the last is full
constexpr size_t kWireRec = SG_HEADER_LEN + SG_RECORD_MAX_LEN + SG_MAC_LEN;

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
    explicit WritePlan(size_t n) : len(n), nrec((n + SG_RECORD_MAX_LEN - 1) / SG_RECORD_MAX_LEN) {}
    uint32_t rec_len(uint64_t r) const {  // plaintext bytes of record r
        const size_t left = len - (size_t)r * SG_RECORD_MAX_LEN;
        return (uint32_t)(left < SG_RECORD_MAX_LEN ? left : SG_RECORD_MAX_LEN);
    }
    size_t wire_off(uint64_t r) const { return (size_t)r * kWireRec; }  // of record r's header
    size_t wire_need() const {  // exact wire bytes (== sg_wire_bound(len))
        return nrec ? wire_off(nrec - 1) + SG_HEADER_LEN + rec_len(nrec - 1) + SG_MAC_LEN : 0;
    }
};

// Explicit-mode nonce and AD of record i of a chunk, for chunks whose records
// do not share type and version: nonce = be64(seq) (tls.rs:250); AD = seq ||
// type || major || minor || be16(len - 16) (tls.rs:252-265).  Layout of `meta`:
// nonces[kChunk][8], then ads[kChunk][13].
constexpr uint32_t kNonceLen = 8, kAdLen = 13;
constexpr uint32_t kMetaBytes = kNonceLen + kAdLen;  // per record
inline void put_explicit_meta(uint8_t* meta, uint32_t i, uint64_t seq, const WireRec& R) {
    put_be64(meta + kNonceLen * i, seq);
    uint8_t* ad = meta + kNonceLen * kChunk + kAdLen * i;
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
};
void chunk_shape(const WireRec* r, uint32_t k, ChunkShape* out);

}  // namespace sg
