// sg_dtls13.h -- what the DTLS 1.3 record batch (sg_*_batch_dtls13, RFC 9147 section 4)
// shares between its kernel (sg_dtls13.hip), its entry points (sg_dtls13_capi.cpp) and the
// host-only code (sg_dtls13_host.cpp): the unified header's length, the inner plaintext's
// length with its padding, the argument rules and the kernel's parameters.  The geometry
// of a record's MAC over the lanes of its group is sg_quic.h's (Geom, lanes_for), with the
// header as the additional data in the slot in front of chunk 0, and the sequence number
// is rebuilt with sg_quic.h's decode_pn at one or two bytes.
// No HIP: plain constexpr functions, which hipcc takes as host and device code, so the
// host-only programs (tests/cpp/test_dtls13_san.cpp) include it too.  Not part of the public ABI.
#pragma once

#include <stdint.h>

#include "../../include/suruga_gpu.h"
#include "sg_quic.h"

namespace sg {
namespace dtls13 {

// the first byte: 0 0 1 C S L E E
constexpr uint32_t kFixedMask = 0xe0u, kFixed = 0x20u, kC = 0x10u, kS = 0x08u, kL = 0x04u, kEpochMask = 0x03u;
constexpr uint32_t kMaxInner = SG_DTLS13_MAX_CONTENT_LEN + 1u;  // content and type byte; padding never goes beyond it
constexpr uint32_t kMaxPadTo = 1u << 14;

// the unified header's length from its first byte's S and L bits
constexpr uint32_t header_len_bits(uint32_t b0, uint32_t cid_len) {
    return 1u + cid_len + ((b0 & kS) ? 2u : 1u) + ((b0 & kL) ? 2u : 0u);
}
// ... and from a seal's flags
constexpr uint32_t first_byte(uint32_t flags, uint32_t cid_len, uint32_t epoch) {
    return kFixed | (cid_len ? kC : 0u) | ((flags & SG_DTLS13_SEQ16) ? kS : 0u) | ((flags & SG_DTLS13_LENGTH) ? kL : 0u) |
           (epoch & kEpochMask);
}
constexpr uint32_t header_len(uint32_t flags, uint32_t cid_len) {
    const uint64_t h = 1ull + cid_len + ((flags & SG_DTLS13_SEQ16) ? 2u : 1u) + ((flags & SG_DTLS13_LENGTH) ? 2u : 0u);
    return h > 0xffffffffull ? 0xffffffffu : (uint32_t)h;
}
// The inner plaintext of a content of len bytes: content, type byte, and under pad_to > 1
// zeros up to a multiple of pad_to, but to no more than 2^14 + 1 bytes in all (a content
// of 2^14 bytes or more is not padded).  0xffffffff where 32 bits do not hold it.
constexpr uint32_t inner_len(uint32_t len, uint32_t pad_to) {
    const uint64_t base = (uint64_t)len + 1u;
    if (base > 0xffffffffull) return 0xffffffffu;
    if (pad_to <= 1u || base >= kMaxInner) return (uint32_t)base;
    const uint64_t up = (base + pad_to - 1u) / pad_to * pad_to;
    return (uint32_t)(up < kMaxInner ? up : kMaxInner);
}
constexpr uint32_t record_len(uint32_t len, uint32_t pad_to, uint32_t flags, uint32_t cid_len) {
    const uint64_t r = (uint64_t)header_len(flags, cid_len) + inner_len(len, pad_to) + SG_MAC_LEN;
    return r > 0xffffffffull ? 0xffffffffu : (uint32_t)r;
}
static_assert(header_len(0u, 0u) == 2u && header_len(SG_DTLS13_SEQ16 | SG_DTLS13_LENGTH, 0u) == 5u, "minimal and full header, no CID");
static_assert(header_len(SG_DTLS13_SEQ16 | SG_DTLS13_LENGTH, 11u) == 16u && header_len(SG_DTLS13_SEQ16 | SG_DTLS13_LENGTH, 12u) == 17u,
              "one and two MAC blocks of additional data");
static_assert(header_len(SG_DTLS13_SEQ16 | SG_DTLS13_LENGTH, SG_DTLS13_MAX_CID_LEN) == SG_MAX_AD_LEN, "the longest header is the longest AD");
static_assert(header_len_bits(first_byte(SG_DTLS13_SEQ16, 3u, 6u), 3u) == header_len(SG_DTLS13_SEQ16, 3u), "both ways agree");
static_assert(first_byte(SG_DTLS13_SEQ16 | SG_DTLS13_LENGTH, 1u, 7u) == 0x3fu && first_byte(0u, 0u, 4u) == 0x20u, "epoch mod 4");
static_assert(inner_len(0u, 0u) == 1u && inner_len(0u, 16u) == 16u && inner_len(15u, 16u) == 16u && inner_len(16u, 16u) == 32u, "type byte, then padding");
static_assert(inner_len(16383u, 256u) == 16384u && inner_len(16384u, 256u) == 16385u && inner_len(10000u, 10000u) == 16385u, "the cap at 2^14 + 1");
static_assert(inner_len(16385u, 256u) == 16386u && inner_len(0xffffffffu, 0u) == 0xffffffffu && inner_len(0xfffffffeu, 64u) == 0xffffffffu, "nothing wraps");
static_assert(record_len(SG_DTLS13_MAX_CONTENT_LEN, 0u, SG_DTLS13_SEQ16 | SG_DTLS13_LENGTH, SG_DTLS13_MAX_CID_LEN) == SG_DTLS13_MAX_RECORD_LEN,
              "the longest record");
static_assert(record_len(0xfffffff0u, 0u, 0u, 0u) == 0xffffffffu, "nothing wraps");

// What sg_seal_batch_dtls13 / sg_open_batch_dtls13 reject before any GPU work: the message,
// or NULL for a batch that may run.  *max_len receives the largest len_i the call processes.
const char* check_args(const sg_dtls13_batch* b, bool open, uint32_t* max_len);

// Kernel parameters (by value as kernarg): sg_dtls13_batch without the stream, the flags taken apart.
struct Params {
    const uint8_t* keys;
    const uint8_t* ivs;
    const uint8_t* sn_keys;
    const uint8_t* cids;
    const uint32_t* key_index;
    const uint64_t* seq;
    const uint8_t* type;
    const uint8_t* epoch;
    const uint64_t* expected;
    uint64_t* seq_out;
    uint8_t* epoch_out;
    uint32_t* content_len;
    uint8_t* type_out;
    const uint8_t* in;
    const uint64_t* in_off;
    uint64_t in_stride;
    uint8_t* out;
    const uint64_t* out_off;
    uint64_t out_stride;
    const uint32_t* len;
    uint8_t* status;
    uint32_t count;
    uint32_t num_conns, cid_len, pad_to;
    uint32_t uniform_type, uniform_epoch;
    uint32_t seal_bits;    // seal: S and L of the first byte, from SG_DTLS13_SEQ16 / SG_DTLS13_LENGTH
    uint32_t epoch_rows;   // 1 = SG_DTLS13_EPOCH_ROWS
    uint32_t keep_failed;  // 1 = SG_DTLS13_KEEP_FAILED
    uint32_t uniform_len, max_len;
};
// One launch of sg_dtls13_kernel<open, quic::lanes_for(p.max_len)> on `stream` (a hipStream_t);
// the hipError_t as an int.  count >= 1.
int launch(const Params& p, bool open, void* stream);

}  // namespace dtls13
}  // namespace sg
