// sg_quic.h -- what the QUIC packet protection batch (sg_*_batch_quic, RFC 9001 section 5)
// shares between its kernel (sg_quic.hip), its entry points (sg_quic_capi.cpp) and the
// host-only code (sg_quic_host.cpp): the packet-number decoding of RFC 9000 appendix A.3,
// the geometry of a packet's MAC over the lanes of its group, and the argument rules.
// No HIP: plain constexpr functions, which hipcc takes as host and device code, so the
// host-only programs (tests/cpp/test_quic_san.cpp) include it too.  Not part of the public ABI.
#pragma once

#include <stdint.h>

#include "../../include/suruga_gpu.h"

namespace sg {
namespace quic {

// RFC 9000 appendix A.3, DecodePacketNumber, with expected_pn = largest_pn + 1 as the
// argument.  pn_len outside 1..4 is taken into that range and `truncated` is cut to
// 8 * pn_len bits; the comparisons are written so that nothing wraps for expected_pn
// below 2^63 (packet numbers end at 2^62 - 1).
constexpr uint64_t decode_pn(uint64_t expected_pn, uint32_t truncated, uint32_t pn_len) {
    const uint32_t nbytes = pn_len < 1u ? 1u : pn_len > 4u ? 4u : pn_len;
    const uint64_t win = 1ull << (8u * nbytes), hwin = win >> 1, mask = win - 1u;
    const uint64_t cand = (expected_pn & ~mask) | ((uint64_t)truncated & mask);
    if (cand + hwin <= expected_pn && cand < (1ull << 62) - win) return cand + win;
    if (cand > expected_pn + hwin && cand >= win) return cand - win;
    return cand;
}
// the example of A.3: largest 0xa82f30ea, two bytes 0x9b32
static_assert(decode_pn(0xa82f30eaull + 1u, 0x9b32u, 2u) == 0xa82f9b32ull, "RFC 9000 A.3");
static_assert(decode_pn(0u, 0xffu, 1u) == 0xffull, "nothing below zero");
static_assert(decode_pn(0x100u, 0x7fu, 1u) == 0x17full && decode_pn(0x100u, 0x81u, 1u) == 0x81ull, "one byte, both sides");
static_assert(decode_pn(0x180u, 0x00u, 1u) == 0x200ull && decode_pn(0x17fu, 0x00u, 1u) == 0x100ull, "the lower edge");
static_assert(decode_pn((1ull << 62) - 1u, 0x00u, 1u) == (1ull << 62) - 256u, "never 2^62 or above");
static_assert(decode_pn(0x123456789ull, 0x23456790u, 4u) == 0x123456790ull, "four bytes");

// ---- a packet over the G lanes of its group --------------------------------------
// The payload (n bytes, ChaCha20 blocks 1 onward) is NF = n / 64 whole 64-byte chunks
// and a tail of n % 64 bytes.  With Q = ceil((NF + 1) / G) slots per lane the chunks are
// laid right-aligned over the G * Q slots: slot v = t * Q + q of lane t holds chunk
// v - zc, zc = G * Q - NF >= 1, or nothing where that is negative.  Every lane runs
// Poly1305 over its own 4 Q blocks from 0, so that with P = r^(4 Q)
//   sum_t H_t P^(G - 1 - t)
// is the accumulator behind the last whole chunk; the additional data's own sum enters
// as the value of the slot in front of chunk 0 (slot zc - 1), and slot 0, which never
// holds a chunk, takes the tail: its keystream block, its up to four MAC blocks and the
// length block, TS.  The tag's accumulator is then S r^(kt + 1) + TS, kt = ceil((n % 64) / 16).
struct Geom {
    uint32_t nf, q, zc, tail, kt;
};
constexpr Geom geom(uint32_t n, uint32_t G) {
    const uint32_t nf = n / 64u, q = (nf + 1u + G - 1u) / G, tail = n % 64u;
    return Geom{nf, q, G * q - nf, tail, (tail + 15u) / 16u};
}
static_assert(geom(0u, 16u).q == 1u && geom(0u, 16u).zc == 16u && geom(0u, 16u).kt == 0u, "an empty payload");
static_assert(geom(15u * 64u, 16u).q == 1u && geom(15u * 64u, 16u).zc == 1u, "fifteen chunks and the tail slot");
static_assert(geom(16u * 64u, 16u).q == 2u && geom(16u * 64u, 16u).zc == 16u, "sixteen chunks need a second slot");
static_assert(geom(1431u, 8u).q == 3u && geom(1431u, 8u).zc == 2u && geom(1431u, 8u).kt == 2u, "a 1,431-byte payload");

// lanes per packet of a call: 8 where no packet exceeds 2 KiB (at most four slots a lane), else 16
constexpr uint32_t kSmallMax = 2048u;
constexpr uint32_t lanes_for(uint32_t max_len) { return max_len <= kSmallMax ? 8u : 16u; }

constexpr uint32_t kMinPnOff = 1u;
constexpr uint32_t kSampleEnd = 20u;  // open: the sample ends pn_off + 4 + 16 bytes into the packet

// What sg_seal_batch_quic / sg_open_batch_quic reject before any GPU work: the message, or
// NULL for a batch that may run.  *max_len receives the largest len_i the call processes.
const char* check_args(const sg_quic_batch* b, bool open, uint32_t* max_len);

// Kernel parameters (by value as kernarg): sg_quic_batch without the stream, the flags taken apart.
struct Params {
    const uint8_t* keys;
    const uint8_t* ivs;
    const uint8_t* hp_keys;
    const uint32_t* key_index;
    const uint64_t* pn;
    uint64_t* pn_out;
    const uint32_t* pn_off;
    const uint8_t* in;
    const uint64_t* in_off;
    uint64_t in_stride;
    uint8_t* out;
    const uint64_t* out_off;
    uint64_t out_stride;
    const uint32_t* len;
    uint8_t* status;
    uint32_t count;
    uint32_t rows;         // connections: num_keys, or num_keys / 2 under key_phase
    uint32_t key_phase;    // 1 = SG_QUIC_KEY_PHASE
    uint32_t keep_failed;  // 1 = SG_QUIC_KEEP_FAILED
    uint32_t uniform_pn_off, uniform_len, max_len;
};
// One launch of sg_quic_kernel<open, lanes_for(p.max_len)> on `stream` (a hipStream_t);
// the hipError_t as an int.  count >= 1.
int launch(const Params& p, bool open, void* stream);

}  // namespace quic
}  // namespace sg
