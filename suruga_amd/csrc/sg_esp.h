// sg_esp.h -- what the IPsec ESP batch (sg_*_batch_esp, RFC 7634 over RFC 4303) shares
// between its kernel (sg_esp.hip), its entry points (sg_esp_capi.cpp) and the host-only
// code (sg_esp_host.cpp): the padded length, the extended sequence number's high half (RFC
// 4303 appendix A2.1), the argument rules and the kernel's parameters.  The geometry of a
// packet's MAC over the lanes of its group is sg_quic.h's (Geom, lanes_for), with the
// 8- or 12-byte additional data in the slot in front of chunk 0.
// No HIP: plain constexpr functions, which hipcc takes as host and device code, so the
// host-only programs (tests/cpp/test_esp_san.cpp) include it too.  Not part of the public ABI.
#pragma once

#include <stdint.h>

#include "../../include/suruga_gpu.h"
#include "sg_quic.h"

namespace sg {
namespace esp {

constexpr uint32_t kOverhead = SG_ESP_HEADER_LEN + SG_MAC_LEN;  // 32: a packet without its ciphertext
constexpr uint32_t kTrailer = 2u;                               // pad length and next header
constexpr uint32_t kMinPacket = kOverhead + kTrailer;           // open: no trailer fits below it
constexpr uint32_t kMinAlign = 4u, kMaxAlign = 256u;
constexpr uint32_t kMaxWindow = 0x80000000u;

// the padding bytes behind a payload of len bytes: payload, padding and the two trailer
// bytes end on a multiple of align (0 is taken as 1); below align, whatever len is
constexpr uint32_t pad_len(uint32_t len, uint32_t align) {
    const uint64_t a = align ? align : 1u;
    return (uint32_t)((a - ((uint64_t)len + kTrailer) % a) % a);
}
// The AEAD's plaintext length P of a payload, and the packet's; 0xffffffff where 32 bits do not hold it.
constexpr uint32_t padded_len(uint32_t len, uint32_t align) {
    const uint64_t p = (uint64_t)len + pad_len(len, align) + kTrailer;
    return p > 0xffffffffull ? 0xffffffffu : (uint32_t)p;
}
constexpr uint32_t packet_len(uint32_t len, uint32_t align) {
    const uint32_t p = padded_len(len, align);
    return p > 0xffffffffu - kOverhead ? 0xffffffffu : p + kOverhead;
}
static_assert(padded_len(0u, 4u) == 4u && padded_len(2u, 4u) == 4u && padded_len(3u, 4u) == 8u, "trailer included, rounded up to align");
static_assert(pad_len(0u, 256u) == 254u && pad_len(255u, 256u) == 255u && pad_len(254u, 256u) == 0u, "pad 0 .. align - 1");
static_assert(padded_len(84u, 4u) == 88u && packet_len(84u, 4u) == 120u, "RFC 7634 appendix A: 84 bytes, pad 2");
static_assert(packet_len(16350u, 4u) == SG_ESP_MAX_PACKET_LEN && packet_len(16350u, 16u) == SG_ESP_MAX_PACKET_LEN, "the largest payload");
static_assert(padded_len(0xfffffffdu, 4u) == 0xffffffffu && padded_len(0xfffffffau, 4u) == 0xfffffffcu, "nothing wraps");
static_assert(packet_len(0xffffffdau, 4u) == 0xfffffffcu && packet_len(0xffffffdbu, 4u) == 0xffffffffu, "nothing wraps");
static_assert(padded_len(7u, 0u) == 9u && padded_len(7u, 1u) == 9u, "align 0 as 1");

// RFC 4303 appendix A2.1: the high half of a received sequence number whose low half is
// seq_lo, given the top T = top (Th, Tl) of the receiver's window of W = window numbers.
// With Bl = Tl - W + 1: where the window lies inside one 2^32 subspace (Tl >= W - 1) a
// seq_lo below Bl belongs to the next subspace, and where it spans two a seq_lo at or above
// Bl belongs to the one before.  All arithmetic mod 2^32, as Linux xfrm_replay_seqhi: the
// result is the one 64-bit number with these low bits in [T - W + 1, T - W + 1 + 2^32),
// taken mod 2^64 -- a wrapped guess fails its ICV.
constexpr uint32_t seq_hi(uint64_t top, uint32_t window, uint32_t seq_lo) {
    const uint32_t th = (uint32_t)(top >> 32), tl = (uint32_t)top;
    const uint32_t bl = tl - window + 1u;
    if (tl >= window - 1u) return seq_lo < bl ? th + 1u : th;
    return seq_lo >= bl ? th - 1u : th;
}
static_assert(seq_hi(0x0000000500000064ull, 64u, 100u) == 5u && seq_hi(0x0000000500000064ull, 64u, 37u) == 5u, "inside the window");
static_assert(seq_hi(0x0000000500000064ull, 64u, 36u) == 6u && seq_hi(0x0000000500000064ull, 64u, 101u) == 5u, "below Bl: the next subspace");
static_assert(seq_hi(0x0000000500000005ull, 64u, 0xffffffc6u) == 4u && seq_hi(0x0000000500000005ull, 64u, 0xffffffc5u) == 5u, "a window over two subspaces");
static_assert(seq_hi(0x000000050000003eull, 64u, 0xffffffffu) == 4u && seq_hi(0x000000050000003full, 64u, 0xffffffffu) == 5u, "Tl at W - 2 and W - 1");
static_assert(seq_hi(0x00000000ffffffffull, 1u, 0xfffffffeu) == 1u && seq_hi(0x00000000ffffffffull, 1u, 0xffffffffu) == 0u, "W = 1");
static_assert(seq_hi(5ull, 64u, 0xffffffc6u) == 0xffffffffu, "Th = 0, behind the start: wraps, and fails its ICV");
static_assert(seq_hi(0xffffffff00000064ull, 64u, 0u) == 0u, "Th + 1 wraps");
static_assert(seq_hi(0x000000057fffffffull, kMaxWindow, 0u) == 5u && seq_hi(0x000000057ffffffeull, kMaxWindow, 0xffffffffu) == 4u, "W = 2^31");

// What sg_seal_batch_esp / sg_open_batch_esp reject before any GPU work: the message, or
// NULL for a batch that may run.  *max_len receives the largest len_i the call processes.
const char* check_args(const sg_esp_batch* b, bool open, uint32_t* max_len);

// Kernel parameters (by value as kernarg): sg_esp_batch without the stream, the flags taken apart.
struct Params {
    const uint8_t* keys;
    const uint32_t* salts;  // a row's four bytes as they lie: state word 13
    const uint32_t* spi;
    const uint32_t* sa_index;
    const uint64_t* seq;
    const uint64_t* iv;
    const uint8_t* next_header;
    uint64_t* seq_out;
    uint32_t* payload_len;
    uint8_t* next_header_out;
    const uint64_t* replay_top;
    const uint8_t* in;
    const uint64_t* in_off;
    uint64_t in_stride;
    uint8_t* out;
    const uint64_t* out_off;
    uint64_t out_stride;
    const uint32_t* len;
    uint8_t* status;
    uint32_t count;
    uint32_t num_sas;
    uint32_t align;
    uint32_t uniform_next_header, window;
    uint32_t esn;          // 1 = SG_ESP_ESN
    uint32_t keep_failed;  // 1 = SG_ESP_KEEP_FAILED
    uint32_t uniform_len, max_len;
};
// One launch of sg_esp_kernel<open, quic::lanes_for(p.max_len)> on `stream` (a hipStream_t);
// the hipError_t as an int.  count >= 1.
int launch(const Params& p, bool open, void* stream);

}  // namespace esp
}  // namespace sg
