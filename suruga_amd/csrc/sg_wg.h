// sg_wg.h -- what the WireGuard transport data batch (sg_*_batch_wg, whitepaper section
// 5.4.6) shares between its kernel (sg_wg.hip), its entry points (sg_wg_capi.cpp) and the
// host-only code (sg_wg_host.cpp): the padded length, the argument rules and the kernel's
// parameters.  The geometry of a packet's MAC over the lanes of its group is sg_quic.h's
// (Geom, lanes_for), with the additional data's slot contributing nothing.
// No HIP: plain constexpr functions, which hipcc takes as host and device code, so the
// host-only programs (tests/cpp/test_wg_san.cpp) include it too.  Not part of the public ABI.
#pragma once

#include <stdint.h>

#include "../../include/suruga_gpu.h"
#include "sg_quic.h"

namespace sg {
namespace wg {

constexpr uint32_t kOverhead = SG_WG_HEADER_LEN + SG_MAC_LEN;  // 32: a message without its payload
constexpr uint32_t kMaxInner = SG_WG_MAX_MESSAGE_LEN - kOverhead;

// The AEAD's plaintext length of an inner packet of len bytes: len rounded up to 16, and
// with a pad_cap at most max(len, pad_cap) -- min(MTU, ALIGN(len, 16)) for len <= MTU.
// Never less than len, less than 16 more; a rounding beyond 32 bits leaves len as it is.
constexpr uint32_t padded_len(uint32_t len, uint32_t pad_cap) {
    const uint64_t up = ((uint64_t)len + 15u) & ~15ull;
    const uint64_t cap = len > pad_cap ? len : pad_cap;
    const uint64_t p = (pad_cap != 0u && up > cap) ? cap : up;
    return p > 0xffffffffull ? len : (uint32_t)p;
}
constexpr uint32_t message_len(uint32_t len, uint32_t pad_cap) {
    const uint32_t p = padded_len(len, pad_cap);
    return p > 0xffffffffu - kOverhead ? 0xffffffffu : p + kOverhead;
}
static_assert(padded_len(0u, 0u) == 0u && padded_len(1u, 0u) == 16u && padded_len(16u, 0u) == 16u, "rounded up to 16");
static_assert(padded_len(1419u, 1420u) == 1420u && padded_len(1420u, 1420u) == 1420u, "a ragged cap");
static_assert(padded_len(1421u, 1420u) == 1421u && padded_len(1405u, 1420u) == 1408u, "never below len, never above the rounding");
static_assert(padded_len(0xfffffff1u, 0u) == 0xfffffff1u && message_len(0xffffffe0u, 0u) == 0xffffffffu, "nothing wraps");
static_assert(message_len(0u, 0u) == 32u && message_len(1500u, 1500u) == 1532u, "header and tag");

// What sg_seal_batch_wg / sg_open_batch_wg reject before any GPU work: the message, or
// NULL for a batch that may run.  *max_len receives the largest len_i the call processes.
const char* check_args(const sg_wg_batch* b, bool open, uint32_t* max_len);

// Kernel parameters (by value as kernarg): sg_wg_batch without the stream, the flags taken apart.
struct Params {
    const uint8_t* keys;
    const uint32_t* receiver;
    const uint32_t* key_index;
    const uint64_t* counter;
    uint64_t* counter_out;
    uint32_t* inner_len;
    const uint8_t* in;
    const uint64_t* in_off;
    uint64_t in_stride;
    uint8_t* out;
    const uint64_t* out_off;
    uint64_t out_stride;
    const uint32_t* len;
    uint8_t* status;
    uint32_t count;
    uint32_t num_keys;
    uint32_t pad_cap;
    uint32_t keep_failed;  // 1 = SG_WG_KEEP_FAILED
    uint32_t uniform_len, max_len;
};
// One launch of sg_wg_kernel<open, quic::lanes_for(p.max_len)> on `stream` (a hipStream_t);
// the hipError_t as an int.  count >= 1.
int launch(const Params& p, bool open, void* stream);

}  // namespace wg
}  // namespace sg
