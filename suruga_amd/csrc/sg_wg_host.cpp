// sg_wg_host.cpp -- the host-only part of the WireGuard transport data batch: the
// argument rules of sg_seal_batch_wg / sg_open_batch_wg, sg_wg_padded_len and
// sg_wg_message_len.  No HIP (tests/cpp/test_wg_san.cpp builds it with g++ under
// sanitizers); the launch is sg_wg_capi.cpp's.
#include "sg_wg.h"

namespace sg {
namespace wg {

const char* check_args(const sg_wg_batch* b, bool open, uint32_t* max_len) {
    if (!b) return "sg_wg_batch is NULL%s";
    static_assert(sizeof(sg_wg_batch) == 144, "sg_wg_batch layout");
    if (b->flags & ~SG_WG_KEEP_FAILED) return "unknown flags in sg_wg_batch%s";
    if (!b->keys || !b->status || !b->in || !b->out) return "keys, status, in or out is NULL%s";
    if (!open && (!b->receiver || !b->counter)) return "seal needs receiver and counter%s";
    if (open && !b->counter_out) return "open needs counter_out%s";
    if (((uintptr_t)b->receiver | (uintptr_t)b->key_index | (uintptr_t)b->inner_len | (uintptr_t)b->len) & 3u)
        return "receiver, key_index, inner_len and len must be 4-byte aligned%s";
    if (((uintptr_t)b->counter | (uintptr_t)b->counter_out | (uintptr_t)b->in_off | (uintptr_t)b->out_off) & 7u)
        return "counter, counter_out, in_off and out_off must be 8-byte aligned%s";
    if (b->num_keys == 0) return "num_keys is 0%s";
    if (b->pad_cap > kMaxInner) return "pad_cap above SG_WG_MAX_MESSAGE_LEN - 32%s";
    const uint32_t bound = b->len ? b->max_len : b->uniform_len;
    if (bound > (open ? SG_WG_MAX_MESSAGE_LEN : kMaxInner))
        return "packets longer than SG_WG_MAX_MESSAGE_LEN (seal: with header and tag)%s";
    if (max_len) *max_len = bound;
    return nullptr;
}

}  // namespace wg
}  // namespace sg

extern "C" {

uint32_t sg_wg_padded_len(uint32_t len, uint32_t pad_cap) { return sg::wg::padded_len(len, pad_cap); }
uint32_t sg_wg_message_len(uint32_t len, uint32_t pad_cap) { return sg::wg::message_len(len, pad_cap); }

}  // extern "C"
