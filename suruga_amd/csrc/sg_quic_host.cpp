// sg_quic_host.cpp -- the host-only part of the QUIC packet protection batch: the
// argument rules of sg_seal_batch_quic / sg_open_batch_quic and sg_quic_decode_pn.
// No HIP (tests/cpp/test_quic_san.cpp builds it with g++ under sanitizers); the launch
// is sg_quic_capi.cpp's.
#include "sg_quic.h"

namespace sg {
namespace quic {

const char* check_args(const sg_quic_batch* b, bool open, uint32_t* max_len) {
    if (!b) return "sg_quic_batch is NULL%s";
    static_assert(sizeof(sg_quic_batch) == 152, "sg_quic_batch layout");
    if (b->flags & ~(SG_QUIC_KEY_PHASE | SG_QUIC_KEEP_FAILED)) return "unknown flags in sg_quic_batch%s";
    if (!b->keys || !b->ivs || !b->hp_keys) return "keys, ivs or hp_keys is NULL%s";
    if (!b->status || !b->in || !b->out || !b->pn) return "status, in, out or pn is NULL%s";
    if (open && !b->pn_out) return "open needs pn_out%s";
    if (((uintptr_t)b->ivs | (uintptr_t)b->key_index | (uintptr_t)b->pn_off | (uintptr_t)b->len) & 3u)
        return "ivs, key_index, pn_off and len must be 4-byte aligned%s";
    if (((uintptr_t)b->pn | (uintptr_t)b->pn_out | (uintptr_t)b->in_off | (uintptr_t)b->out_off) & 7u)
        return "pn, pn_out, in_off and out_off must be 8-byte aligned%s";
    if (!b->pn_off && (b->uniform_pn_off < kMinPnOff || b->uniform_pn_off > SG_QUIC_MAX_PN_OFF))
        return "uniform_pn_off outside 1..251%s";
    const uint32_t bound = b->len ? b->max_len : b->uniform_len;
    if (bound > SG_QUIC_MAX_PACKET_LEN - (open ? 0u : SG_MAC_LEN))
        return "packets longer than SG_QUIC_MAX_PACKET_LEN (seal: with the tag)%s";
    if (b->num_keys == 0) return "num_keys is 0%s";
    if ((b->flags & SG_QUIC_KEY_PHASE) && (b->num_keys & 1u)) return "SG_QUIC_KEY_PHASE needs an even num_keys%s";
    if (max_len) *max_len = bound;
    return nullptr;
}

}  // namespace quic
}  // namespace sg

extern "C" uint64_t sg_quic_decode_pn(uint64_t expected_pn, uint32_t truncated, uint32_t pn_len) {
    return sg::quic::decode_pn(expected_pn, truncated, pn_len);
}
