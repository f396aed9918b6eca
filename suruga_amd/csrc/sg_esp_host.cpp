// sg_esp_host.cpp -- the host-only part of the IPsec ESP batch: the argument rules of
// sg_seal_batch_esp / sg_open_batch_esp, sg_esp_padded_len, sg_esp_packet_len and
// sg_esp_seq_hi.  No HIP (tests/cpp/test_esp_san.cpp builds it with g++ under
// sanitizers); the launch is sg_esp_capi.cpp's.
#include "sg_esp.h"

namespace sg {
namespace esp {

const char* check_args(const sg_esp_batch* b, bool open, uint32_t* max_len) {
    if (!b) return "sg_esp_batch is NULL%s";
    static_assert(sizeof(sg_esp_batch) == 192, "sg_esp_batch layout");
    if (b->flags & ~(SG_ESP_ESN | SG_ESP_KEEP_FAILED)) return "unknown flags in sg_esp_batch%s";
    if (!b->keys || !b->salts || !b->spi || !b->status || !b->in || !b->out)
        return "keys, salts, spi, status, in or out is NULL%s";
    if (!open && !b->seq) return "seal needs seq%s";
    if (open && !b->seq_out) return "open needs seq_out%s";
    if (open && (b->payload_len == nullptr) != (b->next_header_out == nullptr))
        return "payload_len and next_header_out go together%s";
    if (open && (b->flags & SG_ESP_ESN)) {
        if (!b->replay_top) return "open under SG_ESP_ESN needs replay_top%s";
        if (b->window < 1u || b->window > kMaxWindow) return "window outside 1..2^31%s";
    }
    if (((uintptr_t)b->salts | (uintptr_t)b->spi | (uintptr_t)b->sa_index | (uintptr_t)b->payload_len | (uintptr_t)b->len) & 3u)
        return "salts, spi, sa_index, payload_len and len must be 4-byte aligned%s";
    if (((uintptr_t)b->seq | (uintptr_t)b->iv | (uintptr_t)b->seq_out | (uintptr_t)b->replay_top | (uintptr_t)b->in_off |
         (uintptr_t)b->out_off) & 7u)
        return "seq, iv, seq_out, replay_top, in_off and out_off must be 8-byte aligned%s";
    if (b->num_sas == 0) return "num_sas is 0%s";
    if (b->align < kMinAlign || b->align > kMaxAlign || (b->align & 3u)) return "align is no multiple of 4 in 4..256%s";
    if (b->uniform_next_header > 255u) return "uniform_next_header above 255%s";
    const uint32_t bound = b->len ? b->max_len : b->uniform_len;
    // seal: the bound is on P, which grows with the payload: no packet longer than SG_ESP_MAX_PACKET_LEN is written
    if ((open ? bound : packet_len(bound, b->align)) > SG_ESP_MAX_PACKET_LEN)
        return "packets longer than SG_ESP_MAX_PACKET_LEN (seal: with padding, trailer, header and ICV)%s";
    if (max_len) *max_len = bound;
    return nullptr;
}

}  // namespace esp
}  // namespace sg

extern "C" {

uint32_t sg_esp_padded_len(uint32_t len, uint32_t align) { return sg::esp::padded_len(len, align); }
uint32_t sg_esp_packet_len(uint32_t len, uint32_t align) { return sg::esp::packet_len(len, align); }
uint32_t sg_esp_seq_hi(uint64_t top, uint32_t window, uint32_t seq_lo) { return sg::esp::seq_hi(top, window, seq_lo); }

}  // extern "C"
