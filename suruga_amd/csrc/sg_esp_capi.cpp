// sg_esp_capi.cpp -- the IPsec ESP entry points of include/suruga_gpu.h
// (sg_seal_batch_esp / sg_open_batch_esp).  Host-side glue only: the argument rules
// (sg_esp_host.cpp's check_args, all of them before the first GPU call) and the one
// launch of sg_esp.hip.  No workspace and nothing read back, so a call on a capturing
// stream records exactly that launch.  There is no CPU path.
#include <hip/hip_runtime.h>

#include "../../include/suruga_gpu.h"
#include "sg_esp.h"
#include "sg_host.h"

namespace {

int esp_batch(const sg_esp_batch* b, bool open) {
    uint32_t max_len = 0;
    if (const char* why = sg::esp::check_args(b, open, &max_len)) return sg::fail(SG_E_ARG, why);
    if (b->count == 0) return SG_OK;
    sg::esp::Params p{};
    p.keys = b->keys;
    p.salts = reinterpret_cast<const uint32_t*>(b->salts);
    p.spi = b->spi;
    p.sa_index = b->sa_index;
    p.seq = b->seq;
    p.iv = b->iv;
    p.next_header = b->next_header;
    p.seq_out = b->seq_out;
    p.payload_len = b->payload_len;
    p.next_header_out = b->next_header_out;
    p.replay_top = b->replay_top;
    p.in = b->in;
    p.in_off = b->in_off;
    p.in_stride = b->in_stride;
    p.out = b->out;
    p.out_off = b->out_off;
    p.out_stride = b->out_stride;
    p.len = b->len;
    p.status = b->status;
    p.count = b->count;
    p.num_sas = b->num_sas;
    p.align = b->align;
    p.uniform_next_header = b->uniform_next_header;
    p.window = b->window;
    p.esn = (b->flags & SG_ESP_ESN) ? 1u : 0u;
    p.keep_failed = (b->flags & SG_ESP_KEEP_FAILED) ? 1u : 0u;
    p.uniform_len = b->uniform_len;
    p.max_len = max_len;
    SG_HIP((hipError_t)sg::esp::launch(p, open, b->stream));
    if (!b->stream) SG_HIP(hipStreamSynchronize(nullptr));
    return SG_OK;
}

}  // namespace

extern "C" {

int sg_seal_batch_esp(const sg_esp_batch* b) { return esp_batch(b, false); }
int sg_open_batch_esp(const sg_esp_batch* b) { return esp_batch(b, true); }

}  // extern "C"
