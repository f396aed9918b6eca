// sg_dtls13_capi.cpp -- the DTLS 1.3 entry points of include/suruga_gpu.h
// (sg_seal_batch_dtls13 / sg_open_batch_dtls13).  Host-side glue only: the argument rules
// (sg_dtls13_host.cpp's check_args, all of them before the first GPU call) and the one
// launch of sg_dtls13.hip.  No workspace and nothing read back, so a call on a capturing
// stream records exactly that launch.  There is no CPU path.
#include <hip/hip_runtime.h>

#include "../../include/suruga_gpu.h"
#include "sg_dtls13.h"
#include "sg_host.h"

namespace {

int dtls13_batch(const sg_dtls13_batch* b, bool open) {
    uint32_t max_len = 0;
    if (const char* why = sg::dtls13::check_args(b, open, &max_len)) return sg::fail(SG_E_ARG, why);
    if (b->count == 0) return SG_OK;
    sg::dtls13::Params p{};
    p.keys = b->keys;
    p.ivs = b->ivs;
    p.sn_keys = b->sn_keys;
    p.cids = b->cids;
    p.key_index = b->key_index;
    p.seq = b->seq;
    p.type = b->type;
    p.epoch = b->epoch;
    p.expected = b->expected;
    p.seq_out = b->seq_out;
    p.epoch_out = b->epoch_out;
    p.content_len = b->content_len;
    p.type_out = b->type_out;
    p.in = b->in;
    p.in_off = b->in_off;
    p.in_stride = b->in_stride;
    p.out = b->out;
    p.out_off = b->out_off;
    p.out_stride = b->out_stride;
    p.len = b->len;
    p.status = b->status;
    p.count = b->count;
    p.num_conns = b->num_conns;
    p.cid_len = b->cid_len;
    p.pad_to = b->pad_to;
    p.uniform_type = b->uniform_type;
    p.uniform_epoch = b->uniform_epoch;
    p.seal_bits = sg::dtls13::first_byte(b->flags, 0u, 0u) & (sg::dtls13::kS | sg::dtls13::kL);
    p.epoch_rows = (b->flags & SG_DTLS13_EPOCH_ROWS) ? 1u : 0u;
    p.keep_failed = (b->flags & SG_DTLS13_KEEP_FAILED) ? 1u : 0u;
    p.uniform_len = b->uniform_len;
    p.max_len = max_len;
    SG_HIP((hipError_t)sg::dtls13::launch(p, open, b->stream));
    if (!b->stream) SG_HIP(hipStreamSynchronize(nullptr));
    return SG_OK;
}

}  // namespace

extern "C" {

int sg_seal_batch_dtls13(const sg_dtls13_batch* b) { return dtls13_batch(b, false); }
int sg_open_batch_dtls13(const sg_dtls13_batch* b) { return dtls13_batch(b, true); }

}  // extern "C"
