// sg_quic_capi.cpp -- the QUIC packet protection entry points of include/suruga_gpu.h
// (sg_seal_batch_quic / sg_open_batch_quic).  Host-side glue only: the argument rules
// (sg_quic_host.cpp's check_args, all of them before the first GPU call) and the one
// launch of sg_quic.hip.  No workspace and nothing read back, so a call on a capturing
// stream records exactly that launch.  There is no CPU path.
#include <hip/hip_runtime.h>

#include "../../include/suruga_gpu.h"
#include "sg_host.h"
#include "sg_quic.h"

namespace {

int quic_batch(const sg_quic_batch* b, bool open) {
    uint32_t max_len = 0;
    if (const char* why = sg::quic::check_args(b, open, &max_len)) return sg::fail(SG_E_ARG, why);
    if (b->count == 0) return SG_OK;
    const bool phase = (b->flags & SG_QUIC_KEY_PHASE) != 0u;
    sg::quic::Params p{};
    p.keys = b->keys;
    p.ivs = b->ivs;
    p.hp_keys = b->hp_keys;
    p.key_index = b->key_index;
    p.pn = b->pn;
    p.pn_out = b->pn_out;
    p.pn_off = b->pn_off;
    p.in = b->in;
    p.in_off = b->in_off;
    p.in_stride = b->in_stride;
    p.out = b->out;
    p.out_off = b->out_off;
    p.out_stride = b->out_stride;
    p.len = b->len;
    p.status = b->status;
    p.count = b->count;
    p.rows = phase ? b->num_keys / 2u : b->num_keys;
    p.key_phase = phase ? 1u : 0u;
    p.keep_failed = (b->flags & SG_QUIC_KEEP_FAILED) ? 1u : 0u;
    p.uniform_pn_off = b->uniform_pn_off;
    p.uniform_len = b->uniform_len;
    p.max_len = max_len;
    SG_HIP((hipError_t)sg::quic::launch(p, open, b->stream));
    if (!b->stream) SG_HIP(hipStreamSynchronize(nullptr));
    return SG_OK;
}

}  // namespace

extern "C" {

int sg_seal_batch_quic(const sg_quic_batch* b) { return quic_batch(b, false); }
int sg_open_batch_quic(const sg_quic_batch* b) { return quic_batch(b, true); }

}  // extern "C"
