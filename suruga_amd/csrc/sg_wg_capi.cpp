// sg_wg_capi.cpp -- the WireGuard transport data entry points of include/suruga_gpu.h
// (sg_seal_batch_wg / sg_open_batch_wg).  Host-side glue only: the argument rules
// (sg_wg_host.cpp's check_args, all of them before the first GPU call) and the one
// launch of sg_wg.hip.  No workspace and nothing read back, so a call on a capturing
// stream records exactly that launch.  There is no CPU path.
#include <hip/hip_runtime.h>

#include "../../include/suruga_gpu.h"
#include "sg_host.h"
#include "sg_wg.h"

namespace {

int wg_batch(const sg_wg_batch* b, bool open) {
    uint32_t max_len = 0;
    if (const char* why = sg::wg::check_args(b, open, &max_len)) return sg::fail(SG_E_ARG, why);
    if (b->count == 0) return SG_OK;
    sg::wg::Params p{};
    p.keys = b->keys;
    p.receiver = b->receiver;
    p.key_index = b->key_index;
    p.counter = b->counter;
    p.counter_out = b->counter_out;
    p.inner_len = b->inner_len;
    p.in = b->in;
    p.in_off = b->in_off;
    p.in_stride = b->in_stride;
    p.out = b->out;
    p.out_off = b->out_off;
    p.out_stride = b->out_stride;
    p.len = b->len;
    p.status = b->status;
    p.count = b->count;
    p.num_keys = b->num_keys;
    p.pad_cap = b->pad_cap;
    p.keep_failed = (b->flags & SG_WG_KEEP_FAILED) ? 1u : 0u;
    p.uniform_len = b->uniform_len;
    p.max_len = max_len;
    SG_HIP((hipError_t)sg::wg::launch(p, open, b->stream));
    if (!b->stream) SG_HIP(hipStreamSynchronize(nullptr));
    return SG_OK;
}

}  // namespace

extern "C" {

int sg_seal_batch_wg(const sg_wg_batch* b) { return wg_batch(b, false); }
int sg_open_batch_wg(const sg_wg_batch* b) { return wg_batch(b, true); }

}  // extern "C"
