// sg_msg_batch_capi.cpp -- the message-batch entry points of
// include/suruga_gpu.h (sg_seal_msg_batch / sg_open_msg_batch): many
// device-resident messages of any length in one call.  Host-side glue only:
// argument checks (all of them before the first GPU call), the plan
// (sg_msg_batch_plan_for, written straight into the image the kernels read),
// the upload of that image and the launches of sg_msg_batch.hip.  There is no
// CPU path.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/suruga_gpu.h"
#include "sg_host.h"
#include "sg_msg_plan.h"
#include "sg_wire.h"

// nonce_hi lies in what was padding: every size and offset is the one the
// header compiled to before the field existed
static_assert(sizeof(sg_msg_item) == 56 && offsetof(sg_msg_item, nonce) == 4 && offsetof(sg_msg_item, nonce_hi) == 12 &&
                  offsetof(sg_msg_item, ad) == 16,
              "sg_msg_item layout (SG_ABI_VERSION 1)");
static_assert(sizeof(sg_msg_batch) == 64 && offsetof(sg_msg_batch, stream) == 40, "sg_msg_batch layout (SG_ABI_VERSION 1)");

namespace sg {
// sg_msg_batch.hip: the batch kernel, the finish kernel and (open, scrub) the
// zeroing of the failed messages' outputs, all on stream s, reading the tables
// at the front of ws
hipError_t launch_msg_batch(const MsgBatchLayout& l, void* ws, uint32_t count, uint32_t groups, uint8_t* status,
                            bool open, bool scrub, bool rfc8439, hipStream_t s);
}  // namespace sg

namespace {

using sg::fail;

// Pinned host blocks the table image is built in and uploaded from, so that
// the upload is asynchronous and the caller's items array is free once the
// call returns.  A block is reused when the copy out of it has completed
// (`done`, queried, never waited for under the lock); a call that finds none
// free adds one.
struct Staging {
    int device = 0;
    void* host = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool used = false;  // `done` has been recorded
    bool held = false;  // a call is filling it
};
std::mutex g_st_mu;  // the pool's bookkeeping; never held across a launch or a wait
std::vector<Staging*> g_staging;

int staging_acquire(int device, size_t need, Staging** out) {
    Staging* st = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_st_mu);
        for (Staging* c : g_staging) {
            if (c->held || c->device != device) continue;
            if (c->used && hipEventQuery(c->done) != hipSuccess) continue;  // its copy is still in flight
            if (!st || (c->bytes >= need && (st->bytes < need || c->bytes < st->bytes))) st = c;
        }
        if (!st) {
            st = new Staging();
            st->device = device;
            g_staging.push_back(st);
        }
        st->held = true;
    }
    auto release_on_error = [&](int rc) {
        std::lock_guard<std::mutex> lk(g_st_mu);
        st->held = false;
        return rc;
    };
    if (!st->done && hipEventCreateWithFlags(&st->done, hipEventDisableTiming) != hipSuccess)
        return release_on_error(fail(SG_E_HIP, "hipEventCreate failed%s"));
    if (st->bytes < need) {
        if (st->host) (void)hipHostFree(st->host);
        st->host = nullptr;
        st->bytes = 0;
        st->used = false;
        const hipError_t e = hipHostMalloc(&st->host, need, hipHostMallocPortable);
        if (e != hipSuccess) return release_on_error(sg::hip_fail(e, "hipHostMalloc (message batch tables)"));
        st->bytes = need;
    }
    *out = st;
    return SG_OK;
}

void staging_release(Staging* st, hipStream_t s, bool copied) {
    if (copied && hipEventRecord(st->done, s) == hipSuccess) st->used = true;
    std::lock_guard<std::mutex> lk(g_st_mu);
    st->held = false;
}

int run_msg_batch(const sg_msg_batch* b, bool open) {
    if (!b) return fail(SG_E_ARG, "batch is NULL%s");
    if (b->flags & ~sg::kMsgKnownFlags) return fail(SG_E_ARG, "unknown flags%s");
    const bool rfc = (b->flags & SG_MSG_RFC8439) != 0u;  // the whole call; else no nonce_hi is read
    if (b->count > SG_MSG_BATCH_MAX_COUNT) return fail(SG_E_ARG, "count exceeds SG_MSG_BATCH_MAX_COUNT%s");
    if (b->count == 0) return SG_OK;
    if (!b->keys || b->num_keys == 0 || !b->items) return fail(SG_E_ARG, "keys and items must be non-NULL%s");
    if (open && !b->status) return fail(SG_E_ARG, "open requires a status array%s");
    const uint32_t count = b->count;
    const sg::MsgBatchLayout lay = sg::msg_batch_layout(count);
    if (b->workspace) {
        if (b->workspace_size < lay.total) return fail(SG_E_ARG, "workspace too small%s");
        if ((uintptr_t)b->workspace % 16u) return fail(SG_E_ARG, "workspace must be 16-byte aligned%s");
    }
    // the lengths the plan takes; a short open is planned as an empty message
    // that no kernel touches
    std::vector<uint64_t> len(2u * (size_t)count);
    uint64_t* n = len.data();
    uint64_t* adlen = n + count;
    for (uint32_t i = 0; i < count; ++i) {
        const sg_msg_item& m = b->items[i];
        if (m.key_index >= b->num_keys) return fail(SG_E_ARG, "key_index out of range%s");
        bool shrt;  // reported per message (the finish kernel), not by the call
        const sg::MsgArgs a = {b->keys, m.ad, m.ad_len, m.in, m.in_len, m.out, b->status};
        if (const char* bad = sg::msg_check_args(a, open, &n[i], &shrt)) return fail(SG_E_ARG, bad);
        adlen[i] = shrt ? 0u : m.ad_len;
    }

    // ---- from here on the GPU is touched
    // NULL = the null stream, and the call is synchronous (as sg_msg.stream)
    hipStream_t s = (hipStream_t)b->stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    SG_HIP(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail(SG_E_ARG, "a message batch cannot run under stream capture (its tables are uploaded by a copy)%s");
    int device = 0;
    SG_HIP(hipGetDevice(&device));
    void* ws = b->workspace;
    void* cached = nullptr;
    int rc;
    if (!ws && (rc = sg::scratch_acquire(lay.total, s, &ws, &cached)) != SG_OK) return rc;
    Staging* st = nullptr;
    if ((rc = staging_acquire(device, lay.upload_bytes, &st)) != SG_OK) {
        if (cached) sg::scratch_release(cached, s, false);
        return rc;
    }
    uint8_t* h = (uint8_t*)st->host;
    sg::MsgBatchItem* items = (sg::MsgBatchItem*)(h + lay.items);
    for (uint32_t i = 0; i < count; ++i) {
        const sg_msg_item& m = b->items[i];
        sg::MsgBatchItem& d = items[i];
        d.key = b->keys + (size_t)SG_KEY_LEN * m.key_index;
        d.ad = m.ad;
        d.in = m.in;
        d.out = m.out;
        d.n = n[i];
        d.adlen = adlen[i];
        // the nonce as little-endian words (chacha20.rs:45-46); RFC 8439
        // (section 2.3): nonce_hi in front of them, in state word 13
        d.n14 = sg::get_le32(m.nonce);
        d.n15 = sg::get_le32(m.nonce + 4);
        d.skip = open && m.in_len < SG_MAC_LEN ? 1u : 0u;
        d.n13 = rfc ? sg::get_le32(m.nonce_hi) : 0u;
    }
    sg_msg_batch_plan plan;
    rc = sg_msg_batch_plan_for_flags(n, adlen, count, b->flags & SG_MSG_RFC8439, (uint32_t)sg::msg_groups(), &plan,
                                     (sg_msg_plan*)(h + lay.plans), (sg_msg_seg*)(h + lay.segs), lay.seg_cap,
                                     (sg_msg_span*)(h + lay.group_segs), (sg_msg_span*)(h + lay.msg_segs));
    if (rc != SG_OK) {
        staging_release(st, s, false);
        if (cached) sg::scratch_release(cached, s, false);
        return fail(SG_E_ARG, "no plan for the batch%s");
    }
    hipError_t he = hipMemcpyAsync(ws, h, lay.upload_bytes, hipMemcpyHostToDevice, s);
    staging_release(st, s, he == hipSuccess);
    if (he == hipSuccess)
        he = sg::launch_msg_batch(lay, ws, count, plan.groups, b->status, open,
                                  open && !(b->flags & SG_MSG_KEEP_FAILED), rfc, s);
    if (cached) sg::scratch_release(cached, s, true);
    rc = he == hipSuccess ? SG_OK : sg::hip_fail(he, "message batch launch");
    if (!b->stream) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess && rc == SG_OK) rc = sg::hip_fail(e, "hipStreamSynchronize");
    }
    return rc;
}

}  // namespace

extern "C" {

size_t sg_msg_batch_workspace_size(uint32_t count) {
    if (count > SG_MSG_BATCH_MAX_COUNT) count = SG_MSG_BATCH_MAX_COUNT;
    return sg::msg_batch_layout(count).total;
}

int sg_seal_msg_batch(const sg_msg_batch* b) { return run_msg_batch(b, false); }
int sg_open_msg_batch(const sg_msg_batch* b) { return run_msg_batch(b, true); }

}  // extern "C"
