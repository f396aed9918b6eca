// sg_msg_capi.cpp -- the long-message entry points of include/suruga_gpu.h
// (sg_seal_msg_dev / sg_open_msg_dev on device memory, sg_seal_msg /
// sg_open_msg on host memory).  Host-side glue only: argument checks, the plan
// (sg_msg_plan.cpp), the workspace and the launches of sg_msg.hip.  There is
// no CPU path: a message is sealed by the HIP kernels or the call fails.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <mutex>

#include "../../include/suruga_gpu.h"
#include "sg_host.h"
#include "sg_msg_plan.h"

// nonce_hi lies in what was padding: every size and offset is the one the
// header compiled to before the field existed
static_assert(sizeof(sg_msg) == 96 && offsetof(sg_msg, ad) == 16 && offsetof(sg_msg, flags) == 64 &&
                  offsetof(sg_msg, nonce_hi) == 68 && offsetof(sg_msg, stream) == 72,
              "sg_msg layout (SG_ABI_VERSION 1)");

namespace sg {
// sg_msg.hip: the group kernel, the finish kernel and (open, scrub) the zeroing
// of a failed open's output, all on stream s
// (nonce_hi: NULL = the draft, else the first four bytes of the RFC 8439 nonce)
hipError_t launch_msg(const uint8_t* key, const uint8_t nonce[8], const uint8_t* nonce_hi, const uint8_t* ad,
                      uint64_t adlen, const uint8_t* in, uint8_t* out, uint64_t n, uint8_t* status, uint32_t* ws,
                      const sg_msg_plan& plan, bool open, bool scrub, hipStream_t s);
}  // namespace sg

namespace {

using sg::fail;

int run_msg(const sg_msg* m, bool open) {
    if (!m) return fail(SG_E_ARG, "message is NULL%s");
    if (m->flags & ~sg::kMsgKnownFlags) return fail(SG_E_ARG, "unknown flags%s");
    const bool rfc = (m->flags & SG_MSG_RFC8439) != 0u;  // else nonce_hi is never read
    uint64_t n;
    bool shrt;
    const sg::MsgArgs a = {m->key, m->ad, m->ad_len, m->in, m->in_len, m->out, m->status};
    if (const char* bad = sg::msg_check_args(a, open, &n, &shrt)) return fail(SG_E_ARG, bad);
    if (shrt) return SG_E_SHORT;
    sg_msg_plan plan;
    if (sg_msg_plan_for_flags(n, m->ad_len, m->flags & SG_MSG_RFC8439, (uint32_t)sg::msg_groups(), &plan) != SG_OK)
        return fail(SG_E_ARG, "no plan for the message%s");

    // NULL = the null stream, and the call is synchronous (as sg_batch.stream)
    hipStream_t s = (hipStream_t)m->stream;
    void* ws = m->workspace;
    void* cached = nullptr;
    if (ws) {
        if (m->workspace_size < sg_msg_workspace_size()) return fail(SG_E_ARG, "workspace too small%s");
        if ((uintptr_t)ws % 16u) return fail(SG_E_ARG, "workspace must be 16-byte aligned%s");
    } else {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        SG_HIP(hipStreamIsCapturing(s, &cap));
        if (cap != hipStreamCaptureStatusNone)
            return fail(SG_E_ARG, "a call under stream capture needs a caller workspace%s");
        const int rc = sg::scratch_acquire(sg_msg_workspace_size(), s, &ws, &cached);
        if (rc != SG_OK) return rc;
    }
    const hipError_t he = sg::launch_msg(m->key, m->nonce, rfc ? m->nonce_hi : nullptr, m->ad, m->ad_len, m->in, m->out,
                                         n, m->status, (uint32_t*)ws, plan, open,
                                         open && !(m->flags & SG_MSG_KEEP_FAILED), s);
    if (cached) sg::scratch_release(cached, s, true);
    int rc = he == hipSuccess ? SG_OK : sg::hip_fail(he, "message launch");
    if (!m->stream) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess && rc == SG_OK) rc = sg::hip_fail(e, "hipStreamSynchronize");
    }
    return rc;
}

// grow-only device buffer of a context
int grow(uint8_t** p, size_t* cap, size_t need) {
    if (*cap >= need) return SG_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    SG_HIP(hipMalloc((void**)p, need));
    *cap = need;
    return SG_OK;
}

// rfc: RFC 8439 with a 12-byte nonce (nonce_hi = its first four bytes), else
// the draft with its 8
int host_msg(sg_ctx* c, bool open, bool rfc, const uint8_t* nonce, size_t nonce_len, const uint8_t* in, size_t in_len,
             const uint8_t* ad, size_t adlen, uint8_t* out) {
    // the argument errors of sg_seal / sg_open (single() in sg_capi.cpp)
    if (!c) return fail(SG_E_ARG, "context is NULL%s");
    if (rfc) {
        if (nonce_len != SG_RFC8439_NONCE_LEN || !nonce) return fail(SG_E_ARG, "nonce must be 12 bytes%s");
    } else if (nonce_len != SG_NONCE_LEN || !nonce) {
        return fail(SG_E_ARG, "nonce must be 8 bytes%s");
    }
    if (adlen && !ad) return fail(SG_E_ARG, "bad additional data%s");
    if (in_len && !in) return fail(SG_E_ARG, "NULL buffer%s");
    if (open && in_len < SG_MAC_LEN) return SG_E_SHORT;  // chacha20_poly1305.rs:68-70
    const size_t n = open ? in_len - SG_MAC_LEN : in_len;
    if (!out && (open ? n : n + SG_MAC_LEN)) return fail(SG_E_ARG, "NULL buffer%s");
    if ((uint64_t)n > SG_MSG_MAX_LEN) return fail(SG_E_ARG, "message longer than SG_MSG_MAX_LEN%s");
    if ((uint64_t)adlen > SG_MSG_MAX_LEN) return fail(SG_E_ARG, "additional data longer than SG_MSG_MAX_LEN%s");

    std::lock_guard<std::mutex> lk(c->mu);
    sg::DeviceGuard dg(c->device);
    if (!dg.ok) return fail(SG_E_HIP, "hipSetDevice failed%s");
    int rc;
    // one buffer, sealed or opened in place: n + 16 bytes either way
    if ((rc = grow(&c->m_buf, &c->m_cap, n + SG_MAC_LEN)) != SG_OK) return rc;
    if ((rc = grow(&c->m_ad, &c->m_ad_cap, adlen ? adlen : 1)) != SG_OK) return rc;
    if (in_len) SG_HIP(hipMemcpyAsync(c->m_buf, in, in_len, hipMemcpyHostToDevice, c->stream));
    if (adlen) SG_HIP(hipMemcpyAsync(c->m_ad, ad, adlen, hipMemcpyHostToDevice, c->stream));

    sg_msg m;
    std::memset(&m, 0, sizeof m);
    m.key = c->d_key;
    if (rfc) std::memcpy(m.nonce_hi, nonce, 4);
    std::memcpy(m.nonce, nonce + (rfc ? 4 : 0), 8);
    m.ad = c->m_ad;
    m.ad_len = adlen;
    m.in = c->m_buf;
    m.in_len = in_len;
    m.out = c->m_buf;
    m.status = c->d_key + 32;
    // a failed open's plaintext is withheld on the host below: no device scrub
    m.flags = (open ? SG_MSG_KEEP_FAILED : 0u) | (rfc ? SG_MSG_RFC8439 : 0u);
    m.stream = c->stream;
    rc = run_msg(&m, open);
    if (rc != SG_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    uint8_t st = 0;
    if (open) SG_HIP(hipMemcpyAsync(&st, m.status, 1, hipMemcpyDeviceToHost, c->stream));
    SG_HIP(hipStreamSynchronize(c->stream));
    if (open && st != 0) {
        if (n) std::memset(out, 0, n);  // the reference releases no plaintext with Err
        return SG_E_BAD_MAC;
    }
    const size_t out_len = open ? n : n + SG_MAC_LEN;
    if (out_len) SG_HIP(hipMemcpy(out, c->m_buf, out_len, hipMemcpyDeviceToHost));
    return SG_OK;
}

}  // namespace

extern "C" {

size_t sg_msg_workspace_size(void) { return (size_t)sg::kMsgMaxGroups * sg::kMsgPartialWords * 4u; }

int sg_seal_msg_dev(const sg_msg* m) { return run_msg(m, false); }
int sg_open_msg_dev(const sg_msg* m) { return run_msg(m, true); }

int sg_seal_msg(sg_ctx* c, const uint8_t* nonce, size_t nonce_len, const uint8_t* pt, size_t n, const uint8_t* ad,
                size_t adlen, uint8_t* out) {
    return host_msg(c, false, false, nonce, nonce_len, pt, n, ad, adlen, out);
}

int sg_open_msg(sg_ctx* c, const uint8_t* nonce, size_t nonce_len, const uint8_t* in, size_t in_len, const uint8_t* ad,
                size_t adlen, uint8_t* out) {
    return host_msg(c, true, false, nonce, nonce_len, in, in_len, ad, adlen, out);
}

int sg_seal_msg_rfc8439(sg_ctx* c, const uint8_t* nonce, size_t nonce_len, const uint8_t* pt, size_t n,
                        const uint8_t* ad, size_t adlen, uint8_t* out) {
    return host_msg(c, false, true, nonce, nonce_len, pt, n, ad, adlen, out);
}

int sg_open_msg_rfc8439(sg_ctx* c, const uint8_t* nonce, size_t nonce_len, const uint8_t* in, size_t in_len,
                        const uint8_t* ad, size_t adlen, uint8_t* out) {
    return host_msg(c, true, true, nonce, nonce_len, in, in_len, ad, adlen, out);
}

}  // extern "C"
