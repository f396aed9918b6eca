// sg_capi.cpp -- the C ABI declared in include/suruga_gpu.h.
//
// Host-side glue only: argument checking (mirroring the reference's panics /
// errors), per-device state (stream, keying workspace cache, timing events),
// staging for the single-record Encryptor/Decryptor calls, and the launches
// of the gfx950 kernels through sg_internal.h's launch_* functions (uniform
// 16 KiB batches: sg_wpr.hip; every other batch: sg_dispatch.cpp; fill,
// compare, scrub and the TLS 1.3 strip: sg_plumb.hip).  There is no CPU fallback: every
// seal/open goes through the HIP kernels or fails with an error code.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/suruga_gpu.h"
#include "sg_host.h"
#include "sg_internal.h"

namespace {
thread_local std::string g_err;
}  // namespace

namespace sg {

int fail(int code, const char* fmt, const char* detail) {
    char buf[512];
    std::snprintf(buf, sizeof buf, fmt, detail ? detail : "");
    g_err = buf;
    return code;
}

int hip_fail(hipError_t e, const char* where) {
    char buf[512];
    std::snprintf(buf, sizeof buf, "%s: %s", where, hipGetErrorString(e));
    g_err = buf;
    return SG_E_HIP;
}

}  // namespace sg

namespace {

using sg::fail;
using sg::hip_fail;

// A workspace of the library-owned cache.  Calls with no caller workspace
// take one that no other call is enqueuing on, make their stream wait for its
// previous user's work (`done`) and record `done` again after their launches,
// so reuse is ordered on the device even across streams and asynchronous
// calls; the host never blocks on it except to grow a buffer.
struct CachedWs {
    void* ptr = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool used = false;   // `done` has been recorded
    bool held = false;   // a call is enqueuing on it
};

struct DeviceState {
    bool init = false;
    bool ok = false;
    std::vector<CachedWs*> pool;  // guarded by g_mu
};

std::mutex g_mu;  // device table, workspace pool bookkeeping (never held across a launch or a wait)
std::vector<DeviceState> g_dev;

// timing: a batch's events (keying window e0 -> mid, record window mid -> e2), each in one TimedBatch or in the pool
struct TimedBatch {
    hipEvent_t e0, mid, e2;
    bool open;
};
std::mutex g_timing_mu;
bool g_timing = false;
std::vector<TimedBatch> g_timed;
std::vector<hipEvent_t> g_event_pool;

hipEvent_t get_event() {  // caller holds g_timing_mu
    if (!g_event_pool.empty()) {
        hipEvent_t e = g_event_pool.back();
        g_event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// Checks the device is a gfx950 part.  Caller holds g_mu.
int device_state(int dev, DeviceState** out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SG_E_NODEV, "no HIP device visible%s");
    if (dev < 0 || dev >= ndev) return fail(SG_E_ARG, "device ordinal out of range%s");
    if ((int)g_dev.size() < ndev) g_dev.resize(ndev);
    DeviceState& d = g_dev[dev];
    if (!d.init) {
        d.init = true;
        hipDeviceProp_t prop;
        SG_HIP(hipGetDeviceProperties(&prop, dev));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            d.ok = false;
            return fail(SG_E_NODEV, "device is %s, this library is built for gfx950 only", prop.gcnArchName);
        }
        d.ok = true;
    }
    if (!d.ok) return fail(SG_E_NODEV, "device not usable%s");
    *out = &d;
    return SG_OK;
}

int current_device_state(DeviceState** out) {
    int dev = 0;
    SG_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_mu);
    return device_state(dev, out);
}

// Take a cached workspace of >= need bytes for a call on stream s (the current
// device is d's).  Growing a buffer waits for its previous user only.
int ws_acquire(DeviceState* d, size_t need, hipStream_t s, CachedWs** out) {
    CachedWs* w = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        for (CachedWs* c : d->pool)
            if (!c->held && (!w || (c->bytes >= need && (w->bytes < need || c->bytes < w->bytes)))) w = c;
        if (!w) {
            w = new CachedWs();
            d->pool.push_back(w);
        }
        w->held = true;
    }
    auto release_on_error = [&](int rc) {
        std::lock_guard<std::mutex> lk(g_mu);
        w->held = false;
        return rc;
    };
    if (!w->done && hipEventCreateWithFlags(&w->done, hipEventDisableTiming) != hipSuccess)
        return release_on_error(fail(SG_E_HIP, "hipEventCreate failed%s"));
    if (w->bytes < need) {
        if (w->used && hipEventSynchronize(w->done) != hipSuccess)
            return release_on_error(fail(SG_E_HIP, "workspace event wait failed%s"));
        if (w->ptr) (void)hipFree(w->ptr);
        w->ptr = nullptr;
        w->bytes = 0;
        const size_t sz = need < (1u << 20) ? (1u << 20) : need;
        if (hipMalloc(&w->ptr, sz) != hipSuccess) return release_on_error(fail(SG_E_HIP, "workspace hipMalloc failed%s"));
        w->bytes = sz;
        w->used = false;
    }
    if (w->used && hipStreamWaitEvent(s, w->done, 0) != hipSuccess)
        return release_on_error(fail(SG_E_HIP, "hipStreamWaitEvent failed%s"));
    *out = w;
    return SG_OK;
}

void ws_release(CachedWs* w, hipStream_t s, bool launched) {
    if (launched && hipEventRecord(w->done, s) == hipSuccess) w->used = true;
    std::lock_guard<std::mutex> lk(g_mu);
    w->held = false;
}

using sg::RecordForm;
// A call's record form and its extension struct's fields: built by each entry point, read from validate on.
struct BatchForm {
    RecordForm form;
    uint32_t xflags = 0u;             // the extension struct's flags (must be 0)
    const uint8_t* ivs = nullptr;     // write IVs: RFC 8439 TLS mode and TLS 1.3
    uint8_t* inner_type = nullptr;    // TLS 1.3 open
    uint32_t* content_len = nullptr;  // TLS 1.3 open
    // TLS 1.3 seal options (sg_seal_batch_tls13_ex); the plain seal is {NULL, 0, 0}
    const uint8_t* inner_types = nullptr;  // per-record inner types, or NULL: b->content_type
    uint32_t pad_to = 0u;                  // tls13_inner_len's policy (sg_layout.h)
    uint32_t oflags = 0u;                  // sg_tls13_seal_opts.flags (must be 0)
};
int known_flags(const sg_batch* b) {
    return (b->flags & ~(SG_BATCH_TLS | SG_BATCH_KEEP_FAILED)) ? fail(SG_E_ARG, "unknown flags%s") : SG_OK;
}

// TLS 1.3 (sg_*_batch_tls13): RFC 8446 section 5.1 / 5.2 bounds of a record's content (seal) and fragment (open)
constexpr uint32_t kTls13MaxContent = 1u << 14;
constexpr uint32_t kTls13MaxFragment = (1u << 14) + 256u;
// What the TLS 1.3 calls check of the batch itself: all sg_batch_tls13_route checks.
// typed: the records bring their own inner types, so b->content_type is not read.
int validate_tls13(const sg_batch* b, bool open, bool typed = false) {
    if (!b) return fail(SG_E_ARG, "batch is NULL%s");
    if (!(b->flags & SG_BATCH_TLS))
        return fail(SG_E_ARG, "the TLS 1.3 batch builds nonce and AD on the device: SG_BATCH_TLS must be set%s");
    if (known_flags(b) != SG_OK) return SG_E_ARG;
    const uint32_t maxl = b->len ? b->max_len : b->uniform_len;
    if (!open && maxl > kTls13MaxContent) return fail(SG_E_ARG, "TLS 1.3 content longer than 2^14 bytes%s");
    if (open && maxl > kTls13MaxFragment) return fail(SG_E_ARG, "TLS 1.3 fragment longer than 2^14 + 256 bytes%s");
    if (!open && !typed && b->content_type == 0)
        return fail(SG_E_ARG, "the inner content type must be non-zero (a zero byte reads as padding)%s");
    return SG_OK;
}

// Every argument check of a batch call, in the calls' order: the RFC 8439 and TLS 1.3
// extensions (and the batch's flags) even for an empty batch, the rest with records in it.
int validate(const sg_batch* b, const BatchForm& f, bool open) {
    const bool t13 = f.form == RecordForm::kTls13;
    if (t13) {
        if (f.xflags) return fail(SG_E_ARG, "sg_batch_tls13.flags must be 0%s");
        if (f.oflags) return fail(SG_E_ARG, "sg_tls13_seal_opts.flags must be 0%s");
        if (f.pad_to > kTls13MaxContent) return fail(SG_E_ARG, "pad_to above 2^14%s");
        if (const int rc = validate_tls13(b, open, f.inner_types != nullptr)) return rc;
        if (!f.ivs) return fail(SG_E_ARG, "the TLS 1.3 batch needs the write IVs (sg_batch_tls13.ivs)%s");
    }
    if (!b) return fail(SG_E_ARG, "batch is NULL%s");
    if (f.form != RecordForm::kDraft) {
        if (!t13 && f.xflags) return fail(SG_E_ARG, "sg_batch_rfc8439.flags must be 0%s");
        if (((uintptr_t)f.ivs & 3u) != 0) return fail(SG_E_ARG, "IV table must be 4-byte aligned%s");
        if (t13 && open) {
            if (!f.inner_type || !f.content_len)
                return fail(SG_E_ARG, "open needs the inner_type and content_len arrays%s");
            if (((uintptr_t)f.content_len & 3u) != 0) return fail(SG_E_ARG, "content_len must be 4-byte aligned%s");
        }
        if (known_flags(b) != SG_OK) return SG_E_ARG;
        if ((b->flags & SG_BATCH_TLS) && !f.ivs)
            return fail(SG_E_ARG, "RFC 7905 TLS mode needs the write IVs (sg_batch_rfc8439.ivs)%s");
    }
    if (b->count == 0) return SG_OK;
    if (!b->keys || !b->in || !b->out) return fail(SG_E_ARG, "keys/in/out must be non-NULL%s");
    if (((uintptr_t)b->keys & 3u) != 0) return fail(SG_E_ARG, "key table must be 4-byte aligned%s");
    if (b->num_keys == 0) return fail(SG_E_ARG, "num_keys must be >= 1%s");
    if (open && !b->status) return fail(SG_E_ARG, "open requires a status array%s");
    if (known_flags(b) != SG_OK) return SG_E_ARG;
    if (!(b->flags & SG_BATCH_TLS)) {
        if (!b->nonces) return fail(SG_E_ARG, "explicit mode needs nonces%s");
        if (b->ad_len > SG_MAX_AD_LEN) return fail(SG_E_ARG, "ad_len exceeds SG_MAX_AD_LEN%s");
        if (b->ad_len && !b->ads) return fail(SG_E_ARG, "ad_len > 0 needs ads%s");
    }
    uint32_t maxl = b->len ? b->max_len : b->uniform_len;
    if (b->len && b->max_len == 0) return fail(SG_E_ARG, "max_len is required with len[]%s");
    uint32_t max_n = open ? (maxl >= 16 ? maxl - 16 : 0) : maxl;
    if (max_n > SG_MAX_RECORD_LEN) return fail(SG_E_ARG, "record longer than SG_MAX_RECORD_LEN%s");
    if ((b->flags & SG_BATCH_TLS) && max_n > 0xffffu)
        return fail(SG_E_ARG, "TLS mode record length must fit be16%s");
    return SG_OK;
}

// The wave-per-record kernel (sg_wpr.hip) takes uniform batches of full records
// (wpr_len: 2^14 bytes, or the fragment they seal to in this form) in a 16-byte
// aligned strided layout; everything else runs on the size-class kernels.
bool wpr_eligible(const sg_batch* b, RecordForm form, bool open, bool typed = false) {
    if (typed) return false;  // TLS 1.3 seal: its keying pre-pass appends the call's one type
    if (!sg::wpr_enabled() || b->len || b->in_off || b->out_off) return false;
    if (b->uniform_len != sg::wpr_len(form, open)) return false;
    // per-record scalars are read as dwords: key index, sequence numbers, nonces (8 or 12 bytes)
    if (((uintptr_t)b->key_index | (uintptr_t)b->seq) % 4u) return false;
    if (!(b->flags & SG_BATCH_TLS) && (uintptr_t)b->nonces % 4u) return false;
    return ((uintptr_t)b->in | (uintptr_t)b->out | b->in_stride | b->out_stride) % 16u == 0u;
}

// Keying + AEAD launches of one batch on stream s with workspace ws.
int launch_batch(const sg_batch* b, const BatchForm& f, bool open, hipStream_t s, void* ws) {
    const bool t13 = f.form == RecordForm::kTls13;
    sg::KParams p;
    std::memset(&p, 0, sizeof p);
    p.keys = b->keys;
    p.key_index = b->key_index;
    p.num_keys = b->num_keys;
    p.seq = b->seq;
    p.seq0 = b->seq0;
    p.nonces = b->nonces;
    p.ads = b->ads;
    p.in = b->in;
    p.in_off = b->in_off;
    p.in_stride = b->in_stride;
    p.out = b->out;
    p.out_off = b->out_off;
    p.out_stride = b->out_stride;
    p.len = b->len;
    p.status = b->status;
    p.ws = (uint32_t*)ws;
    p.uniform_len = b->uniform_len;
    p.count = b->count;
    p.tls = (b->flags & SG_BATCH_TLS) ? 1u : 0u;
    p.ad_stride = b->ad_stride;
    p.tls_hdr = (uint32_t)b->content_type | ((uint32_t)b->ver_major << 8) | ((uint32_t)b->ver_minor << 16);
    p.rfc = sg::construction_of(f.form) == sg::Construction::kRfc8439 ? 1u : 0u;  // the form, for the kernels:
    p.tls13 = t13 ? 1u : 0u;
    p.ivs = f.ivs;
    p.ad_len = p.tls ? sg::tls_ad_len(f.form) : b->ad_len;
    if (t13) {  // the seal options, in the slots of nonces and ad_stride (explicit mode only; sg_internal.h)
        p.inner_types = f.inner_types;
        p.pad_to = f.pad_to;
    }
    const uint32_t maxl = b->len ? b->max_len : b->uniform_len;
    // (TLS 1.3 seal: the AEAD runs over the inner plaintext, content || type || zeros; the
    // largest one sizes the keying geometry, the classify bound and the LDS slots)
    const uint32_t max_n = open ? (maxl >= 16u ? maxl - 16u : 0u) : t13 ? sg::tls13_inner_len(maxl, f.pad_to) : maxl;
    static_assert(sg::tls13_inner_len(100u, 0u) == 100u + sg::seal_extra(RecordForm::kTls13), "no padding: the one type byte");
    const bool uniform = !b->len || sg::size_class(max_n) == 0u;
    const bool wpr = wpr_eligible(b, f.form, open, f.inner_types != nullptr);
    // mixed TLS batches: full-chunk records (4-16 KiB, multiples of 64 bytes) go to the
    // wave-per-record buckets and the 64 B-4 KiB ones to the packed kernel (sg_pack.hip), in
    // either construction; not under capture (they are launched on the populations read
    // back), and the per-record arrays are read as dwords by the routed kernels
    // (TLS 1.3: the routes go by the inner length -- a seal padded to a multiple of 64, a peer's
    // fragments padded so; the packed kernel always, the J = 2..4 buckets under sg_set_tls13_buckets)
    const bool buckets = sg::wpr_enabled() && max_n > 4096u && (!t13 || sg::tls13_buckets_enabled());
    if (!wpr && !uniform && p.tls && (buckets || (sg::pack_enabled() && max_n >= 64u))) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        SG_HIP(hipStreamIsCapturing(s, &cap));
        const bool ok = cap == hipStreamCaptureStatusNone &&
                        ((uintptr_t)b->key_index | (uintptr_t)b->seq | (uintptr_t)b->len | (uintptr_t)b->in_off |
                         (uintptr_t)b->out_off) % 4u == 0u;
        p.wpr_mix = ok && buckets;
        p.pack_mix = ok && sg::pack_enabled();
    }

    hipEvent_t e[3] = {nullptr, nullptr, nullptr};  // start, between keying and records, end
    bool timing = false;
    {
        std::lock_guard<std::mutex> lk(g_timing_mu);
        timing = g_timing;
        if (timing)
            for (auto& x : e) x = get_event();
    }
    // Every launch of the batch is enqueued before any error return: a record
    // longer than max_len only shows in the population readback, and the
    // other records' launches (and the timing bookkeeping) still follow it.
    uint32_t over = 0;
    hipError_t he = timing ? hipEventRecord(e[0], s) : hipSuccess;
    if (he == hipSuccess) he = wpr ? sg::launch_wpr(p, open, s, e[1]) : sg::launch_aead(p, open, max_n, uniform, s, &over, e[1]);
    // failed opens hand out no plaintext (chacha20_poly1305.rs:89-93)
    if (he == hipSuccess && open && !(b->flags & SG_BATCH_KEEP_FAILED)) he = sg::launch_scrub(p, s);
    // TLS 1.3: inner type and content length of the records that opened (RFC 8446 section 5.4)
    if (he == hipSuccess && open && t13) he = sg::launch_strip(p, f.inner_type, f.content_len, s);
    if (timing) {
        if (he == hipSuccess) he = hipEventRecord(e[2], s);
        std::lock_guard<std::mutex> lk(g_timing_mu);
        if (he == hipSuccess) g_timed.push_back({e[0], e[1], e[2], open});
        for (auto x : e)
            if (he != hipSuccess && x) g_event_pool.push_back(x);
    }
    if (he != hipSuccess) return hip_fail(he, "batch launch");
    if (over) return fail(SG_E_ARG, "records longer than max_len were not processed%s");
    return SG_OK;
}

int run_batch(const sg_batch* b, const BatchForm& f, bool open) {
    sg::routes_reset();  // sg_last_batch_routes speaks of this call from here on
    int rc = validate(b, f, open);
    if (rc != SG_OK || b->count == 0) return rc;

    DeviceState* d = nullptr;
    if ((rc = current_device_state(&d)) != SG_OK) return rc;
    // NULL = the null stream: ordered after the caller's earlier work on it
    // (torch's default stream is the null stream), and the call is synchronous
    hipStream_t s = (hipStream_t)b->stream;

    void* ws = b->workspace;
    CachedWs* cws = nullptr;
    const size_t need = sg_workspace_size(b->count);
    if (ws) {
        if (b->workspace_size < need) return fail(SG_E_ARG, "workspace too small%s");
        if ((uintptr_t)ws % 16u) return fail(SG_E_ARG, "workspace must be 16-byte aligned%s");
    } else {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        SG_HIP(hipStreamIsCapturing(s, &cap));
        if (cap != hipStreamCaptureStatusNone)
            return fail(SG_E_ARG, "a call under stream capture needs a caller workspace%s");
        if ((rc = ws_acquire(d, need, s, &cws)) != SG_OK) return rc;
        ws = cws->ptr;
    }
    rc = launch_batch(b, f, open, s, ws);
    if (cws) ws_release(cws, s, true);
    // NULL stream: the call returns when the batch is done, whatever it returns
    if (!b->stream) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess && rc == SG_OK) rc = hip_fail(e, "hipStreamSynchronize");
    }
    return rc;
}

}  // namespace

namespace sg {

int scratch_acquire(size_t need, hipStream_t s, void** ptr, void** handle) {
    DeviceState* d = nullptr;
    int rc = current_device_state(&d);
    if (rc != SG_OK) return rc;
    CachedWs* w = nullptr;
    if ((rc = ws_acquire(d, need, s, &w)) != SG_OK) return rc;
    *ptr = w->ptr;
    *handle = w;
    return SG_OK;
}

void scratch_release(void* handle, hipStream_t s, bool launched) { ws_release((CachedWs*)handle, s, launched); }

}  // namespace sg

// ---------------------------------------------------------------------------
// single-record contexts (Encryptor / Decryptor)
// ---------------------------------------------------------------------------
using sg::fail;
using sg::hip_fail;

extern "C" {

size_t sg_key_size(void) { return SG_KEY_LEN; }
size_t sg_fixed_iv_len(void) { return 0; }
size_t sg_mac_len(void) { return SG_MAC_LEN; }
int sg_abi_version(void) { return SG_ABI_VERSION; }
const char* sg_last_error(void) { return g_err.c_str(); }
#ifndef SG_SOURCE_HASH
#define SG_SOURCE_HASH "0000000000000000"
#endif
// the hash of the sources this library was built from (suruga_amd/_build.py
// source_hash), also findable in the binary as the marker "sg-src:<hash>"
static const char kSrcMarker[] = "sg-src:" SG_SOURCE_HASH;
const char* sg_source_hash(void) { return kSrcMarker + 7; }
const char* sg_build_info(void) {
    static const std::string src = std::string(" [") + kSrcMarker + "]";
    static const std::string pk = std::string("; small records of mixed batches: ") + sg::pack_kernel_config() + src;
    static const std::string on = std::string("gfx950 ") + sg::wpr_kernel_config() + "; other batches: " +
                                  sg::class_kernel_config();
    static const std::string off = std::string("gfx950 ") + sg::class_kernel_config() + " (wave-per-record kernel off)";
    static const std::string on_pk = on + pk, off_pk = off + pk, on_s = on + src, off_s = off + src;
    const bool w = sg::wpr_enabled(), k = sg::pack_enabled();
    return w ? (k ? on_pk.c_str() : on_s.c_str()) : (k ? off_pk.c_str() : off_s.c_str());
}
size_t sg_workspace_size(uint32_t count) {
    // keying records, one list per size class, the class populations and the
    // count of records longer than max_len
    return (size_t)sg::ws_words(count) * 4u;
}

sg_ctx* sg_ctx_new(const uint8_t key[32], int device) {
    if (!key) {
        fail(SG_E_ARG, "key is NULL%s");
        return nullptr;
    }
    {
        std::lock_guard<std::mutex> lk(g_mu);
        DeviceState* d = nullptr;
        if (device_state(device, &d) != SG_OK) return nullptr;
    }
    sg::DeviceGuard dg(device);
    if (!dg.ok) {
        fail(SG_E_HIP, "hipSetDevice failed%s");
        return nullptr;
    }
    sg_ctx* c = new sg_ctx();
    c->device = device;
    const size_t cap_in = sg::kSingleInOff + SG_MAX_RECORD_LEN + 64;
    const size_t cap_out = sg::kSingleOutOff + SG_MAX_RECORD_LEN + 64;
    bool ok = hipMalloc((void**)&c->d_key, 64) == hipSuccess &&
              hipHostMalloc((void**)&c->h_in, cap_in, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void**)&c->h_out, cap_out, hipHostMallocDefault) == hipSuccess &&
              hipMalloc(&c->d_ws, sg_workspace_size(1)) == hipSuccess &&
              hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMemcpy(c->d_key, key, 32, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        fail(SG_E_HIP, "context allocation failed%s");
        sg_ctx_free(c);
        return nullptr;
    }
    return c;
}

void sg_ctx_free(sg_ctx* c) {
    if (!c) return;
    sg::DeviceGuard dg(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    sg::record_staging_free(c->rec);
    (void)hipFree(c->d_key);
    (void)hipHostFree(c->h_in);
    (void)hipHostFree(c->h_out);
    (void)hipFree(c->d_ws);
    (void)hipFree(c->m_buf);
    (void)hipFree(c->m_ad);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int sg_ctx_set_iv(sg_ctx* c, const uint8_t iv[12]) {
    if (!c || !iv) return fail(SG_E_ARG, "NULL argument%s");
    std::lock_guard<std::mutex> lk(c->mu);
    sg::DeviceGuard dg(c->device);
    if (!dg.ok) return fail(SG_E_HIP, "hipSetDevice failed%s");
    SG_HIP(hipMemcpy(c->d_key + sg::kIvOff, iv, 12, hipMemcpyHostToDevice));
    std::memcpy(c->iv, iv, 12);
    c->has_iv = true;
    return SG_OK;
}

// key and IV of c->secret (after one ratchet step with update) onto the device; c->mu held
static int install_traffic_keys(sg_ctx* c, int update) {
    uint8_t key[32], iv[12];
    int rc = sg_tls13_traffic_keys(1, c->secret, key, iv, update, 1);
    if (rc != SG_OK) return rc;
    sg::DeviceGuard dg(c->device);
    if (!dg.ok) return fail(SG_E_HIP, "hipSetDevice failed%s");
    SG_HIP(hipMemcpy(c->d_key, key, 32, hipMemcpyHostToDevice));
    SG_HIP(hipMemcpy(c->d_key + sg::kIvOff, iv, 12, hipMemcpyHostToDevice));
    std::memcpy(c->iv, iv, 12);
    c->has_iv = true;
    return SG_OK;
}

int sg_ctx_set_traffic_secret(sg_ctx* c, const uint8_t secret[32]) {
    if (!c || !secret) return fail(SG_E_ARG, "NULL argument%s");
    std::lock_guard<std::mutex> lk(c->mu);
    std::memcpy(c->secret, secret, 32);
    c->has_secret = true;
    return install_traffic_keys(c, 0);
}

int sg_ctx_key_update(sg_ctx* c) {
    if (!c) return fail(SG_E_ARG, "NULL argument%s");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_secret) return fail(SG_E_ARG, "the context has no traffic secret (sg_ctx_set_traffic_secret)%s");
    return install_traffic_keys(c, 1);
}

int sg_tls13_traffic_keys_dev(const sg_tls13_keys* k) {
    if (!k) return fail(SG_E_ARG, "sg_tls13_keys is NULL%s");
    static_assert(sizeof(sg_tls13_keys) == 56, "sg_tls13_keys layout");
    if (k->flags & ~SG_TLS13_KEYS_UPDATE) return fail(SG_E_ARG, "unknown flags in sg_tls13_keys%s");
    const bool update = (k->flags & SG_TLS13_KEYS_UPDATE) != 0u;
    if (!k->secrets) return fail(SG_E_ARG, "secrets is NULL%s");
    if (((uintptr_t)k->secrets | (uintptr_t)k->keys | (uintptr_t)k->ivs | (uintptr_t)k->index) & 3u)
        return fail(SG_E_ARG, "secrets, keys, ivs and index must be 4-byte aligned%s");
    if (!k->keys && !k->ivs && !update) return fail(SG_E_ARG, "nothing to do: no keys, no ivs and no update%s");
    if (!k->index && k->count > k->rows) return fail(SG_E_ARG, "count exceeds rows without an index%s");
    if (k->count == 0) return SG_OK;
    SG_HIP(sg::launch_tls13_keys(k->count, k->rows, update, k->index, k->secrets, k->keys, k->ivs,
                                 (hipStream_t)k->stream));
    if (!k->stream) SG_HIP(hipStreamSynchronize(nullptr));
    return SG_OK;
}

int sg_gather_records(const uint8_t* src, uint32_t stride, const uint8_t* status, const uint32_t* content_len,
                      uint32_t count, uint8_t* dst, int use_base, const sg_gather_cursor* in, sg_gather_cursor* out,
                      uint32_t* result, void* stream) {
    if (count > 256u) return fail(SG_E_ARG, "at most 256 records per gather%s");
    if (!in || !out || in == out || !result) return fail(SG_E_ARG, "NULL cursor or result%s");
    if (count && (!src || !status || !content_len)) return fail(SG_E_ARG, "NULL argument%s");
    if (count && (stride < SG_RECORD_MAX_LEN || (stride & 15u) || ((uintptr_t)src & 15u)))
        return fail(SG_E_ARG, "src must be 16-byte aligned, stride a multiple of 16 and at least 2^14%s");
    if (((uintptr_t)content_len & 3u) || ((uintptr_t)result & 3u) || (((uintptr_t)in | (uintptr_t)out) & 7u))
        return fail(SG_E_ARG, "misaligned content_len, result or cursor%s");
    if (count == 0) return fail(SG_E_ARG, "an empty gather has no result: count must be 1..256%s");
    SG_HIP(sg::launch_gather(src, stride, status, content_len, count, dst, use_base != 0, in, out, result,
                             (uint64_t)count * SG_RECORD_MAX_LEN, (hipStream_t)stream));
    if (!stream) SG_HIP(hipStreamSynchronize(nullptr));
    return SG_OK;
}

static int single(sg_ctx* c, bool open, const uint8_t* nonce, size_t nonce_len, const uint8_t* in,
                  size_t in_len, const uint8_t* ad, size_t adlen, uint8_t* out) {
    if (!c) return fail(SG_E_ARG, "context is NULL%s");
    if (nonce_len != SG_NONCE_LEN || !nonce) return fail(SG_E_ARG, "nonce must be 8 bytes%s");
    if (adlen > SG_MAX_AD_LEN || (adlen && !ad)) return fail(SG_E_ARG, "bad additional data%s");
    if (in_len && !in) return fail(SG_E_ARG, "NULL buffer%s");
    if (open && in_len < SG_MAC_LEN) return SG_E_SHORT;  // chacha20_poly1305.rs:68-70
    const size_t n = open ? in_len - SG_MAC_LEN : in_len;
    if (!out && (open ? n : n + SG_MAC_LEN)) return fail(SG_E_ARG, "NULL buffer%s");  // empty pt: out may be NULL
    if (n > SG_MAX_RECORD_LEN) return fail(SG_E_ARG, "record longer than SG_MAX_RECORD_LEN%s");

    std::lock_guard<std::mutex> lk(c->mu);
    sg::DeviceGuard dg(c->device);
    if (!dg.ok) return fail(SG_E_HIP, "hipSetDevice failed%s");
    std::memcpy(c->h_in, nonce, 8);
    if (adlen) std::memcpy(c->h_in + sg::kSingleAdOff, ad, adlen);
    if (in_len) std::memcpy(c->h_in + sg::kSingleInOff, in, in_len);
    // the kernels read nonce | ad | record from the pinned block and write
    // status | output into the pinned out block over PCIe (one record is a few
    // KiB; two copy launches cost more than the transfer)
    uint8_t* src = c->h_in;
    uint8_t* dst = c->h_out;

    sg_batch b;
    std::memset(&b, 0, sizeof b);
    b.count = 1;
    b.keys = c->d_key;
    b.num_keys = 1;
    b.nonces = src;
    b.ads = src + sg::kSingleAdOff;
    b.ad_len = (uint32_t)adlen;
    b.ad_stride = (uint32_t)adlen;
    b.in = src + sg::kSingleInOff;
    b.in_stride = in_len;
    b.out = dst + sg::kSingleOutOff;
    b.out_stride = in_len + 16;
    b.uniform_len = (uint32_t)in_len;
    b.status = dst;
    b.stream = c->stream;
    b.workspace = c->d_ws;
    b.workspace_size = sg_workspace_size(1);
    // a failed open's plaintext is withheld on the host below: no device scrub
    b.flags = open ? SG_BATCH_KEEP_FAILED : 0u;
    int rc = open ? sg_open_batch(&b) : sg_seal_batch(&b);
    if (rc != SG_OK) return rc;
    const size_t out_len = open ? n : n + SG_MAC_LEN;
    SG_HIP(hipStreamSynchronize(c->stream));
    const uint8_t st = open ? c->h_out[0] : 0;
    if (open && st != 0) {
        if (n) std::memset(out, 0, n);  // the reference releases no plaintext with Err
        return st == 2 ? SG_E_SHORT : SG_E_BAD_MAC;
    }
    if (out_len) std::memcpy(out, c->h_out + sg::kSingleOutOff, out_len);
    return SG_OK;
}

int sg_seal(sg_ctx* c, const uint8_t* nonce, size_t nonce_len, const uint8_t* pt, size_t n,
            const uint8_t* ad, size_t adlen, uint8_t* out) {
    return single(c, false, nonce, nonce_len, pt, n, ad, adlen, out);
}

int sg_open(sg_ctx* c, const uint8_t* nonce, size_t nonce_len, const uint8_t* in, size_t in_len,
            const uint8_t* ad, size_t adlen, uint8_t* out) {
    return single(c, true, nonce, nonce_len, in, in_len, ad, adlen, out);
}

int sg_seal_batch(const sg_batch* b) { return run_batch(b, {RecordForm::kDraft}, false); }
int sg_open_batch(const sg_batch* b) { return run_batch(b, {RecordForm::kDraft}, true); }

static int run_batch_rfc8439(const sg_batch* b, const sg_batch_rfc8439* x, bool open) {
    if (!x) return fail(SG_E_ARG, "sg_batch_rfc8439 is NULL%s");
    return run_batch(b, {RecordForm::kRfc8439, x->flags, x->ivs}, open);
}
int sg_seal_batch_rfc8439(const sg_batch* b, const sg_batch_rfc8439* x) { return run_batch_rfc8439(b, x, false); }
int sg_open_batch_rfc8439(const sg_batch* b, const sg_batch_rfc8439* x) { return run_batch_rfc8439(b, x, true); }

static int run_batch_tls13(const sg_batch* b, const sg_batch_tls13* x, bool open) {
    if (!x) return fail(SG_E_ARG, "sg_batch_tls13 is NULL%s");
    return run_batch(b, {RecordForm::kTls13, x->flags, x->ivs, x->inner_type, x->content_len}, open);
}
int sg_seal_batch_tls13(const sg_batch* b, const sg_batch_tls13* x) { return run_batch_tls13(b, x, false); }
int sg_seal_batch_tls13_ex(const sg_batch* b, const sg_batch_tls13* x, const sg_tls13_seal_opts* o) {
    if (!x) return fail(SG_E_ARG, "sg_batch_tls13 is NULL%s");
    if (!o) return fail(SG_E_ARG, "sg_tls13_seal_opts is NULL%s");
    BatchForm f{RecordForm::kTls13, x->flags, x->ivs, x->inner_type, x->content_len};
    f.inner_types = o->inner_types;
    f.pad_to = o->pad_to;
    f.oflags = o->flags;
    return run_batch(b, f, false);
}
uint32_t sg_tls13_inner_len(uint32_t len, uint32_t pad_to) { return sg::tls13_inner_len(len, pad_to); }
int sg_open_batch_tls13(const sg_batch* b, const sg_batch_tls13* x) { return run_batch_tls13(b, x, true); }
int sg_batch_tls13_route(const sg_batch* b, int open) {
    const int rc = validate_tls13(b, open != 0);
    if (rc != SG_OK) return rc;
    return wpr_eligible(b, RecordForm::kTls13, open != 0) ? 1 : 0;
}

int sg_fill_records(uint8_t* buf, uint64_t stride, uint32_t len, uint32_t count, uint64_t seed, uint64_t j0,
                    void* stream) {
    if (!buf && count) return fail(SG_E_ARG, "buf is NULL%s");
    SG_HIP(sg::launch_fill(buf, stride, len, count, seed, j0, (hipStream_t)stream));
    if (!stream) SG_HIP(hipStreamSynchronize(nullptr));
    return SG_OK;
}

int sg_compare_records(const uint8_t* a, uint64_t sa, const uint8_t* b, uint64_t sb, uint32_t len,
                       uint32_t count, unsigned long long* mism, void* stream) {
    if ((!a || !b || !mism) && count) return fail(SG_E_ARG, "NULL pointer%s");
    SG_HIP(sg::launch_compare(a, sa, b, sb, len, count, mism, (hipStream_t)stream));
    if (!stream) SG_HIP(hipStreamSynchronize(nullptr));
    return SG_OK;
}

int sg_set_lockstep(int enable) { return sg::set_wpr(enable); }
int sg_set_packed(int enable) { return sg::set_pack(enable); }
int sg_set_tls13_buckets(int enable) { return sg::set_tls13_buckets(enable); }

int sg_last_batch_routes(sg_batch_routes* out) {
    if (!out) return fail(SG_E_ARG, "sg_batch_routes is NULL%s");
    static_assert(sizeof(sg_batch_routes) == 4u * sg::kRouteWords, "sg_batch_routes layout");
    uint32_t w[sg::kRouteWords];
    sg::routes_get(w);
    std::memcpy(out, w, sizeof w);
    return SG_OK;
}

int sg_set_timing(int enable) {
    std::lock_guard<std::mutex> lk(g_timing_mu);
    for (auto& t : g_timed) {
        (void)hipEventSynchronize(t.e2);
        for (hipEvent_t e : {t.e0, t.mid, t.e2}) g_event_pool.push_back(e);
    }
    g_timed.clear();
    g_timing = enable != 0;
    return SG_OK;
}

int sg_timing_read(double* seal_ms, double* open_ms, double* keying_ms, uint32_t* n_seal, uint32_t* n_open,
                   uint32_t* n_keying) {
    std::lock_guard<std::mutex> lk(g_timing_mu);
    double sum[3] = {0, 0, 0};
    uint32_t cnt[3] = {0, 0, 0};
    for (auto& t : g_timed) {
        SG_HIP(hipEventSynchronize(t.e2));
        float key_ms = 0.f, rec_ms = 0.f;
        SG_HIP(hipEventElapsedTime(&key_ms, t.e0, t.mid));
        SG_HIP(hipEventElapsedTime(&rec_ms, t.mid, t.e2));
        sum[0] += key_ms, sum[t.open ? 2 : 1] += rec_ms;  // kind 0: keying, 1: seal, 2: open
        cnt[0] += 1, cnt[t.open ? 2 : 1] += 1;
    }
    if (keying_ms) *keying_ms = cnt[0] ? sum[0] / cnt[0] : 0.0;
    if (seal_ms) *seal_ms = cnt[1] ? sum[1] / cnt[1] : 0.0;
    if (open_ms) *open_ms = cnt[2] ? sum[2] / cnt[2] : 0.0;
    if (n_keying) *n_keying = cnt[0];
    if (n_seal) *n_seal = cnt[1];
    if (n_open) *n_open = cnt[2];
    return SG_OK;
}

}  // extern "C"
