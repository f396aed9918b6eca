// sg_host.h -- private host-side declarations shared by the C-ABI translation
// units (sg_capi.cpp, sg_record.cpp, sg_msg_capi.cpp).  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/suruga_gpu.h"
#include "sg_err.h"

namespace sg {

int hip_fail(hipError_t e, const char* where);

struct RecordStaging;                   // sg_record.cpp
void record_staging_free(RecordStaging* rs);

// A buffer of >= need bytes from the library's workspace cache (sg_capi.cpp)
// for one call on stream s of the current device, which must be a gfx950 part;
// its reuse is ordered on the device.  scratch_release after the call's launches.
int scratch_acquire(size_t need, hipStream_t s, void** ptr, void** handle);
void scratch_release(void* handle, hipStream_t s, bool launched);

// Makes `dev` the calling thread's current HIP device for a scope and restores
// the previous one on exit, so a context call never leaves the caller's thread
// on another device.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

}  // namespace sg

#define SG_HIP(call)                                                \
    do {                                                            \
        hipError_t e_ = (call);                                     \
        if (e_ != hipSuccess) return sg::hip_fail(e_, #call);       \
    } while (0)

// One context per direction (Aead::new_encryptor / new_decryptor): the key on
// the device, staging for single records, and (lazily) the record-layer
// pipeline of sg_write_records / sg_read_records.
// Single-record staging (sg_seal / sg_open): one pinned host block per
// direction that the kernels read and write over the host link, so a call is
// the keying and AEAD launches and one stream sync:
//   in  block: nonce @0 | ad @kSingleAdOff | record @kSingleInOff
//   out block: status @0 | output @kSingleOutOff
namespace sg {
constexpr size_t kSingleAdOff = 16;
constexpr size_t kSingleInOff = 512;
constexpr size_t kSingleOutOff = 64;
constexpr size_t kIvOff = 48;  // in d_key's 64 bytes: key @0, the message path's status @32, the IV @48
}  // namespace sg
struct sg_ctx {
    int device = 0;
    uint8_t* d_key = nullptr;      // 32 B
    uint8_t* h_in = nullptr;       // pinned blocks the kernels read and write directly:
                                   // kSingleInOff / kSingleOutOff + SG_MAX_RECORD_LEN + 64
    uint8_t* h_out = nullptr;
    void* d_ws = nullptr;
    hipStream_t stream = nullptr;
    sg::RecordStaging* rec = nullptr;
    // long messages (sg_seal_msg / sg_open_msg, sg_msg_capi.cpp): device buffers that
    // only grow -- the message (sealed and opened in place) and its AD; the
    // open status byte is d_key[32]
    uint8_t* m_buf = nullptr;
    size_t m_cap = 0;
    uint8_t* m_ad = nullptr;
    size_t m_ad_cap = 0;
    // the write IV (sg_ctx_set_iv) of the RFC 7905 / TLS 1.3 record calls: the
    // host copy (explicit-mode nonces); the device copy is d_key + kIvOff
    uint8_t iv[12] = {0};
    bool has_iv = false;
    // the TLS 1.3 traffic secret that key and IV were derived from
    // (sg_ctx_set_traffic_secret), kept for sg_ctx_key_update's ratchet
    uint8_t secret[32] = {0};
    bool has_secret = false;
    std::mutex mu;
};
