// sg_hkdf.hip -- the TLS 1.3 traffic keys of a whole key table in one launch
// (RFC 8446 section 7.3, with the KeyUpdate ratchet of section 7.2): a device
// table of traffic secrets becomes the `keys` / `ivs` tables that the record
// batch calls read, in place in HBM (sg_tls13_traffic_keys_dev, suruga_gpu.h).
//
// One lane per row, 256-thread groups on an exact grid; no LDS, no atomics, no
// wait on another lane.  The derivation itself is sg_hkdf.h's traffic_row, the
// code the host call runs: two HMAC midstates per secret and two compressions
// per label, 6 per row and 10 with the ratchet, each 64 unrolled rounds over a
// 16-word rolling schedule whose indices are all constants, so a row lives in
// registers from its load to its stores (no private segment: a secret is never
// spilled to memory).  The label blocks are compile-time constants and fold
// into the rounds as literals.
//
// Memory: a row is 8 dwords of secrets, 8 of keys and 3 of ivs, loaded and
// stored as dwords at 4-byte alignment; with no index list consecutive lanes
// take consecutive rows.  SHA-256 words are big-endian: one byte swap on load
// and one on store.  Row i + 1 of ivs starts 12 bytes after row i: exactly
// three dwords are stored there.  A lane whose row is out of range returns
// before it touches memory.
#include "sg_internal.h"

#include "sg_hkdf.h"

#include <stdint.h>

namespace sg {
namespace {

constexpr uint32_t kHkdfThreads = 256;

__global__ __launch_bounds__(kHkdfThreads) void sg_tls13_keys_kernel(uint32_t count, uint32_t rows, uint32_t update,
                                                                    const uint32_t* __restrict__ index,
                                                                    uint8_t* secrets, uint8_t* keys, uint8_t* ivs) {
    const uint32_t i = blockIdx.x * kHkdfThreads + threadIdx.x;
    if (i >= count) return;
    const uint32_t row = index ? index[i] : i;
    if (row >= rows) return;
    uint32_t* sp = reinterpret_cast<uint32_t*>(secrets + 32ull * row);
    uint32_t s[8], key[8], iv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = __builtin_bswap32(sp[j]);
    hkdf::traffic_row(s, update != 0u, keys != nullptr, ivs != nullptr, key, iv);
    if (update) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sp[j] = __builtin_bswap32(s[j]);
    }
    if (keys) {
        uint32_t* kp = reinterpret_cast<uint32_t*>(keys + 32ull * row);
#pragma unroll
        for (int j = 0; j < 8; ++j) kp[j] = __builtin_bswap32(key[j]);
    }
    if (ivs) {
        uint32_t* vp = reinterpret_cast<uint32_t*>(ivs + 12ull * row);
#pragma unroll
        for (int j = 0; j < 3; ++j) vp[j] = __builtin_bswap32(iv[j]);
    }
}

}  // namespace

hipError_t launch_tls13_keys(uint32_t count, uint32_t rows, bool update, const uint32_t* index, uint8_t* secrets,
                             uint8_t* keys, uint8_t* ivs, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (!secrets || (!index && count > rows) ||
        (((uintptr_t)secrets | (uintptr_t)keys | (uintptr_t)ivs | (uintptr_t)index) & 3u))
        return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)(((uint64_t)count + kHkdfThreads - 1u) / kHkdfThreads);
    hipLaunchKernelGGL(sg_tls13_keys_kernel, dim3(grid), dim3(kHkdfThreads), 0, s, count, rows, update ? 1u : 0u, index,
                       secrets, keys, ivs);
    return hipGetLastError();
}

}  // namespace sg
