// sg_wpr_layout.h -- what the two wave-per-record kernels share: the record
// kernel (sg_wpr.hip) and its keying pre-pass (sg_wpr_keying.hip).  The wave's
// LDS slice, the geometry of the MAC stream and the keying table's layout in
// HBM; the table's words themselves (kW*) are in sg_internal.h.  Device code.
#pragma once

#include "sg_internal.h"

#include <stdint.h>

namespace sg {

constexpr uint32_t kWprWaves = 8;           // records per 512-thread workgroup
constexpr uint32_t kWprChunk = 4096;        // bytes per wave iteration
constexpr uint32_t kWprLines = 40;          // T digit lines per record
constexpr uint32_t kWprLineBytes = 48;
constexpr uint32_t kWprLinesOff = 2 * kWprChunk;  // two chunk buffers, then the T lines
// after the lines (offsets from the line area): 16 zero bytes read past the
// last line, the next record's descriptor (bucket launches), the received tag
constexpr uint32_t kWprDescOff = kWprLines * kWprLineBytes + 16;
constexpr uint32_t kWprRxOff = kWprDescOff + 48;
constexpr uint32_t kWprWaveLds = 2 * kWprChunk + kWprRxOff + 16;  // 10192
// eight waves and the workgroup's next-group slot: two workgroups per CU
constexpr uint32_t kWprWgLds = kWprWaves * kWprWaveLds + 16;
static_assert(2 * kWprWgLds <= 160 * 1024, "two workgroups per CU");
static_assert(kWprDescWords * 4 <= 48, "descriptor slot");

// Geometry of the MAC stream ad || le64(|ad|) || ct || le64(n), n a multiple
// of 16 (C1: n = 2^14).  A record of n < 2^14 bytes runs right-aligned in the
// 2^14-byte frame of the kernel (virtual offset 2^14 - n): shifting the
// ciphertext by a multiple of 16 shifts its MAC block indices and the block
// count B alike, so every ciphertext byte keeps its weight r^(B - b) 2^(8 k)
// and the MFMA part of the MAC is the same for every n; only the constant term
// (AD, length and pad blocks, bias) depends on n.
struct WprGeom {
    uint32_t o, sigma, beta, B, rem, delta, m;
};
// RFC 8439 (ad || 0.. || ct || 0.. || le64(|ad|) || le64(n)): the ciphertext
// starts on a block boundary, o = 16 ceil(adlen / 16), sigma = 0, and one full
// block closes the stream: B = beta + m + 1, rem = 16, delta = 0.
// (o and the stream length: sg_layout.h)
template <Construction C>
__device__ __forceinline__ WprGeom wpr_geom(uint32_t adlen, uint32_t n) {
    WprGeom g;
    g.o = ct_offset<C>(adlen);
    if constexpr (C == Construction::kRfc8439) {
        g.sigma = 0u;
        g.beta = g.o >> 4;
        g.m = n >> 4;
        g.B = g.beta + g.m + 1u;
        g.rem = 16u;
        g.delta = 0u;
        return g;
    }
    g.sigma = g.o & 15u;
    g.beta = g.o >> 4;
    const uint32_t L = stream_bytes<C>(adlen, n);
    g.B = (L + 15u) >> 4;
    g.rem = L - 16u * (g.B - 1u);
    g.m = n >> 4;                        // 16-byte ciphertext chunks
    g.delta = g.B - g.beta - 1u - g.m;  // 0 or 1
    return g;
}

// bytes >= lo of a little-endian word set: mask of the bytes whose index
// (4 w + byte) is >= lo
__device__ __forceinline__ uint32_t bytes_from(uint32_t w, uint32_t lo) {
    if (lo <= 4u * w) return 0xffffffffu;
    if (lo >= 4u * w + 4u) return 0u;
    return 0xffffffffu << (8u * (lo - 4u * w));
}

// p - (2^24 * sum_{c<32} 2^(8c) mod p) in radix 2^26: the seed of the 32 x 32
// accumulator, negated (tests/wpr_model.py keying: cj)
constexpr uint32_t kCJ0 = 0x1bd2d2bu, kCJ1 = 0x36f6f6fu, kCJ2 = 0x3dbdbdbu, kCJ3 = 0x2f6f6f6u, kCJ4 = 0x1bdbdbdu;

// Table layout in HBM (round 3): the records of eight consecutive slots (a
// record kernel's group) interleaved by 16-byte unit, unit u of slot 8 g + w
// at tab + 1280 g + 4 (u rows + w) words (rows = 8, or count mod 8 in the last
// group).  Each lane stores its own record unit by unit straight from
// registers (non-temporal: the table does not sit dirty in the caches while
// the record kernel streams) and every store instruction still writes whole
// 128-byte lines (a group's row of one unit), so the keying kernel needs no
// LDS staging and runs at the occupancy its registers allow; the record
// kernel's 40 unit reads per record touch lines that the other seven waves of
// its group read at the same time (the same 640 bytes per record from HBM).
__device__ __forceinline__ uint32_t* wpr_tab_unit(const WprList& wl, uint32_t slot, uint32_t u) {
    const uint32_t g = slot >> 3, w = slot & 7u;
    const uint32_t rows = g < (wl.count >> 3) ? 8u : (wl.count & 7u);
    return wl.tab + (uint64_t)g * (8u * kWprRecWords) + 4u * (u * rows + w);
}

}  // namespace sg
