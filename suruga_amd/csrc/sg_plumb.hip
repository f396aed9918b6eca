// sg_plumb.hip -- gfx950 plumbing kernels around the AEAD kernels: none of
// them computes ChaCha20 or Poly1305.
//
//   sg_fill_kernel / sg_compare_kernel   synthetic records and their comparison
//                                        (bench and tests)
//   sg_frame_kernel / sg_unframe_kernel  the record layer's wire image in HBM
//   sg_copy_out_kernel                   (sg_record.cpp, zero-copy path)
//   sg_scrub_kernel                      zeroes the output of failed opens
//   sg_strip_kernel                      TLS 1.3 open: inner type and content length
//   sg_gather_kernel                     TLS 1.3 read: the opened records' contents back to back
#include "sg_internal.h"
#include "../../include/suruga_gpu.h"  // SG_HEADER_LEN (record-layer framing kernels)

#include "sg_device.h"

#include <stdint.h>

namespace sg {
namespace {

using namespace dev;

// ---------------------------------------------------------------------------
// synthetic records + compare (bench/test plumbing)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void sg_fill_kernel(uint8_t* buf, uint64_t stride, uint32_t len,
                                                      uint32_t count, uint64_t seed, uint64_t j0) {
    const uint32_t wpr = (len + 7u) >> 3;  // 8-byte words per record
    const uint64_t total = (uint64_t)wpr * count;
    const bool aligned = ((stride | (uintptr_t)buf) & 7u) == 0u && (len & 7u) == 0u;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
         g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = g / wpr;
        const uint32_t w = (uint32_t)(g - j * wpr);
        const uint64_t v = splitmix64(seed ^ ((j0 + j) << 32) ^ (uint64_t)w);
        uint8_t* dst = buf + stride * j + 8ull * w;
        if (aligned) {
            *reinterpret_cast<uint64_t*>(dst) = v;
        } else {
            for (uint32_t b = 0; b < 8u && 8u * w + b < len; ++b) dst[b] = (uint8_t)(v >> (8 * b));
        }
    }
}

__global__ __launch_bounds__(256) void sg_compare_kernel(const uint8_t* a, uint64_t sa, const uint8_t* b,
                                                         uint64_t sb, uint32_t len, uint32_t count,
                                                         unsigned long long* mism) {
    __shared__ uint32_t bad;
    for (uint32_t rec = blockIdx.x; rec < count; rec += gridDim.x) {
        if (threadIdx.x == 0) bad = 0;
        __syncthreads();
        const uint8_t* pa = a + sa * rec;
        const uint8_t* pb = b + sb * rec;
        uint32_t diff = 0;
        const bool vec = (((uintptr_t)pa | (uintptr_t)pb) & 15u) == 0u;
        const uint32_t nvec = vec ? (len >> 4) : 0u;
        for (uint32_t i = threadIdx.x; i < nvec; i += blockDim.x) {
            const uint4 x = reinterpret_cast<const uint4*>(pa)[i];
            const uint4 y = reinterpret_cast<const uint4*>(pb)[i];
            diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
        }
        for (uint32_t i = nvec * 16u + threadIdx.x; i < len; i += blockDim.x) diff |= pa[i] ^ pb[i];
        if (diff) atomicOr(&bad, 1u);
        __syncthreads();
        if (threadIdx.x == 0 && bad) atomicAdd(mism, 1ull);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Record-layer framing on the device (sg_record.cpp, registered caller
// buffers): the wire image of a chunk is built / taken apart in HBM so that
// the host link moves one contiguous run each way (a strided host-side copy
// at the wire's 16,405-byte pitch measured ~1.3 s per GiB).  Wire record r
// sits at r * pitch: the 5-byte header (tls.rs:126-130) and its fragment.
// One thread per 4-byte word of the destination; source words are read
// aligned and funnel-shifted (v_alignbyte) into place.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ld_u32_unaligned(const uint8_t* p) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
    return __builtin_amdgcn_alignbyte(q[1], q[0], (uint32_t)(a & 3u));
}

// dst[0, image) <- headers and fragments; fragment r = src + r * src_stride,
// frag bytes (last: last_frag); hdr = type | major << 8 | minor << 16.
// rdiv: ceil(2^40 / pitch) (r = b * rdiv >> 40 is exact for b < 2^40 / pitch;
// launch_frame caps the image at 2^24 bytes, a chunk is ~4.2 MB).
__global__ __launch_bounds__(256) void sg_frame_kernel(const uint8_t* __restrict__ src, uint32_t src_stride,
                                                       uint8_t* __restrict__ dst, uint32_t pitch, uint64_t rdiv,
                                                       uint32_t count, uint32_t frag, uint32_t last_frag,
                                                       uint32_t hdr) {
    const uint32_t image = (count - 1u) * pitch + SG_HEADER_LEN + last_frag;
    const uint32_t nw = (image + 3u) >> 2;
    for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < nw; w += gridDim.x * 256u) {
        const uint32_t b0 = 4u * w;
        const uint32_t r = (uint32_t)(((uint64_t)b0 * rdiv) >> 40);
        const uint32_t o = b0 - r * pitch;  // offset in record r's wire slot
        const uint32_t fl = r + 1u == count ? last_frag : frag;
        if (o >= SG_HEADER_LEN && o + 4u <= SG_HEADER_LEN + fl) {  // inside one fragment
            reinterpret_cast<uint32_t*>(dst)[w] = ld_u32_unaligned(src + (uint64_t)r * src_stride + (o - SG_HEADER_LEN));
            continue;
        }
        uint32_t v = 0u;
        for (uint32_t k = 0; k < 4u; ++k) {  // header bytes and record boundaries
            const uint32_t b = b0 + k;
            if (b >= image) break;
            uint32_t rr = r, oo = o + k;
            if (oo >= pitch) {
                rr += 1u;
                oo -= pitch;
            }
            const uint32_t f = rr + 1u == count ? last_frag : frag;
            uint32_t byte;
            if (oo < SG_HEADER_LEN) {
                const uint32_t n = f;  // be16 fragment length
                byte = oo < 3u ? (hdr >> (8u * oo)) & 0xffu : (oo == 3u ? (n >> 8) & 0xffu : n & 0xffu);
            } else {
                byte = src[(uint64_t)rr * src_stride + (oo - SG_HEADER_LEN)];
            }
            v |= byte << (8u * k);
        }
        if (b0 + 4u <= image) {
            reinterpret_cast<uint32_t*>(dst)[w] = v;
        } else {
            for (uint32_t k = 0; b0 + k < image; ++k) dst[b0 + k] = (uint8_t)(v >> (8u * k));
        }
    }
}

// dst + r * dst_stride <- the frag bytes of wire record r (src + r * pitch + 5),
// count records of one fragment length.  The image is count * pitch bytes; a
// word whose aligned loads would reach past it is read byte by byte, so that
// no load leaves the image (src may be the caller's registered host buffer,
// read over the host link, whose next page need not be mapped).
__global__ __launch_bounds__(256) void sg_unframe_kernel(const uint8_t* __restrict__ src, uint32_t pitch,
                                                         uint8_t* __restrict__ dst, uint32_t dst_stride,
                                                         uint32_t count, uint32_t frag) {
    const uint32_t wpr = (frag + 3u) >> 2;  // destination words per record
    const uint32_t total = wpr * count;
    const uint64_t image = (uint64_t)count * pitch;
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < total; g += gridDim.x * 256u) {
        const uint32_t r = g / wpr, w = g - r * wpr;
        const uint64_t off = (uint64_t)r * pitch + SG_HEADER_LEN + 4u * w;
        const uint64_t a0 = ((uintptr_t)src + off) & 3u;  // the aligned loads cover [off - a0, off - a0 + 8)
        uint32_t v;
        if (off - a0 + 8u <= image && off >= a0) {
            v = ld_u32_unaligned(src + off);
        } else {
            v = 0u;
            for (uint32_t k = 0; k < 4u && off + k < image; ++k) v |= (uint32_t)src[off + k] << (8u * k);
        }
        uint8_t* d = dst + (uint64_t)r * dst_stride + 4u * w;
        if (4u * w + 4u <= frag) {
            *reinterpret_cast<uint32_t*>(d) = v;
        } else {
            for (uint32_t k = 0; 4u * w + k < frag; ++k) d[k] = (uint8_t)(v >> (8u * k));
        }
    }
}

// dst[0, n) <- src[0, n): the zero-copy read's plaintext from HBM into the
// caller's registered `out` over the host link (sg_record.cpp).  src is 4-byte
// aligned; dst may not be.  Every thread writes one 4-byte aligned word of dst
// (a funnel shift of two source words: the lanes' stores cover whole 256-byte
// segments) and the partial words at either end byte by byte, so that no store
// leaves [dst, dst + n), and no load leaves [src, src + n + 3] rounded to words.
__global__ __launch_bounds__(256) void sg_copy_out_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         uint64_t n) {
    const uint32_t a = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);  // bytes before dst's first aligned word
    const uint64_t nw = n > a ? (n - a) >> 2 : 0;                       // whole aligned words of dst
    const uint64_t tid = blockIdx.x * 256ull + threadIdx.x, nth = (uint64_t)gridDim.x * 256ull;
    if (tid < a && tid < n) dst[tid] = src[tid];
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + a);
    for (uint64_t w = tid; w < nw; w += nth) {
        const uint64_t b = a + 4u * w;  // source byte of the word's first byte
        const uint64_t q = b >> 2;
        const uint32_t lo = s32[q];
        const uint32_t hi = (b & 3u) ? s32[q + 1] : 0u;
        d32[w] = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(b & 3u));
    }
    const uint64_t t0 = a + 4u * nw;  // the byte tail
    if (tid < 4u && t0 + tid < n) dst[t0 + tid] = src[t0 + tid];
}

// Failed opens release no plaintext (chacha20_poly1305.rs:80-93 decrypts
// unconditionally but returns only Err on a tag mismatch): every record whose
// status is 1 (wrong mac) gets its output range zeroed after the open
// kernels, by the wave that finds it.  Records that failed are rare, so the
// launch costs one status byte per record when none did.  Status 2 (too
// short) has no output and status 3 (longer than max_len) was never written.
// Each wave scans 64 statuses and zeroes the output of every failed record in
// its ballot with the whole wave: byte stores up to the first 16-byte boundary,
// then 16-byte stores (1 KiB per wave instruction), then the byte tail
// (one byte per lane made a batch of failed 16 KiB records cost more
// than the AEAD launch itself).
__global__ __launch_bounds__(256) void sg_scrub_kernel(const KParams p) {
    const uint32_t base = blockIdx.x * 256u + (threadIdx.x & ~63u), lane = threadIdx.x & 63u;
    const uint32_t i = base + lane;
    uint64_t m = __ballot(i < p.count && p.status[i] == 1u);
    while (m) {
        const uint32_t rec = base + (uint32_t)__builtin_ctzll(m);
        m &= m - 1ull;
        const uint32_t len = record_len(p, rec);
        const uint32_t n = len >= 16u ? len - 16u : 0u;
        uint8_t* o = p.out + rec_out_off(p, rec);
        const uint32_t head = (uint32_t)((16u - ((uintptr_t)o & 15u)) & 15u);
        const uint32_t h = head < n ? head : n;
        if (lane < h) o[lane] = 0u;
        const uint32_t nv = (n - h) >> 4;  // whole 16-byte units after the head
        u32x4* ov = reinterpret_cast<u32x4*>(o + h);
        for (uint32_t v = lane; v < nv; v += 64u) ov[v] = u32x4{0u, 0u, 0u, 0u};
        const uint32_t t0 = h + 16u * nv;
        if (t0 + lane < n) o[t0 + lane] = 0u;
    }
}

// TLS 1.3 open (RFC 8446 section 5.2, 5.4): the inner plaintext is content ||
// type || zeros.  One thread per record, after the open kernels and the scrub:
// a record whose status is 0 is walked back from its end to its last non-zero
// byte, the inner type; the bytes before it are the content.  Records carry no
// padding as a rule, so the walk ends at its first byte; behind it, whole
// aligned dwords of zeros are taken at a time.  The walk never leaves the
// record's n = len - 16 output bytes.  A record of zeros alone (or an empty
// one) has no type: status 5.  Every other record gets type 0 and length 0.
__global__ __launch_bounds__(256) void sg_strip_kernel(const KParams p, uint8_t* __restrict__ inner_type,
                                                       uint32_t* __restrict__ content_len) {
    const uint32_t rec = blockIdx.x * 256u + threadIdx.x;
    if (rec >= p.count) return;
    uint8_t ty = 0u;
    uint32_t cl = 0u;
    if (p.status[rec] == 0u) {
        const uint32_t len = record_len(p, rec);
        uint32_t k = len >= 16u ? len - 16u : 0u;  // the bytes [0, k) are still to be looked at
        const uint8_t* o = p.out + rec_out_off(p, rec);
        while (k) {
            if (k >= 4u && ((uintptr_t)(o + k) & 3u) == 0u && *reinterpret_cast<const uint32_t*>(o + k - 4u) == 0u) {
                k -= 4u;
                continue;
            }
            if (o[k - 1u]) break;
            --k;
        }
        if (k) {
            ty = o[k - 1u];
            cl = k - 1u;
        } else {
            p.status[rec] = 5u;  // SG_STATUS_NO_TYPE
        }
    }
    inner_type[rec] = ty;
    content_len[rec] = cl;
}

// TLS 1.3 read (sg_record.cpp): the contents of a chunk's opened records, back
// to back.  A record's content length exists only after the open and the strip,
// and its type byte (and padding) lies between its content and the next
// record's, so the host cannot fix output offsets before the kernels run as it
// does for the TLS 1.2 forms.  One launch per chunk of count <= 256 records,
// after the strip, on the chunk's stream:
//   ok      the first record whose status is not 0 or whose content is longer
//           than 2^14 (count if none; 0 if the incoming cursor has stopped)
//   pre[i]  the content bytes of the records before i (i <= ok)
//   dst[base + pre[i], + content_len[i]) <- record i's first content_len[i]
//           bytes, i < ok; base = the incoming cursor's offset (use_base) or 0
//   cout    {cin.offset + pre[ok], cin.stopped | (ok < count)}
//   result  {ok, pre[ok]}
// and no other byte of dst is written.  The chunks of a call run in order on
// one stream and hand the cursor on, so nothing behind a call's first failing
// record ever leaves device memory.
// Every workgroup scans the lengths into LDS; the grid then strides over the
// 4-byte aligned words of dst.  A word finds its record by binary search in the
// prefix; inside a record its source is two aligned words, funnel-shifted
// (ld_u32_unaligned's form, the second word only where the shift needs it: no
// load leaves the record's content rounded up to a word, which lies inside its
// slot as stride >= 2^14 is a multiple of 16); a word across a record seam,
// and the bytes before dst's first and after its last aligned word, are put
// together byte by byte.
constexpr uint32_t kGatherMax = 256;
static_assert(kGatherMax == 256, "one thread per record of a chunk");

// the byte at `pos` of the packed contents (pos < pre[kGatherMax])
__device__ __forceinline__ uint32_t gather_rec(const uint32_t* pre, uint32_t pos) {
    uint32_t r = 0u;  // the last record with pre[r] <= pos: it is not empty
    for (uint32_t step = kGatherMax / 2u; step; step >>= 1)
        if (pre[r + step] <= pos) r += step;
    return r;
}
__device__ __forceinline__ uint8_t gather_byte(const uint8_t* src, uint32_t stride, const uint32_t* pre,
                                               uint32_t pos) {
    const uint32_t r = gather_rec(pre, pos);
    return src[(uint64_t)r * stride + (pos - pre[r])];
}

__global__ __launch_bounds__(256) void sg_gather_kernel(const uint8_t* __restrict__ src, uint32_t stride,
                                                        const uint8_t* __restrict__ status,
                                                        const uint32_t* __restrict__ content_len, uint32_t count,
                                                        uint8_t* __restrict__ dst, uint32_t use_base,
                                                        const sg_gather_cursor* __restrict__ cin,
                                                        sg_gather_cursor* __restrict__ cout,
                                                        uint32_t* __restrict__ result) {
    __shared__ uint32_t pre[kGatherMax + 1u];
    __shared__ uint32_t first_bad;
    const uint32_t t = threadIdx.x;
    uint32_t cl = 0u;
    bool bad = false;
    if (t < count) {
        cl = content_len[t];
        bad = status[t] != 0u || cl > SG_RECORD_MAX_LEN;
    }
    if (t == 0u) first_bad = count;
    __syncthreads();
    if (bad) atomicMin(&first_bad, t);
    __syncthreads();
    const uint64_t base0 = cin->offset;
    const uint32_t stopped = cin->stopped;
    const uint32_t ok = stopped ? 0u : first_bad;
    // inclusive scan of the delivered records' lengths: pre[i + 1] = pre[i] + len_i
    if (t == 0u) pre[0] = 0u;
    pre[t + 1u] = t < ok ? cl : 0u;
    __syncthreads();
    for (uint32_t d = 1u; d < kGatherMax; d <<= 1) {
        const uint32_t x = t >= d ? pre[t + 1u - d] : 0u;
        __syncthreads();
        pre[t + 1u] += x;
        __syncthreads();
    }
    const uint32_t total = pre[kGatherMax];  // == pre[ok]: nothing is counted from record ok on

    uint8_t* d = dst + (use_base ? base0 : 0ull);
    const uint32_t a0 = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u);
    const uint32_t a = a0 < total ? a0 : total;  // bytes before d's first aligned word
    const uint32_t nw = (total - a) >> 2;        // whole aligned words of d
    const uint32_t tid = blockIdx.x * 256u + t, nth = gridDim.x * 256u;
    if (tid < a) d[tid] = gather_byte(src, stride, pre, tid);
    uint32_t* d32 = reinterpret_cast<uint32_t*>(d + a);
    for (uint32_t w = tid; w < nw; w += nth) {
        const uint32_t b = a + 4u * w;  // packed offset of the word's first byte
        const uint32_t r = gather_rec(pre, b);
        const uint32_t o = b - pre[r];
        uint32_t v;
        if (o + 4u <= pre[r + 1u] - pre[r]) {  // inside one record
            const uint32_t* q = reinterpret_cast<const uint32_t*>(src + (uint64_t)r * stride + (o & ~3u));
            const uint32_t lo = q[0];
            const uint32_t hi = (o & 3u) ? q[1] : 0u;
            v = __builtin_amdgcn_alignbyte(hi, lo, o & 3u);
        } else {  // a record seam (empty records between its two sides are skipped)
            v = 0u;
            uint32_t rr = r;
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t pos = b + k;  // < total = pre[kGatherMax]: the walk ends
                while (pre[rr + 1u] <= pos) ++rr;
                v |= (uint32_t)src[(uint64_t)rr * stride + (pos - pre[rr])] << (8u * k);
            }
        }
        d32[w] = v;
    }
    const uint32_t t0 = a + 4u * nw;  // the byte tail
    if (tid < 4u && t0 + tid < total) d[t0 + tid] = gather_byte(src, stride, pre, t0 + tid);
    if (tid == 0u) {
        cout->offset = base0 + total;
        cout->stopped = (stopped || ok < count) ? 1u : 0u;
        cout->_pad = 0u;
        result[0] = ok;
        result[1] = total;
    }
}

}  // namespace

hipError_t launch_gather(const uint8_t* src, uint32_t stride, const uint8_t* status, const uint32_t* content_len,
                         uint32_t count, uint8_t* dst, bool use_base, const sg_gather_cursor* cin,
                         sg_gather_cursor* cout, uint32_t* result, uint64_t capacity, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (count > kGatherMax || stride < SG_RECORD_MAX_LEN || (stride & 15u) || ((uintptr_t)src & 15u) ||
        ((uintptr_t)content_len & 3u) || ((uintptr_t)result & 3u) || (((uintptr_t)cin | (uintptr_t)cout) & 7u) ||
        !src || !status || !content_len || !cin || !cout || cin == cout || !result)
        return hipErrorInvalidValue;
    // capacity: the most the chunk can deliver; every thread a few words of it
    uint64_t grid = (capacity / 4u + 255u) / 256u;
    grid = grid < 256u ? (grid ? grid : 1u) : 256u;
    hipLaunchKernelGGL(sg_gather_kernel, dim3((uint32_t)grid), dim3(256), 0, s, src, stride, status, content_len, count,
                       dst, use_base ? 1u : 0u, cin, cout, result);
    return hipGetLastError();
}

hipError_t launch_scrub(const KParams& p, hipStream_t s) {
    if (p.count == 0) return hipSuccess;
    hipLaunchKernelGGL(sg_scrub_kernel, dim3((p.count + 255u) / 256u), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_strip(const KParams& p, uint8_t* inner_type, uint32_t* content_len, hipStream_t s) {
    if (p.count == 0) return hipSuccess;
    hipLaunchKernelGGL(sg_strip_kernel, dim3((p.count + 255u) / 256u), dim3(256), 0, s, p, inner_type, content_len);
    return hipGetLastError();
}

hipError_t launch_frame(const uint8_t* src, uint32_t src_stride, uint8_t* dst, uint32_t pitch, uint32_t count,
                        uint32_t frag, uint32_t last_frag, uint32_t hdr, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const uint32_t image = (count - 1u) * pitch + SG_HEADER_LEN + last_frag;
    if (image >= (1u << 24) || (src_stride & 3u) || ((uintptr_t)dst & 3u)) return hipErrorInvalidValue;
    const uint64_t rdiv = ((1ull << 40) + pitch - 1u) / pitch;
    uint32_t grid = ((image + 3u) / 4u + 255u) / 256u;
    grid = grid < 4096u ? grid : 4096u;
    hipLaunchKernelGGL(sg_frame_kernel, dim3(grid), dim3(256), 0, s, src, src_stride, dst, pitch, rdiv, count, frag,
                       last_frag, hdr);
    return hipGetLastError();
}

hipError_t launch_copy_out(const uint8_t* src, uint8_t* dst, uint64_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if ((uintptr_t)src & 3u) return hipErrorInvalidValue;
    uint64_t grid = (n / 4u + 255u) / 256u;
    grid = grid < 4096u ? (grid ? grid : 1u) : 4096u;
    hipLaunchKernelGGL(sg_copy_out_kernel, dim3((uint32_t)grid), dim3(256), 0, s, src, dst, n);
    return hipGetLastError();
}

hipError_t launch_unframe(const uint8_t* src, uint32_t pitch, uint8_t* dst, uint32_t dst_stride, uint32_t count,
                          uint32_t frag, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if ((dst_stride & 3u) || ((uintptr_t)dst & 3u)) return hipErrorInvalidValue;
    uint32_t grid = (((frag + 3u) / 4u) * count + 255u) / 256u;
    grid = grid < 4096u ? grid : 4096u;
    hipLaunchKernelGGL(sg_unframe_kernel, dim3(grid), dim3(256), 0, s, src, pitch, dst, dst_stride, count, frag);
    return hipGetLastError();
}

hipError_t launch_fill(uint8_t* buf, uint64_t stride, uint32_t len, uint32_t count, uint64_t seed,
                       uint64_t j0, hipStream_t s) {
    const uint64_t words = (uint64_t)((len + 7u) >> 3) * count;
    uint64_t grid = (words + 255u) / 256u;
    if (grid > 65536u) grid = 65536u;
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(sg_fill_kernel, dim3((uint32_t)grid), dim3(256), 0, s, buf, stride, len, count, seed, j0);
    return hipGetLastError();
}

hipError_t launch_compare(const uint8_t* a, uint64_t sa, const uint8_t* b, uint64_t sb, uint32_t len,
                          uint32_t count, unsigned long long* mism, hipStream_t s) {
    uint32_t grid = count < 16384u ? count : 16384u;
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(sg_compare_kernel, dim3(grid), dim3(256), 0, s, a, sa, b, sb, len, count, mism);
    return hipGetLastError();
}

}  // namespace sg
