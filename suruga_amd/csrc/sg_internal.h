// sg_internal.h -- shared between the HIP kernel files (sg_kernels.hip,
// sg_wpr.hip, sg_wpr_keying.hip, sg_pack.hip, sg_plumb.hip), the mixed-batch dispatcher
// (sg_dispatch.cpp) and the C-ABI host layer (sg_capi.cpp): the workspace and
// keying-record layouts, the kernel parameters and every launch_* function.
// Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sg_layout.h"

struct sg_gather_cursor;  // suruga_gpu.h

namespace sg {

constexpr uint32_t kThreads = 256;        // one record per 256-thread workgroup
constexpr uint32_t kKeyRecWords = 88;     // per-record keying output (u32 words, 352 B)
// keying record layout (u32 words): r[4] clamped Poly1305 r (radix 2^32),
// s[4] (second half of keystream block 0), then with R = r^k (k = MAC blocks
// per lane, see mac_geom in sg_kernels.hip) 5-limb radix-2^26 powers ordered so
// that a record with PL MAC lanes needs only a prefix (kKeyUsedWords(PL)):
//   R^0 (as hi[0]), lo[j] = R^j (j = 0..7), hi[i] = R^(8 i) (i = 1..7)
// MAC lane t scales its partial sum by R^(PL-1-t) = hi[e >> 3] lo[e & 7].
constexpr uint32_t kR32Off = 0;
constexpr uint32_t kSOff = 4;
__host__ __device__ constexpr uint32_t key_lo_off(uint32_t j) { return 13u + 5u * j; }
__host__ __device__ constexpr uint32_t key_hi_off(uint32_t i) { return i == 0u ? 8u : 48u + 5u * i; }
__host__ __device__ constexpr uint32_t key_used_words(uint32_t PL) {
    return PL <= 8u ? 13u + 5u * PL : 53u + 5u * (PL / 8u - 1u);
}
static_assert(key_used_words(64) == kKeyRecWords, "keying record layout");

// Keying record of the wave-per-record kernel (sg_wpr_keying.hip writes it, sg_wpr.hip reads it), u32 words; F26
// entries are 5 radix-2^26 limbs.  With delta = 0/1 from the geometry
// (wpr_geom), R = r^4 and T = r^128:
//   s[4]                                    second half of keystream block 0
//   ctot[5]                                 the record's constant term
//   rd[5][5]  = r^(1 + delta + u)          u = 0..4
//   tk[8][5]  = T^k                         k = 0..7
//   lo[8][5]  = R^b                         b = 0..7
//   hi[2][4][5] = 2^(32 h) R^(8 a)          h = 0..1, a = 0..3
constexpr uint32_t kWS = 0;
constexpr uint32_t kWCtot = 4;
constexpr uint32_t kWRd = 12;
constexpr uint32_t kWTk = 40;
constexpr uint32_t kWLo = 80;
constexpr uint32_t kWHi = 120;
constexpr uint32_t kWprRecWords = 160;
// Record descriptor of a listed wave-per-record record (mixed batches), u32
// words, indexed like the keying records by the record's slot in its bucket:
//   in_off[2] out_off[2] n rec key_index n14 n15 n13 clen type
// (n13: the nonce's first word, Construction::kRfc8439; 0 in the draft.  clen, type: the
// content length and the inner type of a TLS 1.3 bucket seal, n its inner length; else 0)
constexpr uint32_t kWprDescWords = 12;

// Kernel parameters (passed by value as kernarg).
struct KParams {
    const uint8_t* keys;
    const uint32_t* key_index;
    uint32_t num_keys;       // >= 1; key indices are clamped to num_keys - 1 (no read outside the table)
    const uint64_t* seq;
    uint64_t seq0;
    union {                  // (one kernarg slot: the TLS 1.3 form is TLS mode and never reads nonces)
        const uint8_t* nonces;       // explicit mode
        const uint8_t* inner_types;  // TLS 1.3 seal (sg_seal_batch_tls13_ex): the records' inner types [count], or
                                     // NULL: tls_hdr's low byte for every record
    };
    const uint8_t* ads;
    const uint8_t* in;
    const uint64_t* in_off;
    uint64_t in_stride;
    uint8_t* out;
    const uint64_t* out_off;
    uint64_t out_stride;
    const uint32_t* len;
    uint8_t* status;
    uint32_t* ws;            // count * kKeyRecWords (kWprRecWords for sg_wpr_keying.hip) keying records
    uint32_t uniform_len;
    uint32_t count;
    uint32_t ad_len;         // explicit mode
    union {                  // (likewise: the TLS 1.3 AD is the record header, built on the device)
        uint32_t ad_stride;  // explicit mode
        uint32_t pad_to;     // TLS 1.3 seal: the inner plaintext is tls13_inner_len(len, pad_to) bytes,
                             // content || type || zeros
    };
    uint32_t tls;            // 1 = SG_BATCH_TLS
    uint32_t tls_hdr;        // content_type | major << 8 | minor << 16
    uint32_t lds_rec_bytes;  // LDS bytes per record slot of the launched size class
    uint32_t wpr_mix;        // mixed batch: route eligible records to the wave-per-record buckets
    uint32_t pack_mix;       // mixed batch: route eligible small records to the packed kernel (sg_pack.hip)
    // RFC 8439 record batch (sg_*_batch_rfc8439); at the end: the offsets above stay
    const uint8_t* ivs;      // TLS mode under rfc: write IVs [num_keys][12] (RFC 7905), 4-byte aligned
    uint32_t rfc;            // 1 = RFC 8439 (Construction::kRfc8439 kernels), 0 = the draft
    // TLS 1.3 record batch (sg_*_batch_tls13, RFC 8446 section 5.2); at the end again
    uint32_t tls13;          // 1: rfc and tls are 1 too; AD = 17 03 03 be16(fragment length), seal appends
                             // the inner type byte (tls_hdr's low byte) to every record
};
// The TLS 1.3 seal options share the slots of two explicit-mode fields, so the struct is the
// size it was and every kernel argument behind it stays where it was: the kernels of the
// other record forms are the same code objects byte for byte, kernarg offsets included.
static_assert(sizeof(KParams) == 184, "KParams: the kernarg layout of every record kernel");

// Every record kernel exists in both constructions (Construction,
// sg_layout.h): the size classes, the uniform 16 KiB wave-per-record launch,
// the J = 2..4 buckets and the packed kernel, so a mixed TLS batch takes the
// same routes (KParams.wpr_mix / pack_mix) in either.
//
// The launchers' one selector: calls f(OPEN, C, T13) with the run-time triple
// (open, p.rfc, p.tls13) as compile-time constants (OPEN.value and T13.value
// bools, T13 only with C.value == Construction::kRfc8439), so a launcher names
// its kernel once, as K<OPEN.value, ..., C.value, T13.value> (the J = 2..4 bucket record
// kernel: T13 on seal only; its open is the RFC 8439 form).  The message launchers: (rfc, open), f(OPEN, C).
template <class F>
inline void with_form(bool rfc, bool open, F&& f) {
    constexpr std::integral_constant<Construction, Construction::kDraft> D{};
    constexpr std::integral_constant<Construction, Construction::kRfc8439> R{};
    if (rfc) open ? f(std::true_type{}, R) : f(std::false_type{}, R);
    else open ? f(std::true_type{}, D) : f(std::false_type{}, D);
}
template <class F>
inline void with_form(const KParams& p, bool open, F&& f) {
    constexpr std::integral_constant<Construction, Construction::kRfc8439> R{};
    if (p.tls13) open ? f(std::true_type{}, R, std::true_type{}) : f(std::false_type{}, R, std::true_type{});
    else with_form(p.rfc != 0u, open, [&](auto OPEN, auto C) { f(OPEN, C, std::false_type{}); });
}

// Size classes of the AEAD kernel: class c (0..7) holds records of
// n <= 128 << c bytes (class 7: the rest, up to SG_MAX_RECORD_LEN) and gives
// each record L = 2 << c lanes, one 64-byte ChaCha20 block per lane for
// c < 7; the MAC runs on PL = min(L, 64) lanes.  A 256-thread workgroup serves
// 256 / L records.  Mixed sizes are bucketed on the device (sg_classify_kernel).
constexpr uint32_t kNumClasses = 8;
// Mixed batches also route TLS records of 4 KiB < n <= 16 KiB, n a multiple of
// 64, 16-byte aligned, to the wave-per-record kernel (sg_wpr.hip): bucket
// J = ceil(n / 4096) = 2..4 (the record's chunk count), lists kNumClasses + J - 2.
constexpr uint32_t kWprBuckets = 3;
constexpr uint32_t kWprMinJ = 2;
// ... and TLS records of 64 B <= n <= 4 KiB, n a multiple of 64, 16-byte
// aligned, to the packed kernel (sg_pack.hip): list kPackList.  The TLS 1.3
// form takes this route (n: the inner length) and, under sg_set_tls13_buckets,
// the buckets for padded records of 4 KiB < n <= 16 KiB (off by default).
constexpr uint32_t kPackList = kNumClasses + kWprBuckets;
constexpr uint32_t kNumLists = kPackList + 1u;
constexpr uint32_t kListGridPerCU = 8;   // workgroups per CU for list-driven launches

__host__ __device__ inline uint32_t size_class(uint32_t n) {
    if (n <= 128u) return 0u;
    const uint32_t c = 32u - (uint32_t)__builtin_clz((n - 1u) >> 7);
    return c < 7u ? c : 7u;
}
__host__ __device__ constexpr uint32_t class_lanes(uint32_t c) { return 2u << c; }
__host__ __device__ constexpr uint32_t class_mac_lanes(uint32_t c) { return class_lanes(c) < 64u ? class_lanes(c) : 64u; }
__host__ __device__ constexpr uint32_t class_max(uint32_t c) { return c < 7u ? 128u << c : 0xffffffffu; }
// LDS bytes of one record slot: virtual-block space (16 bytes x max virtual blocks
// 2*PL) | ad || le64 (16-rounded) | ct (64-rounded) | le64(n) + zeros
// The slot is the draft's (its ciphertext offset, 16-rounded).  The RFC 8439
// stream fits it: its ciphertext offset is never larger, and behind the
// ciphertext it writes at most 15 zeros and the 16-byte length block, 31 <= 64.
__host__ __device__ inline uint32_t lds_rec_bytes(uint32_t cls, uint32_t adlen, uint32_t max_n) {
    const uint32_t PL = class_mac_lanes(cls);
    return 32u * PL + ((ct_offset<Construction::kDraft>(adlen) + 15u) & ~15u) + ((max_n + 63u) & ~63u) + 64u;
}

// Wave-per-record kernel (sg_wpr.hip): uniform batches of full 16 KiB TLS
// records (n = RECORD_MAX_LEN = 2^14, tls.rs:32, the size TlsWriter::write_data
// gives every record but a stream's tail), 16-byte aligned strided layout, any
// AD length.  One wave per record, eight records per 512-thread workgroup.
// (kWprN: sg_layout.h)
// TLS 1.3 (KParams.tls13): full records of 2^14 content bytes and the inner type
// byte, n = 16385.  The record kernel runs the 2^14 bytes as above; the keying
// kernel takes byte 2^14 (keystream block 257) and its MAC block.
constexpr uint32_t kWprTailBlock = kWprN / 64u + 1u;
// Workspace (u32 words) for a batch of `count` records:
//   [0, 88 count)                   size-class keying records (by record index)
//   [88 count, 248 count)           wave-per-record keying records (by slot)
//   [248 count, 260 count)          wave-per-record descriptors (by slot)
//   [260 count, 272 count)          kNumLists record lists
//   then kNumLists populations, the over-long count, kWprBuckets + 1 group
//   counters and the packed launch's run counter
constexpr uint32_t kWsWprTab = kKeyRecWords;
constexpr uint32_t kWsWprDesc = kWsWprTab + kWprRecWords;
constexpr uint32_t kWsLists = kWsWprDesc + kWprDescWords;
constexpr uint32_t kWsRecWords = kWsLists + kNumLists;
constexpr uint32_t kWsTailWords = kNumLists + 1u + kWprBuckets + 2u;
__host__ __device__ inline uint64_t ws_words(uint32_t count) { return (uint64_t)count * kWsRecWords + kWsTailWords; }
// the counts / counters tail
__host__ __device__ inline uint32_t* ws_tail(uint32_t* ws, uint32_t count) { return ws + (uint64_t)count * kWsRecWords; }
constexpr uint32_t kTailOver = kNumLists;           // records longer than max_n
constexpr uint32_t kTailCtr = kNumLists + 1u;       // + b: group counter of wpr bucket b, + kWprBuckets: uniform C1 launch
constexpr uint32_t kTailPackCtr = kTailCtr + kWprBuckets + 1u;  // run counter of the packed launch
hipError_t device_cus(int* cus);  // CUs of the current device (cached; sg_dispatch.cpp)

// A wave-per-record bucket launch (mixed batch) or the uniform launch (list NULL).
struct WprList {
    const uint32_t* list;    // record indices (bucket list) or NULL: slot = record
    uint32_t count;          // records in the launch
    uint32_t* tab;           // keying records, kWprRecWords per slot
    uint32_t* desc;          // descriptors, kWprDescWords per slot (list launches)
    uint32_t* ctr;           // the launch's group counter (zeroed by its keying kernel)
};

// Keying jobs of the size-class keying kernel: njobs == 0 keys every record
// of the batch by index, otherwise the records of the listed size classes.
struct KeyJobs {
    const uint32_t* list[kNumClasses];
    uint32_t count[kNumClasses];
    uint32_t blk0[kNumClasses];  // first 64-record block of each job
    uint32_t njobs;
};
constexpr uint32_t kKeyingThreads = 64;  // records per keying workgroup

// Launches of the size-class kernels (sg_kernels.hip).  Keying: `grid` blocks
// of kKeyingThreads records over `jobs`, or every record of the batch by index.
hipError_t launch_keying(const KParams& p, bool open, const KeyJobs& jobs, uint32_t grid, hipStream_t s);
hipError_t launch_keying_all(const KParams& p, bool open, hipStream_t s);
// bucket the batch into the kNumLists lists (populations and the over-long
// count in counts); records longer than max_n get no list
hipError_t launch_classify(const KParams& p, bool open, uint32_t* lists, uint32_t* counts, uint32_t max_n,
                           hipStream_t s);
// size class c: the whole batch by index (list NULL), or the listed records
// -- n_exact: the class population when the host knows it (exact grid), or
// UINT32_MAX for a persistent grid capped at kListGridPerCU workgroups per CU
hipError_t launch_class(uint32_t c, const KParams& q, bool open, const uint32_t* list, const uint32_t* cnt,
                        uint32_t n_exact, hipStream_t s);

inline hipError_t mark(hipEvent_t ev, hipStream_t s) { return ev ? hipEventRecord(ev, s) : hipSuccess; }

bool wpr_enabled();  // sg_set_lockstep / SG_LOCKSTEP environment switch (sg_dispatch.cpp, like the next)
int set_wpr(int enable);
// sg_set_tls13_buckets / SG_TLS13_BUCKETS (off by default): padded TLS 1.3 records of
// 4-16 KiB inner length take the J = 2..4 buckets.  A host decision only (launch_batch).
bool tls13_buckets_enabled();
int set_tls13_buckets(int enable);
// keying pre-pass + record kernel; ev_mid (may be NULL) is recorded between them
hipError_t launch_wpr(const KParams& p, bool open, hipStream_t s, hipEvent_t ev_mid);
// the keying pre-pass of a uniform launch alone (sg_wpr_keying.hip)
hipError_t launch_wpr_keying(const KParams& p, bool open, const WprList& wl, hipStream_t s);
// wave-per-record buckets of a mixed batch (wl[b]: J = kWprMinJ + b chunks):
// one keying launch for every bucket (sg_wpr_keying.hip), then the record kernel of one bucket
hipError_t launch_wpr_keying_lists(const KParams& p, bool open, const WprList* wl, hipStream_t s);
hipError_t launch_wpr_list(const KParams& p, bool open, uint32_t J, const WprList& wl, hipStream_t s);
const char* wpr_kernel_config();
const char* class_kernel_config();

// Seal/open launch of a batch that is not a uniform 16 KiB one.  uniform:
// every record is in size_class(max_n) (keying, direct launch); otherwise
// classify into the workspace lists (kNumLists x count, populations in the
// tail), key the listed records and launch per list: the packed kernel
// (p.pack_mix) ahead of the population readback, the wave-per-record buckets
// (p.wpr_mix) and the size classes after it, on up to three streams that are
// joined into s before the call returns.  The tail's over-long count receives
// the records longer than max_n, which are skipped (open: status 3); *over
// receives that count when the populations are read back (not under capture).
// ev_mid (may be NULL) is recorded once, after the keying pre-passes (mixed
// batches: after classify, before the packed launch)  (sg_dispatch.cpp)
hipError_t launch_aead(const KParams& p, bool open, uint32_t max_n, bool uniform, hipStream_t s, uint32_t* over,
                       hipEvent_t ev_mid);
// Eligibility of one record of a mixed batch for the wave-per-record buckets:
// the bucket J (kWprMinJ..4) or 0.  Shared by the classify and keying kernels.
__host__ __device__ inline uint32_t wpr_bucket_of(uint32_t n, uint64_t in_addr, uint64_t out_addr) {
    if (n <= 4096u || n > kWprN || (n & 63u) || ((in_addr | out_addr) & 15u)) return 0u;
    return (n + 4095u) >> 12;
}
// Eligibility of one record of a mixed batch for the packed small-record kernel.
__host__ __device__ inline bool pack_ok(uint32_t n, uint64_t in_addr, uint64_t out_addr) {
    return n >= 64u && n <= 4096u && (n & 63u) == 0u && ((in_addr | out_addr) & 15u) == 0u;
}
bool pack_enabled();  // sg_set_packed / SG_PACK environment switch
int set_pack(int enable);
// packed launch on a persistent grid: the list's population *cnt and the run
// counter *ctr (zero at launch) live on the device
hipError_t launch_pack(const KParams& p, bool open, const uint32_t* list, const uint32_t* cnt, uint32_t* ctr,
                       hipStream_t s);
const char* pack_kernel_config();
// Where the records of this thread's last mixed batch went (sg_last_batch_routes,
// suruga_gpu.h), filled by launch_aead from the populations it reads back.
// Words: known, classes, bucket[kWprBuckets], packed, skipped, 0.
constexpr uint32_t kRouteWords = 8;
void routes_reset();                          // known = 0: at the start of every batch call
void routes_get(uint32_t out[kRouteWords]);
// ---- sg_plumb.hip ----
// zero the output of every record whose open status is 1 (wrong mac)
hipError_t launch_scrub(const KParams& p, hipStream_t s);
// TLS 1.3 open: the inner type and content length of every record whose status
// is 0 (status 5 where the inner plaintext holds no non-zero byte)
hipError_t launch_strip(const KParams& p, uint8_t* inner_type, uint32_t* content_len, hipStream_t s);
// record-layer framing in HBM (sg_record.cpp zero-copy path): build the wire
// image of `count` records (pitch = 5 + frag; the last record's fragment
// last_frag) from aligned fragment slots, or take the fragments of a wire
// image of equal records back into slots
hipError_t launch_frame(const uint8_t* src, uint32_t src_stride, uint8_t* dst, uint32_t pitch, uint32_t count,
                        uint32_t frag, uint32_t last_frag, uint32_t hdr, hipStream_t s);
hipError_t launch_unframe(const uint8_t* src, uint32_t pitch, uint8_t* dst, uint32_t dst_stride, uint32_t count,
                          uint32_t frag, hipStream_t s);
// dst[0, n) <- src[0, n) by a kernel (dst: the caller's registered host memory,
// written over the host link; src 4-byte aligned)
hipError_t launch_copy_out(const uint8_t* src, uint8_t* dst, uint64_t n, hipStream_t s);
// TLS 1.3 read: the contents of the chunk's records before its first failing one, back to
// back at dst (+ cin->offset with use_base); cout and result as sg_gather_records
// (suruga_gpu.h) documents them.  capacity: the most the chunk can deliver (sizes the grid).
hipError_t launch_gather(const uint8_t* src, uint32_t stride, const uint8_t* status, const uint32_t* content_len,
                         uint32_t count, uint8_t* dst, bool use_base, const sg_gather_cursor* cin,
                         sg_gather_cursor* cout, uint32_t* result, uint64_t capacity, hipStream_t s);
hipError_t launch_fill(uint8_t* buf, uint64_t stride, uint32_t len, uint32_t count, uint64_t seed,
                       uint64_t j0, hipStream_t s);
hipError_t launch_compare(const uint8_t* a, uint64_t sa, const uint8_t* b, uint64_t sb, uint32_t len,
                          uint32_t count, unsigned long long* mism, hipStream_t s);
// ---- sg_hkdf.hip ----
// TLS 1.3 traffic keys of `count` rows of device tables of `rows` rows (sg_tls13_traffic_keys_dev,
// suruga_gpu.h): row = index ? index[i] : i, skipped where >= rows; every pointer 4-byte aligned,
// keys / ivs may be NULL
hipError_t launch_tls13_keys(uint32_t count, uint32_t rows, bool update, const uint32_t* index, uint8_t* secrets,
                             uint8_t* keys, uint8_t* ivs, hipStream_t s);

}  // namespace sg
