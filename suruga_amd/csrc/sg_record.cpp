// sg_record.cpp -- batched record layer over host memory (sg_write_records /
// sg_read_records): the throughput form of suruga's TlsWriter::write_data and
// TlsReader::read_record (src/tls.rs:99-147, 217-281).  This file holds the
// HIP orchestration only: the wire parser and the framing arithmetic are in
// sg_wire.cpp, the host threads of the framing copies in sg_copy_pool.cpp.
//
// Records move through a per-context pipeline of four slots (SG_RECORD_SLOTS).
// Each slot owns device buffers, a keying workspace and (staged path,
// allocated on first use) pinned host buffers.  Staged calls run the direct
// pipeline (run_direct): the host frames chunk c+1 into a slot's pinned
// staging while the kernels of chunk c read and write another slot's staging
// over the host link.  Zero-copy calls (sg_host_register'ed buffers) run the
// copy-engine pipeline (run_pipeline): while the GPU seals/opens chunk c, chunk
// c-1's output leaves and chunk c+1 comes in.  Device layout is always 16-byte
// aligned (record slot stride kSlot), so the kernels take their vector path;
// the 5-byte TLS headers are added/stripped by the CPU while copying (staged
// path) or by the frame kernels in HBM (zero-copy path).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include "../../include/suruga_gpu.h"
#include "sg_copy_pool.h"
#include "sg_env.h"
#include "sg_host.h"
#include "sg_wire.h"
#include "sg_internal.h"

namespace sg {

namespace {
constexpr uint32_t kSlot = ((SG_ENC_RECORD_MAX_LEN + 63u) / 64u) * 64u;  // device bytes per record
constexpr int kMaxSlots = 8;                                      // pipeline depth (SG_RECORD_SLOTS)

thread_local double t_h2d = 0, t_kernel = 0, t_d2h = 0, t_host = 0;

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline void cpu_relax() {
#if defined(__x86_64__)
    _mm_pause();
#else
    std::this_thread::yield();
#endif
}

// The pipeline's switches, read from the environment once per process.
struct Switches {
    // The direct pipeline for staged calls (round 6, default; run_direct): the
    // record kernels read the pinned staging and write their output into it
    // over the host link themselves.  SG_RECORD_SDMA=1: the copy-engine
    // pipeline (run_pipeline) for staged calls too.
    bool direct = !env_flag("SG_RECORD_SDMA", false);
    // SG_RECORD_KD2H=1: zero-copy calls move their output by a kernel's stores
    // into the caller's registered memory over the host link (the write's
    // frame kernel builds the wire image straight in `wire`, the read's
    // copy-out kernel moves the plaintext into `out`), after the record
    // kernels on the same stream, instead of an SDMA D2H.  Round 6, same box
    // (profiles/r06/record_path_ab/, r06zz-r06zy): 28.1 / 25.5 GiB/s write /
    // read both in a standalone process and in the bench process, against
    // SDMA's 21.6 / 21.0 standalone and 35.1 / 33.9 in the bench process (the
    // SDMA copies' rate depends on how the process's streams fall on the
    // hardware queues; the kernel's stores serialise with the record kernels
    // of its stream).  The same kernel on the D2H stream measured 21.7 / 21.4
    // and 25.9 / 23.9.  Default: SDMA.
    bool kd2h = env_flag("SG_RECORD_KD2H", false);
    // SG_ZERO_COPY=0 turns the registered-buffer path off
    bool zero_copy = env_flag("SG_ZERO_COPY", true);
    // Pipeline depth (2..8).  Four slots (default since round 6) keep a
    // chunk's H2D, another's kernels and a third's D2H in flight while the
    // host-gated pipeline (run_pipeline) notices each step's end.
    int slots = env_int("SG_RECORD_SLOTS", 2, kMaxSlots, 4);
};
const Switches& switches() {
    static const Switches s{};
    return s;
}
// SG_RECORD13_GATHER / sg_set_record13_gather (sg_env.h)
EnvSwitch g_gather13{"SG_RECORD13_GATHER", -1, kRecord13GatherDefault};

// TLS 1.3 read: a slot's pinned block beside its statuses, written by the strip
// and gather kernels over the host link: content_len[kChunk], the gather's
// result {ok, bytes}, inner_type[kChunk]
constexpr size_t kT13ResOff = (size_t)kChunk * 4u, kT13TypeOff = kT13ResOff + 16u;
constexpr size_t kT13Bytes = kT13TypeOff + kChunk;
}  // namespace

struct RecordStaging {
    struct Slot {
        uint8_t *h_in = nullptr, *h_out = nullptr, *h_meta = nullptr, *h_status = nullptr;
        uint32_t* h_len = nullptr;
        uint8_t *d_in = nullptr, *d_out = nullptr;
        uint8_t* d_wire = nullptr;  // the chunk's wire image (zero-copy path)
        // device addresses of the pinned blocks: the kernels read lengths,
        // nonces / AD and write statuses there over the host link, and the
        // direct pipeline's kernels read and write the record staging there
        uint8_t *dh_in = nullptr, *dh_out = nullptr, *dh_meta = nullptr, *dh_status = nullptr;
        uint32_t* dh_len = nullptr;
        uint8_t *h_t13 = nullptr, *dh_t13 = nullptr;  // TLS 1.3 read (host_staging13, on first use)
        uint32_t* clen(bool dev) const { return (uint32_t*)(dev ? dh_t13 : h_t13); }
        uint32_t* result(bool dev) const { return (uint32_t*)((dev ? dh_t13 : h_t13) + kT13ResOff); }
        uint8_t* itype(bool dev) const { return (dev ? dh_t13 : h_t13) + kT13TypeOff; }
        void* d_ws = nullptr;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // start, after H2D, after kernels, after D2H
        uint32_t nrec = 0;       // records in flight on this slot
        uint64_t first = 0;      // index of its first record in the call
        bool zc = false;         // the chunk goes the zero-copy way
        bool busy = false;
        ChunkShape shape;        // reader: of the chunk's records, set by stage
        uint64_t out0 = 0;       // reader: offset of the chunk's plaintext in `out`
    } slot[kMaxSlots];
    hipStream_t krn = nullptr;  // the copy-engine pipeline's kernel stream
    hipStream_t kst = nullptr;  // the direct pipeline's stream
    // TLS 1.3 read: the call's cursor table, one entry per chunk and one more (sg_gather_kernel)
    sg_gather_cursor* d_cur = nullptr;
    size_t cur_cap = 0;
};
using Slot = RecordStaging::Slot;

// Stream layout of the copy-engine pipeline: the host-link copies of every
// context on one process-wide stream per direction and each context's kernels
// on a stream of its own, so that one slot's H2D runs beside another's kernels
// and a third's D2H, the copies on different DMA engines, while a reader and a
// writer use four streams in all -- within the process's hardware queues
// (GPU_MAX_HW_QUEUES = 4: more streams than that share queues and serialise).
// Round 5, same box, 1 GiB per direction, 8 copy threads (profiles/r05g):
// registered buffers 17.4 -> 27.6 GiB/s write, 23.4 -> 25.8 read against
// per-slot streams; pageable 12.6 -> 15.2 write, 15.8 -> 14.5 read.  Round 6
// (profiles/r06/, r06d): the D2H on a stream of each context's own 14.8
// instead of 29.7 GiB/s registered read, both copy directions per context 24.2
// instead of 31.7 write -- the extra streams share hardware queues.
// The direct pipeline has one stream for everything.
struct PipeStreams {
    hipStream_t h2d, krn, d2h;
};
std::mutex g_cs_mu;
std::vector<std::pair<int, std::pair<hipStream_t, hipStream_t>>> g_copy_streams;  // device -> (h2d, d2h)
hipError_t process_copy_streams(int dev, hipStream_t* h2d, hipStream_t* d2h) {
    std::lock_guard<std::mutex> lk(g_cs_mu);
    for (auto& e : g_copy_streams)
        if (e.first == dev) {
            *h2d = e.second.first;
            *d2h = e.second.second;
            return hipSuccess;
        }
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(h2d, hipStreamNonBlocking)) != hipSuccess) return e;
    if ((e = hipStreamCreateWithFlags(d2h, hipStreamNonBlocking)) != hipSuccess) return e;
    g_copy_streams.push_back({dev, {*h2d, *d2h}});
    return hipSuccess;
}
// The direct pipeline's stream of each context is created at the device's
// greatest stream priority: such streams draw their hardware queues from a
// pool of their own, which the process's other streams do not share, so a
// writer's and a reader's record kernels never queue behind each other or
// behind unrelated work (round 6, profiles/r06/record_path_ab/r06ps: pageable
// 22.1 / 22.2 and 20.7 / 21.6 GiB/s in the bench process against 19.8 / 20.2
// and 19.5 / 19.3 at the default priority, duplex standalone 28.5 / 28.2
// against 25.2 / 25.0; one earlier default-priority run of the bench process
// ran the duplex at 0.91x the serial time, r06pr).  The same for the
// copy-engine pipeline's copy or kernel streams slowed the registered path
// (34.9 -> 26-27 GiB/s, r06pr), so those stay at the default priority.
hipError_t make_priority_stream(hipStream_t* s) {
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess) return e;
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest);
}

void record_staging_free(RecordStaging* rs) {
    if (!rs) return;

    for (hipStream_t t : {rs->krn, rs->kst}) {
        if (!t) continue;
        (void)hipStreamSynchronize(t);
        (void)hipStreamDestroy(t);
    }
    for (auto& s : rs->slot) {
        (void)hipHostFree(s.h_in);
        (void)hipHostFree(s.h_out);
        (void)hipHostFree(s.h_meta);
        (void)hipHostFree(s.h_status);
        (void)hipHostFree(s.h_len);
        (void)hipHostFree(s.h_t13);
        (void)hipFree(s.d_in);
        (void)hipFree(s.d_out);
        (void)hipFree(s.d_wire);
        (void)hipFree(s.d_ws);
        for (auto& e : s.ev)
            if (e) (void)hipEventDestroy(e);
    }
    (void)hipFree(rs->d_cur);
    delete rs;
}

namespace {

int staging(sg_ctx* c, RecordStaging** out) {
    if (!c->rec) {
        auto* rs = new RecordStaging();
        c->rec = rs;  // freed with the context even if allocation below fails
        const size_t bytes = (size_t)kChunk * kSlot;
        // (no stream here: pipe_streams creates them on a call's first use, in
        // the order that the rates depend on)
        for (int i = 0; i < switches().slots; ++i) {  // (h_in / h_out: host_staging, on first use)
            auto& s = rs->slot[i];
            SG_HIP(hipHostMalloc((void**)&s.h_meta, (size_t)kChunk * kMetaBytesMax, hipHostMallocMapped));
            SG_HIP(hipHostMalloc((void**)&s.h_status, kChunk, hipHostMallocMapped));
            SG_HIP(hipHostMalloc((void**)&s.h_len, kChunk * 4u, hipHostMallocMapped));
            SG_HIP(hipHostGetDevicePointer((void**)&s.dh_meta, s.h_meta, 0));
            SG_HIP(hipHostGetDevicePointer((void**)&s.dh_status, s.h_status, 0));
            SG_HIP(hipHostGetDevicePointer((void**)&s.dh_len, s.h_len, 0));
            SG_HIP(hipMalloc((void**)&s.d_in, bytes));
            SG_HIP(hipMalloc((void**)&s.d_out, bytes));
            SG_HIP(hipMalloc((void**)&s.d_wire, bytes + 64));
            SG_HIP(hipMalloc(&s.d_ws, sg_workspace_size(kChunk)));
            for (auto& e : s.ev) SG_HIP(hipEventCreate(&e));
        }
    }
    *out = c->rec;
    return SG_OK;
}

// The staged path's pinned blocks of a slot (the zero-copy path never needs
// them, so a context that only moves registered buffers pins no staging).
int host_staging(Slot& s) {
    const size_t bytes = (size_t)kChunk * kSlot;
    if (!s.h_in) {
        SG_HIP(hipHostMalloc((void**)&s.h_in, bytes, hipHostMallocMapped));
        SG_HIP(hipHostGetDevicePointer((void**)&s.dh_in, s.h_in, 0));
    }
    if (!s.h_out) {
        SG_HIP(hipHostMalloc((void**)&s.h_out, bytes, hipHostMallocMapped));
        SG_HIP(hipHostGetDevicePointer((void**)&s.dh_out, s.h_out, 0));
    }
    return SG_OK;
}

// The TLS 1.3 read's pinned block of a slot and the call's cursor table (no
// kernel of the context is in flight here: a call drains its slots before it
// returns), its first entry {0, not stopped} on stream ks.
int host_staging13(Slot& s) {
    if (s.h_t13) return SG_OK;
    SG_HIP(hipHostMalloc((void**)&s.h_t13, kT13Bytes, hipHostMallocMapped));
    SG_HIP(hipHostGetDevicePointer((void**)&s.dh_t13, s.h_t13, 0));
    return SG_OK;
}
int cursor_table(RecordStaging* rs, uint64_t chunks, hipStream_t ks) {
    if (rs->cur_cap < chunks + 1) {
        (void)hipFree(rs->d_cur);
        rs->d_cur = nullptr;
        rs->cur_cap = 0;
        SG_HIP(hipMalloc((void**)&rs->d_cur, (size_t)(chunks + 1) * sizeof(sg_gather_cursor)));
        rs->cur_cap = chunks + 1;
    }
    SG_HIP(hipMemsetAsync(rs->d_cur, 0, sizeof(sg_gather_cursor), ks));
    return SG_OK;
}

// Account a finished slot's device times (H2D, kernels, D2H).
int account(Slot& s) {
    float a = 0, b = 0, d = 0;
    SG_HIP(hipEventElapsedTime(&a, s.ev[0], s.ev[1]));
    SG_HIP(hipEventElapsedTime(&b, s.ev[1], s.ev[2]));
    SG_HIP(hipEventElapsedTime(&d, s.ev[2], s.ev[3]));
    t_h2d += a;
    t_kernel += b;
    t_d2h += d;
    return SG_OK;
}

// Leaves every pipeline slot idle on every exit path: a call that returns
// early (a launch or copy error) must not hand a half-finished slot, framed
// with its own lengths and sequence numbers, to the next call.  `ps`: the
// call's streams (pipe_streams), drained when a slot is still busy.
struct SlotReset {
    RecordStaging* rs;
    PipeStreams ps = {nullptr, nullptr, nullptr};
    explicit SlotReset(RecordStaging* r) : rs(r) { reset(); }
    ~SlotReset() { reset(); }
    void reset() {
        bool busy = false;
        for (auto& s : rs->slot) busy = busy || s.busy;
        if (busy)
            for (hipStream_t t : {ps.h2d, ps.krn, ps.d2h})
                if (t) (void)hipStreamSynchronize(t);
        for (auto& s : rs->slot) {
            s.busy = false;
            s.nrec = 0;
            s.first = 0;
            s.zc = false;
        }
    }
};

// The streams of this call, each created on its first use and none that the
// call does not use.  Copy-engine pipeline: the process's copy streams first,
// then the context's kernel stream.  HIP hands a process's streams its
// hardware queues round-robin (GPU_MAX_HW_QUEUES = 4), and a kernel stream
// that shares a queue with the D2H stream runs its kernels behind the copies
// (round 6: the standalone write at 22.3 GiB/s registered with the kernels on
// a context stream created before the copy streams, r06l, against 35.1 in a
// process whose other streams happened to separate them).
int pipe_streams(sg_ctx* c, RecordStaging* rs, bool direct, PipeStreams* out) {
    if (direct) {
        if (!rs->kst) SG_HIP(make_priority_stream(&rs->kst));
        *out = {rs->kst, rs->kst, rs->kst};
        return SG_OK;
    }
    hipStream_t h = nullptr, d = nullptr;
    SG_HIP(process_copy_streams(c->device, &h, &d));
    if (!rs->krn) SG_HIP(hipStreamCreateWithFlags(&rs->krn, hipStreamNonBlocking));
    *out = {h, rs->krn, d};
    return SG_OK;
}

// The chunk that a stage takes: its record count, and the bookkeeping once
// the stage has issued it.
uint32_t chunk_count(uint64_t nrec, uint64_t next) { return (uint32_t)std::min<uint64_t>(kChunk, nrec - next); }
void advance(Slot& s, uint64_t& next, uint32_t k) {
    s.nrec = k;
    s.first = next;
    next += k;
}

// The copy-engine pipeline's copies of a chunk with their events.
int h2d(Slot& s, void* dst, const void* src, size_t bytes, hipStream_t hs) {
    SG_HIP(hipEventRecord(s.ev[0], hs));
    SG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, hs));
    SG_HIP(hipEventRecord(s.ev[1], hs));
    return SG_OK;
}
int d2h(Slot& s, void* dst, const void* src, size_t bytes, hipStream_t ds) {
    SG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ds));
    SG_HIP(hipEventRecord(s.ev[3], ds));
    return SG_OK;
}

// The sg_batch fields that a chunk's seal and open share.  A uniform chunk is
// a direct launch; the lengths of a ragged one are read from the pinned block
// over the host link (a few hundred bytes: no copy of their own).
void fill_batch(sg_batch* b, const sg_ctx* c, const Slot& s, bool direct, bool same, uint32_t uniform_len,
                hipStream_t ks) {
    std::memset(b, 0, sizeof *b);
    b->count = s.nrec;
    b->keys = c->d_key;
    b->num_keys = 1;
    // direct: straight from and into the pinned staging
    b->in = direct ? s.dh_in : s.d_in;
    b->out = direct ? s.dh_out : s.d_out;
    b->len = same ? nullptr : s.dh_len;
    b->uniform_len = same ? uniform_len : 0u;
    b->stream = ks;
    b->workspace = s.d_ws;
    b->workspace_size = sg_workspace_size(kChunk);
}

// The direct pipeline (round 6; staged calls): the record kernels read the
// pinned staging and write their output into it over the host link
// themselves, so no copy engine is involved and a chunk's work is the kernels
// of one stream, `st`.  The host keeps up to ns chunks in flight, fills the
// next slot's staging while the GPU works, and waits only for the oldest
// chunk before reusing its slot.  On this host link kernels move data faster
// than the copy engines (tools/hostbw_probe.hip, profiles/r06/hostbw_r06t.txt:
// kernel stores to host memory 54.8 GB/s, loads 57.3 GB/s, against 30.2 / 40.6
// GB/s for SDMA D2H / H2D, and 28.6 GB/s each with a copy in each direction at
// once).  Zero-copy calls keep the copy-engine pipeline: there the seal kernel
// reading the caller's buffer and the frame kernel writing the wire reached
// 20-23 GiB/s against 34.6 / 24.1 GiB/s write / read for SDMA copies
// (profiles/r06/record_path_ab/, r06u-r06v).
// more(): whether another chunk is to be staged (the reader stops at a failed
// record).
template <class More, class Stage, class Launch, class Finish>
int run_direct(RecordStaging* rs, int ns, hipStream_t st, More more, Stage stage, Launch launch, Finish finish) {
    uint64_t staged = 0, done = 0;
    auto slot = [&](uint64_t k) -> Slot& { return rs->slot[k % (uint64_t)ns]; };
    int rc;
    for (;;) {
        if (staged < done + (uint64_t)ns && more()) {
            Slot& s = slot(staged);
            s.busy = true;  // (before the enqueues: SlotReset then drains the streams on an error)
            if ((rc = stage(s)) != SG_OK) return rc;
            SG_HIP(hipEventRecord(s.ev[0], st));
            if ((rc = launch(s)) != SG_OK) return rc;
            SG_HIP(hipEventRecord(s.ev[3], st));
            ++staged;
            continue;
        }
        if (done == staged) return SG_OK;
        Slot& s = slot(done);
        SG_HIP(hipEventSynchronize(s.ev[3]));
        float ms = 0;
        SG_HIP(hipEventElapsedTime(&ms, s.ev[0], s.ev[3]));
        t_kernel += ms;  // (chunks in flight overlap: device time, not wall time)
        if ((rc = finish(s)) != SG_OK) return rc;
        s.busy = false;
        ++done;
    }
}

// The copy-engine pipeline (zero-copy calls; staged ones with
// SG_RECORD_SDMA=1).  Chunk k uses slot k % ns and passes four steps:
//   stage    host framing copy (staged path) and the H2D, when the slot is free;
//   launch   the kernels, once the chunk's H2D has completed;
//   copy_out the D2H, once the chunk's kernels have completed;
//   finish   host framing (oldest chunk first), once the chunk's D2H has completed.
// Each step is enqueued by the calling thread when the step before it has
// completed on the device (hipEventQuery, polled every few microseconds), so
// no stream ever holds a device-side wait.  That matters once two contexts run
// at once (suruga's reader and writer, client.rs:19-24, 269-271): a copy
// enqueued ahead of its input waits inside the DMA engine's queue and holds up
// every later copy of the process on that engine and, when the process has more
// streams than hardware queues (GPU_MAX_HW_QUEUES = 4), every command of the
// streams that share its queue.  Round 5's form enqueued a chunk's whole chain
// at once with hipStreamWaitEvent between the streams: one direction at a time
// it was as fast (33.7 / 31.5 GiB/s registered, in the bench process), but a
// reader and a writer at once ran at 19.9 GiB/s together, 0.61x one after the
// other; host-gated they run at 36.4, 1.1-1.4x (profiles/r06/record_path_ab/).
template <class More, class Stage, class Launch, class CopyOut, class Finish>
int run_pipeline(RecordStaging* rs, int ns, More more, Stage stage, Launch launch, CopyOut copy_out, Finish finish) {
    uint64_t staged = 0, launched = 0, copied = 0, done = 0;
    auto slot = [&](uint64_t k) -> Slot& { return rs->slot[k % (uint64_t)ns]; };
    // 1: the step's event has completed, 0: not yet, < 0: error
    auto ready = [&](Slot& s, int ev) -> int {
        const hipError_t q = hipEventQuery(s.ev[ev]);
        if (q == hipSuccess) return 1;
        if (q == hipErrorNotReady) return 0;
        return hip_fail(q, "hipEventQuery");
    };
    int rc;
    for (;;) {
        bool progress = false;
        if (copied > done) {
            Slot& s = slot(done);
            if ((rc = ready(s, 3)) < 0) return rc;
            if (rc) {
                if ((rc = account(s)) != SG_OK) return rc;
                if ((rc = finish(s)) != SG_OK) return rc;
                s.busy = false;
                ++done;
                progress = true;
            }
        }
        if (launched > copied) {
            if ((rc = ready(slot(copied), 2)) < 0) return rc;
            if (rc) {
                if ((rc = copy_out(slot(copied))) != SG_OK) return rc;
                ++copied;
                progress = true;
            }
        }
        if (staged > launched) {
            if ((rc = ready(slot(launched), 1)) < 0) return rc;
            if (rc) {
                if ((rc = launch(slot(launched))) != SG_OK) return rc;
                ++launched;
                progress = true;
            }
        }
        if (staged < done + (uint64_t)ns && more()) {
            Slot& s = slot(staged);
            s.busy = true;  // (before the enqueues: SlotReset then drains the streams on an error)
            if ((rc = stage(s)) != SG_OK) return rc;
            ++staged;
            progress = true;
        }
        if (done == staged && !more()) return SG_OK;
        if (!progress) {
            // ~5 us between polls: polling back to back slowed the copies
            // (20.6 instead of 33.5 GiB/s registered write,
            // profiles/r06/record_path_hostdriven.json), and a sleep rounds
            // up to the kernel's timer slack (~50 us)
            const auto t0 = std::chrono::steady_clock::now();
            while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(5)) cpu_relax();
        }
    }
}

// Caller buffers registered with sg_host_register (page-locked, device-visible
// host memory).  When a call's source and destination both lie in registered
// ranges, the record bytes move by DMA straight between them and the device
// (no framing copy through the library's pinned staging): sg_write_records
// copies the plaintext in with one contiguous H2D per chunk, builds the
// chunk's wire image (headers and fragments) in HBM and copies it out with one
// contiguous D2H; sg_read_records copies the chunk's wire image in, takes it
// apart in HBM and copies the plaintext out contiguously.
struct RegRange {
    uintptr_t lo, hi, dev;  // [lo, hi) on the host; dev: its device address (hipHostGetDevicePointer)
};
std::mutex g_reg_mu;
std::vector<RegRange> g_reg;
bool registered(const void* p, size_t n) {
    if (!p || !n) return false;
    const uintptr_t lo = (uintptr_t)p, hi = lo + n;
    std::lock_guard<std::mutex> lk(g_reg_mu);
    for (const auto& r : g_reg)
        if (lo >= r.lo && hi <= r.hi) return true;
    return false;
}
// the device address of a byte of a registered range (nullptr if none)
template <class T>
T* reg_dev(T* p) {
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> lk(g_reg_mu);
    for (const auto& r : g_reg)
        if (a >= r.lo && a < r.hi) return (T*)(r.dev + (a - r.lo));
    return nullptr;
}

}  // namespace
}  // namespace sg

using sg::fail;

extern "C" {

int sg_host_register(void* p, size_t len) {
    if (!p || !len) return fail(SG_E_ARG, "NULL or empty range%s");
    // mapped: the zero-copy path's output kernels write the range over the
    // host link (SG_RECORD_KD2H)
    hipError_t e = hipHostRegister(p, len, hipHostRegisterPortable | hipHostRegisterMapped);
    if (e != hipSuccess) return sg::hip_fail(e, "hipHostRegister");
    void* dev = nullptr;
    if ((e = hipHostGetDevicePointer(&dev, p, 0)) != hipSuccess) {
        (void)hipHostUnregister(p);
        return sg::hip_fail(e, "hipHostGetDevicePointer");
    }
    std::lock_guard<std::mutex> lk(sg::g_reg_mu);
    sg::g_reg.push_back({(uintptr_t)p, (uintptr_t)p + len, (uintptr_t)dev});
    return SG_OK;
}

int sg_host_unregister(void* p) {
    {
        std::lock_guard<std::mutex> lk(sg::g_reg_mu);
        auto it = std::find_if(sg::g_reg.begin(), sg::g_reg.end(),
                               [&](const sg::RegRange& r) { return r.lo == (uintptr_t)p; });
        if (it == sg::g_reg.end()) return fail(SG_E_ARG, "range was not registered with sg_host_register%s");
        sg::g_reg.erase(it);
    }
    const hipError_t e = hipHostUnregister(p);
    return e == hipSuccess ? SG_OK : sg::hip_fail(e, "hipHostUnregister");
}

int sg_record_timing(double* h2d_ms, double* kernel_ms, double* d2h_ms, double* host_ms) {
    if (h2d_ms) *h2d_ms = sg::t_h2d;
    if (kernel_ms) *kernel_ms = sg::t_kernel;
    if (d2h_ms) *d2h_ms = sg::t_d2h;
    if (host_ms) *host_ms = sg::t_host;
    return SG_OK;
}

int sg_set_record13_gather(int enable) { return sg::g_gather13.set(enable); }

}  // extern "C"

// ---------------------------------------------------------------------------
// The writer and the reader, one body each for the three record forms
// (RecordForm, sg_layout.h; the per-form wire values: sg_wire.h).  kDraft is
// sg_write_records / sg_read_records, kRfc8439 the *_rfc7905 calls -- the same
// wire with the RFC 8439 batch under it -- and kTls13 the *_tls13 calls.
// ---------------------------------------------------------------------------
namespace sg {
namespace {

// the context's write IV on the device (sg_ctx_set_iv)
const uint8_t* dev_iv(const sg_ctx* c) { return c->d_key + kIvOff; }

// the batch entry point of a chunk in its form
int seal_chunk(RecordForm f, const sg_ctx* c, const sg_batch* b) {
    if (f == RecordForm::kDraft) return sg_seal_batch(b);
    if (f == RecordForm::kRfc8439) {
        const sg_batch_rfc8439 x = {dev_iv(c), 0u, 0u};
        return sg_seal_batch_rfc8439(b, &x);
    }
    const sg_batch_tls13 x = {dev_iv(c), nullptr, nullptr, 0u, 0u};
    return sg_seal_batch_tls13(b, &x);
}
int open_chunk(RecordForm f, const sg_ctx* c, const sg_batch* b, const Slot& s) {
    if (f == RecordForm::kDraft) return sg_open_batch(b);
    if (f == RecordForm::kRfc8439) {
        const sg_batch_rfc8439 x = {dev_iv(c), 0u, 0u};
        return sg_open_batch_rfc8439(b, &x);
    }
    const sg_batch_tls13 x = {dev_iv(c), s.itype(true), s.clen(true), 0u, 0u};
    return sg_open_batch_tls13(b, &x);
}

int needs_iv(RecordForm f, const sg_ctx* c) {
    if (f != RecordForm::kDraft && !c->has_iv)
        return fail(SG_E_ARG, "the context has no write IV: call sg_ctx_set_iv first%s");
    return SG_OK;
}

// content_type: the record type of the TLS 1.2 forms; the inner type of TLS 1.3,
// whose header is 17 03 03 whatever the caller's version
int64_t write_records(RecordForm form, sg_ctx* c, uint64_t seq0, uint8_t content_type, uint8_t ver_major,
                      uint8_t ver_minor, const uint8_t* data, size_t len, uint8_t* wire, size_t wire_cap,
                      size_t* wire_len) {
    if (!c || (!data && len) || !wire_len) return fail(SG_E_ARG, "NULL argument%s");
    if (needs_iv(form, c) != SG_OK) return SG_E_ARG;
    const bool t13 = form == RecordForm::kTls13;
    if (t13 && content_type == 0)
        return fail(SG_E_ARG, "the inner content type must be non-zero (a zero byte reads as padding)%s");
    *wire_len = 0;
    t_h2d = t_kernel = t_d2h = t_host = 0;
    const WritePlan plan(len, form);  // tls.rs:137-147: 2^14-byte fragments
    const uint64_t nrec = plan.nrec;
    if (nrec == 0) return 0;
    if (!wire || wire_cap < plan.wire_need()) return fail(SG_E_ARG, "wire buffer too small%s");
    // the header's bytes
    const uint8_t h_type = t13 ? 23 : content_type, h_major = t13 ? 3 : ver_major, h_minor = t13 ? 3 : ver_minor;
    const uint32_t extra = frag_extra(form);  // fragment bytes beyond the plaintext
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return fail(SG_E_HIP, "hipSetDevice failed%s");
    RecordStaging* rs = nullptr;
    int rc = staging(c, &rs);
    if (rc != SG_OK) return rc;
    const Switches& sw = switches();
    size_t wpos = 0;
    // registered caller buffers: DMA straight between them and the device
    // (the copy-engine pipeline); otherwise the pinned staging, which the
    // kernels read and write over the host link (the direct pipeline)
    const bool zc = sw.zero_copy && registered(data, len) && registered(wire, plan.wire_need());
    const bool direct = sw.direct && !zc;
    // zero-copy: the frame kernel writes the wire image into `wire` itself
    // (its word stores need a 4-byte aligned wire)
    const bool kd2h = zc && ((uintptr_t)wire & 3u) == 0 && sw.kd2h;
    uint64_t next = 0;  // first record of the next chunk to stage
    SlotReset slot_reset(rs);
    PipeStreams& P = slot_reset.ps;
    if ((rc = pipe_streams(c, rs, direct, &P)) != SG_OK) return rc;

    // host framing copy in, H2D
    auto stage = [&](Slot& s) -> int {
        const uint32_t k = chunk_count(nrec, next);
        const uint64_t first = next;
        const double t0 = now_ms();
        // zero-copy: the chunk's plaintext is contiguous in the caller's buffer
        // (in_stride 2^14); staged: each record in its 16-byte aligned slot
        s.zc = zc;
        if (s.zc) {
            for (uint32_t i = 0; i < k; ++i) s.h_len[i] = plan.rec_len(first + i);
        } else {
            int r;
            if ((r = host_staging(s)) != SG_OK) return r;
            copy_run(k, [&](uint32_t i) {
                const uint32_t n = plan.rec_len(first + i);
                std::memcpy(s.h_in + (size_t)i * kSlot, data + (first + i) * SG_RECORD_MAX_LEN, n);
                s.h_len[i] = n;
            });
        }
        t_host += now_ms() - t0;
        advance(s, next, k);
        if (direct) return SG_OK;  // (the kernels read the input themselves)
        if (s.zc)
            return h2d(s, s.d_in, data + first * SG_RECORD_MAX_LEN,
                       (size_t)(k - 1) * SG_RECORD_MAX_LEN + plan.rec_len(first + k - 1), P.h2d);
        return h2d(s, s.d_in, s.h_in, (size_t)k * kSlot, P.h2d);
    };
    // seal (and, zero-copy, the chunk's wire image: headers and fragments,
    // tls.rs:126-130, built in HBM so that it leaves in one contiguous copy --
    // a strided copy at the wire's pitch was ~50x slower on the host link)
    auto launch = [&](Slot& s) -> int {
        // every record but the call's last is full, so a chunk is uniform
        // when its last record is as long as its first (the tail is bucketed)
        const uint32_t k = s.nrec, len0 = plan.rec_len(s.first), last = plan.rec_len(s.first + k - 1);
        sg_batch b;
        fill_batch(&b, c, s, direct, len0 == last, len0, P.krn);
        b.flags = SG_BATCH_TLS;
        b.seq0 = seq0 + s.first;
        b.content_type = content_type;
        b.ver_major = ver_major;
        b.ver_minor = ver_minor;
        b.in_stride = s.zc ? SG_RECORD_MAX_LEN : kSlot;
        b.out_stride = kSlot;
        b.max_len = SG_RECORD_MAX_LEN;
        int r;
        if ((r = seal_chunk(form, c, &b)) != SG_OK) return r;
        if (s.zc) {
            const uint32_t hdr = h_type | ((uint32_t)h_major << 8) | ((uint32_t)h_minor << 16);
            uint8_t* img = kd2h ? reg_dev(wire + plan.wire_off(s.first)) : s.d_wire;
            SG_HIP(launch_frame(s.d_out, kSlot, img, (uint32_t)wire_rec(form), k, SG_RECORD_MAX_LEN + extra,
                                last + extra, hdr, P.krn));
        }
        SG_HIP(hipEventRecord(s.ev[2], P.krn));
        return SG_OK;
    };
    auto copy_out = [&](Slot& s) -> int {
        const uint32_t k = s.nrec;
        if (kd2h) {  // the frame kernel has written the wire already
            SG_HIP(hipEventRecord(s.ev[3], P.krn));
            return SG_OK;
        }
        if (s.zc)
            return d2h(s, wire + plan.wire_off(s.first), s.d_wire,
                       (size_t)(k - 1) * wire_rec(form) + SG_HEADER_LEN + plan.frag_len(s.first + k - 1), P.d2h);
        return d2h(s, s.h_out, s.d_out, (size_t)k * kSlot, P.d2h);
    };
    // frame the chunk's records into the wire (tls.rs:126-130): the headers and
    // (staged path) the fragments from the pinned staging
    auto finish = [&](Slot& s) -> int {
        const double t0 = now_ms();
        if (!s.zc) {
            copy_run(s.nrec, [&](uint32_t i) {
                const uint64_t r = s.first + i;
                const uint32_t flen = plan.frag_len(r);
                uint8_t* h = wire + plan.wire_off(r);
                put_header(h, h_type, h_major, h_minor, flen);
                std::memcpy(h + SG_HEADER_LEN, s.h_out + (size_t)i * kSlot, flen);
            });
        }
        const uint64_t last = s.first + s.nrec - 1;
        wpos = plan.wire_off(last) + SG_HEADER_LEN + plan.frag_len(last);
        t_host += now_ms() - t0;
        return SG_OK;
    };
    auto more = [&] { return next < nrec; };
    if (direct) rc = run_direct(rs, sw.slots, P.krn, more, stage, launch, finish);
    else rc = run_pipeline(rs, sw.slots, more, stage, launch, copy_out, finish);
    if (rc != SG_OK) return rc;
    *wire_len = wpos;
    return (int64_t)nrec;
}

// the read error of a TLS 1.3 record that the gather stopped at
int32_t tls13_error(uint8_t status, uint32_t content_len) {
    if (status == 0) return content_len > SG_RECORD_MAX_LEN ? SG_E_RECORD_OVERFLOW : SG_OK;
    if (status == 2) return SG_E_SHORT;
    if (status == SG_STATUS_NO_TYPE) return SG_E_UNEXPECTED_MESSAGE;  // RFC 8446 section 5.4
    return SG_E_BAD_MAC;
}

int read_records(RecordForm form, sg_ctx* c, uint64_t seq0, const uint8_t* wire, size_t wire_len, uint8_t* out,
                 size_t out_cap, uint8_t* types, uint32_t* frag_lens, size_t max_records, sg_read_result* res) {
    if (!c || (!wire && wire_len) || !res) return fail(SG_E_ARG, "NULL argument%s");
    if (needs_iv(form, c) != SG_OK) return SG_E_ARG;
    const bool t13 = form == RecordForm::kTls13;
    std::memset(res, 0, sizeof *res);
    t_h2d = t_kernel = t_d2h = t_host = 0;

    // 1. parse complete records (tls.rs:218-238), stopping at the first bad header
    // (sg_wire.cpp: host-only, run under ASan/UBSan by tests/test_sanitizers.py)
    using Rec = WireRec;
    std::vector<Rec> recs;
    const int32_t header_error = parse_wire(form, wire, wire_len, max_records, recs);
    size_t need = 0;
    for (const Rec& r : recs) need += frag_capacity(form, r.flen);
    if (need > out_cap || (need && !out)) return fail(SG_E_ARG, "out buffer too small%s");
    if (recs.empty()) {
        res->error = header_error;
        return SG_OK;
    }

    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return fail(SG_E_HIP, "hipSetDevice failed%s");
    RecordStaging* rs = nullptr;
    int rc = staging(c, &rs);
    if (rc != SG_OK) return rc;
    const Switches& sw = switches();

    const uint64_t nrec = recs.size();
    // next: first record of the next chunk to stage; issued: plaintext bytes of
    // the chunks staged so far; good / opos / consumed: records delivered,
    // their plaintext bytes (the records are delivered in order, so record
    // `good` belongs at out + opos) and their wire bytes
    uint64_t next = 0, issued = 0, good = 0, opos = 0, consumed = 0;
    int32_t error = SG_OK;
    // registered caller buffers: the fragments come in by DMA from the wire and
    // the plaintext leaves by DMA into `out` at its final offset (prefix sum of
    // the plaintext lengths, as if every record opens; TLS 1.3: at the offset
    // the gather kernels' cursor has reached)
    const bool zc = sw.zero_copy && registered(wire, wire_len) && registered(out, need);
    const bool direct = sw.direct && !zc;
    const bool kd2h = zc && sw.kd2h;  // zero-copy chunks: a copy-out kernel writes `out`
    // TLS 1.3: the contents are packed by the gather kernel, in a zero-copy call
    // always (every chunk, so that the cursor runs through the staged ones too),
    // else by the switch; off: the host copies record by record
    const bool gather = t13 && (zc || g_gather13.on());
    uint64_t gpos = 0;  // TLS 1.3, copy-engine pipeline: content bytes of the chunks copied out so far
    // Zero-copy: plaintext DMA'd into `out` beyond the delivered records is
    // cleared on every exit (the reference releases none of it, tls.rs:268):
    // collect() clears it chunk by chunk, and an early return (a launch or copy
    // error) clears everything from the first undelivered record to the end of
    // the chunks issued.  Declared before the SlotReset, so that it runs after
    // the pipeline's streams have drained.  (TLS 1.3: only delivered bytes ever
    // reach `out`, so there is nothing to clear.)
    struct ScrubOut {
        uint8_t* out;
        const uint64_t *opos, *issued;
        bool armed;
        ~ScrubOut() {
            if (armed && *issued > *opos) std::memset(out + *opos, 0, *issued - *opos);
        }
    } scrub{out, &opos, &issued, zc && !t13};
    SlotReset slot_reset(rs);
    PipeStreams& P = slot_reset.ps;
    if ((rc = pipe_streams(c, rs, direct, &P)) != SG_OK) return rc;
    if (gather && (rc = cursor_table(rs, (nrec + kChunk - 1) / kChunk, P.krn)) != SG_OK) return rc;

    // TLS 1.3: the chunk's records before its first failing one, their contents
    // packed by the gather kernel (one memcpy) or copied record by record
    auto collect13 = [&](Slot& s) -> int {
        if (error != SG_OK) return SG_OK;  // stopped earlier: the chunk delivered nothing anywhere
        const double t0 = now_ms();
        const uint32_t* cl = s.clen(false);
        const uint8_t* ty = s.itype(false);
        uint32_t hpre[kChunk + 1];
        uint32_t ok = 0;
        hpre[0] = 0;
        for (; ok < s.nrec; ++ok) {
            if (tls13_error(s.h_status[ok], cl[ok]) != SG_OK) break;
            hpre[ok + 1] = hpre[ok] + cl[ok];
        }
        const uint32_t bytes = hpre[ok];
        if (gather && (s.result(false)[0] != ok || s.result(false)[1] != bytes))
            return fail(SG_E_HIP, "the gather kernel's result disagrees with the chunk's statuses%s");
        if (ok < s.nrec) error = tls13_error(s.h_status[ok], cl[ok]);
        if (!s.zc) {
            if (gather) {
                if (bytes) std::memcpy(out + opos, s.h_out, bytes);
            } else {
                copy_run(ok, [&](uint32_t i) {
                    std::memcpy(out + opos + hpre[i], s.h_out + (size_t)i * kSlot, cl[i]);
                });
            }
        }
        for (uint32_t i = 0; i < ok; ++i) {
            if (types) types[s.first + i] = ty[i];
            if (frag_lens) frag_lens[s.first + i] = cl[i];
        }
        good += ok;
        opos += bytes;
        if (ok) consumed = recs[s.first + ok - 1].off + recs[s.first + ok - 1].flen;
        t_host += now_ms() - t0;
        return SG_OK;
    };
    auto collect = [&](Slot& s) -> int {
        if (t13) return collect13(s);
        const double t0 = now_ms();
        const uint32_t* pre = s.shape.pre;
        if (error != SG_OK) {  // stopped earlier: nothing of this chunk is delivered
            if (s.zc) std::memset(out + s.out0, 0, pre[s.nrec]);
            return SG_OK;
        }
        // the records up to the first failing one are delivered (tls.rs:268: the
        // reader stops at its first Err), back to back from the chunk's offset
        uint32_t ok = 0;
        for (; ok < s.nrec; ++ok)
            if (s.h_status[ok] != 0) {  // BadRecordMac "wrong mac": deliver nothing of it
                error = s.h_status[ok] == 2 ? SG_E_SHORT : SG_E_BAD_MAC;
                break;
            }
        auto deliver = [&](uint32_t i) {
            const uint64_t r = s.first + i;
            if (!s.zc) std::memcpy(out + s.out0 + pre[i], s.h_out + (size_t)i * kSlot, pre[i + 1] - pre[i]);
            if (types) types[r] = recs[r].type;
            if (frag_lens) frag_lens[r] = pre[i + 1] - pre[i];
        };
        if (s.zc) {
            // the plaintext is in place already; from a failed record on, the
            // DMA'd bytes are cleared (the reference releases none of them)
            if (ok < s.nrec) std::memset(out + s.out0 + pre[ok], 0, pre[s.nrec] - pre[ok]);
            for (uint32_t i = 0; i < ok; ++i) deliver(i);
        } else {
            copy_run(ok, deliver);
        }
        good += ok;
        opos += pre[ok];
        consumed += pre[ok] + (uint64_t)ok * (SG_HEADER_LEN + SG_MAC_LEN);
        t_host += now_ms() - t0;
        return SG_OK;
    };

    // host framing copy in (staged) and the H2D of the fragments or wire image
    auto stage = [&](Slot& s) -> int {
        const uint32_t k = chunk_count(nrec, next);
        const double t0 = now_ms();
        const Rec* R = &recs[next];
        chunk_shape(R, k, &s.shape, form);
        // zero-copy for chunks of equal, back-to-back records (a stream of
        // full records); any other chunk goes through the staging
        s.zc = zc && s.shape.same && s.shape.dense;
        int r;
        if (t13 && (r = host_staging13(s)) != SG_OK) return r;
        // (a zero-copy call's staged chunks leave through the device chunk buffer and h_out)
        if (!s.zc) {
            if ((r = host_staging(s)) != SG_OK) return r;
            copy_run(k, [&](uint32_t i) {
                std::memcpy(s.h_in + (size_t)i * kSlot, wire + R[i].off, R[i].flen);
                s.h_len[i] = R[i].flen;
            });
        }
        // TLS mode (nonce and AD built on the device, tls.rs:250-265) when the
        // chunk's records share type and version; else explicit nonce / AD.
        // TLS 1.3: the header is a constant, whatever version bytes the peer sent.
        if (t13) s.shape.tls = true;
        if (!s.shape.tls)
            for (uint32_t i = 0; i < k; ++i) put_explicit_meta(s.h_meta, i, seq0 + next + i, R[i], form, c->iv);
        t_host += now_ms() - t0;
        if (!direct) {  // (direct: the kernels read the staging themselves)
            // zero-copy: the chunk's wire image in one contiguous copy, taken apart in HBM
            r = s.zc ? h2d(s, s.d_wire, wire + R[0].off - SG_HEADER_LEN, (size_t)k * (SG_HEADER_LEN + R[0].flen), P.h2d)
                     : h2d(s, s.d_in, s.h_in, (size_t)k * kSlot, P.h2d);
            if (r != SG_OK) return r;
        }
        s.out0 = issued;
        issued += s.shape.pre[k];
        advance(s, next, k);
        return SG_OK;
    };
    auto launch = [&](Slot& s) -> int {
        const uint32_t k = s.nrec, flen = s.shape.flen;
        const Rec& R0 = recs[s.first];
        if (s.zc) SG_HIP(launch_unframe(s.d_wire, SG_HEADER_LEN + flen, s.d_in, kSlot, k, flen, P.krn));
        // lengths, nonces / AD and the per-record status go over the host link
        // in the kernels' own accesses, not in copies of their own (round 6:
        // one small D2H per chunk fewer on the copy engine)
        sg_batch b;
        fill_batch(&b, c, s, direct, s.shape.same, flen, P.krn);
        if (s.shape.tls) {
            b.flags = SG_BATCH_TLS;
            b.seq0 = seq0 + s.first;
            b.content_type = R0.type;
            b.ver_major = R0.major;
            b.ver_minor = R0.minor;
        } else {
            b.nonces = s.dh_meta;
            b.ads = s.dh_meta + explicit_nonce_len(form) * kChunk;
            b.ad_len = kAdLen;
            b.ad_stride = kAdLen;
        }
        b.in_stride = kSlot;
        // zero-copy: plaintext back to back, as it lands in `out` (TLS 1.3: in
        // the records' slots; the gather kernel packs the contents)
        b.out_stride = s.zc && !t13 ? (size_t)(flen - SG_MAC_LEN) : kSlot;
        b.max_len = max_fragment(form);
        b.status = s.dh_status;
        // staged: the reader delivers nothing from a failed record (it stops
        // there), so no device scrub of failed records' output; zero-copy: the
        // output goes to the caller's memory by DMA, so failed records are
        // scrubbed on the device first (TLS 1.3: the gather stops in front of them)
        if (!s.zc || t13) b.flags |= SG_BATCH_KEEP_FAILED;
        // TLS 1.3 with the gather: the inner plaintexts stay in HBM
        if (gather) b.out = s.d_out;
        int r;
        if ((r = open_chunk(form, c, &b, s)) != SG_OK) return r;
        if (gather) {
            // into the caller's registered `out` at the cursor's offset, into the slot's
            // pinned output, or into the device chunk buffer (the wire image is consumed)
            const bool to_out = s.zc && kd2h;
            uint8_t* dst = to_out ? reg_dev(out) : (direct ? s.dh_out : s.d_wire);
            const sg_gather_cursor* cur = rs->d_cur + s.first / kChunk;
            SG_HIP(launch_gather(s.d_out, kSlot, s.dh_status, s.clen(true), k, dst, to_out, cur, rs->d_cur + s.first / kChunk + 1,
                                 s.result(true), s.shape.pre[k], P.krn));
        } else if (s.zc && kd2h) {
            SG_HIP(launch_copy_out(s.d_out, reg_dev(out + s.out0), s.shape.pre[k], P.krn));
        }
        SG_HIP(hipEventRecord(s.ev[2], P.krn));
        return SG_OK;
    };
    auto copy_out = [&](Slot& s) -> int {
        if (s.zc && kd2h) {  // the copy-out (TLS 1.3: gather) kernel has written `out` already
            SG_HIP(hipEventRecord(s.ev[3], P.krn));
            return SG_OK;
        }
        if (gather) {
            // the chunk's kernels have completed: exactly the bytes it delivers leave the device
            const uint32_t bytes = s.result(false)[1];
            uint8_t* dst = s.zc ? out + gpos : s.h_out;
            gpos += bytes;
            if (!bytes) {
                SG_HIP(hipEventRecord(s.ev[3], P.krn));
                return SG_OK;
            }
            return d2h(s, dst, s.d_wire, bytes, P.d2h);
        }
        if (s.zc) return d2h(s, out + s.out0, s.d_out, s.shape.pre[s.nrec], P.d2h);
        return d2h(s, s.h_out, s.d_out, (size_t)s.nrec * kSlot, P.d2h);
    };
    auto more = [&] { return next < nrec && error == SG_OK; };
    if (direct) rc = run_direct(rs, sw.slots, P.krn, more, stage, launch, collect);
    else rc = run_pipeline(rs, sw.slots, more, stage, launch, copy_out, collect);
    if (rc != SG_OK) return rc;
    scrub.armed = false;  // collect() has cleared whatever it did not deliver
    res->records = good;
    res->consumed = consumed;
    res->out_len = opos;
    res->error = error != SG_OK ? error : (good == nrec ? header_error : SG_OK);
    return SG_OK;
}

}  // namespace
}  // namespace sg

extern "C" {

int64_t sg_write_records(sg_ctx* c, uint64_t seq0, uint8_t content_type, uint8_t ver_major, uint8_t ver_minor,
                         const uint8_t* data, size_t len, uint8_t* wire, size_t wire_cap, size_t* wire_len) {
    return sg::write_records(sg::RecordForm::kDraft, c, seq0, content_type, ver_major, ver_minor, data, len, wire,
                             wire_cap, wire_len);
}
int64_t sg_write_records_rfc7905(sg_ctx* c, uint64_t seq0, uint8_t content_type, uint8_t ver_major, uint8_t ver_minor,
                                 const uint8_t* data, size_t len, uint8_t* wire, size_t wire_cap, size_t* wire_len) {
    return sg::write_records(sg::RecordForm::kRfc8439, c, seq0, content_type, ver_major, ver_minor, data, len, wire,
                             wire_cap, wire_len);
}
int64_t sg_write_records_tls13(sg_ctx* c, uint64_t seq0, uint8_t inner_type, const uint8_t* data, size_t len,
                               uint8_t* wire, size_t wire_cap, size_t* wire_len) {
    return sg::write_records(sg::RecordForm::kTls13, c, seq0, inner_type, 3, 3, data, len, wire, wire_cap, wire_len);
}

int sg_read_records(sg_ctx* c, uint64_t seq0, const uint8_t* wire, size_t wire_len, uint8_t* out, size_t out_cap,
                    uint8_t* types, uint32_t* frag_lens, size_t max_records, sg_read_result* res) {
    return sg::read_records(sg::RecordForm::kDraft, c, seq0, wire, wire_len, out, out_cap, types, frag_lens,
                            max_records, res);
}
int sg_read_records_rfc7905(sg_ctx* c, uint64_t seq0, const uint8_t* wire, size_t wire_len, uint8_t* out,
                            size_t out_cap, uint8_t* types, uint32_t* frag_lens, size_t max_records,
                            sg_read_result* res) {
    return sg::read_records(sg::RecordForm::kRfc8439, c, seq0, wire, wire_len, out, out_cap, types, frag_lens,
                            max_records, res);
}
int sg_read_records_tls13(sg_ctx* c, uint64_t seq0, const uint8_t* wire, size_t wire_len, uint8_t* out, size_t out_cap,
                          uint8_t* types, uint32_t* frag_lens, size_t max_records, sg_read_result* res) {
    return sg::read_records(sg::RecordForm::kTls13, c, seq0, wire, wire_len, out, out_cap, types, frag_lens,
                            max_records, res);
}

}  // extern "C"

