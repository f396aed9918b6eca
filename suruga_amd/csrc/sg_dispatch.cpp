// sg_dispatch.cpp -- host-side dispatcher of a batch that is not a uniform
// 16 KiB one (launch_aead, sg_internal.h): a uniform batch is keyed and
// launched directly; a mixed one is bucketed on the device, its populations
// are read back into a pooled pinned buffer, and its lists run on up to three
// streams.  Also the host's other decisions about the record kernels: the CU
// count that sizes the persistent grids and the two environment switches of the
// wave-per-record route.  No device code: every kernel is reached through a
// launch_* function of sg_kernels.hip, sg_wpr.hip, sg_wpr_keying.hip or sg_pack.hip.
#include "sg_internal.h"
#include "sg_env.h"

#include <mutex>
#include <utility>
#include <vector>

namespace sg {
namespace {

int g_cus[64];  // CUs per device ordinal (0: not read yet)

// Pinned host buffers for the population readback of mixed batches, shared by
// every calling thread (a thread_local buffer per caller leaked one pinned
// allocation per thread that ever ran a mixed batch).  The pool holds at most
// as many buffers as calls were ever in flight at once; they live as long as
// the process.
std::mutex g_pop_mu;
std::vector<std::pair<uint32_t*, hipEvent_t>> g_pop_free;
struct PinnedPop {
    uint32_t* p = nullptr;
    hipEvent_t ev = nullptr;          // recorded after the readback copy
    hipStream_t copy_s = nullptr;     // set once a copy into p has been enqueued on it
    bool recorded = false;            // ev was recorded after that copy
    hipError_t acquire(size_t bytes) {
        {
            std::lock_guard<std::mutex> lk(g_pop_mu);
            if (!g_pop_free.empty()) {
                p = g_pop_free.back().first;
                ev = g_pop_free.back().second;
                g_pop_free.pop_back();
                return hipSuccess;
            }
        }
        hipError_t e = hipHostMalloc((void**)&p, bytes < 256u ? 256u : bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) {
            (void)hipHostFree(p);
            p = nullptr;
            ev = nullptr;
        }
        return e;
    }
    void done() { copy_s = nullptr; }  // the copy has been waited for
    ~PinnedPop() {
        if (!p) return;
        // An error return between the copy and the wait: the buffer goes back to
        // the pool only once the copy into it is known to be done -- by its event
        // when that was recorded, else by the copy's stream.  If neither wait
        // succeeds the buffer is dropped (leaked) rather than handed to another
        // call while a DMA may still write it.
        if (copy_s) {
            const hipError_t w = recorded ? hipEventSynchronize(ev) : hipStreamSynchronize(copy_s);
            if (w != hipSuccess) return;
        }
        std::lock_guard<std::mutex> lk(g_pop_mu);
        g_pop_free.emplace_back(p, ev);
    }
};

// Side streams of mixed batches (per device and priority, pooled like the
// pinned population buffers, created non-blocking with the priority of the
// batch's stream; they live as long as the process).  A pooled stream is
// handed out again only when its last join event reports done, i.e. every
// kernel an earlier batch enqueued on it has finished: the SideStream goes
// back to the pool when launch_aead returns, while its keying and bucket
// kernels may still be queued, and a concurrent batch on another caller
// stream must not queue behind them (calls on different streams are
// independent, suruga_gpu.h).  A busy pooled stream is skipped and a new one
// created, up to kSideCap per device and priority (two concurrent mixed
// batches' worth): beyond that the batch runs that part on its own stream
// (the process has four hardware queues, GPU_MAX_HW_QUEUES, and more streams
// share them and serialise anyway; advisor r5).
constexpr int kSideCap = 4;
std::mutex g_side_mu;
struct SidePooled {
    int dev, prio;
    hipStream_t s;
    hipEvent_t done;
};
std::vector<SidePooled> g_side_free;
std::vector<std::pair<std::pair<int, int>, int>> g_side_made;  // (device, priority) -> streams created
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t done = nullptr;
    int dev = -1, prio = 0;
    bool borrowed = false;  // s is the caller's stream (the cap was reached): not pooled, no join
    hipError_t acquire(hipStream_t caller) {
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if ((e = hipStreamGetPriority(caller, &prio)) != hipSuccess) return e;
        {
            std::lock_guard<std::mutex> lk(g_side_mu);
            for (size_t i = 0; i < g_side_free.size(); ++i) {
                const SidePooled& c = g_side_free[i];
                if (c.dev != dev || c.prio != prio || hipEventQuery(c.done) != hipSuccess) continue;
                s = c.s;
                done = c.done;
                g_side_free.erase(g_side_free.begin() + (long)i);
                return hipSuccess;
            }
            int* made = nullptr;
            for (auto& m : g_side_made)
                if (m.first.first == dev && m.first.second == prio) made = &m.second;
            if (!made) {
                g_side_made.push_back({{dev, prio}, 0});
                made = &g_side_made.back().second;
            }
            if (*made >= kSideCap) {
                s = caller;
                borrowed = true;
                return hipSuccess;
            }
            ++*made;
        }
        if ((e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio)) != hipSuccess) {
            s = nullptr;
            return e;
        }
        if ((e = hipEventCreateWithFlags(&done, hipEventDisableTiming)) != hipSuccess) {
            (void)hipStreamDestroy(s);
            s = nullptr;
        }
        return e;
    }
    // the batch's stream s waits for everything enqueued here so far
    hipError_t join_into(hipStream_t t) const {
        if (borrowed) return hipSuccess;
        hipError_t e = hipEventRecord(done, s);
        return e != hipSuccess ? e : hipStreamWaitEvent(t, done, 0);
    }
    ~SideStream() {
        if (!s || borrowed) return;
        std::lock_guard<std::mutex> lk(g_side_mu);
        g_side_free.push_back({dev, prio, s, done});
    }
};
// Every side stream a batch used is joined into its stream on every way out of
// launch_aead (the workspace is released on that stream).
struct SideJoin {
    hipStream_t s;
    const SideStream* side[2];
    bool used[2];
    ~SideJoin() {
        for (int i = 0; i < 2; ++i)
            if (used[i]) (void)side[i]->join_into(s);
    }
};

thread_local uint32_t t_routes[kRouteWords];  // sg_last_batch_routes: host bookkeeping only

}  // namespace

void routes_reset() {
    for (uint32_t& w : t_routes) w = 0u;
}
void routes_get(uint32_t out[kRouteWords]) {
    for (uint32_t i = 0; i < kRouteWords; ++i) out[i] = t_routes[i];
}

hipError_t device_cus(int* cus) {
    int dev = 0;
    hipError_t e;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    *cus = dev >= 0 && dev < 64 ? __atomic_load_n(&g_cus[dev], __ATOMIC_RELAXED) : 0;
    if (*cus <= 0) {
        if ((e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
        if (dev >= 0 && dev < 64) __atomic_store_n(&g_cus[dev], *cus, __ATOMIC_RELAXED);
    }
    return hipSuccess;
}

static EnvSwitch g_wpr{"SG_LOCKSTEP"};
bool wpr_enabled() { return g_wpr.on(); }
int set_wpr(int enable) { return g_wpr.set(enable); }
static EnvSwitch g_tls13_buckets{"SG_TLS13_BUCKETS", -1, false};  // off unless set
bool tls13_buckets_enabled() { return g_tls13_buckets.on(); }
int set_tls13_buckets(int enable) { return g_tls13_buckets.set(enable); }

hipError_t launch_aead(const KParams& p, bool open, uint32_t max_n, bool uniform, hipStream_t s, uint32_t* over,
                       hipEvent_t ev_mid) {
    *over = 0;
    hipError_t e;
    if (uniform) {  // every record in one class: keying, then a direct launch
        if ((e = launch_keying_all(p, open, s)) != hipSuccess || (e = mark(ev_mid, s)) != hipSuccess) return e;
        KParams q = p;
        const uint32_t c = size_class(max_n);
        q.lds_rec_bytes = lds_rec_bytes(c, q.ad_len, max_n);
        return launch_class(c, q, open, nullptr, nullptr, 0, s);
    }
    uint32_t* const tail = ws_tail(p.ws, p.count);
    uint32_t* const lists = p.ws + (uint64_t)p.count * kWsLists;
    // populations, over-long count and the group / run counters (the keying
    // kernel resets the bucket ones again): one dword fill
    if ((e = hipMemsetD32Async((hipDeviceptr_t)tail, 0, kWsTailWords, s)) != hipSuccess) return e;
    if ((e = launch_classify(p, open, lists, tail, max_n, s)) != hipSuccess) return e;
    // Read the list populations back (one host wait per mixed batch) so that
    // the keying kernels run over exactly the listed records and every list
    // on an exact grid; under stream capture the host cannot wait, so every
    // record is keyed and the classes run on persistent grids instead (and the
    // caller leaves p.wpr_mix and p.pack_mix off: the wave-per-record buckets
    // need their populations).
    // (into a pinned buffer from a process-wide pool: a DMA, no staging copy;
    // the buffer goes back to the pool when this call is done with it)
    uint32_t pop[kNumLists + 1];
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    if ((e = hipStreamIsCapturing(s, &cap_status)) != hipSuccess) return e;
    const bool exact = cap_status == hipStreamCaptureStatusNone;
    // Mixed batches run on up to three streams (round 4): the packed launch
    // (its population stays on the device) goes ahead of the host's wait for
    // the readback, so the GPU does not idle while the host waits and
    // launches; the keying launches run on a side stream ks beside the packed
    // launch's tail; the J = 4 and J = 3 buckets follow the keying on ks and on
    // a second side stream, and J = 2 and the size classes on s, so that each
    // persistent bucket grid takes the CU slots that the launches before it
    // free and their tails overlap instead of adding up.
    SideStream side[2];
    SideJoin join{s, {&side[0], &side[1]}, {false, false}};
    hipStream_t ks = s;
    if (exact) {
        PinnedPop pin;
        if ((e = pin.acquire(sizeof pop)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(pin.p, tail, sizeof pop, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        pin.copy_s = s;
        if ((e = hipEventRecord(pin.ev, s)) != hipSuccess) return e;
        pin.recorded = true;
        // the batch's record window starts with the packed launch
        if ((e = mark(ev_mid, s)) != hipSuccess) return e;
        ev_mid = nullptr;
        if (p.pack_mix && (e = launch_pack(p, open, lists + (uint64_t)kPackList * p.count, tail + kPackList,
                                           tail + kTailPackCtr, s)) != hipSuccess)
            return e;
        if ((e = hipEventSynchronize(pin.ev)) != hipSuccess) return e;
        pin.done();
        for (uint32_t i = 0; i <= kNumLists; ++i) pop[i] = pin.p[i];
        *over = pop[kTailOver];
        {  // the routes the records took (sg_last_batch_routes)
            static_assert(kRouteWords == 2u + kWprBuckets + 3u, "sg_batch_routes");
            t_routes[0] = 1u;
            t_routes[1] = 0u;
            for (uint32_t c = 0; c < kNumClasses; ++c) t_routes[1] += pop[c];
            for (uint32_t b = 0; b < kWprBuckets; ++b) t_routes[2u + b] = pop[kNumClasses + b];
            t_routes[2u + kWprBuckets] = pop[kPackList];
            t_routes[3u + kWprBuckets] = pop[kTailOver];
            t_routes[4u + kWprBuckets] = 0u;
        }
        uint32_t nbuckets = 0;
        for (uint32_t b = 0; b < kWprBuckets; ++b) nbuckets += pop[kNumClasses + b];
        if (((p.pack_mix && pop[kPackList] != 0u) || (p.wpr_mix && nbuckets != 0u)) && side[0].acquire(s) == hipSuccess) {
            ks = side[0].s;
            join.used[0] = true;
            if ((e = hipStreamWaitEvent(ks, pin.ev, 0)) != hipSuccess) return e;  // after classify
        }
        // size-class keying over the class lists only
        KeyJobs jobs = {};
        uint32_t grid = 0;
        for (uint32_t c = 0; c < kNumClasses; ++c) {
            if (pop[c] == 0) continue;
            jobs.list[jobs.njobs] = lists + (uint64_t)c * p.count;
            jobs.count[jobs.njobs] = pop[c];
            jobs.blk0[jobs.njobs] = grid;
            grid += (pop[c] + kKeyingThreads - 1u) / kKeyingThreads;
            ++jobs.njobs;
        }
        if ((e = launch_keying(p, open, jobs, grid, ks)) != hipSuccess) return e;
    } else if ((e = launch_keying_all(p, open, s)) != hipSuccess) {
        return e;
    }
    // wave-per-record buckets (J = 2..4 chunks): their keying records and
    // descriptors are packed by slot in bucket order
    WprList wl[kWprBuckets] = {};
    if (p.wpr_mix && exact) {
        uint64_t base = 0;
        for (uint32_t b = 0; b < kWprBuckets; ++b) {
            const uint32_t nb = pop[kNumClasses + b];
            wl[b].list = lists + (uint64_t)(kNumClasses + b) * p.count;
            wl[b].count = nb;
            wl[b].tab = p.ws + (uint64_t)p.count * kWsWprTab + base * kWprRecWords;
            wl[b].desc = p.ws + (uint64_t)p.count * kWsWprDesc + base * kWprDescWords;
            wl[b].ctr = tail + kTailCtr + b;
            base += nb;
        }
        if ((e = launch_wpr_keying_lists(p, open, wl, ks)) != hipSuccess) return e;
    }
    hipStream_t js[kWprBuckets] = {s, ks, ks};  // bucket b (J = 2 + b)
    if (ks != s) {  // s (J = 2, classes) and the second side stream (J = 3) wait for the keying
        if ((e = side[0].join_into(s)) != hipSuccess) return e;
        if (p.wpr_mix && side[1].acquire(s) == hipSuccess) {
            join.used[1] = true;
            if ((e = hipStreamWaitEvent(side[1].s, side[0].done, 0)) != hipSuccess) return e;
            js[1] = side[1].s;
        }
    }
    if ((e = mark(ev_mid, s)) != hipSuccess) return e;
    if (p.wpr_mix && exact) {  // most chunks first
        for (int b = (int)kWprBuckets - 1; b >= 0; --b)
            if ((e = launch_wpr_list(p, open, kWprMinJ + (uint32_t)b, wl[b], js[b])) != hipSuccess) return e;
    }
    // one launch per populated class, largest records first
    KParams q = p;
    for (int c = (int)size_class(max_n); c >= 0; --c) {
        const uint32_t cap = max_n < class_max((uint32_t)c) ? max_n : class_max((uint32_t)c);
        q.lds_rec_bytes = lds_rec_bytes((uint32_t)c, q.ad_len, cap);
        if ((e = launch_class((uint32_t)c, q, open, lists + (uint64_t)c * p.count, tail + c,
                              exact ? pop[c] : 0xffffffffu, s)) != hipSuccess)
            return e;
    }
    return hipSuccess;  // (join: s waits for the side streams)
}

}  // namespace sg
