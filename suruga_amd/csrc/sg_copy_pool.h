// sg_copy_pool.h -- host threads for the record layer's framing copies (host
// only, no HIP; tests/cpp/test_host_san.cpp runs it under ASan/UBSan and TSan).
#pragma once

#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace sg {

// The record bytes move between the caller's buffers and the pinned staging
// at memcpy speed; one thread alone caps a direction near 9 GB/s.  One pool
// serves the whole process: it is created on the first call that moves more
// than one record and its workers then park on a condition variable, so N
// connections (two contexts each, cipher/mod.rs:18-23) share
// SG_COPY_THREADS - 1 threads instead of owning 7 each.  run(n, fn) calls
// fn(i) for every i < n on the workers and the calling thread and returns when
// all are done; concurrent callers (a reader and a writer thread) each queue a
// job and the workers take indices from the oldest job that still has some, so
// both progress.  SG_COPY_THREADS sets the total (1..32, default 8:
// tools/record_path_bench.py measured 9.8 / 11.5 / 15.5 / 15.2 GiB/s per
// direction with 1 / 4 / 8 / 16 in round 4; with round 6's direct pipeline
// 20.7 / 22.6 / 19.4 / 20.0 GiB/s write with 8 / 12 / 16 / 24,
// profiles/r06/record_path_ab/threads_r06.json: the host's memory, not the
// thread count, bounds it).
class CopyPool {
  public:
    // never destroyed: parked workers must not be joined from a static
    // destructor while the runtime is tearing down
    static CopyPool& shared();
    void run(uint32_t n, const std::function<void(uint32_t)>& fn);

  private:
    // A job lives on its caller's stack.  Workers reach it only through the
    // queue and count themselves into `active` under the same lock, so once
    // run() has taken it off the queue and seen active == 0 nothing refers to
    // it any more.
    struct Job {
        const std::function<void(uint32_t)>* fn = nullptr;
        uint32_t n = 0;
        std::atomic<uint32_t> next{0};
        uint32_t active = 0;  // workers inside the job (guarded by mu_)
    };
    CopyPool();
    static void drain(Job& j);
    void worker();
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::deque<Job*> q_;
};

// The framing copies of one call: inline for n <= 1, otherwise on the shared
// pool (created by the first call that moves more than one record).
void copy_run(uint32_t n, const std::function<void(uint32_t)>& fn);

}  // namespace sg
