// sg_copy_pool.cpp -- see sg_copy_pool.h.
#include "sg_copy_pool.h"

#include "sg_env.h"

namespace sg {

CopyPool& CopyPool::shared() {
    static CopyPool* pool = new CopyPool();
    return *pool;
}

CopyPool::CopyPool() {
    const int total = env_int("SG_COPY_THREADS", 1, 32, 8);
    for (int i = 1; i < total; ++i) th_.emplace_back([this] { worker(); });
    for (auto& t : th_) t.detach();
}

void CopyPool::run(uint32_t n, const std::function<void(uint32_t)>& fn) {
    if (n == 0) return;
    if (th_.empty() || n == 1) {
        for (uint32_t i = 0; i < n; ++i) fn(i);
        return;
    }
    Job job;
    job.fn = &fn;
    job.n = n;
    {
        std::lock_guard<std::mutex> lk(mu_);
        q_.push_back(&job);
    }
    cv_.notify_all();
    drain(job);
    std::unique_lock<std::mutex> lk(mu_);
    // no worker can pick the job up once it is off the queue; the ones that
    // did finish their last index before dropping `active`
    for (auto it = q_.begin(); it != q_.end(); ++it)
        if (*it == &job) {
            q_.erase(it);
            break;
        }
    done_.wait(lk, [&] { return job.active == 0; });
}

void CopyPool::drain(Job& j) {
    for (uint32_t i = j.next.fetch_add(1); i < j.n; i = j.next.fetch_add(1)) (*j.fn)(i);
}

void CopyPool::worker() {
    for (;;) {
        Job* j = nullptr;
        {
            std::unique_lock<std::mutex> lk(mu_);
            for (;;) {
                while (!q_.empty() && q_.front()->next.load() >= q_.front()->n) q_.pop_front();  // exhausted
                if (!q_.empty()) break;
                cv_.wait(lk);
            }
            j = q_.front();
            ++j->active;
        }
        drain(*j);
        {
            std::lock_guard<std::mutex> lk(mu_);
            --j->active;
        }
        done_.notify_all();
    }
}

void copy_run(uint32_t n, const std::function<void(uint32_t)>& fn) {
    if (n <= 1) {
        for (uint32_t i = 0; i < n; ++i) fn(i);
        return;
    }
    CopyPool::shared().run(n, fn);
}

}  // namespace sg
