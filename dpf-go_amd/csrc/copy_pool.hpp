// copy_pool.hpp — CopyPool, the host thread pool of the pipelined host-buffer
// paths (dpf_capi.hip): parallel memcpy between pinned staging and caller
// buffers, and parallel first touch of a fresh output buffer.  Host-only and
// header-only (no HIP), so tests/c/copy_pool_test.cpp runs it under ASan/UBSan
// and TSan without a device.
#pragma once
#include <sched.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

namespace dpfh {

// Parallel host memcpy for the pinned -> caller-buffer leg of the pipelined
// copies (one thread reaches ~10 GB/s; PCIe delivers ~50).  A fixed pool of
// workers takes 2 MiB pieces; the caller works too and waits for the rest.
class CopyPool {
   public:
    static CopyPool& get() {
        static CopyPool pool;
        return pool;
    }
    // memcpy over the pool in 2 MiB pieces.
    void memcpy_par(void* dst, const void* src, size_t n) {
        if (n == 0) return;   // nothing to copy; dst and src may be null
        if (n <= kPiece || workers_.empty()) {
            memcpy(dst, src, n);
            return;
        }
        struct Ctx {
            uint8_t* d;
            const uint8_t* s;
            size_t n;
        } c{static_cast<uint8_t*>(dst), static_cast<const uint8_t*>(src), n};
        parallel_for((n + kPiece - 1) / kPiece, &c, [](void* p, size_t i) {
            const Ctx& x = *static_cast<const Ctx*>(p);
            const size_t off = i * kPiece;
            memcpy(x.d + off, x.s + off, std::min(kPiece, x.n - off));
        });
    }
    // First touch of a (fresh) destination, one write per 4 KiB page, so the
    // page faults -- one per 2 MiB with transparent huge pages -- are taken
    // by all workers at once instead of inside the timed copies.
    void prefault_par(void* dst, size_t n) {
        struct Ctx {
            volatile uint8_t* d;
            size_t n;
        } c{static_cast<volatile uint8_t*>(dst), n};
        parallel_for((n + kPiece - 1) / kPiece, &c, [](void* p, size_t i) {
            const Ctx& x = *static_cast<const Ctx*>(p);
            const size_t off = i * kPiece, end = std::min(off + kPiece, x.n);
            for (size_t o = off; o < end; o += 4096) x.d[o] = 0;
        });
    }

   private:
    static constexpr size_t kPiece = (size_t)2 << 20;
    struct Job {
        void (*fn)(void*, size_t);
        void* ctx;
        size_t npieces;
        size_t active = 0;   // workers inside run(); guarded by mu_
        std::atomic<size_t> next{0}, done{0};
        Job(void (*f)(void*, size_t), void* c, size_t np) : fn(f), ctx(c), npieces(np) {}
    };
    // fn(ctx, i) for i < npieces over the caller and the workers.
    void parallel_for(size_t npieces, void* ctx, void (*fn)(void*, size_t)) {
        Job job{fn, ctx, npieces};
        {
            std::lock_guard<std::mutex> lk(mu_);
            jobs_.push_back(&job);
        }
        cv_.notify_all();
        run(job);
        // Workers that picked the job leave it (active == 0) before it goes out of scope.
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [&] { return job.done.load() == job.npieces && job.active == 0; });
        jobs_.erase(std::find(jobs_.begin(), jobs_.end(), &job));
    }
    // Run pieces of `job` until none is left.
    static void run(Job& job) {
        for (size_t i; (i = job.next.fetch_add(1)) < job.npieces;) {
            job.fn(job.ctx, i);
            job.done.fetch_add(1);
        }
    }
    // One worker per CPU this process may use (affinity mask, capped by a
    // cgroup CPU quota), minus the caller, at most 31: first-touch page
    // faults of a fresh caller buffer and the copy itself both scale with
    // threads (one thread copies ~10 GB/s; PCIe delivers ~50).
    CopyPool() {
        const unsigned n = std::min(31u, usable_cpus() > 1 ? usable_cpus() - 1 : 0u);
        for (unsigned i = 0; i < n; ++i) workers_.emplace_back([this] { loop(); });
    }
    static unsigned usable_cpus() {
        unsigned n = std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) n = (unsigned)CPU_COUNT(&set);
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[32] = {0};
            unsigned long per = 0;
            if (fscanf(f, "%31s %lu", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) {
                const unsigned long quota = strtoul(q, nullptr, 10) / per;
                if (quota >= 1 && quota < n) n = (unsigned)quota;
            }
            fclose(f);
        }
        return n > 0 ? n : 1;
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    void loop() {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            // Take the job the predicate found, under the same lock hold: the
            // piece counter (`next`) moves without the lock, so a second
            // pending() call could find the job already exhausted.
            Job* j = nullptr;
            cv_.wait(lk, [&] { return stop_ || (j = pending()) != nullptr; });
            if (stop_) return;
            ++j->active;
            lk.unlock();
            run(*j);
            lk.lock();
            --j->active;
            done_cv_.notify_all();
        }
    }
    Job* pending() {
        for (Job* j : jobs_)
            if (j->next.load() < j->npieces) return j;
        return nullptr;
    }
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<Job*> jobs_;
    std::vector<std::thread> workers_;
    bool stop_ = false;
};

}  // namespace dpfh
