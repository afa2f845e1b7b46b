// ttx_host_pool.h -- worker threads for the host integrand (host only, no HIP in here).  The reference evaluates `fun` inside
// !$OMP PARALLEL DO regions (lib/dmrgg.f90:169,222,455,520,553); `fun` must be thread-safe there and here.  The process-wide pool
// lives in ttx_engine.hip (host_pool); tests/host_pool_main.cpp drives pools of its own on the CPU.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// threads of the process-wide pool: TTX_HOST_THREADS where set, else OMP_NUM_THREADS (each as atoi reads it, nullptr where unset);
// where that gives nothing positive, the hardware's count (0: unknown) up to 32
inline int host_pool_threads(const char *ttx_host_threads, const char *omp_num_threads, unsigned hardware)
{
    int nt = 0;
    if (ttx_host_threads) nt = atoi(ttx_host_threads);
    else if (omp_num_threads) nt = atoi(omp_num_threads);
    if (nt <= 0) nt = (int)std::min(32u, std::max(1u, hardware));
    return nt;
}

class HostPool {
  public:
    explicit HostPool(int nt) { for (int t = 1; t < nt; t++) workers.emplace_back([this] { loop(); }); }   // the caller of run is one of the nt
    ~HostPool()
    {
        { std::lock_guard<std::mutex> lk(mu); quit = true; gen++; }
        cv.notify_all();
        for (auto &w : workers) w.join();
    }
    HostPool(const HostPool &) = delete;
    HostPool &operator=(const HostPool &) = delete;
    int threads() const { return (int)workers.size() + 1; }
    // fn(i) for i in [0, n): the calling thread takes part; returns when all are done.  Callers on different host threads
    // take turns on a pool, one batch at a time (`turn`).
    void run(size_t n, const std::function<void(size_t)> &fn)
    {
        if (n == 0) return;
        if (workers.empty() || n < 32) { for (size_t i = 0; i < n; i++) fn(i); return; }
        std::lock_guard<std::mutex> one_batch(turn);
        {
            std::lock_guard<std::mutex> lk(mu);
            job = &fn; total = n; next = 0; pending = workers.size(); gen++;
        }
        cv.notify_all();
        work();
        std::unique_lock<std::mutex> lk(mu);
        done.wait(lk, [&] { return pending == 0; });
        job = nullptr;
    }
  private:
    void work()
    {
        for (;;) {
            size_t lo, hi;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (next >= total) return;
                lo = next; hi = std::min(total, lo + std::max<size_t>(1, total / (8 * (workers.size() + 1)))); next = hi;
            }
            for (size_t i = lo; i < hi; i++) (*job)(i);
        }
    }
    void loop()
    {
        unsigned long long seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return gen != seen; });
                seen = gen;
                if (quit) return;
            }
            work();
            { std::lock_guard<std::mutex> lk(mu); if (--pending == 0) done.notify_all(); }
        }
    }
    std::vector<std::thread> workers;
    std::mutex mu, turn;
    std::condition_variable cv, done;
    const std::function<void(size_t)> *job = nullptr;
    size_t total = 0, next = 0, pending = 0;
    unsigned long long gen = 0;
    bool quit = false;
};
