// Stand-alone check of ttcross_amd/csrc/ttx_host_pool.h (host code only): pools of 1, 2 and 5 threads run batches on both sides
// of the serial cut (n < 32) and every index must be visited exactly once; two caller threads share the 5-thread pool; a pool
// is destroyed with idle workers; the sizing rule of the process-wide pool.  One line per case (tests/test_host_pool_cpu.py
// holds them), built plain, with -fsanitize=address,undefined and with -fsanitize=thread by that test.
#include "ttx_host_pool.h"

#include <atomic>
#include <cstdio>
#include <memory>

// one batch of n on `pool`: how many indices were not visited exactly once
static size_t batch(HostPool &pool, size_t n)
{
    std::unique_ptr<std::atomic<int>[]> seen(new std::atomic<int>[n + 1]);
    for (size_t i = 0; i <= n; i++) seen[i] = 0;
    pool.run(n, [&](size_t i) { seen[i < n ? i : n]++; });
    size_t wrong = seen[n] != 0;                // an index past the end
    for (size_t i = 0; i < n; i++) wrong += seen[i] != 1;
    return wrong;
}

int main()
{
    int bad = 0;
    for (int nt : {1, 2, 5}) {
        HostPool pool(nt);
        if (pool.threads() != nt) { printf("pool of %d threads: threads() = %d\n", nt, pool.threads()); bad++; }
        for (size_t n : {0, 1, 31, 32, 33, 1000}) {
            const size_t wrong = batch(pool, n);
            printf("threads=%d n=%zu: %zu indices not visited exactly once\n", nt, n, wrong);
            bad += wrong != 0;
        }
        if (nt == 5) {
            // two callers at the same time: each batch is complete when its run returns, whatever the other caller does
            std::atomic<size_t> wrong{0};
            auto caller = [&] { for (int b = 0; b < 50; b++) wrong += batch(pool, 200); };
            std::thread a(caller), b(caller);
            a.join(); b.join();
            printf("threads=5 two callers, 50 batches of n=200 each: %zu indices not visited exactly once\n", wrong.load());
            bad += wrong != 0;
        }
    }
    { HostPool idle(5); }                       // workers that never saw a batch
    { HostPool once(5); bad += batch(once, 64) != 0; }
    printf("pools destroyed with idle workers\n");
    struct { const char *ttx, *omp; unsigned hw; } rule[] = {{"3", nullptr, 8}, {nullptr, "2", 8}, {"0", "7", 8}, {nullptr, nullptr, 64}, {nullptr, nullptr, 1}, {nullptr, nullptr, 0}};
    for (const auto &c : rule)
        printf("TTX_HOST_THREADS=%s OMP_NUM_THREADS=%s hardware=%u -> %d threads\n", c.ttx ? c.ttx : "unset", c.omp ? c.omp : "unset", c.hw, host_pool_threads(c.ttx, c.omp, c.hw));
    printf(bad ? "host pool: %d checks FAILED\n" : "host pool: ok\n", bad);
    return bad != 0;
}
