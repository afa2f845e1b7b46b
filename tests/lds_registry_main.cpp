// Stand-alone check of ttcross_amd/csrc/ttx_lds.h (host code only): the record of the dynamic-LDS ceilings, driven from two host
// threads with a stub in place of the runtime call.  Built with -fsanitize=address,undefined by tests/test_lds_registry_cpu.py.
#include "ttx_lds.h"

#include <atomic>
#include <cstdio>
#include <thread>

static std::atomic<int> calls{0};
static std::atomic<size_t> last{0};
static int stub(const void *, size_t bytes) { calls++; last = bytes; return 0; }
static int failing(const void *, size_t) { return 7; }
static int k1, k2, kk[4];                   // stand-ins for kernels: only their addresses are used

int main()
{
    int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); bad++; } } while (0)
    CHECK(ttx_lds_raise(0, &k1, 100000, stub) == 0 && calls == 1 && last == 100000);
    CHECK(ttx_lds_raise(0, &k1, 70000, stub) == 0 && calls == 1);                     // a smaller request after a larger one: no call
    CHECK(ttx_lds_raise(0, &k1, 100000, stub) == 0 && calls == 1);
    CHECK(ttx_lds_raise(1, &k1, 70000, stub) == 0 && calls == 2 && last == 70000);    // another device keeps its own record
    CHECK(ttx_lds_raise(0, &k1, 70001, stub) == 0 && calls == 2);                     // ... and leaves the first one alone
    CHECK(ttx_lds_raise(0, &k2, 1, stub) == 0 && calls == 3);                         // another function
    CHECK(ttx_lds_raise(0, &k2, 50, failing) == 7);                                   // a failed call is passed on and records nothing
    CHECK(ttx_lds_raise(0, &k2, 50, stub) == 0 && calls == 4 && last == 50);
    // two threads, one asking in ascending and one in descending order, for 4 functions on 2 devices
    std::atomic<int> failed{0};
    auto work = [&](int t) {
        for (int i = 0; i < 20000; i++) {
            const size_t need = 1000 + (t ? (size_t)i : (size_t)(20000 - i));
            if (ttx_lds_raise(10 + ((i >> 2) & 1), &kk[i & 3], need, stub)) failed++;
        }
    };
    std::thread a(work, 0), b(work, 1);
    a.join(); b.join();
    CHECK(failed == 0);
    const int after = calls;                // every key has been asked for at least 1000 + 19992 by now
    for (int dev = 0; dev < 2; dev++) for (int k = 0; k < 4; k++) CHECK(ttx_lds_raise(10 + dev, &kk[k], 1000 + 19992, stub) == 0);
    CHECK(calls == after);
    printf(bad ? "lds registry: %d checks FAILED\n" : "lds registry: ok\n", bad);
    return bad != 0;
}
