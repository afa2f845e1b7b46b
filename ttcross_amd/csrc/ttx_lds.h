// ttx_lds.h -- the record of the dynamic-LDS ceilings the engine has set (host only, no HIP in here).
//
// A kernel may use more than the default 64 KB of dynamic LDS only after its ceiling was raised, and the runtime call that
// raises it SETS it: a smaller request after a larger one would lower it again.  So every site asks through this one record,
// keyed by (device, function) -- engines live on any device and may be driven from several host threads -- and the runtime is
// called only by a request larger than every earlier one for that key.
#pragma once
#include <cstddef>
#include <map>
#include <mutex>
#include <utility>

typedef int (*ttx_lds_setter)(const void *fn, size_t bytes);   // the runtime call; 0: done

// 0: the ceiling of `fn` on `device` is at least `need` bytes now; else what `set` returned (nothing is recorded then)
inline int ttx_lds_raise(int device, const void *fn, size_t need, ttx_lds_setter set)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> ceiling;
    std::lock_guard<std::mutex> lk(mu);
    size_t &cur = ceiling[std::make_pair(device, fn)];
    if (need <= cur) return 0;
    if (int rc = set(fn, need)) return rc;
    cur = need;
    return 0;
}
