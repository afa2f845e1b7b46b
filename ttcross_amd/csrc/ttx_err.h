// ttx_err.h -- the text of the calling thread's last error (ttx_last_error) and the two ways the host code sets it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <string>
#include "../../include/ttx.h"

// g_err and fail have internal linkage: the library is ONE translation unit (ttx_engine.hip), and ttx_last_error reads the g_err of
// that unit.  A second translation unit that included this header would set a g_err of its own, which ttx_last_error never sees;
// splitting the library needs an extern definition here first.
static thread_local std::string g_err;
static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(TTX_EHIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
