// Shared host-side helpers for libsemidetr_hip.so (error reporting, launch checks, the grant of large dynamic LDS).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "semidetr_hip.h"

namespace semidetr {

char *error_buffer();            // thread-local, 512 bytes
int fail(int code, const char *fmt, ...);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Turns the status of the launch just issued into the C-ABI return code.
inline int launch_status(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, "%s: %s", what, hipGetErrorString(e));
    return SEMIDETR_OK;
}

// Dynamic LDS above 64 KB has to be allowed per kernel AND per device (function attributes are per device).  Remembers what
// this thread was granted per (kernel, device); `bytes` <= 64 KB needs no grant and costs no HIP call.  `what` prefixes the
// error text.
int allow_big_lds(const void *kernel, size_t bytes, const char *what);
// (The only template of this header: it takes a __global__ function as it is launched and does the cast, nothing else.  It
// lets any object pointer in as well; what identifies a kernel is the address.)
template <typename K>
inline int allow_big_lds(K *kernel, size_t bytes, const char *what)
{
    return allow_big_lds(reinterpret_cast<const void *>(kernel), bytes, what);
}

// the smallest power of two >= v, at least 2 (a bitonic network needs a pair)
inline int next_pow2(int v)
{
    int p = 2;
    while (p < v) p <<= 1;
    return p;
}

#define SEMIDETR_REQUIRE(cond, code, ...) \
    do { if (!(cond)) return ::semidetr::fail((code), __VA_ARGS__); } while (0)

}  // namespace semidetr
