// Shared host-side helpers for libsemidetr_hip.so (error reporting, launch checks, the grant of large dynamic LDS, the split
// rule of the MSDA forwards).
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

// SPLIT of the D == 32 MSDA forwards (fp32: msda_dispatch.h, 16-bit value maps: msda_h16.hip) = the number of 8-lane groups that
// share one query row: with enough 32-row workgroups to fill 256 CUs several times over no split; otherwise the samples of a
// row are spread over more lanes, so that small problems (decoder, 300-900 queries) still fill the chip.  forced: 1 / 2 / 4
// takes that split (the experiments dispatch), anything else the rule.
inline int pick_split(int forced, int N, int Lq, int M)
{
    if (forced == 1 || forced == 2 || forced == 4) return forced;
    const int64_t wg32 = (int64_t)N * M * ((Lq + 31) / 32);
    if (wg32 >= 2048) return 1;
    if (wg32 >= 1024) return 2;
    return 4;
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
