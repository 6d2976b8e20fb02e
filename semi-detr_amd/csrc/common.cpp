#include "common.h"

namespace semidetr {

char *error_buffer()
{
    static thread_local char buf[512] = {0};
    return buf;
}

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

int allow_big_lds(const void *kernel, size_t bytes, const char *what)
{
    if (bytes <= 64 * 1024) return SEMIDETR_OK;
    // The product's users: 25 MSDA kernels (9 region-window forwards, 6 window gathers, 2 region scatters, 4 merged backwards and
    // the 2 + 2 wide-pyramid strips, over the two IO contracts), qsel_topk_kernel, det_merge_decode_kernel and lsap_kernel: 28
    // kernels, 224 (kernel, device) pairs when one thread drives 8 GPUs.  32 slots per device keep all of them in the table;
    // a launcher that adds a kernel with more than 64 KB of dynamic LDS adds to this count.
    constexpr int kSlots = 32 * 8;
    struct Granted { const void *kern; int dev; size_t bytes; };
    static thread_local Granted table[kSlots];
    static thread_local int used = 0;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail((int)e, "%s: hipGetDevice: %s", what, hipGetErrorString(e));
    Granted *g = nullptr;
    for (int i = 0; i < used && !g; ++i)
        if (table[i].kern == kernel && table[i].dev == dev) g = &table[i];
    if (g && g->bytes >= bytes) return SEMIDETR_OK;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail((int)e, "%s: hipFuncSetAttribute(%zu bytes of LDS): %s", what, bytes, hipGetErrorString(e));
    if (!g && used < kSlots) g = &table[used++];
    if (g) *g = Granted{kernel, dev, bytes};       // a full table only costs a repeated hipFuncSetAttribute
    return SEMIDETR_OK;
}

}  // namespace semidetr

extern "C" int semidetr_abi_version(void) { return SEMIDETR_ABI_VERSION; }
extern "C" const char *semidetr_last_error(void) { return semidetr::error_buffer(); }
