// Host-side check of csrc/common.cpp: next_pow2 and the bookkeeping of allow_big_lds, with the two HIP calls stubbed.  Built
// for the host by tools/common_host_check.sh (under -fsanitize=address,undefined by hand, plain by tests/test_common_host.py);
// no GPU, no HIP runtime.
#include <string.h>

#include "common.h"

static int g_device = 0, g_get_device_calls = 0, g_set_calls = 0, g_last_value = 0;
static const void *g_last_kernel = nullptr;
static hipError_t g_get_device_result = hipSuccess, g_set_result = hipSuccess;

extern "C" hipError_t hipGetDevice(int *dev)
{
    ++g_get_device_calls;
    *dev = g_device;
    return g_get_device_result;
}
extern "C" hipError_t hipFuncSetAttribute(const void *kernel, hipFuncAttribute attr, int value)
{
    if (attr != hipFuncAttributeMaxDynamicSharedMemorySize) return hipErrorInvalidValue;
    ++g_set_calls;
    g_last_kernel = kernel;
    g_last_value = value;
    return g_set_result;
}
extern "C" const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub error"; }
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }

#define CHECK(cond) \
    do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main()
{
    using semidetr::allow_big_lds;
    using semidetr::next_pow2;
    CHECK(next_pow2(0) == 2 && next_pow2(1) == 2 && next_pow2(2) == 2 && next_pow2(3) == 4 && next_pow2(4) == 4);
    CHECK(next_pow2(5) == 8 && next_pow2(300) == 512 && next_pow2(2048) == 2048 && next_pow2(2049) == 4096);

    static char kernels[400];                      // 400 distinct "kernel" addresses
    // 64 KB and less: no grant, no HIP call
    CHECK(allow_big_lds(&kernels[0], 0, "t") == SEMIDETR_OK && allow_big_lds(&kernels[0], 64 * 1024, "t") == SEMIDETR_OK);
    CHECK(g_get_device_calls == 0 && g_set_calls == 0);
    // first grant, then remembered; a smaller request is covered, a larger one asks again
    CHECK(allow_big_lds(&kernels[0], 100000, "t") == SEMIDETR_OK && g_set_calls == 1 && g_last_kernel == &kernels[0] && g_last_value == 100000);
    CHECK(allow_big_lds(&kernels[0], 100000, "t") == SEMIDETR_OK && allow_big_lds(&kernels[0], 70000, "t") == SEMIDETR_OK && g_set_calls == 1);
    CHECK(allow_big_lds(&kernels[0], 150000, "t") == SEMIDETR_OK && g_set_calls == 2 && g_last_value == 150000);
    CHECK(allow_big_lds(&kernels[0], 100000, "t") == SEMIDETR_OK && g_set_calls == 2);
    // the same kernel on a second device is a grant of its own, and does not disturb the first
    g_device = 1;
    CHECK(allow_big_lds(&kernels[0], 100000, "t") == SEMIDETR_OK && g_set_calls == 3);
    CHECK(allow_big_lds(&kernels[0], 100000, "t") == SEMIDETR_OK && g_set_calls == 3);
    g_device = 0;
    CHECK(allow_big_lds(&kernels[0], 150000, "t") == SEMIDETR_OK && g_set_calls == 3);
    // a refused grant: the runtime's code, the caller's prefix in the text, nothing remembered
    g_set_result = hipErrorInvalidValue;
    CHECK(allow_big_lds(&kernels[1], 100000, "some_entry") == (int)hipErrorInvalidValue && g_set_calls == 4);
    CHECK(strcmp(semidetr::error_buffer(), "some_entry: hipFuncSetAttribute(100000 bytes of LDS): stub error") == 0);
    g_set_result = hipSuccess;
    CHECK(allow_big_lds(&kernels[1], 100000, "some_entry") == SEMIDETR_OK && g_set_calls == 5);
    g_get_device_result = hipErrorInvalidDevice;
    CHECK(allow_big_lds(&kernels[2], 100000, "some_entry") == (int)hipErrorInvalidDevice && g_set_calls == 5);
    CHECK(strcmp(semidetr::error_buffer(), "some_entry: hipGetDevice: stub error") == 0);
    g_get_device_result = hipSuccess;
    // growth past the table's capacity: the product's 28 kernels on 8 devices (224 pairs) are all remembered ...
    int before = g_set_calls;
    for (int dev = 0; dev < 8; ++dev)
        for (int k = 10; k < 38; ++k) {
            g_device = dev;
            CHECK(allow_big_lds(&kernels[k], 150000, "t") == SEMIDETR_OK);
        }
    CHECK(g_set_calls == before + 224);
    for (int dev = 0; dev < 8; ++dev)
        for (int k = 10; k < 38; ++k) {
            g_device = dev;
            CHECK(allow_big_lds(&kernels[k], 150000, "t") == SEMIDETR_OK);
        }
    CHECK(g_set_calls == before + 224);
    // ... and far more pairs than any table holds still succeed, each at the cost of a repeated call
    g_device = 0;
    before = g_set_calls;
    for (int round = 0; round < 2; ++round)
        for (int k = 40; k < 400; ++k) CHECK(allow_big_lds(&kernels[k], 150000, "t") == SEMIDETR_OK);
    CHECK(g_set_calls > before + 360 && g_set_calls <= before + 720 && g_last_kernel == &kernels[399]);
    CHECK(allow_big_lds(&kernels[0], 150000, "t") == SEMIDETR_OK && g_last_kernel != &kernels[0]);      // the early entries stand
    printf("common_host_check: ok\n");
    return 0;
}
