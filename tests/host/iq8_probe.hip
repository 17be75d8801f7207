// iq8_probe.hip — TEST INFRASTRUCTURE: the 8-bit conversion helper of engine.hpp (iq8_to_f2, with the mask iq8_mask gives a format) alone behind
// one extern "C" entry (tests/test_gpu_iq8_convert.py).  The header is included as it is and no arithmetic is restated here.  Built with the
// HIPFLAGS of qradiolink_amd/csrc/Makefile into tests/host/libqrl_iq8_probe.so; not linked into libqrl_hip.so, nothing in the product refers to it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../qradiolink_amd/csrc/engine.hpp"

namespace {

__global__ void k_iq8_to_f2(const uint16_t* w, size_t n, int fmt, float bias, float scale, float* re, float* im)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float2 r = qrl::iq8_to_f2(w[i], qrl::iq8_mask(fmt), bias, scale);
    re[i] = r.x; im[i] = r.y;
}

}  // namespace

// words[n] (host): the 16-bit word of each sample, I in the low byte.  fmt: 2 = sc8 (the caller passes the bias 128, as the library does), 3 = cu8.
// re[n], im[n] (host) receive the converted components.  Returns the HIP error code (0 = hipSuccess).
extern "C" int qrl_probe_iq8_to_f2(const uint16_t* words, size_t n, int fmt, float bias, float scale, float* re, float* im)
{
    uint16_t* dw = nullptr; float* dre = nullptr; float* dim = nullptr;
    hipError_t err = hipMalloc((void**)&dw, n * sizeof(uint16_t));
    if (err == hipSuccess) err = hipMalloc((void**)&dre, n * sizeof(float));
    if (err == hipSuccess) err = hipMalloc((void**)&dim, n * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(dw, words, n * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_iq8_to_f2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dw, n, fmt, bias, scale, dre, dim);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(re, dre, n * sizeof(float), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(im, dim, n * sizeof(float), hipMemcpyDeviceToHost);
    if (dw) (void)hipFree(dw);
    if (dre) (void)hipFree(dre);
    if (dim) (void)hipFree(dim);
    return (int)err;
}
