// fec_probe.hip — TEST INFRASTRUCTURE: the product's K=7 Viterbi decoder + descrambler (k_fec behind qrl::launch_fec of libqrl_hip.so) alone, on
// soft symbols of the caller's choosing (tests/test_gpu_fec_probe.py).  Host code only: it fills a FecParams as engine.cpp does, makes ONE call of
// qrl::launch_fec on the null stream and synchronises.  No decoder arithmetic is restated here and no kernel is compiled here.  Built with the HIPFLAGS
// of qradiolink_amd/csrc/Makefile into tests/host/libqrl_fec_probe.so, linked against libqrl_hip.so; not linked into it, and nothing in the product
// refers to it.
// The caller keeps the soft ring and the decoder state between calls, as a handle does: every argument is a host array that is copied up, and what
// the decoder may write (state, bits, counts) is copied down again.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../qradiolink_amd/csrc/engine.hpp"

namespace {

// device array: hipMalloc + optional upload; the first error sticks in *err
template <class T>
struct Dev {
    T* p = nullptr; size_t n; hipError_t* err;
    Dev(size_t n_, const T* host, hipError_t* e) : n(n_), err(e)
    {
        if (*err != hipSuccess) return;
        *err = hipMalloc((void**)&p, (n ? n : 1) * sizeof(T));
        if (*err == hipSuccess && host && n) *err = hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
    }
    ~Dev() { if (p) (void)hipFree(p); }
    void down(T* host) { if (*err == hipSuccess && host && n) *err = hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost); }
    Dev(const Dev&) = delete; Dev& operator=(const Dev&) = delete;
};

}  // namespace

extern "C" {

// soft: [batch][mask + 1] ring (mask + 1 a power of two), item i of a stream at i & mask; avail: [batch] items written so far, the decoder may read
// avail[b] * avail_mul soft symbols of stream b; branches: 1 or 2 (2: unit 2b + 1 decodes stream b delayed by one symbol); st: [batch][2] FecState, read
// and written back; bits_a / bits_b: [batch][bits_cap] or null, read (the caller's guard fill) and written back; counts: [batch * 4], read and written back
// (the decoder writes [4b + 2] and, with two branches, [4b + 3]).  Returns the HIP error code (0 = hipSuccess), -1 for arguments the decoder's
// contract does not cover.
int qrl_probe_fec(const uint8_t* soft, uint32_t mask, const uint64_t* avail, uint32_t avail_mul, int branches, int batch, void* st, size_t bits_cap,
                  uint8_t* bits_a, uint8_t* bits_b, uint32_t* counts)
{
    if (!soft || !avail || !st || !counts || batch < 1 || (branches != 1 && branches != 2) || (mask & (mask + 1u)) != 0u || mask < 63u) return -1;
    hipError_t e = hipSuccess;
    const size_t B = (size_t)batch;
    Dev<uint8_t> dsoft(B * ((size_t)mask + 1), soft, &e);
    Dev<uint64_t> davail(B, avail, &e);
    Dev<qrl::FecState> dst(B * 2, static_cast<const qrl::FecState*>(st), &e);
    Dev<uint8_t> da(bits_a ? B * bits_cap : 0, bits_a, &e), db(bits_b ? B * bits_cap : 0, bits_b, &e);
    Dev<uint32_t> dcounts(B * 4, counts, &e);
    if (e == hipSuccess) {
        qrl::FecParams f{};
        f.soft = qrl::RingB{dsoft.p, mask};
        f.avail = davail.p; f.avail_stride = sizeof(uint64_t); f.avail_mul = avail_mul;
        f.st = dst.p;
        f.bits_a = bits_a ? da.p : nullptr; f.bits_b = bits_b ? db.p : nullptr; f.bits_cap = bits_cap;
        f.counts = dcounts.p; f.branches = branches;
        qrl::launch_fec(f, batch, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    dst.down(static_cast<qrl::FecState*>(st));
    da.down(bits_a); db.down(bits_b);
    dcounts.down(counts);
    return (int)e;
}

}  // extern "C"
