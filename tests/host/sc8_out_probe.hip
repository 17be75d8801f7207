// sc8_out_probe.hip — TEST INFRASTRUCTURE: f2_to_sc8 and sc8_store of devmath.hpp alone, each behind one extern "C" entry
// (tests/test_gpu_sc8_convert.py).  The header is included as it is and no arithmetic is restated here.  Built with the HIPFLAGS of
// qradiolink_amd/csrc/Makefile into tests/host/libqrl_sc8_out_probe.so; not linked into libqrl_hip.so, and nothing in the product refers to it.
// Every entry takes host arrays, copies them up, runs its kernel, copies the result down and returns the HIP error code (0 = hipSuccess).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../qradiolink_amd/csrc/devmath.hpp"

namespace {

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
    void down(T* host) { if (*err == hipSuccess && n) *err = hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost); }
    Dev(const Dev&) = delete; Dev& operator=(const Dev&) = delete;
};
inline void ran(hipError_t* err)
{
    if (*err == hipSuccess) *err = hipGetLastError();
    if (*err == hipSuccess) *err = hipDeviceSynchronize();
}

__global__ void k_f2_to_sc8(const float* vi, const float* vq, size_t n, float scale, uint16_t* w, uint32_t* nclip)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t nc;
    w[i] = qrl::f2_to_sc8(make_float2(vi[i], vq[i]), scale, nc);
    nclip[i] = nc;
}
// sc8_store under divergence: lane t of row blockIdx.y takes the branch branch[.] names (0..3; anything else leaves before the ladder), so up to four
// groups of lanes of one wave call sc8_store separately, each with its own scale; all waves and workgroups of a row add to clip[row]
struct Scales4 { float s[4]; };
__global__ void k_sc8_store_divergent(const float* vi, const float* vq, const uint8_t* valid, const uint8_t* branch, uint32_t n, Scales4 sc,
                                      uint16_t* out, uint32_t* clip)
{
    const uint32_t b = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const size_t g = (size_t)b * n + t;
    const uint32_t id = branch[g];
    if (id > 3u) return;
    uint16_t* row = out + (size_t)b * n;
    const float2 v = make_float2(vi[g], vq[g]);
    const bool ok = valid[g] != 0;
    if (id == 0u) qrl::sc8_store(row, t, v, ok, sc.s[0], clip + b);
    else if (id == 1u) qrl::sc8_store(row, t, v, ok, sc.s[1], clip + b);
    else if (id == 2u) qrl::sc8_store(row, t, v, ok, sc.s[2], clip + b);
    else qrl::sc8_store(row, t, v, ok, sc.s[3], clip + b);
}
// the word-sharing rule: one workgroup of two waves, wave w writes samples w, w + 2, w + 4, ... of the row: every 32-bit word of the row holds one sample
// of each wave (or, at the row's ends, one sample and a piece of what lies outside)
__global__ __launch_bounds__(128) void k_sc8_store_alternate(const float* vi, const float* vq, uint32_t n, float scale, uint16_t* row)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t k = lane; 2u * k + wave < n; k += 64u) {
        const uint32_t idx = 2u * k + wave;
        qrl::sc8_store(row, idx, make_float2(vi[idx], vq[idx]), true, scale, nullptr);
    }
}

}  // namespace

extern "C" {

int qrl_probe_f2_to_sc8(const float* vi, const float* vq, size_t n, float scale, uint16_t* word, uint32_t* nclip)
{
    hipError_t e = hipSuccess;
    Dev<float> di(n, vi, &e), dq(n, vq, &e); Dev<uint16_t> dw(n, nullptr, &e); Dev<uint32_t> dn(n, nullptr, &e);
    if (e == hipSuccess && n) { k_f2_to_sc8<<<dim3((unsigned)((n + 255) / 256)), 256>>>(di.p, dq.p, n, scale, dw.p, dn.p); ran(&e); }
    dw.down(word); dn.down(nclip);
    return (int)e;
}
// vi, vq, valid, branch: [batch][n]; scales: the four branches' scales; out: [batch][n] 16-bit words, read (the caller's sentinel) and written back;
// clip: [batch] counters, read and written back
int qrl_probe_sc8_store_divergent(const float* vi, const float* vq, const uint8_t* valid, const uint8_t* branch, uint32_t n, uint32_t batch,
                                  const float* scales4, uint16_t* out, uint32_t* clip)
{
    hipError_t e = hipSuccess;
    const size_t tot = (size_t)n * batch;
    Dev<float> di(tot, vi, &e), dq(tot, vq, &e); Dev<uint8_t> dv(tot, valid, &e), db(tot, branch, &e);
    Dev<uint16_t> dout(tot, out, &e); Dev<uint32_t> dclip(batch, clip, &e);
    if (e == hipSuccess && tot) {
        Scales4 sc; for (int k = 0; k < 4; ++k) sc.s[k] = scales4[k];
        k_sc8_store_divergent<<<dim3((n + 255) / 256, batch), 256>>>(di.p, dq.p, dv.p, db.p, n, sc, dout.p, dclip.p);
        ran(&e);
    }
    dout.down(out); dclip.down(clip);
    return (int)e;
}
// buf: `total` 16-bit words, read (the caller's sentinel) and written back; the row of n samples starts at word `first` of it (hipMalloc's base is
// 256-byte aligned, so an odd `first` puts the row at an address = 2 mod 4).  -1: the row does not fit.
int qrl_probe_sc8_store_alternate(const float* vi, const float* vq, uint32_t n, float scale, uint16_t* buf, uint32_t total, uint32_t first)
{
    if ((uint64_t)first + n > total) return -1;
    hipError_t e = hipSuccess;
    Dev<float> di(n, vi, &e), dq(n, vq, &e); Dev<uint16_t> dbuf(total, buf, &e);
    if (e == hipSuccess && n) { k_sc8_store_alternate<<<1, 128>>>(di.p, dq.p, n, scale, dbuf.p + first); ran(&e); }
    dbuf.down(buf);
    return (int)e;
}

}  // extern "C"
