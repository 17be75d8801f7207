// devmath_probe.hip — TEST INFRASTRUCTURE: the device math primitives of devmath.hpp / engine.hpp / qrl_contracts.h, each alone behind one
// extern "C" entry (tests/test_gpu_devmath.py).  The headers are included as they are and no arithmetic is restated here: a kernel loads its
// operands, calls the primitive, stores the result.  Built with the HIPFLAGS of qradiolink_amd/csrc/Makefile into tests/host/libqrl_devmath_probe.so;
// not linked into libqrl_hip.so, and nothing in the product refers to it.
// Every entry takes host arrays, copies them up, runs 256-thread blocks, copies the result down and returns the HIP error code (0 = hipSuccess).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../qradiolink_amd/csrc/devmath.hpp"
#include "../../qradiolink_amd/csrc/engine.hpp"
#include "../../include/qrl_contracts.h"

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
    void down(T* host) { if (*err == hipSuccess && n) *err = hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost); }
    Dev(const Dev&) = delete; Dev& operator=(const Dev&) = delete;
};
inline void ran(hipError_t* err)
{
    if (*err == hipSuccess) *err = hipGetLastError();
    if (*err == hipSuccess) *err = hipDeviceSynchronize();
}
inline dim3 grid1(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
#define IDX const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x

__global__ void k_sincos_rad(const float* x, size_t n, float* c, float* s)
{
    IDX; if (i >= n) return;
    const float2 r = qrl::sincos_rad(x[i]); c[i] = r.x; s[i] = r.y;
}
__global__ void k_sincos_turn(const uint64_t* a, size_t n, float* c, float* s)
{
    IDX; if (i >= n) return;
    const float2 r = qrl::sincos_turn(a[i]); c[i] = r.x; s[i] = r.y;
}
__global__ void k_fast_atan2(const float* y, const float* x, size_t n, const float* T, float* o)
{
    IDX; if (i >= n) return;
    o[i] = qrl::fast_atan2f_lut(y[i], x[i], T);
}
__global__ void k_tanh_lut(const float* x, size_t n, const float* T, float* o)
{
    IDX; if (i >= n) return;
    o[i] = qrl::tanhf_lut(x[i], T);
}
__global__ void k_clip(const float* x, const float* lim, size_t n, float* o)
{
    IDX; if (i >= n) return;
    o[i] = qrl::branchless_clip(x[i], lim[i]);
}
__global__ void k_ted_error(const float* u, size_t n, float* ff, float* cc)
{
    using qrl::branchless_clip;
    IDX; if (i >= n) return;
    ff[i] = QRL_TED_MODMM_ERROR(QRL_TED_MODMM_FF, u[i], branchless_clip);
    cc[i] = QRL_TED_MODMM_ERROR(QRL_TED_MODMM_CC, u[i], branchless_clip);
}
// the wave stays converged up to the call, as in the loops: the lanes past the end carry an in-range 0
__global__ void k_phase_wrap(const float* x, size_t n, float* o)
{
    IDX;
    const float v = i < n ? x[i] : 0.0f;
    const float r = qrl::phase_wrap(v);
    if (i < n) o[i] = r;
}
__global__ void k_det_log2(const float* x, size_t n, float* o)
{
    IDX; if (i >= n) return;
    o[i] = qrl::det_log2f(x[i]);
}
__global__ void k_det_log10(const float* x, size_t n, float* o)
{
    IDX; if (i >= n) return;
    o[i] = qrl::det_log10f(x[i]);
}
__global__ void k_f2_to_sc16(const float* vi, const float* vq, size_t n, float scale, uint32_t* w, uint32_t* nclip)
{
    IDX; if (i >= n) return;
    uint32_t nc;
    w[i] = qrl::f2_to_sc16(make_float2(vi[i], vq[i]), scale, nc);
    nclip[i] = nc;
}
__global__ void k_sc16_to_f2(const uint32_t* w, size_t n, float scale, float* oi, float* oq)
{
    IDX; if (i >= n) return;
    const float2 r = qrl::sc16_to_f2(w[i], scale);
    oi[i] = r.x; oq[i] = r.y;
}
// sc16_store under divergence: lane t of row blockIdx.y takes the branch branch[.] names (0..3; anything else leaves before the ladder), so up to four
// groups of lanes of one wave call sc16_store separately, each with its own scale; all waves and workgroups of a row add to clip[row]
struct Scales4 { float s[4]; };
__global__ void k_sc16_store_divergent(const float* vi, const float* vq, const uint8_t* valid, const uint8_t* branch, uint32_t n, Scales4 sc,
                                       uint32_t* out, uint32_t* clip)
{
    const uint32_t b = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const size_t g = (size_t)b * n + t;
    const uint32_t id = branch[g];
    if (id > 3u) return;
    uint32_t* row = out + (size_t)b * n;
    const float2 v = make_float2(vi[g], vq[g]);
    const bool ok = valid[g] != 0;
    if (id == 0u) qrl::sc16_store(row, t, v, ok, sc.s[0], clip + b);
    else if (id == 1u) qrl::sc16_store(row, t, v, ok, sc.s[1], clip + b);
    else if (id == 2u) qrl::sc16_store(row, t, v, ok, sc.s[2], clip + b);
    else qrl::sc16_store(row, t, v, ok, sc.s[3], clip + b);
}

}  // namespace

extern "C" {

int qrl_probe_sincos_rad(const float* x, size_t n, float* c, float* s)
{
    hipError_t e = hipSuccess;
    Dev<float> dx(n, x, &e), dc(n, nullptr, &e), ds(n, nullptr, &e);
    if (e == hipSuccess && n) { k_sincos_rad<<<grid1(n), 256>>>(dx.p, n, dc.p, ds.p); ran(&e); }
    dc.down(c); ds.down(s);
    return (int)e;
}
int qrl_probe_sincos_turn(const uint64_t* a, size_t n, float* c, float* s)
{
    hipError_t e = hipSuccess;
    Dev<uint64_t> da(n, a, &e); Dev<float> dc(n, nullptr, &e), ds(n, nullptr, &e);
    if (e == hipSuccess && n) { k_sincos_turn<<<grid1(n), 256>>>(da.p, n, dc.p, ds.p); ran(&e); }
    dc.down(c); ds.down(s);
    return (int)e;
}
int qrl_probe_fast_atan2(const float* y, const float* x, size_t n, const float* table257, float* out)
{
    hipError_t e = hipSuccess;
    Dev<float> dy(n, y, &e), dx(n, x, &e), dt(257, table257, &e), dout(n, nullptr, &e);
    if (e == hipSuccess && n) { k_fast_atan2<<<grid1(n), 256>>>(dy.p, dx.p, n, dt.p, dout.p); ran(&e); }
    dout.down(out);
    return (int)e;
}
int qrl_probe_tanh_lut(const float* x, size_t n, const float* table256, float* out)
{
    // one float past the table (upstream's tanhf_lut reads [256] at x == 2; the restated one clamps): in bounds here, and no value of tanh
    float guarded[257];
    for (int k = 0; k < 256; ++k) guarded[k] = table256[k];
    guarded[256] = 99.0f;
    hipError_t e = hipSuccess;
    Dev<float> dx(n, x, &e), dt(257, guarded, &e), dout(n, nullptr, &e);
    if (e == hipSuccess && n) { k_tanh_lut<<<grid1(n), 256>>>(dx.p, n, dt.p, dout.p); ran(&e); }
    dout.down(out);
    return (int)e;
}
int qrl_probe_clip(const float* x, const float* limit, size_t n, float* out)
{
    hipError_t e = hipSuccess;
    Dev<float> dx(n, x, &e), dl(n, limit, &e), dout(n, nullptr, &e);
    if (e == hipSuccess && n) { k_clip<<<grid1(n), 256>>>(dx.p, dl.p, n, dout.p); ran(&e); }
    dout.down(out);
    return (int)e;
}
int qrl_probe_ted_error(const float* u, size_t n, float* ff, float* cc)
{
    hipError_t e = hipSuccess;
    Dev<float> du(n, u, &e), dff(n, nullptr, &e), dcc(n, nullptr, &e);
    if (e == hipSuccess && n) { k_ted_error<<<grid1(n), 256>>>(du.p, n, dff.p, dcc.p); ran(&e); }
    dff.down(ff); dcc.down(cc);
    return (int)e;
}
int qrl_probe_phase_wrap(const float* x, size_t n, float* out)
{
    hipError_t e = hipSuccess;
    Dev<float> dx(n, x, &e), dout(n, nullptr, &e);
    if (e == hipSuccess && n) { k_phase_wrap<<<grid1(n), 256>>>(dx.p, n, dout.p); ran(&e); }
    dout.down(out);
    return (int)e;
}
int qrl_probe_det_log2(const float* x, size_t n, float* out)
{
    hipError_t e = hipSuccess;
    Dev<float> dx(n, x, &e), dout(n, nullptr, &e);
    if (e == hipSuccess && n) { k_det_log2<<<grid1(n), 256>>>(dx.p, n, dout.p); ran(&e); }
    dout.down(out);
    return (int)e;
}
int qrl_probe_det_log10(const float* x, size_t n, float* out)
{
    hipError_t e = hipSuccess;
    Dev<float> dx(n, x, &e), dout(n, nullptr, &e);
    if (e == hipSuccess && n) { k_det_log10<<<grid1(n), 256>>>(dx.p, n, dout.p); ran(&e); }
    dout.down(out);
    return (int)e;
}
int qrl_probe_f2_to_sc16(const float* vi, const float* vq, size_t n, float scale, uint32_t* word, uint32_t* nclip)
{
    hipError_t e = hipSuccess;
    Dev<float> di(n, vi, &e), dq(n, vq, &e); Dev<uint32_t> dw(n, nullptr, &e), dn(n, nullptr, &e);
    if (e == hipSuccess && n) { k_f2_to_sc16<<<grid1(n), 256>>>(di.p, dq.p, n, scale, dw.p, dn.p); ran(&e); }
    dw.down(word); dn.down(nclip);
    return (int)e;
}
int qrl_probe_sc16_to_f2(const uint32_t* word, size_t n, float scale, float* oi, float* oq)
{
    hipError_t e = hipSuccess;
    Dev<uint32_t> dw(n, word, &e); Dev<float> di(n, nullptr, &e), dq(n, nullptr, &e);
    if (e == hipSuccess && n) { k_sc16_to_f2<<<grid1(n), 256>>>(dw.p, n, scale, di.p, dq.p); ran(&e); }
    di.down(oi); dq.down(oq);
    return (int)e;
}
// vi, vq, valid, branch: [batch][n]; scales: the four branches' scales; out: [batch][n] words, read (the caller's sentinel) and written back;
// clip: [batch] counters, read and written back
int qrl_probe_sc16_store_divergent(const float* vi, const float* vq, const uint8_t* valid, const uint8_t* branch, uint32_t n, uint32_t batch,
                                   const float* scales4, uint32_t* out, uint32_t* clip)
{
    hipError_t e = hipSuccess;
    const size_t tot = (size_t)n * batch;
    Dev<float> di(tot, vi, &e), dq(tot, vq, &e); Dev<uint8_t> dv(tot, valid, &e), db(tot, branch, &e);
    Dev<uint32_t> dout(tot, out, &e), dclip(batch, clip, &e);
    if (e == hipSuccess && tot) {
        Scales4 sc; for (int k = 0; k < 4; ++k) sc.s[k] = scales4[k];
        k_sc16_store_divergent<<<dim3((n + 255) / 256, batch), 256>>>(di.p, dq.p, dv.p, db.p, n, sc, dout.p, dclip.p);
        ran(&e);
    }
    dout.down(out); dclip.down(clip);
    return (int)e;
}

}  // extern "C"
