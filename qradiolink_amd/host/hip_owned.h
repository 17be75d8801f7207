// hip_owned.h — move-only owners of what the host layer takes from HIP and from the C ABI: device and pinned buffers, events, streams
// and qrl_* handles.  The host layer sits above the C ABI and throws: every failure becomes a std::runtime_error through chk / hchk.
// Members of these types are released in reverse order of declaration, so a class declares a stream before everything created on it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>

#include "qrl_hip.h"

namespace qrl_host {

inline void chk(int rc, const char* what)
{
    if (rc != QRL_OK) throw std::runtime_error(std::string(what) + ": " + qrl_strerror(rc) + " (" + qrl_last_error() + ")");
}
inline void hchk(hipError_t e, const char* what)
{
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// `count` items of T in device (dev_buf) or pinned host (pinned_buf) memory
template <class T, bool pinned>
class hip_buf {
public:
    hip_buf() = default;
    hip_buf(hip_buf&& o) noexcept : d_p(std::exchange(o.d_p, nullptr)), d_n(std::exchange(o.d_n, 0)) {}
    hip_buf& operator=(hip_buf&& o) noexcept { std::swap(d_p, o.d_p); std::swap(d_n, o.d_n); return *this; }
    ~hip_buf() { reset(); }
    void alloc(size_t count)   // releases what it held, then allocates; empty after a failure
    {
        reset();
        void* p = nullptr;
        if (pinned) hchk(hipHostMalloc(&p, count * sizeof(T), hipHostMallocDefault), "hipHostMalloc");
        else hchk(hipMalloc(&p, count * sizeof(T)), "hipMalloc");
        d_p = static_cast<T*>(p); d_n = count;
    }
    void reset()
    {
        if (d_p) (void)(pinned ? hipHostFree(d_p) : hipFree(d_p));
        d_p = nullptr; d_n = 0;
    }
    T* get() const { return d_p; }
    size_t size() const { return d_n; }
private:
    T* d_p = nullptr; size_t d_n = 0;
};
template <class T> using dev_buf = hip_buf<T, false>;
template <class T> using pinned_buf = hip_buf<T, true>;

// a device buffer and the pinned buffer its content is copied out to
template <class T>
struct mirror {
    dev_buf<T> d; pinned_buf<T> h;
    void alloc(size_t count) { d.alloc(count); h.alloc(count); }
    T* dev() const { return d.get(); }
    T* host() const { return h.get(); }
    void download(hipStream_t s) const { download(s, d.get()); }
    // the whole pinned side from another device array of the same size
    void download(hipStream_t s, const T* src) const { hchk(hipMemcpyAsync(h.get(), src, h.size() * sizeof(T), hipMemcpyDeviceToHost, s), "D2H"); }
};

class hip_event {
public:
    hip_event() { hchk(hipEventCreateWithFlags(&d_e, hipEventDisableTiming), "hipEventCreate"); }
    hip_event(hip_event&& o) noexcept : d_e(std::exchange(o.d_e, nullptr)) {}
    hip_event& operator=(hip_event&& o) noexcept { std::swap(d_e, o.d_e); return *this; }
    ~hip_event() { if (d_e) (void)hipEventDestroy(d_e); }
    hipEvent_t get() const { return d_e; }
private:
    hipEvent_t d_e = nullptr;
};

class hip_stream {   // non-blocking
public:
    // lowest priority -- not for the scheduling: streams of one priority share a few hardware queues, and a wait queued on such a
    // stream would otherwise hold back the kernels of a handle stream that happens to sit on the same queue (csrc/engine.cpp, stream creation)
    explicit hip_stream(bool lowest_priority = false)
    {
        int prio_lo = 0, prio_hi = 0;
        if (lowest_priority) (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        hchk(hipStreamCreateWithPriority(&d_s, hipStreamNonBlocking, prio_lo), "hipStreamCreate");
    }
    hip_stream(hip_stream&& o) noexcept : d_s(std::exchange(o.d_s, nullptr)) {}
    hip_stream& operator=(hip_stream&& o) noexcept { std::swap(d_s, o.d_s); return *this; }
    ~hip_stream() { if (d_s) (void)hipStreamDestroy(d_s); }
    hipStream_t get() const { return d_s; }
private:
    hipStream_t d_s = nullptr;
};

// a C-ABI handle and its qrl_*_destroy
template <class T, void (*destroy)(T*)> struct handle_deleter { void operator()(T* p) const { destroy(p); } };
template <class T, void (*destroy)(T*)> using handle = std::unique_ptr<T, handle_deleter<T, destroy>>;
using demod_handle = handle<qrl_demod, qrl_demod_destroy>;
using mod_handle = handle<qrl_mod, qrl_mod_destroy>;
using amod_handle = handle<qrl_amod, qrl_amod_destroy>;
using rssi_handle = handle<qrl_rssi, qrl_rssi_destroy>;
using fft_handle = handle<qrl_fft, qrl_fft_destroy>;
using framesync_handle = handle<qrl_framesync, qrl_framesync_destroy>;
using deframer_handle = handle<qrl_deframer, qrl_deframer_destroy>;
using dmr_rx_handle = handle<qrl_dmr_rx, qrl_dmr_rx_destroy>;
using dmr_sink_handle = handle<qrl_dmr_sink, qrl_dmr_sink_destroy>;
using m17_rx_handle = handle<qrl_m17_rx, qrl_m17_rx_destroy>;

}  // namespace qrl_host
