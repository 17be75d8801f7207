// host_common.hpp — what every host translation unit of libqrl_hip.so shares: the context, error reporting, the owning device
// buffer, the streams, events, fences and profile spans of a handle, its carrier NCO, the checks of an sc16 input.  Host only: no .hip file includes it.
#pragma once
#include "../../include/qrl_hip.h"
#include "engine.hpp"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

struct qrl_ctx { int device; };

int qrl_set_error(int code, const std::string& msg);   // host_common.cpp: records the text of qrl_last_error (per thread), returns code

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return qrl_set_error(QRL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace qrl {

inline uint32_t pow2_at_least(size_t v, uint32_t floor) { uint32_t c = floor; while (c < v) c <<= 1; return c; }

// Owning device buffer of n items (at least one is allocated).  alloc() replaces what it held and zeroes the new buffer.
template <class T> struct DevBuf {
    T* p = nullptr; size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    size_t bytes() const { return std::max<size_t>(n, 1) * sizeof(T); }
    // alloc() without the zeroing: one hipFree and one hipMalloc -- for a buffer that grows inside a process() call, or one its first kernel fills whole
    int grow(size_t count) {
        if (p) { (void)hipFree(p); p = nullptr; }
        n = count;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes());
        if (e == hipSuccess) return QRL_OK;
        const std::string what = "hipMalloc(" + std::to_string(bytes()) + " bytes): ";
        p = nullptr; n = 0;
        return qrl_set_error(QRL_ERR_NOMEM, what + hipGetErrorString(e));
    }
    int alloc(size_t count) { if (int r = grow(count)) return r; return zero(); }
    // v followed by `pad` zero items (a kernel that reads its table unguarded)
    int upload(const std::vector<T>& v, size_t pad = 0) {
        if (int r = alloc(v.size() + pad)) return r;
        if (!v.empty() && hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return QRL_ERR_HIP;
        return QRL_OK;
    }
    int zero() { return hipMemset(p, 0, bytes()) == hipSuccess ? QRL_OK : QRL_ERR_HIP; }
    // `count` byte-copies of proto (padding included) into the buffer alloc() made: the initial state of `count` identical streams
    int fill(size_t count, const T& proto) {
        std::vector<unsigned char> h(count * sizeof(T));
        for (size_t i = 0; i < count; ++i) std::memcpy(h.data() + i * sizeof(T), &proto, sizeof(T));
        return hipMemcpy(p, h.data(), h.size(), hipMemcpyHostToDevice) == hipSuccess ? QRL_OK : QRL_ERR_HIP;
    }
};

// A stream of a handle.  open(): the caller's, or one of the handle's own (hipStreamNonBlocking; with a role, the QRL_CU_<ROLE> stream of
// create_role_stream when that variable is set; else, when the variable `low_prio_env` names is set, a stream of the lowest priority).
// open_internal(): an internal stream of the handle, create_role_stream(priority, role).  Null until opened; destroys only what it made.
struct HandleStream {
    HandleStream() = default;
    HandleStream(const HandleStream&) = delete; HandleStream& operator=(const HandleStream&) = delete;
    ~HandleStream() { if (own && s) (void)hipStreamDestroy(s); }
    int open(void* user_stream, const char* role = nullptr, const char* low_prio_env = nullptr);
    int open_internal(int priority, const char* role) { if (int r = create_role_stream(&s, priority, role)) return r; own = true; return QRL_OK; }
    operator hipStream_t() const { return s; }
    bool owned() const { return own; }
private:
    hipStream_t s = nullptr; bool own = false;
};

#define QRLCHK(expr) do { if (int r_ = (expr)) return r_; } while (0)   // for the int-status members below

// Owning event, made on first record() or by create() (before its raw handle is given to a launcher); hipEventDisableTiming.
struct Event {
    Event() = default;
    Event(const Event&) = delete; Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    int create() { if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return QRL_OK; }
    int record(hipStream_t s) { QRLCHK(create()); HIPCHK(hipEventRecord(e, s)); return QRL_OK; }
    int wait(hipStream_t s) const { HIPCHK(hipStreamWaitEvent(s, e, 0)); return QRL_OK; }
    int relay(hipStream_t from, hipStream_t to) { QRLCHK(record(from)); return wait(to); }   // `to` goes on behind what `from` holds now
    operator hipEvent_t() const { return e; }
private:
    hipEvent_t e = nullptr;
};

// An event that orders a later call behind an earlier one, and whether it has been recorded since the last disarm().  Two rules:
// STICKY (wait): every call waits again -- the guard of a ring slot that is reused every second or third call;
// ONE-SHOT (wait_once): the first waiter takes it -- "the call before has left this buffer", needed once per record.
struct Fence {
    int create() { return ev.create(); }
    int record(hipStream_t s) { QRLCHK(ev.record(s)); armed = true; return QRL_OK; }
    int wait(hipStream_t s) const { return armed ? ev.wait(s) : QRL_OK; }
    int wait_once(hipStream_t s) { if (!armed) return QRL_OK; armed = false; return ev.wait(s); }
    void disarm() { armed = false; }
    operator hipEvent_t() const { return ev; }
private:
    Event ev; bool armed = false;
};

// The timing-event pairs around one kernel set of the profiled calls (default flags, a new pair per call).  A span begun and not
// ended (an error return in between) is freed by the next begin(), by read() or with the set.
struct ProfSpans {
    ProfSpans() = default;
    ProfSpans(const ProfSpans&) = delete; ProfSpans& operator=(const ProfSpans&) = delete;
    ~ProfSpans() { clear(); }
    int begin(hipStream_t s);
    int end(hipStream_t s);
    bool open() const { return b0 != nullptr; }       // begun, not yet ended
    int read(double& ms, uint64_t& count);             // sum and number of the ended spans; empties the set, on an error return too
    void clear();
private:
    void drop_open();
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans; hipEvent_t b0 = nullptr, b1 = nullptr;
};

// ---- sc16 input (qrl_*_process_sc16 of the receivers and the spectrum tap): false = refused, with the error text set ----
bool sc16_scale_ok(const char* who, float scale);                       // finite and non-zero
bool sc16_rows_ok(const char* who, const void* iq, size_t stride);     // 16-byte aligned base, stride a multiple of 4 samples
// ---- 8-bit input (qrl_*_process_sc8 / _cu8): the scale by sc16_scale_ok; each broken rule has its own text ----
bool iq8_bias_ok(const char* who, float bias);                         // finite
bool iq8_rows_ok(const char* who, const void* iq, size_t stride);      // 16-byte aligned base, stride a multiple of 8 samples

// ---- the carrier NCO of a handle (qrl_demod, qrl_mod, qrl_amod): exact 2^-64-turn accumulator, phase continuous across retunes ----
// Shared form: one (acc, inc) for every stream, phase of sample n = acc + (n - nbase) inc, and the 512-entry fine table of inc.
// Per-stream form (from the first retune_streams on): device arrays acc_s[B], inc_s[B], lo_s[B][512]; nbase stays shared.
// The caller turns Hz into increments (its sign and rate), says which sample counter is "now" and drains its streams before a retune.
struct Rotator {
    uint64_t inc = 0, acc = 0, nbase = 0;
    DevBuf<float2> lo;                                     // allocated once by init(), rewritten in place
    DevBuf<uint64_t> acc_s, inc_s; DevBuf<float2> lo_s;
    std::vector<uint64_t> h_inc;                           // host copy of inc_s
    bool per_stream() const { return lo_s.p != nullptr; }   // (the last of the three to be allocated)
    int init(uint64_t inc0) { inc = inc0; return lo.upload(rot_fine_table(inc)); }
    // every stream to new_inc.  Per-stream form: each goes on from its own phase.  Host-synchronous on s.
    int retune(uint64_t n_now, uint64_t new_inc, hipStream_t s);
    // stream b to new_inc[b]; only streams whose increment changes get a table upload.  The first call starts every stream at the shared
    // phase.  Host-synchronous on s.
    int retune_streams(uint64_t n_now, const std::vector<uint64_t>& new_inc, hipStream_t s);
    int reset(hipStream_t s);   // every phase and nbase to 0; the offsets stay
    template <class Pp> void fill(Pp& p) const {
        p.rot_acc = acc; p.rot_inc = inc; p.rot_nbase = nbase; p.rot_lo = lo.p;
        if (per_stream()) { p.rot_acc_s = acc_s.p; p.rot_inc_s = inc_s.p; p.rot_lo = lo_s.p; }
    }
private:
    uint64_t advance(uint64_t n_now) { const uint64_t delta = n_now - nbase; acc += delta * inc; nbase = n_now; return delta; }
};
// the increments of B carrier offsets: sign * hz[b] cycles per `rate` samples.  QRL_ERR_ARG unless every offset is finite.
int carrier_incs(const double* hz, int B, double sign, double rate, std::vector<uint64_t>& inc);

}  // namespace qrl
