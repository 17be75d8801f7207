// host_common.cpp — what every host translation unit of libqrl_hip.so links against: error text, launch-error marks, streams, the sc16 input checks, the carrier NCO.
#include "host_common.hpp"
#include "firdes.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>

using namespace qrl;

static thread_local std::string g_last_error;
int qrl_set_error(int code, const std::string& msg) { g_last_error = msg; return code; }

namespace qrl {
static thread_local bool t_launch_error = false;
hipError_t dyn_lds_limit(const void* kernel, int bytes)
{
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) { t_launch_error = true; qrl_set_error(QRL_ERR_HIP, std::string("hipGetDevice: ") + hipGetErrorString(e)); return e; }
    std::lock_guard<std::mutex> g(mu);
    if (done.count({kernel, dev})) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.insert({kernel, dev});
    else { t_launch_error = true; qrl_set_error(QRL_ERR_HIP, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e)); }
    return e;
}
bool take_launch_error() { const bool r = t_launch_error; t_launch_error = false; return r; }
int create_role_stream(hipStream_t* s, int priority, const char* role)
{
    const char* e = role ? std::getenv((std::string("QRL_CU_") + role).c_str()) : nullptr;
    int first = 0, count = 0;
    hipError_t err;
    if (e && std::sscanf(e, "%d:%d", &first, &count) == 2 && first >= 0 && count > 0 && first + count <= 32) {
        uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // 256 CUs
        for (int b = 8 * first; b < 8 * (first + count); ++b) mask[b >> 5] |= 1u << (b & 31);
        err = hipExtStreamCreateWithCUMask(s, 8, mask);
    } else {
        err = hipStreamCreateWithPriority(s, hipStreamNonBlocking, priority);
    }
    if (err != hipSuccess) { qrl_set_error(QRL_ERR_HIP, std::string("stream creation: ") + hipGetErrorString(err)); return QRL_ERR_HIP; }
    return QRL_OK;
}

int HandleStream::open(void* user_stream, const char* role, const char* low_prio_env)
{
    if (user_stream) { s = static_cast<hipStream_t>(user_stream); return QRL_OK; }
    if (role && std::getenv((std::string("QRL_CU_") + role).c_str())) return open_internal(0, role);
    if (low_prio_env && std::getenv(low_prio_env)) {   // experiment: a CU-masked stream has no priority argument (it is a NORMAL stream), so a masked
        int plo = 0, phi = 0;                          // internal stream only outranks this one when this one is created BELOW normal
        (void)hipDeviceGetStreamPriorityRange(&plo, &phi);
        HIPCHK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, plo));
    }
    else HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    own = true;
    return QRL_OK;
}

int ProfSpans::begin(hipStream_t s)
{
    drop_open();
    HIPCHK(hipEventCreate(&b0)); HIPCHK(hipEventCreate(&b1));
    HIPCHK(hipEventRecord(b0, s));
    return QRL_OK;
}
int ProfSpans::end(hipStream_t s)
{
    HIPCHK(hipEventRecord(b1, s));
    spans.emplace_back(b0, b1);
    b0 = b1 = nullptr;
    return QRL_OK;
}
int ProfSpans::read(double& ms, uint64_t& count)
{
    hipError_t err = hipSuccess;
    double total = 0;
    for (auto& e : spans) {
        float t = 0;
        if (err == hipSuccess) err = hipEventElapsedTime(&t, e.first, e.second);
        total += t;
    }
    count = spans.size();
    clear();
    if (err != hipSuccess) return qrl_set_error(QRL_ERR_HIP, std::string("hipEventElapsedTime: ") + hipGetErrorString(err));
    ms = total;
    return QRL_OK;
}
void ProfSpans::clear()
{
    for (auto& e : spans) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    spans.clear();
    drop_open();
}
void ProfSpans::drop_open()
{
    if (b0) (void)hipEventDestroy(b0);
    if (b1) (void)hipEventDestroy(b1);
    b0 = b1 = nullptr;
}
bool sc16_scale_ok(const char* who, float scale)
{
    if (std::isfinite(scale) && scale != 0.0f) return true;
    qrl_set_error(QRL_ERR_ARG, std::string(who) + ": scale must be finite and non-zero");
    return false;
}
bool sc16_rows_ok(const char* who, const void* iq, size_t stride)
{
    if (!(reinterpret_cast<uintptr_t>(iq) & 15u) && !(stride & 3u)) return true;
    qrl_set_error(QRL_ERR_ARG, std::string(who) + ": sc16 iq must be 16-byte aligned, stride a multiple of 4 samples");
    return false;
}
bool iq8_bias_ok(const char* who, float bias)
{
    if (std::isfinite(bias)) return true;
    qrl_set_error(QRL_ERR_ARG, std::string(who) + ": bias must be finite");
    return false;
}
bool iq8_rows_ok(const char* who, const void* iq, size_t stride)
{
    if (reinterpret_cast<uintptr_t>(iq) & 15u) { qrl_set_error(QRL_ERR_ARG, std::string(who) + ": 8-bit iq must be 16-byte aligned"); return false; }
    if (stride & 7u) { qrl_set_error(QRL_ERR_ARG, std::string(who) + ": the stride of 8-bit iq must be a multiple of 8 samples (16 bytes)"); return false; }
    return true;
}

std::vector<float2> rot_fine_table(uint64_t inc)
{
    std::vector<float2> lo(512);
    for (int r = 0; r < 512; ++r) { float sn, cs; sincos_turn_host((uint64_t)r * inc, sn, cs); lo[r] = make_float2(cs, sn); }
    return lo;
}
int Rotator::retune(uint64_t n_now, uint64_t new_inc, hipStream_t s)
{
    const uint64_t delta = advance(n_now);
    inc = new_inc;
    if (hipMemcpy(lo.p, rot_fine_table(inc).data(), 512 * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) return QRL_ERR_HIP;
    if (!per_stream()) return QRL_OK;
    const int B = (int)h_inc.size();
    launch_rot_ps_advance(acc_s.p, inc_s.p, B, delta, s);
    launch_rot_ps_fill(acc_s.p, inc_s.p, lo_s.p, B, 0, 0, inc, lo.p, s);
    if (hipStreamSynchronize(s) != hipSuccess) return qrl_set_error(QRL_ERR_HIP, "per-stream rotator: hipStreamSynchronize failed");
    h_inc.assign((size_t)B, inc);
    return QRL_OK;
}
int Rotator::retune_streams(uint64_t n_now, const std::vector<uint64_t>& new_inc, hipStream_t s)
{
    const uint64_t delta = advance(n_now);
    const int B = (int)new_inc.size();
    if (!per_stream()) {   // first per-stream set: every stream starts where the shared NCO is (acc = its phase at the new nbase)
        int r;
        if ((r = acc_s.grow((size_t)B)) || (r = inc_s.grow((size_t)B)) || (r = lo_s.grow((size_t)B * 512))) return r;
        launch_rot_ps_fill(acc_s.p, inc_s.p, lo_s.p, B, 1, acc, inc, lo.p, s);
        h_inc.assign((size_t)B, inc);
    } else {
        launch_rot_ps_advance(acc_s.p, inc_s.p, B, delta, s);
    }
    // only the streams whose increment changes: their increments and tables, one copy per run of consecutive streams
    std::vector<uint32_t> idx;
    for (int b = 0; b < B; ++b) if (new_inc[(size_t)b] != h_inc[(size_t)b]) idx.push_back((uint32_t)b);
    std::vector<uint64_t> st_inc(idx.size());
    std::vector<float2> st_lo(idx.size() * 512);
    for (size_t j = 0; j < idx.size(); ++j) {
        st_inc[j] = new_inc[idx[j]];
        const std::vector<float2> t = rot_fine_table(st_inc[j]);
        std::copy(t.begin(), t.end(), st_lo.begin() + (ptrdiff_t)(j * 512));
    }
    for (size_t j0 = 0; j0 < idx.size();) {
        size_t j1 = j0 + 1;
        while (j1 < idx.size() && idx[j1] == idx[j1 - 1] + 1) ++j1;
        const size_t n = j1 - j0;
        if (hipMemcpyAsync(inc_s.p + idx[j0], st_inc.data() + j0, n * sizeof(uint64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(lo_s.p + (size_t)idx[j0] * 512, st_lo.data() + j0 * 512, n * 512 * sizeof(float2), hipMemcpyHostToDevice, s) != hipSuccess)
            return qrl_set_error(QRL_ERR_HIP, "per-stream rotator: upload failed");
        j0 = j1;
    }
    if (hipStreamSynchronize(s) != hipSuccess) return qrl_set_error(QRL_ERR_HIP, "per-stream rotator: hipStreamSynchronize failed");
    for (uint32_t b : idx) h_inc[b] = new_inc[b];
    return QRL_OK;
}
int Rotator::reset(hipStream_t s)
{
    acc = 0; nbase = 0;
    if (!per_stream()) return QRL_OK;
    if (hipMemsetAsync(acc_s.p, 0, h_inc.size() * sizeof(uint64_t), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return qrl_set_error(QRL_ERR_HIP, "per-stream rotator: reset failed");
    return QRL_OK;
}
int carrier_incs(const double* hz, int B, double sign, double rate, std::vector<uint64_t>& inc)
{
    for (int b = 0; b < B; ++b) if (!std::isfinite(hz[b])) return qrl_set_error(QRL_ERR_ARG, "carrier offsets must be finite");
    inc.resize((size_t)B);
    for (int b = 0; b < B; ++b) inc[(size_t)b] = phase_inc_to_turn(2 * M_PI * (sign * hz[b]) / rate);
    return QRL_OK;
}
}  // namespace qrl

// ---- C ABI (C linkage from the declarations in qrl_hip.h)
const char* qrl_last_error(void) { return g_last_error.c_str(); }
const char* qrl_strerror(int s)
{
    switch (s) {
    case QRL_OK: return "ok";
    case QRL_ERR_ARG: return "invalid argument or unsupported mode";
    case QRL_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
    case QRL_ERR_HIP: return "HIP runtime error";
    case QRL_ERR_NOMEM: return "out of device memory";
    case QRL_ERR_TOO_BIG: return "chunk larger than max_chunk";
    case QRL_ERR_STATE: return "invalid handle state";
    }
    return "unknown";
}
