// m17_link.cpp — C ABI of the M17 link layer (kernels_m17_link.hip, m17_link_core.hpp): a handle that keeps, per stream, what the reference's
// M17FrameDecoder and gr_modem keep between frames (lsf, lsfFromLich, lsfSegmentMap, _m17_decoder_locked; src/M17/M17/M17FrameDecoder.cpp:37-159,
// src/gr_modem.cpp:1370-1439), and the stateless transmit framing of a call (src/M17/M17/M17Transmitter.cpp:46-143).  qrl_m17_rx_process runs
// behind qrl_framesync_process on the caller's stream.
#include "host_common.hpp"
#include <cstdint>

using namespace qrl;

struct qrl_m17_rx {
    qrl_ctx* ctx = nullptr;
    size_t batch = 0;
    int can_rx = 0, decode_all_can = 1;
    DevBuf<uint8_t> states;    // M17_RX_STATE_BYTES per stream (m17_link_core.hpp's m17_rx_state)
    DevBuf<uint8_t> scratch;   // the decode stage's 40-byte records, [batch][cap_frames] of the largest call so far
};

static_assert(QRL_M17_RX_RECORD_BYTES == M17_RX_RECORD_BYTES && QRL_M17_RX_STATE_BYTES == M17_RX_PUBLIC_BYTES, "qrl_hip.h and engine.hpp agree");

static bool config_ok(const qrl_m17_rx_config* c)
{
    return c && c->can_rx >= 0 && c->can_rx <= 15 && (c->decode_all_can == 0 || c->decode_all_can == 1);
}

extern "C" {

int qrl_m17_rx_create(qrl_ctx* ctx, size_t batch, const qrl_m17_rx_config* config, qrl_m17_rx** out)
{
    if (out) *out = nullptr;
    if (!ctx || !out || !batch) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_create: null argument or empty batch");
    if (!config_ok(config)) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_create: can_rx outside 0..15 or decode_all_can outside 0..1");
    HIPCHK(hipSetDevice(ctx->device));
    qrl_m17_rx* h = new qrl_m17_rx;
    h->ctx = ctx; h->batch = batch;
    h->can_rx = config->can_rx; h->decode_all_can = config->decode_all_can;
    if (int r = h->states.grow(batch * M17_RX_STATE_BYTES)) { delete h; return r; }
    launch_m17_rx_reset(h->states.p, batch, nullptr);
    const hipError_t e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { delete h; return qrl_set_error(QRL_ERR_HIP, std::string("qrl_m17_rx_create: ") + hipGetErrorString(e)); }
    *out = h;
    return QRL_OK;
}

void qrl_m17_rx_destroy(qrl_m17_rx* h)
{
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    delete h;
}

int qrl_m17_rx_reset(qrl_m17_rx* h, void* hip_stream)
{
    if (!h) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_reset: null handle");
    HIPCHK(hipSetDevice(h->ctx->device));
    launch_m17_rx_reset(h->states.p, h->batch, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

int qrl_m17_rx_set_config(qrl_m17_rx* h, const qrl_m17_rx_config* config)
{
    if (!h) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_set_config: null handle");
    if (!config_ok(config)) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_set_config: can_rx outside 0..15 or decode_all_can outside 0..1");
    h->can_rx = config->can_rx; h->decode_all_can = config->decode_all_can;
    return QRL_OK;
}

int qrl_m17_rx_process(qrl_m17_rx* h, void* hip_stream, const uint8_t* frames, size_t frame_stride, const uint32_t* counts, size_t cap_frames,
                       uint8_t* out)
{
    if (!h || !frames || !counts || !out || !cap_frames) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_process: null argument or cap_frames 0");
    if (cap_frames > frame_stride / M17_FS_RECORD_BYTES) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_process: 56 * cap_frames > frame_stride");
    if ((reinterpret_cast<uintptr_t>(frames) & 3u) || (frame_stride & 3u))
        return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_process: frames or frame_stride is not a multiple of 4 bytes");
    if (reinterpret_cast<uintptr_t>(out) & 15u) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_process: out is not 16-byte aligned");
    HIPCHK(hipSetDevice(h->ctx->device));
    const size_t need = h->batch * cap_frames * M17_DEC_RECORD_BYTES;
    if (h->scratch.n < need) {   // a larger mailbox than any call before: hipFree waits for what is queued on the old array
        if (int r = h->scratch.grow(need)) return r;
    }
    launch_m17_rx(frames, frame_stride, counts, h->batch, cap_frames, h->can_rx, h->decode_all_can, h->scratch.p, h->states.p, out,
                  static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

int qrl_m17_rx_get_state(qrl_m17_rx* h, void* hip_stream, uint8_t* out)
{
    if (!h || !out) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_get_state: null argument");
    if (reinterpret_cast<uintptr_t>(out) & 15u) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_rx_get_state: out is not 16-byte aligned");
    HIPCHK(hipSetDevice(h->ctx->device));
    launch_m17_rx_state(h->states.p, h->batch, out, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

// ---- transmit: stateless, beside qrl_m17_encode_frames ----
int qrl_m17_call_start(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls, size_t batch, uint8_t* out, size_t out_stride)
{
    if (!ctx || !calls || !out) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_call_start: null argument");
    if (!batch || out_stride < QRL_M17_CALL_START_BYTES) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_call_start: empty batch or out_stride < 96");
    HIPCHK(hipSetDevice(ctx->device));
    launch_m17_call(0, calls, nullptr, nullptr, batch, 1, out, out_stride, QRL_M17_CALL_START_BYTES, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

int qrl_m17_call_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls, const uint8_t* payloads, const uint32_t* first, size_t batch, size_t n,
                        uint8_t* out, size_t out_stride, size_t slot_bytes)
{
    if (!ctx || !calls || !payloads || !out) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_call_encode: null argument");
    if (!batch || !n || slot_bytes < 48 || n > SIZE_MAX / slot_bytes || out_stride < n * slot_bytes)
        return qrl_set_error(QRL_ERR_ARG, "qrl_m17_call_encode: empty batch, slot_bytes < 48 or out_stride < n * slot_bytes");
    HIPCHK(hipSetDevice(ctx->device));
    launch_m17_call(1, calls, payloads, first, batch, n, out, out_stride, slot_bytes, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

int qrl_m17_call_end(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls, const uint32_t* first, size_t batch, uint8_t* out, size_t out_stride)
{
    if (!ctx || !calls || !first || !out) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_call_end: null argument");
    if (!batch || out_stride < QRL_M17_CALL_END_BYTES) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_call_end: empty batch or out_stride < 64");
    HIPCHK(hipSetDevice(ctx->device));
    launch_m17_call(2, calls, nullptr, first, batch, 1, out, out_stride, QRL_M17_CALL_END_BYTES, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

}
