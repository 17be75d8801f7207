// dmr_rx.cpp — C ABI of the DMR receive call layer (kernels_dmr_rx.hip, dmr_rx_core.hpp): a handle that keeps, per stream, the protocol state
// of the reference's DMRControl on the receive side (src/DMR/dmrcontrol.cpp:225-665) and the embedded-LC assembly of CDMREmbeddedData
// (src/MMDVM/DMREmbeddedData.cpp) between calls.  qrl_dmr_rx_process runs behind qrl_dmr_l2_decode on the caller's stream.
#include "host_common.hpp"
#include <cstdint>

using namespace qrl;

struct qrl_dmr_rx {
    qrl_ctx* ctx = nullptr;
    size_t batch = 0;
    int color_code = 0, promiscuous = 0;
    int mode = QRL_DMR_MODE_DMO, timeslot = 1;   // Settings::dmr_mode, dmr_timeslot; a fresh handle is in DMO mode
    DevBuf<uint8_t> states;             // DMR_RX_STATE_BYTES per stream (dmr_rx_core.hpp's dmr_rx_state); all zero bytes = a fresh DMRControl
};

static_assert(QRL_DMR_RX_RECORD_BYTES == DMR_RX_RECORD_BYTES && QRL_DMR_RX_STATE_BYTES == DMR_RX_PUBLIC_BYTES, "qrl_hip.h and engine.hpp agree");

static bool config_ok(const qrl_dmr_rx_config* c)
{
    return c && c->color_code >= 0 && c->color_code <= 15 && (c->promiscuous == 0 || c->promiscuous == 1);
}

extern "C" {

int qrl_dmr_rx_create(qrl_ctx* ctx, size_t batch, const qrl_dmr_rx_config* config, qrl_dmr_rx** out)
{
    if (out) *out = nullptr;
    if (!ctx || !out || !batch) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_create: null argument or empty batch");
    if (!config_ok(config)) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_create: colour code outside 0..15 or promiscuous flag outside 0..1");
    HIPCHK(hipSetDevice(ctx->device));
    qrl_dmr_rx* h = new qrl_dmr_rx;
    h->ctx = ctx; h->batch = batch;
    h->color_code = config->color_code; h->promiscuous = config->promiscuous;
    if (int r = h->states.alloc(batch * DMR_RX_STATE_BYTES)) { delete h; return r; }
    *out = h;
    return QRL_OK;
}

void qrl_dmr_rx_destroy(qrl_dmr_rx* h)
{
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    delete h;
}

int qrl_dmr_rx_reset(qrl_dmr_rx* h, void* hip_stream)
{
    if (!h) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_reset: null handle");
    HIPCHK(hipSetDevice(h->ctx->device));
    HIPCHK(hipMemsetAsync(h->states.p, 0, h->states.bytes(), static_cast<hipStream_t>(hip_stream)));
    return QRL_OK;
}

int qrl_dmr_rx_set_config(qrl_dmr_rx* h, const qrl_dmr_rx_config* config)
{
    if (!h) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_set_config: null handle");
    if (!config_ok(config)) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_set_config: colour code outside 0..15 or promiscuous flag outside 0..1");
    h->color_code = config->color_code; h->promiscuous = config->promiscuous;
    return QRL_OK;
}

int qrl_dmr_rx_set_mode(qrl_dmr_rx* h, int mode, int timeslot)
{
    if (!h) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_set_mode: null handle");
    if (mode != QRL_DMR_MODE_REPEATER && mode != QRL_DMR_MODE_DMO) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_set_mode: mode outside 0..1");
    if (mode == QRL_DMR_MODE_REPEATER && (timeslot < 1 || timeslot > 2)) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_set_mode: timeslot outside 1..2");
    h->mode = mode;
    if (mode == QRL_DMR_MODE_REPEATER) h->timeslot = timeslot;
    return QRL_OK;
}

// without slot records every burst reads as cachDecoded() == false, slot 0
int qrl_dmr_rx_process(qrl_dmr_rx* h, void* hip_stream, const uint8_t* l2_records, const uint32_t* counts, size_t cap_frames, uint8_t* out)
{
    if (!h || !l2_records || !out || !cap_frames) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_process: null argument or cap_frames 0");
    if (reinterpret_cast<uintptr_t>(out) & 15u) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_process: out is not 16-byte aligned");
    HIPCHK(hipSetDevice(h->ctx->device));
    launch_dmr_rx(l2_records, counts, h->batch, cap_frames, h->color_code, h->promiscuous, h->states.p, out, static_cast<hipStream_t>(hip_stream),
                  nullptr, h->mode == QRL_DMR_MODE_REPEATER, h->timeslot);
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

int qrl_dmr_rx_process_slots(qrl_dmr_rx* h, void* hip_stream, const uint8_t* l2_records, const uint8_t* slot_info, const uint32_t* counts, size_t batch,
                             size_t cap_frames, uint8_t* out)
{
    if (!h || !l2_records || !slot_info || !out || !cap_frames) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_process_slots: null argument or cap_frames 0");
    if (batch != h->batch) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_process_slots: batch is not the handle's");
    if (reinterpret_cast<uintptr_t>(out) & 15u) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_process_slots: out is not 16-byte aligned");
    HIPCHK(hipSetDevice(h->ctx->device));
    launch_dmr_rx(l2_records, counts, h->batch, cap_frames, h->color_code, h->promiscuous, h->states.p, out, static_cast<hipStream_t>(hip_stream),
                  slot_info, h->mode == QRL_DMR_MODE_REPEATER, h->timeslot);
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

int qrl_dmr_rx_get_state(qrl_dmr_rx* h, void* hip_stream, uint8_t* out)
{
    if (!h || !out) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_get_state: null argument");
    if (reinterpret_cast<uintptr_t>(out) & 3u) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_rx_get_state: out is not 4-byte aligned");
    HIPCHK(hipSetDevice(h->ctx->device));
    launch_dmr_rx_state(h->states.p, h->batch, out, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

}
