// dmr_sink.cpp — C ABI of the repeater-mode DMR burst sink (kernels_dmr_sink.hip, dmr_sink_core.hpp): a handle that keeps, per stream, the two
// slot contexts of the reference's gr_dmr_sink (src/gr/gr_dmr_sink.cpp:29-49) between calls.  Shaped like qrl_deframer_*: it consumes the
// unpacked bits of a demodulator port with a per-stream count, asynchronously on the handle's stream.
#include "host_common.hpp"
#include <cstdint>
#include <memory>
#include <new>

using namespace qrl;

struct qrl_dmr_sink {
    qrl_ctx* ctx = nullptr;
    int batch = 1;
    HandleStream stream;
    DevBuf<uint8_t> states;   // DMR_SINK_STATE_BYTES per stream (dmr_sink_core.hpp's dmr_sink_state); all zero bytes = a fresh gr_dmr_sink
};

extern "C" {

int qrl_dmr_sink_create(qrl_ctx* ctx, int batch, void* hip_stream, qrl_dmr_sink** out)
{
    if (out) *out = nullptr;
    if (!ctx || !out) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_sink_create: null argument");
    if (batch < 1) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_sink_create: batch must be >= 1");
    std::unique_ptr<qrl_dmr_sink> h(new (std::nothrow) qrl_dmr_sink);
    if (!h) return QRL_ERR_NOMEM;
    h->ctx = ctx; h->batch = batch;
    HIPCHK(hipSetDevice(ctx->device));
    if (int r0 = h->stream.open(hip_stream)) return r0;
    if (int r = h->states.alloc((size_t)batch * DMR_SINK_STATE_BYTES)) return r;
    *out = h.release();
    return QRL_OK;
}

void qrl_dmr_sink_destroy(qrl_dmr_sink* h)
{
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

int qrl_dmr_sink_reset(qrl_dmr_sink* h)
{
    if (!h) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_sink_reset: null handle");
    HIPCHK(hipSetDevice(h->ctx->device));
    HIPCHK(hipMemsetAsync(h->states.p, 0, (size_t)h->batch * DMR_SINK_STATE_BYTES, h->stream));
    return QRL_OK;
}

int qrl_dmr_sink_flush(qrl_dmr_sink* h)
{
    if (!h) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_sink_flush: null handle");
    HIPCHK(hipSetDevice(h->ctx->device));
    launch_dmr_sink_flush(h->states.p, h->batch, h->stream);
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

int qrl_dmr_sink_process(qrl_dmr_sink* h, const uint8_t* bits, size_t stride, size_t n, const uint32_t* counts, size_t count_stride,
                         uint8_t* frames, uint8_t* slot_info, size_t cap_frames, uint32_t* out_counts)
{
    if (!h || !bits || !frames || !slot_info || !out_counts || !cap_frames)
        return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_sink_process: null argument or cap_frames 0");
    if (n > stride) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_sink_process: n is larger than the stride between streams");
    if ((reinterpret_cast<uintptr_t>(frames) & 7u) || (reinterpret_cast<uintptr_t>(slot_info) & 15u))
        return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_sink_process: frames is not 8-byte aligned or slot_info not 16-byte aligned");
    // the kernel counts bits and tiles of 128 bits in 32 bits: n + 127 must not wrap
    if (n > 0xFFFFFFFFull - 128u || cap_frames > 0xFFFFFFFFull) return qrl_set_error(QRL_ERR_TOO_BIG, "qrl_dmr_sink_process: n or cap_frames too large");
    HIPCHK(hipSetDevice(h->ctx->device));
    DmrSinkParams p{};
    p.bits = bits; p.stride = stride; p.n = (uint32_t)n; p.counts = counts; p.count_stride = count_stride;
    p.st = h->states.p; p.frames = frames; p.info = slot_info; p.cap = (uint32_t)cap_frames; p.out_counts = out_counts;
    launch_dmr_sink(p, h->batch, h->stream);
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

int qrl_dmr_sink_sync(qrl_dmr_sink* h)
{
    if (!h) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_sink_sync: null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    return QRL_OK;
}

}
