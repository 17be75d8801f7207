// framefec.cpp — C ABI of the frame FEC kernels (kernels_framefec.hip): stateless batch calls on a caller-chosen HIP stream.
//   qrl_bptc19696_decode / _encode   CBPTC19696::decode / encode    reference src/MMDVM/BPTC19696.cpp:47-87
//   qrl_m17_decode_frames            M17FrameDecoder::decodeFrame   reference src/M17/M17/M17FrameDecoder.cpp:44-215
//   qrl_dmr_l2_decode                DMRFrame::DMRFrame / validate / runAudioFEC, CDMREMB::putData   reference src/DMR/dmrframe.cpp:36-253,
//                                    src/DMR/dmrcontrol.cpp:233-248 (kernels_dmr_l2.hip)
//   qrl_dmr_trellis34_decode / _encode   CDMRTrellis::decode / encode   reference src/MMDVM/DMRTrellis.cpp:50-107
//   qrl_dmr_l2_encode / qrl_dmr_voice_call_encode   DMRFrame::constructLCFrame / constructCSBKFrame / setVoice / setEmbeddedData, DMRControl::getTxAudio
//                                    reference src/DMR/dmrframe.cpp:399-501, src/DMR/dmrcontrol.cpp:128-223 (kernels_dmr_tx.hip)
#include "host_common.hpp"
#include <cstdint>
#include <string>

using namespace qrl;

extern "C" {

int qrl_bptc19696_decode(qrl_ctx* ctx, void* hip_stream, const uint8_t* bursts, size_t n, uint8_t* payloads)
{
    if (!ctx || (n && (!bursts || !payloads))) return qrl_set_error(QRL_ERR_ARG, "qrl_bptc19696_decode: null argument");
    HIPCHK(hipSetDevice(ctx->device));
    launch_bptc_decode(bursts, n, payloads, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}
int qrl_bptc19696_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* payloads, size_t n, uint8_t* bursts)
{
    if (!ctx || (n && (!bursts || !payloads))) return qrl_set_error(QRL_ERR_ARG, "qrl_bptc19696_encode: null argument");
    HIPCHK(hipSetDevice(ctx->device));
    launch_bptc_encode(payloads, n, bursts, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}
int qrl_m17_encode_frames(qrl_ctx* ctx, void* hip_stream, const uint8_t* records, size_t n, uint8_t* frames)
{
    if (!ctx || (n && (!frames || !records))) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_encode_frames: null argument");
    HIPCHK(hipSetDevice(ctx->device));
    launch_m17_encode(records, n, frames, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}
int qrl_m17_decode_frames(qrl_ctx* ctx, void* hip_stream, const uint8_t* frames, size_t n, uint8_t* records)
{
    if (!ctx || (n && (!frames || !records))) return qrl_set_error(QRL_ERR_ARG, "qrl_m17_decode_frames: null argument");
    HIPCHK(hipSetDevice(ctx->device));
    launch_m17_decode(frames, n, records, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}
int qrl_dmr_l2_decode(qrl_ctx* ctx, void* hip_stream, const uint8_t* records, const uint32_t* counts, size_t batch, size_t cap_frames,
                      int audio_fec, uint8_t* out)
{
    if (!ctx || !records || !out || !batch || !cap_frames) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_l2_decode: null argument or empty mailbox");
    HIPCHK(hipSetDevice(ctx->device));
    launch_dmr_l2(records, counts, batch, cap_frames, audio_fec, out, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}
int qrl_dmr_trellis34_decode(qrl_ctx* ctx, void* hip_stream, const uint8_t* bursts, size_t n, uint8_t* payloads, uint8_t* ok)
{
    if (!ctx || !bursts || !payloads || !ok) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_trellis34_decode: null argument");
    HIPCHK(hipSetDevice(ctx->device));
    launch_trellis34_decode(bursts, n, payloads, ok, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}
int qrl_dmr_trellis34_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* payloads, size_t n, uint8_t* bursts)
{
    if (!ctx || !payloads || !bursts) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_trellis34_encode: null argument");
    HIPCHK(hipSetDevice(ctx->device));
    launch_trellis34_encode(payloads, n, bursts, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}
// what both encoders ask of their output geometry: slots of at least a burst, rows that hold their slots
static bool dmr_tx_geometry_ok(size_t batch, size_t slots, size_t out_stride, size_t slot_bytes)
{
    return batch && slots && slot_bytes >= 33 && slots <= SIZE_MAX / slot_bytes && out_stride >= slots * slot_bytes;
}
int qrl_dmr_l2_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* records, const uint32_t* counts, size_t batch, size_t cap_frames,
                      uint8_t* out, size_t out_stride, size_t slot_bytes)
{
    if (!ctx || !records || !out) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_l2_encode: null argument");
    if (!dmr_tx_geometry_ok(batch, cap_frames, out_stride, slot_bytes))
        return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_l2_encode: empty batch, slot_bytes < 33 or out_stride < cap_frames * slot_bytes");
    HIPCHK(hipSetDevice(ctx->device));
    launch_dmr_tx(records, counts, batch, cap_frames, out, out_stride, slot_bytes, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}
int qrl_dmr_voice_call_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls, const uint8_t* voice, const uint32_t* first, size_t batch,
                              size_t n, uint8_t* out, size_t out_stride, size_t slot_bytes)
{
    if (!ctx || !calls || !voice || !out) return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_voice_call_encode: null argument");
    if (!dmr_tx_geometry_ok(batch, n, out_stride, slot_bytes))
        return qrl_set_error(QRL_ERR_ARG, "qrl_dmr_voice_call_encode: empty batch, slot_bytes < 33 or out_stride < n * slot_bytes");
    HIPCHK(hipSetDevice(ctx->device));
    launch_dmr_tx_call(calls, voice, first, batch, n, out, out_stride, slot_bytes, static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return QRL_OK;
}

}
