/*
 * qrl_hip.h — C ABI of libqrl_hip.so, the MI355X-native drop-in for QRadioLink's gr_modem
 * RX DSP hot path (the per-mode demod flowgraphs under src/gr/ of the reference).
 *
 * Nothing like this exists in the reference: there the path is a GNU Radio flowgraph
 * (gr::top_block "demodulator", src/gr/gr_demod_base.cpp:32) whose blocks run on CPU threads.
 * Each entry point below names the reference interface it replaces; INTEGRATION.md shows the
 * C++ stub a maintainer would add inside gr_demod_base / a gr::sync_block to bind it.
 *
 * Rules: plain C types; no exceptions cross the ABI; every function returns QRL_OK (0) or a
 * negative qrl_status; the caller owns every buffer it passes, the library owns device state.
 * One handle is single-threaded (like one GNU Radio block: work() calls never overlap,
 * SURVEY.md 8b); different handles may be driven concurrently on different HIP streams.
 *
 * Data layout: "cf32" = interleaved complex<float> (gr_complex, 8 bytes). A demodulator
 * handle processes `batch` independent streams per call: iq[b*stride + i], i < n.
 * All data pointers are DEVICE pointers unless the function name ends in _host.
 */
#ifndef QRL_HIP_H
#define QRL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    QRL_OK = 0,
    QRL_ERR_ARG = -1,        /* invalid argument / unsupported mode */
    QRL_ERR_NO_DEVICE = -2,  /* no HIP device / wrong architecture */
    QRL_ERR_HIP = -3,        /* a HIP runtime call failed (see qrl_last_error) */
    QRL_ERR_NOMEM = -4,
    QRL_ERR_TOO_BIG = -5,    /* n exceeds max_chunk given at creation */
    QRL_ERR_STATE = -6
} qrl_status;

/* values of gr_modem_types (reference src/modem_types.h:5-50) accepted by qrl_demod_create */
enum {
    QRL_MODEM_BPSK2K = 0, QRL_MODEM_QPSK20K = 1, QRL_MODEM_QPSKVIDEO = 2, QRL_MODEM_4FSK2K = 3, QRL_MODEM_4FSK10KFM = 4, QRL_MODEM_4FSK2KFM = 5, QRL_MODEM_4FSK1KFM = 6, QRL_MODEM_QPSK2K = 7,
    QRL_MODEM_NBFM2500 = 8, QRL_MODEM_NBFM5000 = 9, QRL_MODEM_WBFM = 10, QRL_MODEM_USB2500 = 11, QRL_MODEM_LSB2500 = 12, QRL_MODEM_CW600USB = 13 /* TX only: qrl_amod */, QRL_MODEM_AM5000 = 14,   /* analogue voice receivers: port 1 = audio */
    QRL_MODEM_2FSK2KFM = 15, QRL_MODEM_2FSK1KFM = 16, QRL_MODEM_2FSK2K = 17, QRL_MODEM_2FSK1K = 18,
    QRL_MODEM_2FSK10KFM = 19, QRL_MODEM_GMSK2K = 20, QRL_MODEM_GMSK1K = 21, QRL_MODEM_GMSK10K = 22,
    QRL_MODEM_BPSK1K = 24, QRL_MODEM_BPSK8 = 25 /* DSSS, Barker 13 */, QRL_MODEM_QPSK250K = 26, QRL_MODEM_4FSK100K = 27, QRL_MODEM_M17 = 40, QRL_MODEM_DMR = 41
};

typedef struct qrl_ctx qrl_ctx;
typedef struct qrl_demod qrl_demod;

/* replaces: process-level GNU Radio/VOLK initialisation (gr::make_top_block, gr_demod_base.cpp:32).
 * Fails with QRL_ERR_NO_DEVICE when no gfx950-class HIP device is usable: there is no CPU fallback. */
int qrl_init(int device, qrl_ctx** ctx);
void qrl_shutdown(qrl_ctx* ctx);
const char* qrl_strerror(int status);
const char* qrl_last_error(void);
/* compile-time identification of the library (no GPU needed) */
const char* qrl_version(void);

/*
 * Configuration of one RX chain = the constructor arguments the reference passes.
 * replaces: make_gr_demod_2fsk(sps,samp_rate,carrier_freq,filter_width,fm) gr_demod_2fsk.cpp:19-37,
 *           make_gr_demod_gmsk(...) gr_demod_gmsk.cpp:19-37, make_gr_demod_qpsk(...) gr_demod_qpsk.cpp:20-37,
 *           make_gr_demod_4fsk(..., fm) gr_demod_4fsk.cpp:19-36, make_gr_demod_bpsk(...) gr_demod_bpsk.cpp:19-35,
 *           make_gr_demod_dmr(sps, samp_rate) gr_demod_dmr.cpp:19-35
 *           with the literals of gr_demod_base.cpp:203-253 when use_mode_defaults != 0;
 *           gr_demod_base::set_samp_rate (gr_demod_base.cpp:1303-1362) via device_samp_rate;
 *           gr_demod_base::set_carrier_offset (gr_demod_base.cpp:1220-1225) via carrier_offset_hz.
 */
typedef struct {
    int modem_type;          /* gr_modem_types value */
    int use_mode_defaults;   /* 1: take sps/filter_width/fm from the reference's table for modem_type */
    int sps, samp_rate, carrier_freq, filter_width, fm; /* make_gr_demod_X args (samp_rate = 1000000) */
    int device_samp_rate;    /* SDR rate; >= 2e6 inserts rotator + 1:fs/1e6 decimator, else rotator only */
    double carrier_offset_hz;
    int batch;               /* independent streams per call (>= 1) */
    size_t max_chunk;        /* largest n (samples per stream) of any process call */
    void* hip_stream;        /* hipStream_t to run on, NULL = the library creates one */
    int enable_side_outputs; /* 1: also produce port 0 (filtered) and port 1 (constellation) */
    /* the time-domain scope tap's resampler (qrl_demod_set_time_domain_output), 0 = the constructor's 1:10 with low_pass(1, 1e6, 50000, 25000, HAMMING):
     * time_domain_samp_rate replaces gr_demod_base::set_time_sink_samp_rate(samp_rate) (src/gr/gr_demod_base.cpp:1249-1290): decimation 1e6 / samp_rate
     * (integer), taps low_pass(1, 1e6, samp_rate / 2 - samp_rate / 8, samp_rate / 4, HAMMING) (integer divisions as in the reference);
     * time_domain_filter_width > 0 replaces gr_demod_base::set_time_domain_filter_width(width) (:1292-1301) called after it: taps low_pass(1, 1e6, width, width,
     * HAMMING), same decimation.  Create-time values: the history a handle keeps depends on the filter (the host facade re-opens its handle, the reference
     * re-creates the block under lock()). */
    int time_domain_samp_rate;
    double time_domain_filter_width;
} qrl_demod_config;

/* per-call outputs, all caller-allocated DEVICE buffers laid out [batch][cap];
 * counts[b*4 + k] = items written for stream b on port k (0 filtered, 1 constellation, 2 bits A, 3 bits B).
 * A NULL data pointer skips that port (its count is still reported). */
typedef struct {
    float* filtered;      size_t filtered_cap;      /* cf32, port 0: gr_demod_2fsk.cpp:133 */
    float* constellation; size_t constellation_cap; /* cf32, port 1: gr_demod_2fsk.cpp:153-154 */
    uint8_t* bits_a;      size_t bits_cap;          /* u8 one bit per byte, port 2 */
    uint8_t* bits_b;                                /* port 3 (two-branch modes), same cap */
    uint32_t* counts;                               /* [batch][4] */
    float* audio;         size_t audio_cap;         /* analogue modes: port 1 = f32 audio at 8 ksps (counts[b][1] = samples of the call);
                                                       written whether or not side outputs are enabled */
} qrl_demod_out;

int qrl_demod_create(qrl_ctx* ctx, const qrl_demod_config* cfg, qrl_demod** out);
void qrl_demod_destroy(qrl_demod* d);
/* replaces: top_block lock/flush on set_mode (gr_demod_base.cpp:302-311): zero all DSP state */
int qrl_demod_reset(qrl_demod* d);
/* replaces: rotator_cc::set_phase_inc (gr_demod_base.cpp:1220-1225); phase-continuous retune */
int qrl_demod_set_carrier_offset(qrl_demod* d, double carrier_offset_hz);
/* per-stream rotator_cc::set_phase_inc (gr_demod_base::set_carrier_offset of each radio): hz[b] is stream b's carrier offset, a host array of
 * `batch` doubles.  Each stream's phase runs on and its increment changes from the next sample, as with the scalar setter; samples already in a
 * decimator's history keep their old rotation.  Once a handle has per-stream offsets, qrl_demod_set_carrier_offset sets every stream to one
 * offset and each stream goes on from its own phase; qrl_demod_reset restarts every phase and keeps the offsets.  hz == NULL or a non-finite
 * value: QRL_ERR_ARG, nothing changes.  Blocks the host like the scalar setter; only the streams whose offset changes get a new table. */
int qrl_demod_set_carrier_offsets(qrl_demod* d, const double* hz);
/* capacities (items per stream) a call with n input samples can need */
/* a37b, QRL_MODEM_DMR only: gr_dmr_dmo_sink (reference src/gr/gr_dmr_dmo_sink.cpp:63-357) on the device, fed from port 3 of
 * gr_demod_dmr (RRC-filtered discriminator output, gr_demod_dmr.cpp:94).  Every following qrl_demod_process call also runs the
 * MS-sync correlator / 4-level slicer / slot-type state machine over the call's new samples and appends the DMR bursts it cuts to
 * frames[b * cap_frames * 40 + i * 40]: 40-byte records {frame type (DMRFrameType 0 data, 1 voice, 2 voice sync), FN, colour code,
 * 0, 33 frame bytes, 3 pad}; counts[b] = bursts found by the call (device pointers; replaces gr_dmr_dmo_sink::get_data); only the first
 * cap_frames records are written, so counts[b] > cap_frames means bursts were dropped (one burst lasts 30 ms: size cap_frames for the chunk).
 * frames == NULL switches it off.  The stream position must be the start of the stream (call it before the first process / after
 * a reset) or the slicer starts with an empty 1440-sample history. */
#define QRL_DMO_RECORD_BYTES 40
int qrl_demod_set_dmo_output(qrl_demod* d, uint8_t* frames, size_t cap_frames, uint32_t* counts);
/* Per-handle run-time options (none of them changes results; tests/test_gpu_parity.py checks each value of each option against the oracle).  QRL_OPT_OVERLAP (2FSK family only, default 1 since round 3): value 1 runs
 * everything behind the first decimated ring of call k on a second stream under the front end of call k + 1; value 0 runs the
 * kernels of a call one after another.  QRL_OPT_UNFUSED_DEC2 (QPSK chains with sps <= 4, default 0): value 1 runs the 1:2 resampler
 * and the shaping filter (gr_demod_qpsk.cpp:92-103) as the two kernels of rounds 1-2 instead of the fused one (A/B and parity checks);
 * only before the first sample of a stream.  QRL_OPT_GROUPED (gr_demod_qpsk chain; default: 1 when the batch gives the recursion kernel a
 * workgroup for at least every second CU, else 0): the order in which a call's three kernels are put on the device -- value 1: front
 * end of call k + 1 behind the recursion of call k, the decoder of call k - 1 launched with the recursion of call k (flushed by every
 * function that waits for results); value 0: three free-running streams.  QRL_OPT_INPUT_RESIDENT (default 0; a handle that owns its
 * streams): value 1 is the caller's promise that the IQ of every call is COMPLETE in device memory when qrl_demod_process is called -- not
 * the product of work the caller has queued on qrl_demod_stream() and not yet waited for.  The two helper kernels of the front end
 * (the history kept for the next call, the edge scratch of this one) then read it on a fourth internal stream beside the front end of the
 * call before instead of in line with it; qrl_demod_sync / qrl_demod_stream_wait cover that stream too.  With value 0 everything that reads
 * the caller's buffer is ordered behind the handle's stream, as qrl_demod_process documents.  QRL_OPT_SC16_BASEBAND (default 0): value 1
 * lets a handle WITHOUT a device-rate front end (device_samp_rate 1000000) take int16 IQ through qrl_demod_process_sc16 /
 * qrl_demod_process_sc16_host; value 0 refuses such calls with QRL_ERR_ARG, as before the option existed.  It allocates nothing and may be
 * set at any stream position (the format belongs to the call, the carried history is rotated cf32); on a handle with a front end it is
 * accepted and does nothing.  QRL_OPT_IQ8_BASEBAND (default 0): the same for 8-bit IQ -- value 1 lets a handle without a device-rate front
 * end take qrl_demod_process_sc8 / _cu8 and their _host forms (16-byte aligned base, pitch a multiple of 8 samples, as everywhere); value 0
 * refuses them with QRL_ERR_ARG.  The two options are independent: QRL_OPT_SC16_BASEBAND alone keeps refusing 8-bit input, this one alone
 * does not admit int16.  Nothing is allocated, any stream position, no effect on a handle with a front end. */
enum { QRL_OPT_OVERLAP = 1, QRL_OPT_UNFUSED_DEC2 = 2, QRL_OPT_FLL_SLIM = 3 /* tuning: single-wave FLL workgroups; for 2FSK-1k / -2k also the FLL and the FIR stages as the two kernels k_fll + k_2fsk_ff instead of k_2fsk_tail (same results) */, QRL_OPT_GROUPED = 4, QRL_OPT_INPUT_RESIDENT = 5, QRL_OPT_SC16_BASEBAND = 6, QRL_OPT_IQ8_BASEBAND = 7 };
int qrl_demod_set_option(qrl_demod* d, int option, int value);
int qrl_demod_out_caps(const qrl_demod* d, size_t n, size_t* filtered_cap, size_t* constellation_cap, size_t* bits_cap);
/* analogue voice receivers (QRL_MODEM_NBFM2500 / NBFM5000 / AM5000 / WBFM / USB2500 / LSB2500; replace make_gr_demod_nbfm / _am /
 * _wbfm / _ssb, reference src/gr/gr_demod_nbfm.cpp:19-88, gr_demod_am.cpp:19-79, gr_demod_wbfm.cpp:19-72, gr_demod_ssb.cpp:19-81
 * (with src/gr/cessb/clipper_cc_impl.cc, stretcher_cc_impl.cc), instances gr_demod_base.cpp:215,219,220,226-228):
 * port 0 = the channel-filtered IQ, port 1 = audio.  The squelch gates (pwr_squelch_cc(-140, 0.01, ramp, true)), so the number of
 * audio samples a call returns depends on the signal; audio_cap(n) is the bound for a call of n input samples (0 for other modes). */
int qrl_demod_audio_cap(const qrl_demod* d, size_t n, size_t* audio_cap);
/* replaces gr_demod_nbfm/am/wbfm::set_squelch (pwr_squelch_cc::set_threshold, gr_demod_base.cpp:1186-1199): threshold in dB */
int qrl_demod_set_squelch(qrl_demod* d, double db);
/* replaces the time-domain scope tap of gr_demod_base: enable_time_domain (src/gr/gr_demod_base.cpp:1115-1147) connects _demod_valve ->
 * rational_resampler_ccf(1, 10, low_pass(1, 1e6, 50000, 25000, HAMMING)) (:62-63) -> gr_sample_sink (src/gr/gr_sample_sink.cpp), read
 * through get_sample_data (:988-1013).  samples != NULL switches the tap on: every following qrl_demod_process also decimates the
 * 1 Msps signal behind the front end (the caller's rotated IQ when the device runs at 1 Msps) 1:10 and writes the call's new
 * 100 ksps items to samples[b*cap + k] (cf32 pairs, device memory), counts[b] = items written; NULL switches it off.
 * qrl_demod_time_domain_cap: the bound for a call of n input samples.  The sink's mailbox rules (window, drop threshold) are host
 * logic: qrl_host::gr_demod_base_hip::get_sample_data. */
int qrl_demod_time_domain_cap(const qrl_demod* d, size_t n, size_t* cap);
int qrl_demod_set_time_domain_output(qrl_demod* d, float* samples, size_t cap, uint32_t* counts);
/* replaces gr_demod_nbfm::set_ctcss(value) (src/gr/gr_demod_nbfm.cpp:97-123): tone_hz != 0 switches analog::ctcss_squelch_ff(8000, tone,
 * 0.01, 8000, 160, true) (:59-60) in between the audio resampler and the audio filter and the audio filter to band_pass_2(1, 8000,
 * 300, 3500, 200, 35, BH); 0 switches it out again (the constructor's graph).  Switching it in or out restarts the chain from a
 * fresh state (the reference re-wires the graph under lock()); a different tone while it is on re-initialises the tone detector
 * only (ctcss_squelch_ff::set_frequency).  NBFM receivers only.  The block gates: audio leaves only while the tone is present. */
int qrl_demod_set_ctcss(qrl_demod* d, float tone_hz);
/* replaces gr_demod_am / gr_demod_ssb::set_agc_attack / set_agc_decay (gr_demod_am.cpp:90-98, gr_demod_ssb.cpp:104-112) */
int qrl_demod_set_agc(qrl_demod* d, float attack, float decay);
/* replaces gr_demod_base::set_filter_width(filter_width, mode) (src/gr/gr_demod_base.cpp:1155-1185), which forwards to the analogue receiver of
 * `mode`: gr_demod_nbfm::set_filter_width (gr_demod_nbfm.cpp:82-90), gr_demod_am (gr_demod_am.cpp:84-91), gr_demod_wbfm (gr_demod_wbfm.cpp:76-84),
 * gr_demod_ssb (gr_demod_ssb.cpp:89-101).  The setters do NOT repeat the constructors' designs: NBFM / WBFM low_pass(1, fs, w, 1200, BH) and the
 * discriminator gain fs / (4 pi w) resp. fs / (2 pi w); AM complex_band_pass(1, fs, -w, w, 1200, BH); SSB the constructor's band-pass with w and the
 * audio filter band_pass_2(2, 8000, 200, w, 200, 90, BH) -- gain 2.  The reference swaps the taps of a running graph at a sample its scheduler decides;
 * here the chain restarts from a fresh state (like qrl_demod_reset; squelch / CTCSS / AGC settings are kept).  Analogue receivers only. */
int qrl_demod_set_filter_width(qrl_demod* d, int filter_width);
/* replaces gr_demod_base::set_gain(value) (src/gr/gr_demod_base.cpp:1206-1210) -> gr_demod_ssb::set_gain = _if_gain->set_k(value) (gr_demod_ssb.cpp:118-121;
 * constructor: 0.9).  Takes effect with the next qrl_demod_process call.  SSB receivers only. */
int qrl_demod_set_gain(qrl_demod* d, float value);

/* replaces: one scheduler pass of the "demodulator" top_block over n new samples per stream:
 * (the serial tail of a call runs on an internal second HIP stream and overlaps the next call; only
 * qrl_demod_sync() -- not a sync of the handle's own stream -- guarantees the outputs are complete)
 * gr::sync_block::work()/general_work() of every block on the chain (SURVEY.md 8b block ABI).
 * iq: device pointer, stream b at iq + 2*b*stride floats, n <= max_chunk samples each, base and
 * stride*8 bytes 16-byte aligned.  Asynchronous on the handle's stream; results are valid after
 * qrl_demod_sync().  Results are independent of how the stream is cut into calls.
 * Calls in flight together need DISTINCT output buffers: for the QPSK / BPSK / 4FSK-discriminator families the recursion and the
 * Viterbi decoder of a call run on internal streams up to two calls behind the front end, so a caller that reuses one qrl_demod_out
 * for back-to-back calls must put qrl_demod_sync() or qrl_demod_stream_wait() between them (or alternate two buffer sets). */
int qrl_demod_process(qrl_demod* d, const float* iq, size_t stride, size_t n, const qrl_demod_out* out);
/* like qrl_demod_process, but iq is interleaved int16 I, Q (sc16, 4 bytes per sample: what UHD / SoapySDR / LimeSuite / HackRF put on the
 * wire): stream b at iq + 2*b*stride int16s.  Replaces the driver's own sc16 -> fc32 conversion: the front end reads the raw pairs (half
 * the HBM bytes, half the upload) and converts in registers, x = (float)v * scale per component (one exact int -> float conversion, one
 * rounded f32 multiply, in front of the rotator) -- bit for bit what qrl_demod_process computes when fed (float)v * scale.
 * scale: qrl_demod_set_sc16_scale, default 1.0f / 32768; the setter takes effect from the next call and refuses a non-finite or zero
 * value with QRL_ERR_ARG.  The format belongs to the CALL, not the handle: the carried state is cf32, so cf32 and sc16 calls may
 * alternate on one handle and give the result of the concatenated stream; options, per-stream carrier offsets, profiling (the same
 * kernel names) and the scope tap work as with cf32.
 * iq must be 16-byte aligned and stride a multiple of 4 samples, else QRL_ERR_ARG; any n <= max_chunk (the LDS-DMA kernel streams calls
 * with n % 4 == 0, other n take the per-output kernels).
 * Handles with device_samp_rate >= 2000000 (every modem type, every rate qrl_demod_create accepts) take it as they are: there the
 * device-rate front end and the history keeper are all that read the caller's buffer.  A 1 Msps handle takes it once
 * qrl_demod_set_option(d, QRL_OPT_SC16_BASEBAND, 1) has been called: the per-mode first stage then reads the raw pairs -- the decimators
 * (the 1:50 matrix-pipe stage streams them with LDS-DMA, 4 bytes per sample), k_resamp, k_dec2_fir, the analogue and DSSS receivers'
 * first stage and the scope tap -- with the same conversion in front of the rotator, every modem type.  Without the option (the
 * default) a 1 Msps handle returns QRL_ERR_ARG (qrl_last_error says so), changes nothing and stays usable. */
int qrl_demod_process_sc16(qrl_demod* d, const int16_t* iq, size_t stride, size_t n, const qrl_demod_out* out);
int qrl_demod_set_sc16_scale(qrl_demod* d, float scale);
/* like qrl_demod_process_sc16, but iq is interleaved 8-bit I, Q, 2 bytes per sample: stream b at iq + 2*b*stride bytes.
 *   sc8 (signed: HackRF, cs8):      x = (float)v * scale per component, scale default 1.0f / 128 (qrl_demod_set_sc8_scale);
 *   cu8 (unsigned: RTL-SDR dongles): x = ((float)u - bias) * scale, defaults bias 127.5f, scale 1.0f / 128 (qrl_demod_set_cu8_scale; the bias is
 *   a parameter because drivers differ).
 * One exact conversion, one f32 subtract (cu8), one rounded f32 multiply, in that order and in front of the rotator: the result of a call is
 * bit for bit what qrl_demod_process gives for those floats.  The front end reads the raw pairs -- a quarter of the cf32 bytes in HBM and on
 * the upload -- and converts in registers.  The carried state stays rotated cf32: cf32, sc16, sc8 and cu8 calls may alternate on one handle and
 * give the result of the concatenated stream; options, per-stream carrier offsets, profiling (the same kernel names) and the scope tap work as
 * with cf32.  The setters refuse a zero or non-finite scale and a non-finite bias with QRL_ERR_ARG and take effect from the next call.
 * iq must be 16-byte aligned and stride a multiple of 8 samples, else QRL_ERR_ARG before anything is launched (qrl_last_error names the rule);
 * any n <= max_chunk (the LDS-DMA kernel streams calls with n % 8 == 0, other n take the per-output kernels).
 * Handles with device_samp_rate >= 2000000 take 8-bit calls as they are, every modem type and every rate qrl_demod_create accepts.  A 1 Msps
 * handle (an RTL-SDR at the internal rate) takes them once qrl_demod_set_option(d, QRL_OPT_IQ8_BASEBAND, 1) has been called: the per-mode first
 * stage then reads the raw pairs under the same rule -- the 1:50 matrix-pipe stage streams them with LDS-DMA, 2 bytes per sample (calls with
 * n % 8 == 0); k_dec2_fir, k_resamp, the other decimators, the analogue and DSSS receivers' first stage and the scope tap convert at the
 * load, exact but untuned.  Without that option (the default) a 1 Msps handle has nothing that converts and returns QRL_ERR_ARG, also under
 * QRL_OPT_SC16_BASEBAND (which admits int16 only); it changes nothing and stays usable. */
int qrl_demod_process_sc8(qrl_demod* d, const int8_t* iq, size_t stride, size_t n, const qrl_demod_out* out);
int qrl_demod_process_cu8(qrl_demod* d, const uint8_t* iq, size_t stride, size_t n, const qrl_demod_out* out);
int qrl_demod_set_sc8_scale(qrl_demod* d, float scale);
int qrl_demod_set_cu8_scale(qrl_demod* d, float scale, float bias);
int qrl_demod_sync(qrl_demod* d);
void* qrl_demod_stream(qrl_demod* d); /* hipStream_t */
/* Profiling aid: the HIP streams a call's stages are launched on -- out[0] the handle's stream (front end), out[1] the stream of the
 * decimated-rate / recursion kernels, out[2] the decoder's.  An event recorded on one of them orders nothing (unlike
 * qrl_demod_stream_wait, whose wait on the caller's stream sits in a hardware queue that stream may share with this handle's);
 * bench.py takes its per-step completion times this way.  Not a synchronisation interface: use qrl_demod_sync / _stream_wait. */
int qrl_demod_internal_streams(qrl_demod* d, void* out[3]);
/* makes the caller's stream wait (on the device, without blocking the host) for everything this handle has enqueued so far on its
 * internal streams: how a host layer chains its own asynchronous copies of the output ports behind a qrl_demod_process call
 * (host/gr_modem_hip.cpp: double-buffered mailboxes) instead of calling qrl_demod_sync. */
int qrl_demod_stream_wait(qrl_demod* d, void* hip_stream);

/* Per-kernel timing of the dominant (HBM-facing) kernel with HIP events recorded on the handle's own
 * stream (bench.py roofline leg).  enable!=0 starts recording one event pair per process call;
 * qrl_demod_profile_read syncs, returns the summed duration and launch count, and clears the record. */
int qrl_demod_profile(qrl_demod* d, int enable);
int qrl_demod_profile_read(qrl_demod* d, double* kernel_ms, uint64_t* launches, const char** kernel_name);

/* host-buffer convenience used by the C++ adaptor (gr_bit_sink-style mailboxes): copies iq H2D,
 * runs one pass, copies bits back.  bits_x_host: [batch][bits_cap]; counts_host: [batch][4]. */
int qrl_demod_process_host(qrl_demod* d, const float* iq_host, size_t stride, size_t n,
                           uint8_t* bits_a_host, uint8_t* bits_b_host, size_t bits_cap, uint32_t* counts_host);
/* the same for int16 I, Q host samples (iq_host[b*2*stride + 2*i], 4 bytes per sample staged and uploaded): qrl_demod_process_sc16 */
int qrl_demod_process_sc16_host(qrl_demod* d, const int16_t* iq_host, size_t stride, size_t n,
                                uint8_t* bits_a_host, uint8_t* bits_b_host, size_t bits_cap, uint32_t* counts_host);
/* the same for 8-bit I, Q host samples (iq_host[b*2*stride + 2*i], 2 bytes per sample staged and uploaded; the device pitch is rounded up to
 * 8 samples): qrl_demod_process_sc8 / qrl_demod_process_cu8 */
int qrl_demod_process_sc8_host(qrl_demod* d, const int8_t* iq_host, size_t stride, size_t n,
                               uint8_t* bits_a_host, uint8_t* bits_b_host, size_t bits_cap, uint32_t* counts_host);
int qrl_demod_process_cu8_host(qrl_demod* d, const uint8_t* iq_host, size_t stride, size_t n,
                               uint8_t* bits_a_host, uint8_t* bits_b_host, size_t bits_cap, uint32_t* counts_host);

/* ---- TX: the "modulator" top_block (reference src/gr/gr_mod_base.cpp:25) ----------------------------------
 * One handle = make_gr_mod_qpsk(sps, samp_rate, carrier_freq, filter_width) (src/gr/gr_mod_qpsk.cpp:19-30;
 * instance make_gr_mod_qpsk(4,1000000,1700,160000) src/gr/gr_mod_base.cpp:175) for `batch` independent streams.
 * Built: QPSK 250k / video / 20k / 2k (gr_mod_qpsk.cpp), 2FSK incl. FM variants (gr_mod_2fsk.cpp:19-99), GMSK
 * (gr_mod_gmsk.cpp:19-95), 4FSK incl. the non-FM 2k mode (gr_mod_4fsk.cpp:19-115), BPSK (gr_mod_bpsk.cpp:19-67), and
 * gr_mod_base's rotator + rate-matching interpolator (device_samp_rate / carrier_offset_hz below). */
typedef struct qrl_mod qrl_mod;
typedef struct {
    int modem_type;          /* gr_modem_types value (QRL_MODEM_QPSK250K) */
    int use_mode_defaults;   /* 1: sps/filter_width from gr_mod_base.cpp:175 */
    int sps, samp_rate, carrier_freq, filter_width, fm;   /* make_gr_mod_qpsk / make_gr_mod_2fsk / make_gr_mod_gmsk arguments */
    int batch;               /* independent streams per call */
    size_t max_bytes;        /* largest nbytes of any process call */
    void* hip_stream;        /* hipStream_t, NULL = the library creates one (RX and TX handles on different streams run
                                concurrently: full duplex, reference src/radiocontroller.cpp:2043-2078) */
    float bb_gain;           /* gr_mod_qpsk::set_bb_gain, 0 = 1.0 */
    /* gr_mod_base back end (src/gr/gr_mod_base.cpp:38,215-258): modulator (1 Msps) -> rotator_cc(2 pi offset / 1e6) ->
     * rational_resampler_ccf(fs/1e6, 1, low_pass(I, fs, 480k, 20k, BLACKMAN_HARRIS)) when fs >= 2 Msps -> SDR sink */
    /* device_samp_rate: gr_mod_base::set_samp_rate: 0 / 1e6 = no resampler, else a multiple of 1e6 in [2e6, 183e6], the receivers' range (anything
     * else: QRL_ERR_ARG).  Output counts are 32-bit: a handle whose largest call (max_bytes) would produce 2^32 or more device-rate samples per
     * stream is refused with QRL_ERR_TOO_BIG.  Finite input gives the reference's sum bit for bit at every rate.  From 4e6 up the interpolator
     * runs on the matrix pipe with its 209-tap phases padded to 210 lags by zero taps, and a zero tap times inf / NaN is NaN: a NON-FINITE
     * 1 Msps sample can reach the outputs of one more 1 Msps sample than in the reference (the only departure). */
    int device_samp_rate;
    double carrier_offset_hz;/* gr_mod_base::set_carrier_offset (rotator at 1 Msps) */
} qrl_mod_config;
int qrl_mod_create(qrl_ctx* ctx, const qrl_mod_config* cfg, qrl_mod** out);
void qrl_mod_destroy(qrl_mod* m);
/* replaces: flush of the modulator graph on mode change (gr_mod_base.cpp:354-360): scrambler seed, encoder, filter history */
int qrl_mod_reset(qrl_mod* m);
/* replaces: gr_mod_qpsk::set_bb_gain (src/gr/gr_mod_qpsk.cpp:91-94) */
int qrl_mod_set_bb_gain(qrl_mod* m, float value);
/* replaces: gr_mod_base::set_carrier_offset -> rotator_cc::set_phase_inc (src/gr/gr_mod_base.cpp:799-805); phase-continuous.
 * Only for handles created with the back end (device_samp_rate >= 2e6 or a non-zero initial offset). */
int qrl_mod_set_carrier_offset(qrl_mod* m, double hz);
/* per-stream gr_mod_base::set_carrier_offset: hz[b] for stream b (host array of `batch` doubles); same rules as qrl_demod_set_carrier_offsets.
 * A handle without the gr_mod_base back end returns QRL_ERR_ARG, like the scalar setter. */
int qrl_mod_set_carrier_offsets(qrl_mod* m, const double* hz);
size_t qrl_mod_samples_per_byte(const qrl_mod* m);
typedef struct { int stream; int channel; uint64_t start; uint64_t count; } qrl_zero_run;
/* QRL_MODEM_DMR (replaces make_gr_mod_dmr(), reference src/gr/gr_mod_dmr.cpp:19-90, instance gr_mod_base.cpp:207, fed by gr_mod_base::setDMRData
 * :788 -> gr_dmr_source): raw dibits -> map{2,3,1,0} -> 4 levels -> RRC(5, 24000, 4800, 0.2, 125) x5 -> x0.66666666 -> frequency_modulator_fc
 * (pi 4800 0.85 / 24000) -> gr_zero_idle_bursts(62) -> x0.9 -> bb gain -> rational_resampler_ccf(125, 3, low_pass_2(125, 3e6, 5000, 2000, 60, BH)):
 * 2500 samples per 3 bytes, like QRL_MODEM_M17.  The zero-idle block is restated as ONE work() call over the stream sees it: its history of
 * 2 x 720 items delays the signal by 1439 items at 24 ksps, and a "zero_samples" tag {offset T, count} zeroes the block's OUTPUT items
 * T - 62 ... T - 62 + count - 1 (a later tag ends an earlier run).  qrl_mod_add_zero_runs hands over those tags (T in the block's 24 ksps
 * input coordinates = 20 x the byte offset gr_dmr_source put the tag on; `channel` ignored); they apply to the following qrl_mod_process calls.
 * (Across scheduler calls the reference only matches tags inside a call's own window, so it misses tags within the first 62 items of a window:
 * not restated.)  The bursts themselves can be built on the device (qrl_dmr_l2_encode / qrl_dmr_voice_call_encode, below); CACH, the slot
 * timing and the tags of gr_dmr_source stay with the caller. */
int qrl_mod_add_zero_runs(qrl_mod* m, const qrl_zero_run* runs, size_t n);
/* QRL_MODEM_M17 (replaces make_gr_mod_m17(), reference src/gr/gr_mod_m17.cpp:19-81, gr_mod_base.cpp:206): its 125 / 3 output resampler
 * makes 833 1/3 samples per byte, so calls take multiples of 3 bytes (an M17 frame is 48) and return 2500 samples per 3 bytes;
 * qrl_mod_samples_per_byte is 0 for it.  Other modes: bytes_per_block 1, the value of qrl_mod_samples_per_byte. */
size_t qrl_mod_samples_per_block(const qrl_mod* m, size_t* bytes_per_block);   /* at the DEVICE rate: 8*sps (QPSK) or 16*sps*interp (FSK), times fs/1e6 */
/* replaces: gr_mod_base::set_data (src/gr/gr_mod_base.cpp:783-786) + gr_byte_source::work (src/gr/gr_byte_source.cpp:75-106)
 * + one scheduler pass of every block of gr_mod_qpsk: bytes[b*stride + i], i < nbytes (device, packed, MSB first) ->
 * iq[2*(b*out_stride + k)], k < nbytes*8*sps (device cf32).  State (scrambler, encoder, differential symbol, pulse-shaping
 * history) carries across calls; asynchronous on the handle's stream. */
int qrl_mod_process(qrl_mod* m, const uint8_t* bytes, size_t stride, size_t nbytes, float* iq, size_t out_stride);
/* like qrl_mod_process, but iq is interleaved int16 I, Q (sc16, 4 bytes per sample: what UHD / SoapySDR / LimeSuite / HackRF put on the
 * wire): sample k of stream b at iq[2*(b*out_stride + k)] (I) and iq[2*(b*out_stride + k) + 1] (Q).  Replaces the driver's own
 * fc32 -> sc16 converter: the kernel that would store the cf32 sample converts it in registers in front of the store (half the output
 * buffer, half the download, no device-rate cf32 copy in memory).  Per component r = rintf(x * scale) -- one rounded f32 multiply, round
 * to nearest even -- saturated to [-32768, 32767]; NaN gives 0 (the float_to_short rule); x is exactly the float qrl_mod_process stores.
 * scale: qrl_mod_set_sc16_scale, default 32767.0f (1.0 -> 32767); the setter takes effect from the next call and refuses a non-finite or
 * zero value with QRL_ERR_ARG.  The format belongs to the CALL, not the handle: the carried state is cf32, so cf32 and sc16 calls may
 * alternate on one handle and give the converted concatenated stream; counts, M17's multiples of 3 bytes, zero runs, carrier offsets,
 * retune, reset and asynchrony are those of qrl_mod_process.  Every modem type, with or without the back end, every device rate.
 * iq must be 4-byte aligned (one packed store per sample), else QRL_ERR_ARG; out_stride (samples) may be any value >= the call's sample
 * count, nothing outside those samples of a row is written.
 * qrl_mod_set_sc16_clip_counts: counts = device pointer to `batch` uint32, or NULL (the default: no counting).  Every following sc16 call
 * ADDS to counts[b] the components of stream b whose r lay outside [-32768, 32767] (I and Q separately; +-inf counts, NaN does not); the
 * caller zeroes the array; the values are valid once the handle's stream has passed the call.  cf32 calls never touch it. */
int qrl_mod_process_sc16(qrl_mod* m, const uint8_t* bytes, size_t stride, size_t nbytes, int16_t* iq, size_t out_stride);
int qrl_mod_set_sc16_scale(qrl_mod* m, float scale);
int qrl_mod_set_sc16_clip_counts(qrl_mod* m, uint32_t* counts);
/* like qrl_mod_process, but iq is interleaved int8 I, Q (sc8, 2 bytes per sample: what a HackRF takes on the wire): sample k of stream b
 * has I at iq[2*(b*out_stride + k)] and Q one byte behind it.  Per component r = rintf(x * scale) -- one rounded f32 multiply, round to
 * nearest even -- saturated to [-128, 127]; NaN gives 0; x is exactly the float qrl_mod_process stores.
 * scale: qrl_mod_set_sc8_scale, default 127.0f (1.0 -> 127); the setter takes effect from the next call and refuses a non-finite or zero
 * value with QRL_ERR_ARG.  The format belongs to the CALL: cf32, sc16 and sc8 calls may alternate on one handle and give the converted
 * concatenated stream; counts, M17's multiples of 3 bytes, zero runs, carrier offsets, retune, reset and asynchrony are those of
 * qrl_mod_process.  Every modem type, with or without the back end, every device rate from 1 to 183 Msps.
 * iq must be 2-byte aligned, else QRL_ERR_ARG (the handle goes on working); out_stride (samples) may be any value >= the call's sample
 * count.  A sample is one 2-byte store: nothing outside a row's samples is written, not even the other half of a 4-byte word that a row
 * shares with its neighbour.
 * qrl_mod_set_sc8_clip_counts: counts = device pointer to `batch` uint32, or NULL (the default: no counting).  Every following sc8 call
 * ADDS to counts[b] the components of stream b with r > 127 or r < -128 (I and Q separately; +-inf counts, NaN does not; -128 reached
 * without saturation is not a clip); the caller zeroes the array; the values are valid once the handle's stream has passed the call.
 * cf32 and sc16 calls never touch it, and sc8 calls never touch the sc16 counters; the two setters may name the same array. */
int qrl_mod_process_sc8(qrl_mod* m, const uint8_t* bytes, size_t stride, size_t nbytes, int8_t* iq, size_t out_stride);
int qrl_mod_set_sc8_scale(qrl_mod* m, float scale);
int qrl_mod_set_sc8_clip_counts(qrl_mod* m, uint32_t* counts);
int qrl_mod_sync(qrl_mod* m);
void* qrl_mod_stream(qrl_mod* m);

/* ---- multi-carrier MMDVM receiver (reference src/gr/gr_demod_mmdvm_multi2.cpp:19-38,58-135) ---------------------
 * make_gr_demod_mmdvm_multi2(burst_timer, num_channels, channel_separation, use_tdma, sps, samp_rate, carrier_freq,
 * filter_width): stream_to_streams + pfb_channelizer_ccf + per channel {24/25 resampler, LPF, FM discriminator,
 * level, float_to_short}.  The reference fixes 10 branches at 250 ksps (src/config_mmdvm.h:4); here num_channels = M
 * (2..64) at fs = 25 kHz * M; num_channels = 1 selects the SINGLE-carrier receiver gr_demod_mmdvm (src/gr/gr_demod_mmdvm.cpp:29-61:
 * 250 ksps in, rational_resampler_ccf(12, 125), rssi tag, 43-tap LPF, quadrature_demod_cf(24000/(2 pi 10000)), int16).  Channel c is centred at +c*fs/M (c > M/2: negative offsets); the reference's port
 * order {0,1,2,3,9,8,7} and the TDMA tagging / ZeroMQ framing of gr_mmdvm_sink (src/gr/gr_mmdvm_sink.cpp:66-176)
 * stay with the caller.  channel_first/channel_count select the channels THIS handle produces: ranks of a multi-GPU job
 * take disjoint ranges (no data-path collective). */
typedef struct qrl_chan qrl_chan;
typedef struct {
    int num_channels;        /* M: PFB branches = channels on the fs/M grid */
    int channel_first, channel_count;   /* produced range; channel_count <= 0: all */
    int batch;               /* independent wideband inputs per call */
    size_t max_chunk;        /* largest n (wideband samples per input) of any call */
    void* hip_stream;
    /* form 1 = the legacy "freq-xlating" receiver make_gr_demod_mmdvm_multi(burst_timer, num_channels, channel_separation,
     * use_tdma, sps, samp_rate, carrier_freq, filter_width) (src/gr/gr_demod_mmdvm_multi.cpp:19-38,58-123): per channel
     * rotator_cc(2 pi (-channel_separation) ct / fs) -> rational_resampler_ccf(1, decimation, low_pass(1, fs, filter_width,
     * 3500, BH)) -> fft_filter_ccf -> rssi tag -> discriminator -> int16, fs = 24 kHz * decimation (240 ksps in the
     * reference).  The wideband input is read once per channel (compute-bound form); 0 = PFB channelizer (multi2).
     * form 2 = BASELINE.json configs[3] taken literally ("64x freq-xlating-FIR channelizer + 4FSK demod"): channel i
     * = rotator_cc(2 pi (-25000) ct / fs) -> rational_resampler_ccf(1, num_channels, low_pass_2(1, fs, 5000, 2000, 60, BH)) at
     * fs = 25 kHz * num_channels with the PFB form's channel map (ct = i, i <= N/2; i - N above), followed by the per-channel
     * chain of form 0 (24/25 resampler, LPF, RSSI, discriminator -> int16, optional 4FSK tail).  The same channels as form 0 from
     * num_channels separate FIRs: the compute-bound way of doing what the PFB does; it exists to be measured next to it.
     * form 3 = the per-channel chain alone (qrl_chan_process_channels): `batch` counts 25 ksps channel streams, max_chunk channel samples. */
    int form;
    int channel_separation;  /* form 1: Hz, 0 = 25000 */
    int decimation;          /* form 1: 0 = 10 */
    int filter_width;        /* form 1: 0 = 8000 (header default, gr_demod_mmdvm_multi.h:37-40) */
} qrl_chan_config;
int qrl_chan_create(qrl_ctx* ctx, const qrl_chan_config* cfg, qrl_chan** out);
void qrl_chan_destroy(qrl_chan* c);
int qrl_chan_reset(qrl_chan* c);
/* path selection for tests (results are identical): the 64-channel geometry runs on k_pfb_stream64 + the fused per-channel kernel; every other
 * shape (other channel counts, unaligned rows, the single-carrier and frequency-translating forms) on the general-M channelizer and the separate
 * per-channel kernels.  QRL_CHAN_OPT_LEGACY_PFB = 1 / QRL_CHAN_OPT_LEGACY_TAIL = 1 send the 64-channel geometry down those general paths so that
 * the parity tests cover them at the bench shape too (round 6 deleted the third channelizer, round 3's tiled k_pfb_chan64).  LEGACY_TAIL only before the first samples of a stream or after qrl_chan_reset (QRL_ERR_STATE
 * otherwise: the fused kernel does not fill the intermediate rings the separate kernels take their history from).
 * QRL_CHAN_OPT_SERIAL_TAIL = 1 keeps the per-channel kernel of a call on the handle's stream, behind its channelizer and in front of the
 * next one (rounds 1-4); 0, the default for a PFB-form handle that owns its stream: it runs on an internal stream BESIDE the channelizer
 * of the next call (the channel ring holds two calls) -- int16 / RSSI outputs are then valid after qrl_chan_sync() or behind
 * qrl_chan_stream_wait(), like the 4FSK outputs.  A handle created on the caller's hip_stream always runs the serial order.
 * (environment: QRL_CHAN_SERIAL_TAIL=1 at qrl_chan_create, for A/B runs of unmodified callers) */
enum { QRL_CHAN_OPT_LEGACY_PFB = 1, QRL_CHAN_OPT_LEGACY_TAIL = 2, QRL_CHAN_OPT_SERIAL_TAIL = 3 };
int qrl_chan_set_option(qrl_chan* c, int option, int value);
int qrl_chan_set_level(qrl_chan* c, float level);   /* _level_control multiply_const_ff, gr_demod_mmdvm_multi2.cpp:84 */
/* replaces: gr_demod_mmdvm_multi2::calibrate_rssi / gr_demod_mmdvm::calibrate_rssi -> rssi_tag_block::calibrate_rssi
 * (src/gr/gr_demod_mmdvm_multi2.cpp:138-144, src/gr/gr_demod_mmdvm.cpp:64-67) */
int qrl_chan_calibrate_rssi(qrl_chan* c, float level);
/* replaces: the RSSI stream tags of rssi_tag_block::work (src/gr/rssi_tag_block.cpp:43-68): one dB value per 300 samples at
 * 24 ksps.  rssi[(b*channel_count + ch)*cap + k], k < counts[b*channel_count + ch], holds the tags completed by each
 * following qrl_chan_process call (device pointers; NULL switches the block off). */
int qrl_chan_set_rssi_output(qrl_chan* c, float* rssi, size_t cap, uint32_t* counts);
/* optional 4FSK symbol tail behind every produced channel (BASELINE config 4: channelizer + 4FSK demod): the chain of
 * gr_demod_dmr after its resampler (src/gr/gr_demod_dmr.cpp:62-105: quadrature_demod_cf(24000/(pi/2*4800)) ->
 * fft_filter_fff(RRC(1, 24k, 4.8k, 0.2, 125)) -> symbol_sync_ff(M&M, 5 sps, 4-level) -> x0.9 -> phase_modulator -> slicer ->
 * map{3,1,2,0}) applied to the 24 ksps channel signal (after _filter[i], gr_demod_mmdvm_multi2.cpp:62-63,75).
 * bits[s*bits_cap + k]: two bits per symbol; constellation (cf32, may be NULL); counts[s*4 + 1] = symbols, [s*4 + 2] = bits
 * produced by each following qrl_chan_process call, s = b*channel_count + ch.  bits == NULL switches the tail off.
 * The symbol synchroniser runs on an internal stream of the handle (it overlaps the next call's channelizer): bits, constellation
 * and counts of a call are valid after qrl_chan_sync() or, on the device, behind qrl_chan_stream_wait() -- synchronising only the
 * cfg.hip_stream the caller passed in is NOT enough for these three outputs (it is for the int16 / RSSI outputs of such a handle). */
int qrl_chan_set_4fsk_output(qrl_chan* c, uint8_t* bits, size_t bits_cap, float* constellation, size_t constellation_cap, uint32_t* counts);
size_t qrl_chan_out_cap(const qrl_chan* c, size_t n);   /* int16 samples per channel a call with n inputs can produce */
/* replaces one scheduler pass of the multi-carrier graph: iq[b*stride + i] device cf32, n a multiple of num_channels;
 * out[(b*channel_count + c)*out_cap + k] device int16 @24 ksps, counts[b*channel_count + c] = samples written. */
int qrl_chan_process(qrl_chan* c, const float* iq, size_t stride, size_t n, int16_t* out, size_t out_cap, uint32_t* counts);
/* like qrl_chan_process / qrl_chan_channelize, but iq is interleaved int16 I, Q (sc16, 4 bytes per sample: what a LimeSDR or UHD stream
 * delivers): stream b at iq + 2*b*stride int16s.  The semantics are those of qrl_demod_process_sc16: x = (float)v * scale per component
 * (one exact conversion, one rounded f32 multiply), bit for bit what the cf32 entry point computes when fed (float)v * scale -- int16
 * channel samples, counts, RSSI tags, 4FSK dibits and constellation, and chan_out of the channelize half.  scale: qrl_chan_set_sc16_scale,
 * default 1.0f / 32768; the setter takes effect from the next call and refuses a non-finite or zero value with QRL_ERR_ARG.  The format
 * belongs to the CALL, not the handle: history and rings are cf32, so cf32 and sc16 calls may alternate on one handle and give the result
 * of the concatenated stream; options, profiling (the same kernel names), channel ranges and the overlap of the internal streams work as
 * with cf32.  Forms 0 (the 64-channel streaming kernel fetches the raw pairs with LDS-DMA and converts them as they land; docs/KERNELS.md),
 * 1, 2 and the single carrier.  iq must be 16-byte aligned and stride a multiple of 4 samples, else QRL_ERR_ARG; the constraints on n are
 * those of the cf32 call.  A form 3 handle (qrl_chan_process_channels) takes channel samples, not SDR samples: both calls return
 * QRL_ERR_ARG on it (qrl_last_error says why), change nothing and leave the handle usable. */
int qrl_chan_process_sc16(qrl_chan* c, const int16_t* iq, size_t stride, size_t n, int16_t* out, size_t out_cap, uint32_t* counts);
int qrl_chan_channelize_sc16(qrl_chan* c, const int16_t* iq, size_t stride, size_t n, float* chan_out, size_t pitch, int groups);
int qrl_chan_set_sc16_scale(qrl_chan* c, float scale);
int qrl_chan_sync(qrl_chan* c);
/* ---- the two halves of qrl_chan_process for a CHANNEL-SHARDED multi-GPU job (PFB form: "channelize, then scatter the
 * channel streams"; reference: one channelizer feeds per-channel chains, src/gr/gr_demod_mmdvm_multi2.cpp:98-135, and every channel
 * has its own sink socket, src/gr/gr_mmdvm_sink.cpp:77-173).  Each rank channelizes ITS wideband inputs, an all-to-all moves every
 * channel's samples to the rank that owns the channel, and that rank runs the per-channel chains:
 *   qrl_chan_channelize        (PFB handle, form 0) stream_to_streams + pfb_channelizer_ccf only.  chan_out = device cf32,
 *                              [groups][batch][channel_count / groups][pitch]: the rows of destination rank g are contiguous, n / M
 *                              valid items per row.  The handle keeps the filter history; it must not be mixed with qrl_chan_process.
 *   qrl_chan_process_channels  (form 3 handle: `batch` = number of 25 ksps channel streams, num_channels ignored) the per-channel chain
 *                              of qrl_chan_process on chan_in[row * pitch + i], i < n1; outputs as qrl_chan_process with
 *                              channel_count = 1 (row index = stream index).  The per-channel kernel reads chan_in IN PLACE (no copy
 *                              into the handle's rings; the handle keeps the ~1.6 k samples per row it needs of it for the next call):
 *                              the buffer must stay untouched until the handle's stream has passed this call (an event recorded on
 *                              qrl_chan_stream() after the call, or qrl_chan_sync).
 *   qrl_chan_wait_for          the handle's stream waits (on the device) for what the given stream has queued so far: the collective. */
int qrl_chan_channelize(qrl_chan* c, const float* iq, size_t stride, size_t n, float* chan_out, size_t pitch, int groups);
int qrl_chan_process_channels(qrl_chan* c, const float* chan_in, size_t pitch, size_t n1, int16_t* out, size_t out_cap, uint32_t* counts);
int qrl_chan_wait_for(qrl_chan* c, void* hip_stream);
/* like qrl_demod_stream_wait: the caller's stream waits, on the device, for everything this handle has enqueued so far -- how a C4
 * caller chains its own copies / collectives (the all-to-all of a multi-GPU job) behind a call without a host synchronisation. */
int qrl_chan_stream_wait(qrl_chan* c, void* hip_stream);
void* qrl_chan_stream(qrl_chan* c);   /* hipStream_t the handle enqueues on */
int qrl_chan_internal_streams(qrl_chan* c, void* out[3]);   /* profiling aid, as qrl_demod_internal_streams: out[0] the handle's stream, out[1] the symbol-sync stream (or NULL), out[2] the per-channel kernel's stream (or NULL) */
/* like qrl_demod_profile / qrl_demod_profile_read: HIP events on the handle's stream around the kernel(s) that read the caller's
 * wideband IQ (k_pfb_chan; forms 1 / 2: the per-channel decimator launches of a call, summed) -- bench.py's roofline leg */
int qrl_chan_profile(qrl_chan* c, int enable);
int qrl_chan_profile_read(qrl_chan* c, double* kernel_ms, uint64_t* launches, const char** kernel_name);
/* the same for the three kernels of a C4 call, each timed with HIP events on the stream it is launched on: ms[0] / launches[0] the
 * kernel(s) qrl_chan_profile_read reports (channelizer), [1] the fused per-channel kernel k_chan_tail, [2] the symbol synchroniser
 * k_symsync_ff (sums over the profiled calls; a duration includes the time a kernel shares the chip with the others of the step) */
int qrl_chan_profile_read_kernels(qrl_chan* c, double ms[3], uint64_t launches[3]);

/* ---- multi-carrier MMDVM transmitter (reference src/gr/gr_mod_mmdvm_multi2.cpp:30-128) -------------------------------------
 * make_gr_mod_mmdvm_multi2(burst_timer, num_channels, channel_separation, use_tdma, sps, samp_rate, carrier_freq,
 * filter_width): per channel short_to_float(1, 32767) -> frequency_modulator_fc(2 pi 12500 / 24000) -> fft_filter_ccf ->
 * x0.8 -> rational_resampler_ccf(25, 24) -> pfb_synthesizer_ccf(10, ..., false) on ports {0,1,2,3,9,8,7} -> x(1 / num_channels)
 * -> bb gain.  in[(b*num_channels + ch)*stride + i], i < n: the int16 FM baseband gr_mmdvm_source hands out at 24 ksps
 * (src/gr/gr_mmdvm_source.cpp:180-243; its ZeroMQ framing and the tag-driven gr_zero_idle_bursts stay with the caller);
 * iq[2*(b*out_stride + k)]: the 250 ksps cf32 wideband signal, *produced (host) samples per stream for this call
 * (<= qrl_synth_out_cap(n)).  State carries across calls; asynchronous on the handle's stream. */
typedef struct qrl_synth qrl_synth;
typedef struct {
    int num_channels;        /* 1..7 (MAX_MMDVM_CHANNELS) */
    int filter_width;        /* 0 = 5000 (gr_mod_mmdvm_multi2.h:38-41) */
    int batch;               /* independent transmitters */
    size_t max_samples;      /* largest n of any call */
    void* hip_stream;
    float bb_gain;           /* gr_mod_mmdvm_multi2::set_bb_gain, 0 = 1.0 */
    int single_carrier;      /* 1 (with num_channels = 1): make_gr_mod_mmdvm (src/gr/gr_mod_mmdvm.cpp:17-64): FM -> LPF -> x0.8 -> bb
                                gain -> rational_resampler_ccf(125, 12): no synthesizer, 24 ksps -> 250 ksps */
} qrl_synth_config;
int qrl_synth_create(qrl_ctx* ctx, const qrl_synth_config* cfg, qrl_synth** out);
void qrl_synth_destroy(qrl_synth* s);
int qrl_synth_reset(qrl_synth* s);
/* gr_zero_idle_bursts (reference src/gr/gr_zero_idle_bursts.cpp:45-84; gr_mod_mmdvm_multi2.cpp:88,108, gr_mod_mmdvm.cpp:51-58):
 * the zero_samples tags gr_mmdvm_source attaches to idle slots, as absolute runs at the rate of that block's input (25 ksps behind
 * the 25/24 resampler in the multi-carrier graph, 24 ksps behind the FM modulator in the single-carrier one; item index counted from
 * the handle's creation / last reset).  Items start .. start + count - 1 of (stream, channel) become 0 + 0j in whichever following
 * qrl_synth_process calls they fall into.  host/mmdvm_wire.h zero_idle_runs() turns the source's tags into these runs. */
/* (qrl_zero_run is declared with qrl_mod_add_zero_runs above) */
int qrl_synth_add_zero_runs(qrl_synth* h, const qrl_zero_run* runs, size_t n);
int qrl_synth_set_bb_gain(qrl_synth* s, float value);
size_t qrl_synth_out_cap(const qrl_synth* s, size_t n);
int qrl_synth_process(qrl_synth* s, const int16_t* in, size_t stride, size_t n, float* iq, size_t out_stride, size_t* produced);
/* sc16 output, as qrl_mod_process_sc16 (same rule, layout, alignment, default scale 32767.0f, clip counters per stream of the batch):
 * `produced` and everything else as qrl_synth_process.  Multi-carrier: the synthesizer converts in its store.  Single carrier: the
 * resampler's ring row of the call is converted by a small kernel of its own (250 ksps; the resampler is shared with the receivers). */
int qrl_synth_process_sc16(qrl_synth* s, const int16_t* in, size_t stride, size_t n, int16_t* iq, size_t out_stride, size_t* produced);
int qrl_synth_set_sc16_scale(qrl_synth* s, float scale);
int qrl_synth_set_sc16_clip_counts(qrl_synth* s, uint32_t* counts);
/* sc8 output, as qrl_mod_process_sc8: interleaved int8 I, Q, 2 bytes per sample, r = rintf(x * scale) saturated to [-128, 127], NaN -> 0,
 * default scale 127.0f (a non-finite or zero scale is QRL_ERR_ARG), iq 2-byte aligned else QRL_ERR_ARG, one 2-byte store per sample and
 * nothing else written, clip counters of its own per stream of the batch (r > 127 or r < -128; the sc16 counters stay untouched).
 * `produced` and everything else as qrl_synth_process; the kernels that convert are those of qrl_synth_process_sc16. */
int qrl_synth_process_sc8(qrl_synth* s, const int16_t* in, size_t stride, size_t n, int8_t* iq, size_t out_stride, size_t* produced);
int qrl_synth_set_sc8_scale(qrl_synth* s, float scale);
int qrl_synth_set_sc8_clip_counts(qrl_synth* s, uint32_t* counts);
int qrl_synth_sync(qrl_synth* s);

/* ---- device deframer (reference src/gr/gr_deframer_bb.cpp:24-48,83-185; instances gr_demod_base.cpp:171-178) -----------
 * make_gr_deframer_bb(modem_type): 1 = 2k modes (16/24-bit sync words, 64 bits per frame), 2 = 1k modes (0xB5, 32 bits),
 * 3 = 10k modes (384 bits).  qrl_deframer_process consumes the unpacked bits of one demodulator port (bits[b*stride + i];
 * i < n, or i < counts[b*count_stride] when counts != NULL: pass the demodulator's counts + 2 or + 3 with count_stride 4)
 * and appends what gr_deframer_bb::work pushes into its mailbox -- the sync bits followed by the frame bits -- to
 * out[b*out_cap + k], k < out_counts[b] (out_cap >= 2 n + 24 never overflows).  Search state carries across calls.
 * All pointers are device pointers; asynchronous on the handle's stream (give it the demodulator's stream to chain). */
typedef struct qrl_deframer qrl_deframer;
int qrl_deframer_create(qrl_ctx* ctx, int deframer_type, int batch, void* hip_stream, qrl_deframer** out);
void qrl_deframer_destroy(qrl_deframer* d);
int qrl_deframer_reset(qrl_deframer* d);   /* gr_deframer_bb::flush (:58-65) */
int qrl_deframer_process(qrl_deframer* d, const uint8_t* bits, size_t stride, size_t n, const uint32_t* counts, size_t count_stride,
                         uint8_t* out, size_t out_cap, uint32_t* out_counts);
int qrl_deframer_sync(qrl_deframer* d);

/* ---- L1 frame synchroniser (reference gr_modem::synchronize / findSync / packBytes, src/gr_modem.cpp:1119-1282, 980-994;
 * frame types src/layer1framing.h:8-24; mode table gr_modem::toggleRxMode :203-322) ------------------------------------------
 * Consumes the unpacked bits of a demodulator port like qrl_deframer_process and emits, per stream, the frames the
 * reference would pass to gr_modem::processReceivedData as records
 *     { uint32 frame_type (FrameTypeVoice1 0xB5, FrameTypeVoice 0xED89, FrameTypeText 0x89EDAA, ...);
 *       uint32 nbytes | _modem_sync << 16  (low 16 bits: payload bytes; high 16 bits: the _modem_sync counter at the moment the frame
 *       completed, 0..39 -- what processReceivedData's voice gate of the 1k modes tests, src/gr_modem.cpp:1376-1390);
 *       nbytes payload bytes, MSB-first packed, padded to a multiple of 4 }
 * appended to out[b*out_cap ...]; out_counts[2b] = bytes written, out_counts[2b+1] = frames.  A frame that does not fit is
 * dropped (out_cap >= n/8 + qrl_framesync_frame_bytes() + 96 + 16 per frame never overflows: a frame begun in earlier calls may
 * complete in this one).  Search state, a partial frame
 * and the _modem_sync counter carry across calls.  QRL_MODEM_M17: the M17 sync words (LSF 0x55F7, stream 0xFF5D, EOT
 * 0x555D555D, :1186-1210) and 46-byte frames (:309-313); qrl_m17_rx_process takes these records as they are. */
typedef struct qrl_framesync qrl_framesync;
int qrl_framesync_create(qrl_ctx* ctx, int modem_type, int batch, void* hip_stream, qrl_framesync** out);
void qrl_framesync_destroy(qrl_framesync* f);
int qrl_framesync_reset(qrl_framesync* f);
int qrl_framesync_frame_bytes(const qrl_framesync* f);   /* _rx_frame_length of the mode */
int qrl_framesync_process(qrl_framesync* f, const uint8_t* bits, size_t stride, size_t n, const uint32_t* counts, size_t count_stride,
                          uint8_t* out, size_t out_cap, uint32_t* out_counts);
/* Optional: activity[b] (device, [batch]) receives with every qrl_framesync_process call the number of bits of stream b that were collected into a
 * frame while a sync was held -- non-zero exactly when gr_modem::synchronize would return data_to_process = true for the bits of this call
 * (src/gr_modem.cpp:1121-1175: "RX active", what radiocontroller.cpp:1298 polls through gr_modem::demodulate()).  NULL switches it off. */
int qrl_framesync_set_activity_output(qrl_framesync* f, uint32_t* activity);
int qrl_framesync_sync(qrl_framesync* f);

/* ---- RSSI side output (reference src/gr/rssi_block.cpp:25-50; wired src/gr/gr_demod_base.cpp:199-200: port 0 of the current
 * demodulator -> rssi_valve -> rssi_block -> probe_signal_f) -----------------------------------------------------------------
 * rssi_block(level): complex_to_mag_squared -> moving_average_ff(2000, 1, 2000) -> single_pole_iir_filter_ff(0.04) -> nlog10_ff
 * -> multiply_const_ff(10) -> add_const_ff(level).  qrl_rssi_process consumes the port-0 items of one qrl_demod_process call
 * (filtered[b*stride + i] cf32 pairs, i < counts[b*count_stride], counts == NULL: n items for every stream; device memory) and
 * writes one dB value per item to out[b*out_cap + i] (may be NULL) and the latest value of every stream to last[b] (what
 * probe_signal_f::level() returns; may be NULL).  State (2000-item window, IIR) carries across calls; results do not depend on
 * how the stream is cut into calls (the moving average restarts its running sum at every absolute multiple of 2000 items: the
 * reference's block does so at every work() call of at most max_iter = 2000 items). */
typedef struct qrl_rssi qrl_rssi;
int qrl_rssi_create(qrl_ctx* ctx, int batch, float level, void* hip_stream, qrl_rssi** out);
void qrl_rssi_destroy(qrl_rssi* r);
int qrl_rssi_reset(qrl_rssi* r);
int qrl_rssi_set_level(qrl_rssi* r, float level);   /* rssi_block::set_level (:47-50) */
int qrl_rssi_process(qrl_rssi* r, const float* filtered, size_t stride, size_t n, const uint32_t* counts, size_t count_stride,
                     float* out, size_t out_cap, float* last, uint32_t* out_counts);
int qrl_rssi_sync(qrl_rssi* r);
void* qrl_rssi_stream(qrl_rssi* r);

/* ---- spectrum side output (reference src/gr/rx_fft.cpp:44-213, instance make_rx_fft_c(32768, WIN_BLACKMAN_HARRIS)
 * src/gr/gr_demod_base.cpp:166,185 on the device-rate IQ) ---------------------------------------------------------------------
 * qrl_fft_process = rx_fft_c::work on n new samples of every stream: while enabled and nobody is behind on reading (d_push == 0)
 * the samples are multiplied by the window into the FFT buffer; when the buffer is full the next sample triggers the transform
 * (hipFFT, batched over the streams) and volk_32fc_s32f_power_spectrum_32f (10 log10 |X / N|^2), after which the block stops
 * taking samples until qrl_fft_get_fft_data has been called.  qrl_fft_get_fft_data = rx_fft_c::get_fft_data: the spectrum with its
 * halves swapped (negative frequencies first) to fft_points[b*out_stride + i] (device), *fft_size = 0 when nothing is ready.
 * wintype: gr::fft::window::win_type (0 Hamming, 1 Hann, 2 Blackman, 3 rectangular, 4 Kaiser(6.76), 5 Blackman-Harris,
 * 6 Bartlett, 7 flat top; anything else -> Hamming, :200-203). */
typedef struct qrl_fft qrl_fft;
int qrl_fft_create(qrl_ctx* ctx, int batch, unsigned fftsize, int wintype, void* hip_stream, qrl_fft** out);
void qrl_fft_destroy(qrl_fft* f);
int qrl_fft_set_enabled(qrl_fft* f, int enabled);            /* :102-107 (a new block is disabled, :58) */
int qrl_fft_set_fft_size(qrl_fft* f, unsigned fftsize);      /* :134-163 */
unsigned qrl_fft_get_fft_size(const qrl_fft* f);             /* :166-169 */
int qrl_fft_set_window_type(qrl_fft* f, int wintype);        /* :172-190 */
int qrl_fft_get_window_type(const qrl_fft* f);               /* :193-196 */
int qrl_fft_process(qrl_fft* f, const float* iq, size_t stride, size_t n);
/* qrl_fft_process on interleaved int16 I, Q (sc16): stream b at iq + 2*b*stride int16s, x = (float)v * scale per component in front of the
 * window multiply (scale: qrl_fft_set_sc16_scale, default 1.0f / 32768, a non-finite or zero value is QRL_ERR_ARG) -- the power spectrum
 * and the fill / transform / hold state machine are bit for bit those of qrl_fft_process fed (float)v * scale; cf32 and sc16 calls may
 * alternate.  iq must be 16-byte aligned and stride a multiple of 4 samples, else QRL_ERR_ARG. */
int qrl_fft_process_sc16(qrl_fft* f, const int16_t* iq, size_t stride, size_t n);
int qrl_fft_set_sc16_scale(qrl_fft* f, float scale);
/* qrl_fft_process on interleaved 8-bit I, Q, stream b at iq + 2*b*stride bytes: sc8 x = (float)v * scale, cu8 x = ((float)u - bias) * scale
 * (defaults 1.0f / 128 and 127.5f; the setters refuse a zero or non-finite scale and a non-finite bias with QRL_ERR_ARG), in front of the window
 * multiply -- bit for bit qrl_fft_process fed those floats; the formats may alternate.  iq must be 16-byte aligned and stride a multiple of
 * 8 samples, else QRL_ERR_ARG. */
int qrl_fft_process_sc8(qrl_fft* f, const int8_t* iq, size_t stride, size_t n);
int qrl_fft_process_cu8(qrl_fft* f, const uint8_t* iq, size_t stride, size_t n);
int qrl_fft_set_sc8_scale(qrl_fft* f, float scale);
int qrl_fft_set_cu8_scale(qrl_fft* f, float scale, float bias);
int qrl_fft_get_fft_data(qrl_fft* f, float* fft_points, size_t out_stride, unsigned* fft_size);
int qrl_fft_sync(qrl_fft* f);
void* qrl_fft_stream(qrl_fft* f);

/* ---- filter design & tables (host side, no GPU needed): what the kernels are loaded with ----
 * replaces: gr::filter::firdes::* calls at gr_demod_2fsk.cpp:82-97, gr_demod_gmsk.cpp:80-98,
 * gr_demod_qpsk.cpp:92-103, gr_demod_base.cpp:1333-1336.  taps==NULL returns the count. */
enum { QRL_WIN_HAMMING = 0, QRL_WIN_HANN = 1, QRL_WIN_BLACKMAN = 2, QRL_WIN_RECTANGULAR = 3, QRL_WIN_BLACKMAN_HARRIS = 5 };
int qrl_firdes_low_pass(double gain, double fs, double fc, double tw, int window, float* taps);
int qrl_firdes_low_pass_2(double gain, double fs, double fc, double tw, double atten_db, int window, float* taps);
int qrl_firdes_complex_band_pass(double gain, double fs, double lo, double hi, double tw, int window, float* taps_cf32);
int qrl_firdes_root_raised_cosine(double gain, double fs, double symrate, double alpha, int ntaps, float* taps);
int qrl_table_mmse(float* t129x8);
int qrl_table_atan(float* t257);
int qrl_table_tanh(float* t256);
uint64_t qrl_phase_inc_to_turn(double radians_per_sample);

/* ---- analogue voice modulator: replaces make_gr_mod_nbfm(sps, samp_rate, carrier_freq, filter_width) (reference
 * src/gr/gr_mod_nbfm.cpp:19-77, instances gr_mod_base.cpp:171-172) for `batch` independent radios.  audio: device f32 at 8 ksps,
 * stream b at audio + b * stride, n samples per call (a multiple of 4, <= max_samples); iq: device cf32 at 1 Msps, stream b at
 * iq + 2 * b * out_stride floats, n * qrl_amod_samples_per_sample() (= 125 n) samples.  Asynchronous on the handle's stream;
 * results are independent of how the audio is cut into calls.   */
typedef struct qrl_amod qrl_amod;
typedef struct qrl_amod_config {
    int modem_type;        /* QRL_MODEM_NBFM2500 | QRL_MODEM_NBFM5000 | QRL_MODEM_USB2500 | QRL_MODEM_LSB2500 | QRL_MODEM_CW600USB | QRL_MODEM_AM5000 */
    int batch;
    size_t max_samples;    /* audio samples per stream and call */
    void* hip_stream;      /* hipStream_t or NULL (own stream) */
    float bb_gain;         /* gr_mod_nbfm::set_bb_gain; 0 = 1.0 */
    /* gr_mod_base back end (src/gr/gr_mod_base.cpp:38,215-258), as in qrl_mod_config: 0 / 1000000 = none; >= 2e6 (a multiple of 1e6): the chain's 1 Msps
     * output goes through rotator_cc(2 pi offset / 1e6) and rational_resampler_ccf(rate / 1e6, 1, low_pass(interp, rate, 480000, 20000, BH)); a non-zero
     * initial offset alone gives the rotator only.  All sample counts (samples_per_sample, out_cap, last_count) then count device-rate samples.
     * device_samp_rate: a multiple of 1e6 in [2e6, 183e6], else QRL_ERR_ARG; QRL_ERR_TOO_BIG when max_samples would give 2^32 or more device-rate
     * samples per stream and call; the same note on non-finite samples as at qrl_mod_config.device_samp_rate. */
    int device_samp_rate;
    double carrier_offset_hz;
} qrl_amod_config;
int qrl_amod_create(qrl_ctx* ctx, const qrl_amod_config* cfg, qrl_amod** out);
void qrl_amod_destroy(qrl_amod* m);
int qrl_amod_reset(qrl_amod* m);
int qrl_amod_set_bb_gain(qrl_amod* m, float value);
/* replaces gr_mod_base::set_carrier_offset (src/gr/gr_mod_base.cpp:799-805) for handles created with the back end; phase-continuous like rotator_cc::set_phase_inc */
int qrl_amod_set_carrier_offset(qrl_amod* m, double carrier_offset_hz);
/* per-stream form of qrl_amod_set_carrier_offset (see qrl_mod_set_carrier_offsets) */
int qrl_amod_set_carrier_offsets(qrl_amod* m, const double* hz);
/* replaces gr_mod_nbfm::set_ctcss(value) (src/gr/gr_mod_nbfm.cpp:101-135; gr_mod_base::set_ctcss :872-877 forwards to both NBFM instances):
 * tone_hz != 0: _audio_amplify 0.85, the audio filter becomes band_pass_2(1, 8000, 300, 3500, 200, 35, BH) and analog::sig_source_f(8000,
 * GR_COS_WAVE, tone, 0.15) is added to the audio in front of the pre-emphasis; 0: the low-pass again and _audio_amplify 0.98 (sic: the
 * constructor's 0.99 does not come back).  Takes effect with the next qrl_amod_process call; the tone's phase runs over the samples produced
 * while it is on.  NBFM handles only.  [The tone source is GNU Radio's fixed-point NCO with its 1024-row sine table, restated from memory.] */
int qrl_amod_set_ctcss(qrl_amod* m, float tone_hz);
/* replaces gr_mod_base::set_filter_width(filter_width, mode) (src/gr/gr_mod_base.cpp:878-905) -> gr_mod_nbfm::set_filter_width (gr_mod_nbfm.cpp:78-93:
 * _if_resampler low_pass_2(25, 200000, w, w, 60, BH), _filter low_pass_2(1, 50000, w, 1200, 60, BH), _resampler low_pass_2(sps, 1e6, w, w, 60, BH),
 * sensitivity 4 pi w / 50000 -- the constructor uses a 3500 Hz transition everywhere), gr_mod_am (gr_mod_am.cpp:75-85: the constructor's designs with w),
 * gr_mod_ssb (gr_mod_ssb.cpp:85-100: _resampler as constructed with w, the sideband filter complex_band_pass_2(1, 8000, 300, w | -w, -300, 250, 90, BH);
 * the audio filter keeps the constructor's width).  The chain restarts from a fresh state (see qrl_demod_set_filter_width); bb_gain and the CTCSS
 * switch are kept.  Widths whose filters do not fit the kernels' tables are refused (NBFM < 540, SSB < 500, AM < 295 Hz). */
int qrl_amod_set_filter_width(qrl_amod* m, int filter_width);
/* QRL_MODEM_CW600USB (TX only): replaces the CW branch of gr_mod_base (src/gr/gr_mod_base.cpp:144,180,679-683): _signal_source = analog::sig_source_f(8000,
 * GR_SIN_WAVE, 600, 0.001, 1) -> _usb_cw = make_gr_mod_ssb(125, 1000000, 1700, 1000, 0).  qrl_amod_process(m, NULL, 0, n, iq, stride) produces what n samples
 * of the tone source give (whole chunks of 1024 like every SSB handle; an audio pointer is ignored); qrl_amod_set_cw_k replaces gr_mod_base::set_cw_k (:948-956):
 * key down = amplitude 0.98, up = 0.001, from the next call on, the tone's phase runs on.  qrl_amod_set_filter_width works as for USB.  [The tone source is
 * GNU Radio's fixed-point NCO with its 1024-row sine table, restated from memory.] */
int qrl_amod_set_cw_k(qrl_amod* m, int key_down);
size_t qrl_amod_samples_per_sample(const qrl_amod* m);
/* SSB (replaces make_gr_mod_ssb(125, 1000000, 1700, 2700, sb), reference src/gr/gr_mod_ssb.cpp:19-82, gr_mod_base.cpp:178-179): the
 * cessb stretcher emits whole chunks of 1024 audio-rate items and looks two items ahead, so a call returns 125 x (chunks completed
 * by it) samples -- any n is accepted; qrl_amod_last_count = IQ samples per stream the last call wrote, qrl_amod_out_cap(n) = the
 * bound for a call of n audio samples (what out_stride must hold).  NBFM: both are 125 n. */
size_t qrl_amod_last_count(const qrl_amod* m);
size_t qrl_amod_out_cap(const qrl_amod* m, size_t n);
int qrl_amod_process(qrl_amod* m, const float* audio, size_t stride, size_t n, float* iq, size_t out_stride);
/* sc16 output, as qrl_mod_process_sc16 (same rule, layout, alignment, default scale 32767.0f, clip counters): qrl_amod_last_count, SSB's
 * whole chunks of 1024 and the out_stride bound (qrl_amod_out_cap) are those of qrl_amod_process. */
int qrl_amod_process_sc16(qrl_amod* m, const float* audio, size_t stride, size_t n, int16_t* iq, size_t out_stride);
int qrl_amod_set_sc16_scale(qrl_amod* m, float scale);
int qrl_amod_set_sc16_clip_counts(qrl_amod* m, uint32_t* counts);
/* sc8 output, as qrl_mod_process_sc8: interleaved int8 I, Q, 2 bytes per sample, r = rintf(x * scale) saturated to [-128, 127], NaN -> 0,
 * default scale 127.0f (a non-finite or zero scale is QRL_ERR_ARG), iq 2-byte aligned else QRL_ERR_ARG, one 2-byte store per sample and
 * nothing else written, clip counters of its own (r > 127 or r < -128; the sc16 counters stay untouched).  qrl_amod_last_count, SSB's
 * whole chunks of 1024 and the out_stride bound (qrl_amod_out_cap) are those of qrl_amod_process. */
int qrl_amod_process_sc8(qrl_amod* m, const float* audio, size_t stride, size_t n, int8_t* iq, size_t out_stride);
int qrl_amod_set_sc8_scale(qrl_amod* m, float scale);
int qrl_amod_set_sc8_clip_counts(qrl_amod* m, uint32_t* counts);
int qrl_amod_sync(qrl_amod* m);
void* qrl_amod_stream(qrl_amod* m);

/* ---- frame FEC of the DMR / M17 protocol stacks over batches of frames.  Stateless; device pointers;
 * asynchronous on hip_stream (NULL = the default stream), the caller synchronises it.
 * qrl_bptc19696_decode replaces CBPTC19696::decode (reference src/MMDVM/BPTC19696.cpp:47-64; users: CDMRFullLC, CDMRCSBK, CDMRDataHeader
 * in src/MMDVM): the 196 code bits of each 33-byte DMR burst -> de-interleave -> up to 5 rounds of Hamming (13,9,3) column and
 * (15,11,3) row correction -> the 96 payload bits as 12 bytes.  qrl_bptc19696_encode replaces CBPTC19696::encode (:67-87): payload
 * -> row / column parities -> interleave -> written into the code-bit positions of the burst (its other bits are kept). */
int qrl_bptc19696_decode(qrl_ctx* ctx, void* hip_stream, const uint8_t* bursts /* [n][33] */, size_t n, uint8_t* payloads /* [n][12] */);
int qrl_bptc19696_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* payloads /* [n][12] */, size_t n, uint8_t* bursts /* [n][33] in/out */);
/* qrl_m17_decode_frames replaces the per-frame work of M17FrameDecoder::decodeFrame (reference src/M17/M17/M17FrameDecoder.cpp:44-215:
 * decorrelate, de-interleave, sync-word classification, punctured K = 5 Viterbi of the LSF / stream payload, Golay(24,12) of the LICH).
 * frames: [n][48] (sync word + 46 bytes, as the frame synchroniser delivers them).  records: [n][QRL_M17_RECORD_BYTES] =
 * {type (M17FrameType: 0 preamble, 1 link setup, 2 stream, 4 unknown), LICH ok, payload[30] (30 LSF bytes | 18 stream-frame bytes),
 * LICH segment[6] (5 LSF bytes + segment number), 0, 0}.  The LSF reassembly from LICH segments (:130-147, per-stream state + CRC)
 * is qrl_m17_rx_process's on the device, or host/m17_frame_decoder_hip's above this call. */
#define QRL_M17_RECORD_BYTES 40
int qrl_m17_decode_frames(qrl_ctx* ctx, void* hip_stream, const uint8_t* frames, size_t n, uint8_t* records);
/* the inverse: replaces the per-frame work of M17FrameEncoder::encodeLsf / encodeStreamFrame (reference
 * src/M17/M17/M17FrameEncoder.cpp:52-118): records of the same layout (type 1: the 30 LSF bytes with their CRC; type 2: the 18
 * stream-frame bytes = frame number (EOS bit in its top bit) + 16 payload bytes, and the 6-byte LICH segment = 5 LSF bytes +
 * segment number) -> 48-byte frames.  Frame numbering, the LICH round robin and the LSF CRC are a function of the frame's index in its
 * call: qrl_m17_call_start / _encode / _end below. */
int qrl_m17_encode_frames(qrl_ctx* ctx, void* hip_stream, const uint8_t* records, size_t n, uint8_t* frames);

/* ---- M17 link layer, receive: what gr_modem::processReceivedData does with the M17 frames of a stream (reference src/gr_modem.cpp:1370-1439)
 * and what M17FrameDecoder keeps between them (src/M17/M17/M17FrameDecoder.cpp:37-43 reset, :111-117 decodeLSF, :119-159 decodeStream), per
 * stream, on the device between calls: lsf[30], lsfFromLich[30], lsfSegmentMap, _m17_decoder_locked.  A fresh or reset handle is the decoder
 * after reset() with the lock clear (the reference leaves lsfSegmentMap uninitialised before the first reset()).
 * config: Settings::m17_can_rx 0..15, m17_decode_all_can 0 / 1 (src/gr_modem.cpp:1406, :1432); set_config holds from the next process on.
 * qrl_m17_rx_process consumes the output of a QRL_MODEM_M17 frame synchroniser as qrl_framesync_process wrote it: record i of stream b at
 * frames + b * frame_stride + 56 i = {u32 frame type, u32 nbytes | _modem_sync << 16, 46 payload bytes padded to 48}, i <
 * min(counts[2 b + 1], cap_frames) (counts: the synchroniser's out_counts).  Asynchronous on hip_stream, two kernels: the per-frame decode
 * of qrl_m17_decode_frames on every LSF / stream frame where it lies (an EOT frame is never decoded), then one lane per stream through the
 * frames in order.  out: [batch][cap_frames][QRL_M17_RX_RECORD_BYTES], 16-byte aligned, one record per slot, zeros behind the count:
 *   0..1   flags, little endian (QRL_M17_RX_*)      2  M17FrameType (1 link setup, 2 stream, EOT: 0xFF)      3  CAN
 *   4..5   frame number of a stream frame, EOS bit 0x8000 included, little endian      6  LICH segment number      7  segment map after the frame
 *   8..13  encoded source (M17LinkSetupFrame.cpp:49-52)      14..19  encoded destination
 *   20     source text length, 21..30 the text of getSource() (decode_callsign, src/M17/M17/M17Callsign.cpp:70-105)
 *   31     destination text length, 32..41 the text of getDestination() (src/M17/M17/M17LinkSetupFrame.cpp:83-97)
 *   42..47 zero      48..63  the 16 payload bytes with QRL_M17_RX_AUDIO, else zero
 * Bytes 3 and 8..41 are filled where the reference reads them: where lsf.valid().  A record whose nbytes is not 46, or whose frame type is
 * none of the three M17 words, is passed over: its output record is zero and the state untouched.
 * QRL_ERR_ARG before any device work: a null pointer, cap_frames 0, 56 * cap_frames > frame_stride, frames / frame_stride not multiples of
 * 4 bytes, out not 16-byte aligned.  The calls of one handle share its state and its scratch array: the caller orders them (one stream, or
 * events between streams).  The scratch array grows with the first call of a larger batch x cap_frames than any before: a hipFree and a
 * hipMalloc, which wait for the device; every other call is asynchronous.
 * qrl_m17_rx_get_state: asynchronous, out [batch][QRL_M17_RX_STATE_BYTES], 16-byte aligned = {_m17_decoder_locked, lsf.valid(), CAN, segment
 * map, encoded source[6], encoded destination[6]}, the last three as the LSF holds them, valid or not. */
#define QRL_M17_RX_RECORD_BYTES 64
#define QRL_M17_RX_STATE_BYTES 16
#define QRL_M17_FRAMESYNC_RECORD_BYTES 56
#define QRL_M17_RX_FRAME 0x0001          /* an M17 frame went through processReceivedData */
#define QRL_M17_RX_LSF_VALID 0x0002      /* lsf.valid() after the frame */
#define QRL_M17_RX_INFO 0x0004           /* m17FrameInfoReceived(source, destination, CAN) */
#define QRL_M17_RX_AUDIO 0x0008          /* digitalAudio(payload, 16) */
#define QRL_M17_RX_END 0x0010            /* endAudioTransmission() + receiveEnd() */
#define QRL_M17_RX_LICH_OK 0x0020        /* the four Golay words of the LICH decoded */
#define QRL_M17_RX_LSF_FROM_LICH 0x0040  /* a LICH round completed with a good CRC and replaced the LSF */
#define QRL_M17_RX_LOCKED 0x0080         /* _m17_decoder_locked after the frame */
typedef struct qrl_m17_rx qrl_m17_rx;
typedef struct { int can_rx; int decode_all_can; } qrl_m17_rx_config;
int qrl_m17_rx_create(qrl_ctx* ctx, size_t batch, const qrl_m17_rx_config* config, qrl_m17_rx** out);
void qrl_m17_rx_destroy(qrl_m17_rx* h);
int qrl_m17_rx_reset(qrl_m17_rx* h, void* hip_stream);                               /* M17FrameDecoder::reset + the lock clear */
int qrl_m17_rx_set_config(qrl_m17_rx* h, const qrl_m17_rx_config* config);
int qrl_m17_rx_process(qrl_m17_rx* h, void* hip_stream, const uint8_t* frames, size_t frame_stride, const uint32_t* counts, size_t cap_frames,
                       uint8_t* out);
int qrl_m17_rx_get_state(qrl_m17_rx* h, void* hip_stream, uint8_t* out);
/* the HIP stream of a frame synchroniser, to queue qrl_m17_rx_process behind qrl_framesync_process */
void* qrl_framesync_stream(qrl_framesync* f);

/* ---- M17 link layer, transmit: a call as a function of the frame index.  Stateless; device pointers; asynchronous on hip_stream.
 * calls: [batch][QRL_M17_CALL_BYTES] descriptors = {0..8 source characters, 9 their number (10: more than nine), 10..18 destination
 * characters, 19 their number, 20 CAN, 21 destination_type 0..4, zeros}.  The LSF is M17Transmitter::start's (reference
 * src/M17/M17/M17Transmitter.cpp:46-72): encode_callsign as it stands (src/M17/M17/M17Callsign.cpp:26-68, not strict: an unknown character is
 * digit 0, more than nine characters give the zero address), an empty destination with type 0 keeps the cleared LSF's 0xFF bytes, types 1..4
 * the byte strings of setDestination(int) (src/M17/M17/M17LinkSetupFrame.cpp:59-81), type field stream 1, dataType 2, encType 0, CAN, the CRC.
 * qrl_m17_call_start (gr_modem::startTransmission, src/gr_modem.cpp:687-697; M17Transmitter.cpp:74-105): out[b * out_stride ...] = 48 preamble
 *   bytes 0x77, the LSF frame; 96 bytes.
 * qrl_m17_call_encode (gr_modem::transmitM17Audio, src/gr_modem.cpp:868-884; M17Transmitter::send, M17Transmitter.cpp:108-143): slot i of stream b,
 *   out[b * out_stride + i * slot_bytes ...], = stream frame k = first[b] + i (first NULL: 0) with payloads[b][i][16]: frame number k & 0x7FF,
 *   LICH segment k % 6 of the call's LSF; 48 bytes and zeros up to slot_bytes >= 48.  A call can be cut anywhere.
 * qrl_m17_call_end (gr_modem::endTransmission, src/gr_modem.cpp:718-729): out[b * out_stride ...] = the last frame (index first[b], zero
 *   payload, EOS bit), the sixteen EOT bytes 0x55 0x5D; 64 bytes.
 * Rows are whole multiples of the modulator's 3-byte block: qrl_mod_process (QRL_MODEM_M17) takes them as they are. */
#define QRL_M17_CALL_BYTES 32
#define QRL_M17_CALL_START_BYTES 96
#define QRL_M17_CALL_END_BYTES 64
int qrl_m17_call_start(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls, size_t batch, uint8_t* out, size_t out_stride);
int qrl_m17_call_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls, const uint8_t* payloads, const uint32_t* first, size_t batch, size_t n,
                        uint8_t* out, size_t out_stride, size_t slot_bytes);
int qrl_m17_call_end(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls, const uint32_t* first, size_t batch, uint8_t* out, size_t out_stride);
/* DMR layer 2, the stateless per-burst work behind the DMO slicer's mailbox (qrl_demod_set_dmo_output): what the reference does to every
 * burst gr_dmr_dmo_sink::get_data() returns -- DMRFrame::DMRFrame (slot type, Golay(20,8)), DMRFrame::validate (reference
 * src/DMR/dmrframe.cpp:115-246: BPTC(196,96) + RS(12,9) or CRC-CCITT per data type, the rate 3/4 trellis, the burst re-encoded from the
 * corrected payload), DMRFrame::runAudioFEC (:248, CAMBEFEC::regenerateDMR) and CDMREMB::putData (QR(16,7,6), src/DMR/dmrcontrol.cpp:247).
 * records / counts are the slicer's mailbox; slot i of stream b is decoded when i < min(counts[b], cap_frames) (counts == NULL: every
 * slot), every other output slot is 80 zero bytes.  Runs behind qrl_demod_process on qrl_demod_stream() without a host synchronisation.
 * The 80-byte record (each byte = one accessor of the reference's DMRFrame after those calls; host/dmr_frame_hip.h reads it):
 *   0 frame type, 1 FN (copied) | 2 colour code (data: slot type; voice A: input byte 2; voice B-F: EMB) | 3 getDataType(): 0..15, or
 *   QRL_DMR_DT_VOICE_SYNC / QRL_DMR_DT_VOICE | 4 validate() | 5 runAudioFEC() (voice, audio_fec != 0) | 6 EMB PI, 7 EMB LCSS (voice B-F)
 *   | 8 payload length: 12 BPTC types, 18 rate 3/4, 27 voice, 0 invalid / rate 1 | 9 getFLCO(), 10 getFID(), 11 zero | 12..15 getSrcId(),
 *   16..19 getDstId(), little endian | 20..52 getData(): the regenerated burst, or the input burst where validate() returns before
 *   rewriting it | 53..79 payload, zero padded: the 12 BPTC bytes as the class keeps them after put() (masks in place), the 18 trellis
 *   bytes, or the 27 getVoice() bytes after the FEC.
 * The protocol state above this (DMRControl, the four-burst embedded LC) is qrl_dmr_rx_process, below. */
#define QRL_DMR_L2_RECORD_BYTES 80
#define QRL_DMR_DT_VOICE_SYNC 0xF0
#define QRL_DMR_DT_VOICE 0xF1
int qrl_dmr_l2_decode(qrl_ctx* ctx, void* hip_stream, const uint8_t* records /* [batch][cap_frames][40] */, const uint32_t* counts /* [batch] or NULL */,
                      size_t batch, size_t cap_frames, int audio_fec, uint8_t* out /* [batch][cap_frames][80] */);
/* CDMRTrellis::decode / encode (reference src/MMDVM/DMRTrellis.cpp:50-107) on bare bursts: the 196 code bits of a rate 3/4 burst -> 49
 * constellation points -> checkCode, and for a burst that fails it the two-go fixCode search (16 candidate points of a round in 16 lanes)
 * -> 18 payload bytes, ok = 1; a burst the search gives up on gets ok = 0 and a zero payload.  encode writes the code bits of the
 * payload into the burst and keeps its 68 middle bits. */
int qrl_dmr_trellis34_decode(qrl_ctx* ctx, void* hip_stream, const uint8_t* bursts /* [n][33] */, size_t n, uint8_t* payloads /* [n][18] */, uint8_t* ok /* [n] */);
int qrl_dmr_trellis34_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* payloads /* [n][18] */, size_t n, uint8_t* bursts /* [n][33] in/out */);
/* DMR layer 2, transmit side: the stateless per-burst work in front of the DMR modulator's bytes (QRL_MODEM_DMR), what the reference's frame
 * layer does before gr_mod_base::setDMRData -- DMRFrame::constructLCFrame / constructCSBKFrame (src/DMR/dmrframe.cpp:460-487: RS(12,9) or
 * CRC-CCITT, BPTC(196,96), slot type through Golay(20,8), data sync), CDMRDataHeader::get, CBPTC19696::encode, CDMRTrellis::encode,
 * DMRFrame::setVoice + addVoiceSync (:399-411, :498-501) and setEmbeddedData (:413-421: the fragment of the embedded LC -- seven Hamming
 * (16,11,4) rows, column parity, 5-bit checksum, column interleave -- and the EMB through QR(16,7,6)).
 * qrl_dmr_l2_encode: one 48-byte TX record per output slot.
 *   0 kind | 1 FN | 2 colour code | 3 data type (slot type; kind 1 also picks the header (1) / terminator (2) mask by it, any other value
 *   gives a zero burst) | 4..12 the nine LC bytes as CDMRLC(const unsigned char*) reads them | 13..15 zero | 16..42 payload | 43..47 zero
 *   kind 0 empty frame (33 zero bytes) | 1 full LC of bytes 4..12 | 2 CSBK, payload 10 bytes | 3 data header, 10 | 4 rate 1/2 block, 12 |
 *   5 rate 3/4 block, 18 | 7 voice A, 27 | 8 voice B-F, 27: FN 1..4 carries fragment FN of the embedded form of the LC in bytes 4..12
 *   (LCSS 1, 3, 3, 2), any other FN a null fragment with LCSS 0.  Kinds 6 and 9..255 are reserved and give 33 zero bytes.
 * qrl_dmr_voice_call_encode: the voice bursts of a call from a 40-byte call descriptor and the codec frames.  Slot i of stream b is voice
 * burst k = first[b] + i of its call: FN = k mod 6 (0 = voice A), superframe (k div 6) mod 5 carries the call's LC, then the talker-alias
 * header and blocks 1..3, exactly as DMRControl::getTxAudio rotates them (src/DMR/dmrcontrol.cpp:128-223); a function of k alone, so a
 * call may be cut into calls of any length.  Descriptor: 0..2 source id, 3..5 destination id (high byte first) | 6 FLCO | 7 FID |
 * 8 colour code | 9..35 talker alias, zero padded | 36..39 zero.
 * Output: slot i of stream b at out + b * out_stride + i * slot_bytes: the 33-byte burst, then zeros up to slot_bytes (slot_bytes = 72:
 * the 39 idle bytes gr_dmr_source appends, rows qrl_mod_process takes as they are).  Slots i >= min(counts[b], cap_frames) are slot_bytes
 * zeros (counts == NULL: every slot holds a record).  Bytes of a row behind cap_frames * slot_bytes are not written.  Stateless,
 * asynchronous on hip_stream.  QRL_ERR_ARG: a null pointer, an empty batch, slot_bytes < 33, out_stride < cap_frames * slot_bytes.
 * CACH, the slot timing, rate 1 data and the CRCs of data messages stay host work. */
#define QRL_DMR_TX_RECORD_BYTES 48
#define QRL_DMR_CALL_BYTES 40
int qrl_dmr_l2_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* records /* [batch][cap_frames][48] */, const uint32_t* counts /* [batch] or NULL */,
                      size_t batch, size_t cap_frames, uint8_t* out, size_t out_stride /* bytes per stream */, size_t slot_bytes /* >= 33 */);
int qrl_dmr_voice_call_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls /* [batch][40] */, const uint8_t* voice /* [batch][n][27] */,
                              const uint32_t* first /* [batch]: absolute index of voice[b][0] in its call, or NULL = 0 */, size_t batch, size_t n,
                              uint8_t* out, size_t out_stride, size_t slot_bytes);

/* DMR receive call layer: the per-stream protocol state above layer 2, the receive half of the reference's DMRControl in DMO mode with an
 * idle transmitter (src/DMR/dmrcontrol.cpp: addFrames :625-665, processVoiceHeader / processTerminator / processDataHeader / processCSBK /
 * processAudio, processColorCode, processEmbeddedData, the completion rule of processTalkerAlias) and CDMREmbeddedData's receive side
 * (src/MMDVM/DMREmbeddedData.cpp:47-109, :213-322: the LCSS state machine, the column de-interleave, seven Hamming (16,11,4) rows with
 * single-error correction, the column parity, the 5-bit checksum).  The receive counterpart of qrl_dmr_voice_call_encode: a handle keeps the
 * state of `batch` streams on the device between calls; qrl_dmr_rx_process walks, per stream, slots i < min(counts[b], cap_frames) of the
 * records qrl_dmr_l2_decode wrote (counts == NULL: every slot), in order, and writes one 128-byte record per slot; every other output slot is
 * 128 zero bytes.  It runs behind qrl_dmr_l2_decode on the same HIP stream with no host synchronisation; the calls of one handle must be
 * ordered by the caller (one stream, or events).  The reference is reproduced as it stands: without promiscuous mode a burst of another
 * colour code is refused whatever its type; a voice burst is checked with _color_code_RX, not its own colour code, so late entry works in
 * promiscuous mode and, with a fixed colour code other than 0, only behind a header; a terminator with source and destination 0 is passed over.
 * The output record (nothing is compacted: slot i answers slot i of the layer-2 records):
 *   0..1 flags, little endian: QRL_DMR_RX_VALID the burst passed validate() | _PROCESSED its process* call returned true (also set for a
 *   valid burst addFrames has no call for) | _HEADER_VOICE, _HEADER_DATA headerReceived fired | _TERMINATOR terminatorReceived | _END_BEEP
 *   endBeep | _AUDIO digitalAudio: the 27 codec bytes are bytes 53..79 of the layer-2 record of the same slot | _EMBEDDED an embedded LC
 *   completed and was valid, processEmbeddedData ran | _TALKER_ALIAS talkerAlias fired | _GPS gpsInfo fired | _UNKNOWN_FLCO an embedded FLCO
 *   the reference only logs
 *   | 2 receiver state after the burst (RECEIVER_STATE: 0 idle, 1 late entry, 2 audio, 3 data) | 3 _color_code_RX | 4 _FLCO_RX | 5 _timeslot_RX | 6..7 zero
 *   | 8..11 _srcId_RX, 12..15 _dstId_RX, little endian
 *   | 16 FLCO of the embedded LC, 17..25 its nine getRawData bytes (with _EMBEDDED, else zero)
 *   | 26 talker-alias format (0 7-bit, 1 ISO 8-bit, 2 UTF-8, 3 UTF-16BE), 27 its length field, 28 the number of bytes collected (at most 68:
 *   blocks are only appended to an incomplete alias, and the largest need is 2 x 31), 32..99 those bytes: the header's six (format 0: first
 *   the low bit of its options byte, as a byte), then seven per block (with _TALKER_ALIAS, else zero) | 29..31, 100..127 zero.
 * Turning the alias bytes into text, the GPS arithmetic of CUtils::extractGPSPosition and the signals' HTML strings stay host work
 * (host/dmr_frame_hip.h), as do the data messages of dmrmessagehandler, the short LC of the CACH (CDMRShortLC has no user in the
 * reference) and trunked mode.
 * Repeater mode (dmr_mode != DMR_MODE_DMO): qrl_dmr_rx_set_mode(h, QRL_DMR_MODE_REPEATER, timeslot 1 or 2) from the next process call on; a
 * fresh handle is in DMO mode.  qrl_dmr_rx_process_slots takes, beside the layer-2 records, the slot records [batch][cap_frames][16] of
 * qrl_dmr_sink_process for the same slots and adds what dmrcontrol.cpp does outside DMO mode: addFrames passes over a burst whose CACH
 * was not decoded (:636-640) and one of the other timeslot unless promiscuous (:641-644); every process* call runs processTimeslot
 * (:444-462), which in promiscuous mode locks _timeslot_RX to the first slot seen until processTerminator releases it (:373).  The order
 * of the checks is the reference's: processAudio asks the timeslot before the colour code (:227-230), the other calls the colour code
 * first (:275-278 ...), and each check takes its lock before the other refuses the burst.  qrl_dmr_rx_process works in either mode: with
 * no slot records every burst reads as cachDecoded() == false, slot 0.  Byte 5 of the output record and byte 3 of the public state carry
 * _timeslot_RX (0 in DMO mode); QRL_DMR_RX_SLOT_REFUSED: the burst was dropped by one of the CACH or timeslot rules (then _PROCESSED is not set).
 * qrl_dmr_rx_set_mode: mode outside 0..1, or a repeater-mode timeslot outside 1..2, is QRL_ERR_ARG; the timeslot is ignored in DMO mode.
 * qrl_dmr_rx_process_slots: batch must be the handle's.  The transmitter stays idle.
 * qrl_dmr_rx_create: config = colour code 0..15 and promiscuous 0 / 1, anything else QRL_ERR_ARG.  _set_config: from the next
 * qrl_dmr_rx_process on.  _reset: every stream back to a fresh handle's state, asynchronous on hip_stream.  _process: out 16-byte aligned;
 * a null pointer or cap_frames == 0 is QRL_ERR_ARG before any device work.  _get_state: the public 12 bytes per stream (0 receiver state,
 * 1 _color_code_RX, 2 _FLCO_RX, 3 _timeslot_RX, 4..7 source, 8..11 destination, little endian), out 4-byte aligned, asynchronous on hip_stream. */
#define QRL_DMR_RX_RECORD_BYTES 128
#define QRL_DMR_RX_STATE_BYTES 12
#define QRL_DMR_RX_VALID 0x0001
#define QRL_DMR_RX_PROCESSED 0x0002
#define QRL_DMR_RX_HEADER_VOICE 0x0004
#define QRL_DMR_RX_HEADER_DATA 0x0008
#define QRL_DMR_RX_TERMINATOR 0x0010
#define QRL_DMR_RX_END_BEEP 0x0020
#define QRL_DMR_RX_AUDIO 0x0040
#define QRL_DMR_RX_EMBEDDED 0x0080
#define QRL_DMR_RX_TALKER_ALIAS 0x0100
#define QRL_DMR_RX_GPS 0x0200
#define QRL_DMR_RX_UNKNOWN_FLCO 0x0400
#define QRL_DMR_RX_SLOT_REFUSED 0x0800
#define QRL_DMR_MODE_REPEATER 0
#define QRL_DMR_MODE_DMO 1
typedef struct qrl_dmr_rx qrl_dmr_rx;
typedef struct qrl_dmr_rx_config { int color_code; int promiscuous; } qrl_dmr_rx_config;
int qrl_dmr_rx_create(qrl_ctx* ctx, size_t batch, const qrl_dmr_rx_config* config, qrl_dmr_rx** out);
void qrl_dmr_rx_destroy(qrl_dmr_rx* h);
int qrl_dmr_rx_reset(qrl_dmr_rx* h, void* hip_stream);
int qrl_dmr_rx_set_config(qrl_dmr_rx* h, const qrl_dmr_rx_config* config);
int qrl_dmr_rx_process(qrl_dmr_rx* h, void* hip_stream, const uint8_t* l2_records /* [batch][cap_frames][80] */, const uint32_t* counts /* [batch] or NULL */,
                       size_t cap_frames, uint8_t* out /* [batch][cap_frames][128] */);
int qrl_dmr_rx_get_state(qrl_dmr_rx* h, void* hip_stream, uint8_t* out /* [batch][12], device */);
int qrl_dmr_rx_set_mode(qrl_dmr_rx* h, int mode, int timeslot /* 1 or 2; ignored in DMO mode */);
int qrl_dmr_rx_process_slots(qrl_dmr_rx* h, void* hip_stream, const uint8_t* l2_records, const uint8_t* slot_info /* [batch][cap_frames][16] */,
                             const uint32_t* counts, size_t batch, size_t cap_frames, uint8_t* out);

/* ---- DMR repeater-mode burst sink (reference src/gr/gr_dmr_sink.cpp; gr_demod_base connects it to port 2 of gr_demod_dmr, src/gr/gr_demod_base.cpp:814,
 * and getDMRData(false) returns its frames, :947-966) -------------------------------------------------------------------------------------
 * The sink behind a repeater's downlink: BS- and MS-sourced sync on the hard bits, the 24-bit CACH in front of every burst, two
 * alternating slot contexts.  A handle shaped like qrl_deframer_*: qrl_dmr_sink_process consumes the unpacked bits of one demodulator
 * port (bits[b*stride + i]; i < n, or i < min(n, counts[b*count_stride]) when counts != NULL: the demodulator's counts + 2 with count_stride 4
 * for port 2) and the state is carried from call to call on the device.  gr_dmr_sink::work / processBits / findSync (:79-260) as they
 * stand: a bit goes only to the context _next_slot, which changes hands after each burst emitted (a context waiting for sync keeps the
 * other one's voice call waiting); the four 48-bit sync words of src/DMR/constants.h:9-12 match on equality only (errs < 1, :207-218);
 * a sync found with fewer than DATA_AND_SYNC_BITS = 180 buffered bits clears the context (:238-245); 108 more bits make a data or
 * voice-sync burst (:88-110), and the five 288-bit bursts behind a voice sync get FN 1..5 (setFN(6 - frames_to_receive), :113-131).
 * The erase at work()'s entry (:163-169) cannot change a result and is not run (qradiolink_amd/csrc/dmr_sink_core.hpp says why).
 * frames [batch][cap_frames][40]: the DMO sink's record, so qrl_dmr_l2_decode takes the array as it is: 0 DMRFrameType (0 data, 1 voice,
 *   2 voice sync) | 1 FN | 2, 3 zero | 4..36 the 33 frame bytes, DMRFrame::packFrame of bits 24..287 (src/DMR/dmrframe.cpp:58-63, :370-384)
 *   | 37..39 zero.
 * slot_info [batch][cap_frames][16]: what DMRFrame(bits, type) + setDownlink() leave (src/DMR/dmrframe.cpp:255-288): 0 downlink (a BS-sourced
 *   sync) | 1 cachDecoded() | 2 getSlotNo() 0, 1, 2 | 3 LCSS | 4 AT | 5..7 the three CACH bytes | 8..15 end_bit, u64 little endian: the
 *   number of bits the stream has consumed since creation or reset, up to and including the bit that completed the burst.  The TACT
 *   bits sit at CACH bits 0 (AT), 4 (TC), 8, 12 (LCSS), the Hamming (7,4) parity at 14, 18, 22; a parity mismatch or an MS-sourced sync
 *   leaves cachDecoded 0, slot 0, LCSS 0, AT 0.
 * out_counts[b]: the number of bursts the call found; nothing is written past cap_frames, so out_counts[b] > cap_frames says that bursts
 * were dropped, as with the DMO mailbox.  Slots behind the count are left as they were.
 * _reset: a fresh handle's state.  _flush: gr_dmr_sink::flush() (:55-60): only the two bit buffers, the state machines untouched; in the
 * middle of a data burst the reference then reads past the end of its buffer, here the missing bits read as zero.
 * _process: frames 8-byte aligned, slot_info 16-byte aligned, n <= stride (whatever the batch), else QRL_ERR_ARG; n > 2^32 - 129 is QRL_ERR_TOO_BIG;
 * a null pointer or cap_frames == 0 is QRL_ERR_ARG before any device work.
 * All pointers are device pointers; asynchronous on the handle's stream (give it the demodulator's stream to chain).
 * Python hands the slot records to the call layer through DmrRx.process_slots(l2, slot_info, ...), a method of its own beside DmrRx.process(),
 * whose parameter list stays what it was.
 * Still host work: the short LC carried by the CACH payload (CDMRShortLC has no user in the reference), dmrmessagehandler, trunked mode. */
#define QRL_DMR_SINK_FRAME_BYTES 40
#define QRL_DMR_SINK_INFO_BYTES 16
typedef struct qrl_dmr_sink qrl_dmr_sink;
int qrl_dmr_sink_create(qrl_ctx* ctx, int batch, void* hip_stream, qrl_dmr_sink** out);
void qrl_dmr_sink_destroy(qrl_dmr_sink* h);
int qrl_dmr_sink_reset(qrl_dmr_sink* h);
int qrl_dmr_sink_flush(qrl_dmr_sink* h);
int qrl_dmr_sink_process(qrl_dmr_sink* h, const uint8_t* bits, size_t stride, size_t n, const uint32_t* counts, size_t count_stride,
                         uint8_t* frames /* [batch][cap_frames][40] */, uint8_t* slot_info /* [batch][cap_frames][16] */, size_t cap_frames,
                         uint32_t* out_counts /* [batch] */);
int qrl_dmr_sink_sync(qrl_dmr_sink* h);

/* ---- developer aids (NOT part of the drop-in surface; tools/prof_phases.py): shader-clock phase profile of k_decim_mfma ---- */
void qrl_debug_decim_prof(unsigned long long* out8);
void qrl_debug_decim_prof_enable(int on);

#ifdef __cplusplus
}
#endif
#endif
