// tx_common.cpp — the gr_mod_base back end and the zero-run device step of the transmitters (tx_common.hpp).
#include "tx_common.hpp"
#include "firdes.hpp"
#include <cmath>

namespace qrl {

std::vector<float> tx_mfma_taps(const std::vector<float>& h, int interp)
{
    const int tiles = (interp + kTxMfmaPhases - 1) / kTxMfmaPhases;
    std::vector<float> lay((size_t)tiles * kTxMfmaLags * kTxMfmaPhases, 0.0f);
    for (size_t k = 0; k < h.size(); ++k) {
        const size_t ph = k % (size_t)interp, j = k / (size_t)interp;
        lay[((ph / kTxMfmaPhases) * kTxMfmaLags + j) * kTxMfmaPhases + ph % kTxMfmaPhases] = h[k];
    }
    return lay;
}

int TxBackEnd::init(const char* who, const char* noun, int rate, double offset_hz, int batch, size_t stride)
{
    noun_ = noun;
    if (rate != 0 && rate != 1000000 && (rate < 2000000 || rate % 1000000 != 0 || rate > kTxMaxRate))
        return qrl_set_error(QRL_ERR_ARG, std::string(who) + ": device_samp_rate must be 1e6 or a multiple of 1e6 in [2e6, 183e6]");
    interp_ = rate >= 2000000 ? rate / 1000000 : 1;
    on_ = interp_ > 1 || offset_hz != 0.0;
    if (!on_) return QRL_OK;
    // the interpolator's output count of a call (n1 * interp) and its ring mask (n1 + the filter's history, to a power of two) are 32-bit
    if (interp_ > 1 && ((uint64_t)stride + 1024) * (uint64_t)interp_ >= (1ull << 32))
        return qrl_set_error(QRL_ERR_TOO_BIG, std::string(who) + ": the largest call would produce " + std::to_string(stride) + " x " + std::to_string(interp_) +
                             " device-rate samples per stream, which with the filter's history reaches 2^32 (output counts are 32-bit): lower the per-call maximum");
    int r;
    bb_stride = stride;
    if ((r = bb.alloc((size_t)batch * bb_stride)) || (r = rot.init(phase_inc_to_turn(2 * M_PI * offset_hz / 1000000.0)))) return r;
    if (interp_ > 1) {
        const std::vector<float> lp = low_pass(interp_, rate, 480000, 20000, WIN_BLACKMAN_HARRIS);
        nt = (int)lp.size();
        mfma_ = interp_ >= kTxMfmaMinInterp;
        if (mfma_ && (nt + interp_ - 1) / interp_ > kTxMfmaLags)
            return qrl_set_error(QRL_ERR_ARG, std::string(who) + ": back-end filter longer than " + std::to_string(kTxMfmaLags) + " taps per phase");
        if ((r = taps.upload(mfma_ ? tx_mfma_taps(lp, interp_) : lp, kTapPad))) return r;
        mask = pow2_at_least(bb_stride + (size_t)nt / interp_ + 64, 1024) - 1;
        if ((r = ring.alloc((size_t)batch * (mask + 1)))) return r;
    }
    return QRL_OK;
}
int TxBackEnd::reset(hipStream_t s)
{
    if (ring.p) if (int r = ring.zero()) return r;
    n_bb = 0;
    return rot.reset(s);
}
int TxBackEnd::retune(double hz, hipStream_t s)
{
    if (!on_) return refuse();
    HIPCHK(hipStreamSynchronize(s));   // rot_lo is rewritten below
    return rot.retune(n_bb, phase_inc_to_turn(2 * M_PI * hz / 1000000.0), s);
}
int TxBackEnd::retune_streams(const double* hz, int batch, hipStream_t s)
{
    if (!on_) return refuse();
    std::vector<uint64_t> ni;
    if (int r = carrier_incs(hz, batch, 1.0, 1000000.0, ni)) return r;
    HIPCHK(hipStreamSynchronize(s));
    return rot.retune_streams(n_bb, ni, s);
}
void TxBackEnd::run(uint32_t n1, void* iq, size_t out_stride, TxOut sc, int batch, hipStream_t s)
{
    if (!on_ || !n1) return;
    TxRotParams rp{}; rp.in = bb.p; rp.in_stride = bb_stride; rp.n0 = n_bb; rp.count = n1;
    rot.fill(rp);
    if (interp_ > 1) rp.out_ring = RingC{ring.p, mask};
    else { rp.out = reinterpret_cast<float2*>(iq); rp.out_stride = out_stride; rp.sc = sc; }
    launch_tx_rot(rp, batch, s);
    if (mfma_) {
        TxInterpMfmaParams mp{}; mp.in = rp.out_ring; mp.n0 = n_bb; mp.n1 = n1; mp.taps = taps.p; mp.interp = interp_;
        mp.out = reinterpret_cast<float2*>(iq); mp.out_stride = out_stride; mp.sc = sc;
        launch_tx_interp_mfma(mp, batch, s);
    } else if (interp_ > 1) {
        TxInterpCParams bp{}; bp.in = rp.out_ring; bp.n0 = n_bb * (uint64_t)interp_; bp.count = n1 * (uint32_t)interp_;
        bp.taps = taps.p; bp.nt = nt; bp.interp = interp_;
        bp.out = reinterpret_cast<float2*>(iq); bp.out_stride = out_stride; bp.sc = sc;
        launch_tx_interp_c(bp, batch, s);
    }
    n_bb += n1;
}

int ZeroRuns::apply(RingC r, uint64_t lo, uint64_t hi, hipStream_t s)
{
    if (runs.empty()) return QRL_OK;
    std::vector<ZeroRun> live;
    split(lo, hi, live);
    if (live.empty()) return QRL_OK;
    if (live.size() > dev.n) {   // the previous call's launch_zero_runs may still read the old copy
        HIPCHK(hipStreamSynchronize(s));
        if (int rz = dev.grow(live.size() * 2)) return rz;
    }
    HIPCHK(hipMemcpyAsync(dev.p, live.data(), live.size() * sizeof(ZeroRun), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // `live` is pageable host memory: the copy has left it
    launch_zero_runs(r, dev.p, (uint32_t)live.size(), lo, hi, s);
    return QRL_OK;
}

}  // namespace qrl
