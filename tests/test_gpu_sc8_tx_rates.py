"""sc8 output behind the gr_mod_base back end at 2, 3, 4, 33 and 183 Msps: k_tx_interp_c on both sides of the dispatch threshold, the smallest
k_tx_interp_mfma shape, a second phase tile of one phase, and six tiles with a 23-phase last tile -- in the ragged CUTS of tests/test_gpu_tx_rates.py
(calls of 32, 224, 96 and 1280 samples at 1 Msps: blocks of 128 ring samples with one, three and four live waves), at a bb_gain under which components clip, counts exact.  And a
loopback in the format: TX sc8 at 8 Msps (GMSK-10k) -> the same int8 buffer into Demod.process_sc8 at 8 Msps."""
import numpy as np
import pytest

import sc8_output_cases as K
import test_gpu_tx_rates as R
from sc8_output_cases import B, conv8
from test_gpu_front_end_rates import _same_as_oracle

pytestmark = pytest.mark.gpu

RATES = [2000000, 3000000, 4000000, 33000000, 183000000]
SENTINEL = 0x5A


def _buffer(torch, count):
    buf = torch.full((B, count + 3 + count % 2, 2), SENTINEL, dtype=torch.int8, device="cuda")
    assert buf.stride(0) % 4 == 2                                     # odd pitch: row 1 starts at an address = 2 mod 4
    return buf


@pytest.mark.parametrize("rate", RATES, ids=["%dM" % (r // 1000000) for r in RATES])
def test_sc8_output_and_clip_counts_at_rate(qrl_ctx, rate):
    """process_sc8 against rint(ref * scale) saturated, bb_gain 4: rows exact, nothing behind them, counts exact per stream and summed over the calls"""
    import torch
    import qradiolink_amd as q
    I = rate // 1000000
    refs = R._ref(rate, 4.0)
    e = np.cumsum([0] + R.CUTS) * 32 * I
    parts = [[x[e[i]:e[i + 1]] for x in refs] for i in range(len(R.CUTS))]
    K.saturation_preconditions(refs)
    d = torch.from_numpy(np.array(R._payloads())).cuda()
    mod = q.Mod(qrl_ctx, R.QPSK250K, batch=B, max_bytes=max(R.CUTS), device_samp_rate=rate, carrier_offset_hz=R.OFFSET)
    mod.set_bb_gain(4.0)
    clip = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mod.set_sc8_clip_counts(clip)
    total, pos = [0] * B, 0
    for i, c in enumerate(R.CUTS):
        buf = _buffer(torch, parts[i][0].size)
        view = mod.process_sc8(d[:, pos:pos + c].contiguous(), out=buf)
        pos += c
        host = buf.cpu().numpy()
        for b in range(B):
            want, nclip = conv8(parts[i][b])
            assert view.shape[1] == want.shape[0]
            assert np.array_equal(host[b, :want.shape[0]], want), "%d Msps, call %d, stream %d differs from the converted oracle output" % (I, i, b)
            assert np.all(host[b, want.shape[0]:] == SENTINEL), "%d Msps, call %d, stream %d: written behind its samples" % (I, i, b)
            total[b] += nclip
        assert clip.cpu().numpy().tolist() == total, "call %d: clip counters" % i
    assert all(n > 0 for n in total)
    mod.close()


def test_tx_sc8_into_rx_sc8_at_8_msps(qrl_ctx):
    """the transmitter's int8 rows, laid out as the receiver demands (16-byte base, pitch a multiple of 8 samples), go into Demod.process_sc8 as they
    are: the transmitter's samples are the converted oracle's, every receiver output is bit for bit the oracle's for the floats (float)v / 128, and the
    sent payloads come back"""
    import torch
    import qradiolink_amd as q
    data, payloads, codes, rx = K.loopback()
    count = codes[0].shape[0]
    pitch = (count + 8 + 7) // 8 * 8
    buf = torch.full((B, pitch, 2), SENTINEL, dtype=torch.int8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and count % 8 == 0 and pitch > count
    mod = q.Mod(qrl_ctx, K.GMSK10K, batch=B, max_bytes=data.shape[1], device_samp_rate=K.LOOP_RATE, carrier_offset_hz=K.LOOP_OFFSET)
    view = mod.process_sc8(torch.from_numpy(np.array(data)).cuda(), out=buf)
    mod.close()
    assert view.shape == (B, count, 2)
    host = buf.cpu().numpy()
    for b in range(B):
        assert np.array_equal(host[b, :count], codes[b]), "TX stream %d differs from the converted oracle output" % b
        assert np.all(host[b, count:] == SENTINEL)
    dem = q.Demod(qrl_ctx, K.GMSK10K, batch=B, max_chunk=count, device_samp_rate=K.LOOP_RATE, carrier_offset_hz=K.LOOP_OFFSET)
    out = dem.process_sc8(buf.view(B, 2 * pitch)[:, :2 * count])
    cnt = out["counts"].cpu().numpy()
    ports = {}
    for j, name in enumerate(("filtered", "constellation", "bits_a", "bits_b")):
        h = out[name].cpu().numpy()
        ports[name] = [h[b, :cnt[b, j]].copy() for b in range(B)]
    dem.close()
    _same_as_oracle(ports, rx)
    for b in range(B):
        assert K.recovered(ports["bits_a"][b], ports["bits_b"][b], payloads[b]), "stream %d: the sent payloads did not come back" % b
