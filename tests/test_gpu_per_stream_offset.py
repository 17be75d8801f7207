"""Per-stream carrier offsets (qrl_*_set_carrier_offsets) on the GPU against the CPU oracle: every stream of a handle with its own
rotator_cc increment and phase, bit-exact with orc.frontend(x_b, rate, offset_b) -- or with orc.rotator piecewise where a stream is retuned --
behind every front-end geometry, cut into calls, on the TX back ends, and at a batch of many workgroups."""
import numpy as np
import pytest

import orc
import sig
from test_gpu_parity import PARITY_LIST, _compare, _oracle

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


def _offsets(rate):
    """Four distinct offsets, 0 and both signs included."""
    return [25000.0, 0.0, -18750.0, 9300.0] if rate >= 2000000 else [1200.0, 0.0, -1150.0, 640.0]


def _streams(mode_name, rate, offsets, nframes=2, seed=3, impair=None):
    ss = [sig.make_stream(mode_name, nframes, rate, rx_offset_hz=f, seed=seed + 101 * b, lead=37 * b, impair=impair)[0] for b, f in enumerate(offsets)]
    n = min(s.size for s in ss) & ~1
    return np.stack([s[:n] for s in ss]).astype(np.complex64)


def _run(qrl_ctx, modem, rate, offsets, iq, chunk, first_offset=0.0):
    import torch
    import qradiolink_amd as q
    dem = q.Demod(qrl_ctx, modem, batch=iq.shape[0], max_chunk=chunk, device_samp_rate=rate, carrier_offset_hz=first_offset)
    dem.set_carrier_offsets(offsets)
    out = q.collect(dem, torch.from_numpy(iq).cuda(), chunk)
    dem.close()
    return out


def _compare_each(iq, out, mode_name, rate, offsets):
    for b, f in enumerate(offsets):
        _compare(iq[b:b + 1], {k: [v[b]] for k, v in out.items()}, mode_name, rate, f)


@pytest.mark.parametrize("mode_name,modem,rate,chunk", PARITY_LIST)
def test_distinct_offsets_every_front_end(qrl_ctx, mode_name, modem, rate, chunk):
    offsets = _offsets(rate)
    iq = _streams(mode_name, rate, offsets)
    out = _run(qrl_ctx, modem, rate, offsets, iq, chunk, first_offset=offsets[0])
    _compare_each(iq, out, mode_name, rate, offsets)


@pytest.mark.parametrize("mode_name,modem,rate,chunk", [
    ("2fsk1k", 18, 1000000, 50000), ("gmsk10k", 22, 1000000, 30000), ("gmsk10k", 22, 25000000, 750000), ("gmsk1k", 21, 2000000, 100002),
    ("qpsk250k", 26, 100000000, 3000000), ("qpsk2k", 7, 1000000, 60000), ("4fsk10kfm", 4, 4000000, 200000), ("4fsk100k", 27, 1000000, 30000),
])
def test_distinct_offsets_cut_into_calls(qrl_ctx, mode_name, modem, rate, chunk):
    """The carried history (k_hist) and the edge units / edge scratch of the front ends, per stream."""
    offsets = _offsets(rate)
    iq = _streams(mode_name, rate, offsets, seed=6, impair=sig.SPEC)
    out = _run(qrl_ctx, modem, rate, offsets, iq, chunk)
    _compare_each(iq, out, mode_name, rate, offsets)


def _retune_run(qrl_ctx, modem, rate, iq, n1, first, second, scalar=False, per_call=None):
    """Process iq[:, :n1] with per-stream offsets `first`, then set `second` (a list, or a float through the scalar setter) and process the rest."""
    import torch
    import qradiolink_amd as q
    B = iq.shape[0]
    dem = q.Demod(qrl_ctx, modem, batch=B, max_chunk=iq.shape[1], device_samp_rate=rate)
    dem.set_carrier_offsets(first)
    d = torch.from_numpy(iq).cuda()
    parts = []
    for lo, hi, f in ((0, n1, None), (n1, iq.shape[1], second)):
        if f is not None:
            dem.set_carrier_offset(f) if scalar else dem.set_carrier_offsets(f)
        o = dem.process(d[:, lo:hi].contiguous())
        c = o["counts"].cpu().numpy()
        parts.append({k: [o[k][b, :c[b, j]].cpu().numpy().copy() for b in range(B)] for k, j in (("filtered", 0), ("bits_a", 2))})
    dem.close()
    return parts


def _check_piecewise(parts, iq, mode_name, rate, n1, first, second):
    for b in range(iq.shape[0]):
        inc1 = orc.phase_inc_to_turn(2 * np.pi * -first[b] / rate)
        inc2 = orc.phase_inc_to_turn(2 * np.pi * -second[b] / rate)
        y = np.concatenate([orc.rotator(iq[b, :n1], inc1, 0), orc.rotator(iq[b, n1:], inc2, (n1 * inc1) & M64)])
        ref = _oracle(mode_name, y, rate, 0.0)   # offset 0: the oracle front end's phasor is exactly (1, 0)
        got_f = np.concatenate([p["filtered"][b] for p in parts]).view(np.float32) + np.float32(0)
        got_a = np.concatenate([p["bits_a"][b] for p in parts])
        assert np.array_equal(got_f.view(np.uint32), (ref["filtered"].view(np.float32) + np.float32(0)).view(np.uint32)), "stream %d" % b
        assert got_a.size == ref["bits_a"].size and np.array_equal(got_a, ref["bits_a"]), "stream %d" % b


@pytest.mark.parametrize("mode_name,modem,rate", [("2fsk1k", 18, 1000000), ("gmsk10k", 22, 25000000), ("qpsk250k", 26, 100000000), ("gmsk10k", 22, 4000000)])
def test_retune_of_a_subset_is_phase_continuous(qrl_ctx, mode_name, modem, rate):
    """Streams 0 and 2 get new offsets mid-stream, 1 and 3 keep theirs: each stream equals the oracle on its piecewise-rotated input."""
    first = _offsets(rate)
    second = list(first)
    second[0], second[2] = (-800.0, 300.0) if rate < 2000000 else (-12500.0, 31000.0)
    iq = sig.make_batch(mode_name, 4, nframes=2, device_rate=rate, rx_offset_hz=first[0], seed=13)
    n1 = (iq.shape[1] // 3) & ~1
    parts = _retune_run(qrl_ctx, modem, rate, iq, n1, first, second)
    _check_piecewise(parts, iq, mode_name, rate, n1, first, second)


def test_equal_per_stream_offsets_match_the_scalar_setter(qrl_ctx):
    import torch
    import qradiolink_amd as q
    iq = sig.make_batch("2fsk1k", 3, nframes=2, device_rate=1000000, rx_offset_hz=1200.0, seed=21)
    d = torch.from_numpy(iq).cuda()
    outs = []
    for per_stream in (False, True):
        dem = q.Demod(qrl_ctx, 18, batch=3, max_chunk=50000, carrier_offset_hz=0.0 if per_stream else 1200.0)
        if per_stream:
            dem.set_carrier_offsets([1200.0] * 3)
        outs.append(q.collect(dem, d, 50000))
        dem.close()
    for k in ("filtered", "bits_a", "bits_b"):
        for b in range(3):
            assert np.array_equal(outs[0][k][b].view(np.uint8), outs[1][k][b].view(np.uint8)), (k, b)


@pytest.mark.parametrize("mode_name,modem,rate", [("2fsk1k", 18, 1000000), ("gmsk10k", 22, 4000000)])
def test_scalar_set_after_per_stream_keeps_each_phase(qrl_ctx, mode_name, modem, rate):
    """After per-stream offsets the scalar setter moves every stream to one offset, each from its OWN phase."""
    first = _offsets(rate)
    f2 = -700.0 if rate < 2000000 else -20000.0
    iq = sig.make_batch(mode_name, 4, nframes=2, device_rate=rate, rx_offset_hz=first[0], seed=17)
    n1 = (iq.shape[1] // 2) & ~1
    parts = _retune_run(qrl_ctx, modem, rate, iq, n1, first, f2, scalar=True)
    _check_piecewise(parts, iq, mode_name, rate, n1, first, [f2] * 4)


def test_reset_keeps_offsets_and_restarts_phases(qrl_ctx):
    import torch
    import qradiolink_amd as q
    offsets = _offsets(1000000)
    iq = _streams("2fsk1k", 1000000, offsets, seed=9)
    d = torch.from_numpy(iq).cuda()
    dem = q.Demod(qrl_ctx, 18, batch=4, max_chunk=65536)
    dem.set_carrier_offsets(offsets)
    first = q.collect(dem, d, 65536)
    dem.reset()
    again = q.collect(dem, d, 65536)
    dem.close()
    _compare_each(iq, again, "2fsk1k", 1000000, offsets)
    for k in ("filtered", "bits_a"):
        for b in range(4):
            assert np.array_equal(first[k][b].view(np.uint8), again[k][b].view(np.uint8)), (k, b)


# ---- TX: the gr_mod_base back end (rotator at 1 Msps, then the interpolator to the device rate)
@pytest.mark.parametrize("modem,nbytes,rate", [(26, 600, 4000000), (26, 300, 1000000), (22, 60, 10000000)], ids=["qpsk-4M", "qpsk-1M-rot", "gmsk10k-10M"])
def test_mod_per_stream_offsets_and_subset_retune(qrl_ctx, modem, nbytes, rate):
    import torch
    import qradiolink_amd as q
    oracle = {26: lambda x: orc.mod_qpsk(x), 22: lambda x: orc.mod_gmsk(x, sps=10, filter_width=20000)}[modem]
    first = [25000.0, 0.0, -12500.0, 40000.0]
    second = [-30000.0, 0.0, 7000.0, 40000.0]            # streams 0 and 2 retuned
    rng = np.random.default_rng(nbytes + 1)
    data = rng.integers(0, 256, (4, nbytes), dtype=np.uint8)
    cut = nbytes // 3
    mod = q.Mod(qrl_ctx, modem, batch=4, max_bytes=nbytes, device_samp_rate=rate, carrier_offset_hz=first[0])
    mod.set_carrier_offsets(first)
    d = torch.from_numpy(data).cuda()
    p1 = mod.process(d[:, :cut].contiguous()).cpu().numpy()
    mod.set_carrier_offsets(second)
    p2 = mod.process(d[:, cut:].contiguous()).cpu().numpy()
    mod.close()
    got = np.concatenate([p1, p2], axis=1)
    k = p1.shape[1] // (rate // 1000000)                  # 1 Msps samples before the retune
    for b in range(4):
        x1 = oracle(data[b])
        inc1 = orc.phase_inc_to_turn(2 * np.pi * first[b] / 1e6)
        inc2 = orc.phase_inc_to_turn(2 * np.pi * second[b] / 1e6)
        rot = np.concatenate([orc.rotator(x1[:k], inc1), orc.rotator(x1[k:], inc2, (k * inc1) & M64)])
        ref = orc.tx_interp(rot, rate) if rate != 1000000 else rot
        assert got[b].size == ref.size, (got[b].size, ref.size)
        assert np.array_equal(got[b].view(np.uint32), ref.view(np.uint32)), "stream %d differs" % b


def test_mod_without_back_end_rejects_per_stream_offsets(qrl_ctx):
    import qradiolink_amd as q
    mod = q.Mod(qrl_ctx, 26, batch=2, max_bytes=16)    # 1 Msps, offset 0: no back end
    with pytest.raises(q.QrlError):
        mod.set_carrier_offsets([100.0, 200.0])
    with pytest.raises(ValueError):
        mod.set_carrier_offsets([100.0])
    mod.close()


def test_amod_per_stream_offsets(qrl_ctx):
    import torch
    import qradiolink_amd as q
    n, rate = 1200, 4000000
    t = np.arange(n) / 8000.0
    audio = np.stack([0.6 * np.sin(2 * np.pi * (500 + 200 * b) * t) for b in range(3)]).astype(np.float32)
    first, second = [25000.0, -10000.0, 0.0], [25000.0, 15000.0, 0.0]
    mod = q.AMod(qrl_ctx, 9, batch=3, max_samples=800, bb_gain=0.75, device_samp_rate=rate)
    mod.set_carrier_offsets(first)
    p1 = mod.process(torch.from_numpy(np.ascontiguousarray(audio[:, :400])).cuda()).cpu().numpy()
    mod.set_carrier_offsets(second)
    p2 = mod.process(torch.from_numpy(np.ascontiguousarray(audio[:, 400:])).cuda()).cpu().numpy()
    mod.close()
    got = np.concatenate([p1, p2], axis=1)
    k = p1.shape[1] // (rate // 1000000)
    for b in range(3):
        x1 = orc.mod_nbfm(audio[b], filter_width=5000, bb_gain=0.75)
        inc1 = orc.phase_inc_to_turn(2 * np.pi * first[b] / 1e6)
        inc2 = orc.phase_inc_to_turn(2 * np.pi * second[b] / 1e6)
        ref = orc.tx_interp(np.concatenate([orc.rotator(x1[:k], inc1), orc.rotator(x1[k:], inc2, (k * inc1) & M64)]), rate)
        assert got[b].size == ref.size
        assert np.array_equal((got[b].view(np.float32) + np.float32(0)).view(np.uint32), (ref.view(np.float32) + np.float32(0)).view(np.uint32)), b


def test_large_batch_all_offsets_distinct(qrl_ctx):
    """B = 640 streams, every offset distinct: many workgroups of the matrix front end, edge units of several streams in one workgroup.
    Four distinct signals tiled over the batch; a sample of streams is checked against the oracle."""
    import torch
    import qradiolink_amd as q
    B = 640
    base = _streams("2fsk1k", 1000000, [1200.0, -900.0, 300.0, 0.0], nframes=1, seed=31)
    iq = np.ascontiguousarray(np.tile(base, (B // 4, 1)))
    offsets = [-1500.0 + 4.75 * b for b in range(B)]
    chunk = (iq.shape[1] // 3 + 1) & ~1
    dem = q.Demod(qrl_ctx, 18, batch=B, max_chunk=chunk)
    dem.set_carrier_offsets(offsets)
    out = q.collect(dem, torch.from_numpy(iq).cuda(), chunk)
    dem.close()
    for b in (0, 1, 2, 3, 255, 316, 317, 511, 638, 639):
        _compare(iq[b:b + 1], {k: [v[b]] for k, v in out.items()}, "2fsk1k", 1000000, offsets[b])
