"""The profile events of the receiver and the channelizer handle (qrl_demod_profile*, qrl_chan_profile*): what a read returns, that a read
empties what it read, what reset() and a switched-off profile leave, and handles that are closed with unread events.  bench.py takes every
headline figure through these calls.  The expected counts and kernel names are those of the library before the handles' events and
streams became owning members; the calls are tiny (batch 2, noise in): nothing here looks at the demodulated data except the last test,
which compares two runs of the same handle types with each other."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 2
RX_CHUNK = 1024          # samples per receiver call: the smallest max_chunk the suite gives a receiver
CH_M, CH_CHUNK = 10, 10 * 25   # channelizer: 25 channel-rate instants per call, the smallest chunk of tests/test_gpu_chan.py


def _noise(n, seed):
    import torch
    rng = np.random.default_rng(seed)
    x = 0.05 * (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n)))
    return torch.from_numpy(x.astype(np.complex64)).cuda()


def _calls(h, x, chunk, k):
    for i in range(k):
        h.process_async(x[:, i * chunk:(i + 1) * chunk])
    return k


@pytest.mark.parametrize("rate,kernel", [(1000000, "k_resamp"), (2000000, "k_decim")])
def test_receiver_profile_reads(qrl_ctx, rate, kernel):
    import qradiolink_amd as q
    x = _noise(8 * RX_CHUNK, seed=rate // 1000000)
    dem = q.Demod(qrl_ctx, q.MODEM_GMSK10K, batch=B, max_chunk=RX_CHUNK, device_samp_rate=rate)
    try:
        dem.profile(True)
        _calls(dem, x, RX_CHUNK, 3)
        ms, n, name = dem.profile_read()
        print("rate %d: %d launches, %.6f ms, %s" % (rate, n, ms, name))
        assert n == 3 and ms > 0 and name == kernel
        assert dem.profile_read()[:2] == (0.0, 0)          # the read emptied the set
        dem.profile(False)
        _calls(dem, x[:, 3 * RX_CHUNK:], RX_CHUNK, 3)
        assert dem.profile_read()[:2] == (0.0, 0)          # nothing is timed while the profile is off
        dem.profile(True)
        _calls(dem, x[:, 6 * RX_CHUNK:], RX_CHUNK, 2)
        dem.reset()                                        # reset() leaves the events of the calls before it to the next read
        ms, n, name = dem.profile_read()
        print("rate %d after reset: %d launches, %.6f ms, %s" % (rate, n, ms, name))
        assert n == 2 and ms > 0 and name == kernel
    finally:
        dem.close()


def test_channelizer_profile_reads(qrl_ctx):
    import qradiolink_amd as q
    x = _noise(6 * CH_CHUNK, seed=7)
    ch = q.Channelizer(qrl_ctx, CH_M, batch=B, max_chunk=CH_CHUNK)
    try:
        ch.enable_4fsk()
        ch.profile(True)
        _calls(ch, x, CH_CHUNK, 3)
        got = ch.profile_read_kernels()
        print(got)
        assert [k for k, _, _ in got] == ["channelizer", "k_chan_tail", "k_symsync_ff"]
        assert [n for _, _, n in got] == [3, 3, 3]
        assert all(ms > 0 for _, ms, n in got if n)
        assert [(ms, n) for _, ms, n in ch.profile_read_kernels()] == [(0.0, 0)] * 3
        _calls(ch, x[:, 3 * CH_CHUNK:], CH_CHUNK, 3)
        ms, n, name = ch.profile_read()                    # reads the channelizer's set and drops the other two unread
        print(ms, n, name)
        assert n == 3 and ms > 0 and name == "k_pfb_chan"
        assert [(ms, n) for _, ms, n in ch.profile_read_kernels()] == [(0.0, 0)] * 3
    finally:
        ch.close()


def test_handles_closed_with_unread_profile_events(qrl_ctx):
    """Twenty rounds of: a receiver and a channelizer, two profiled calls on each, on odd rounds a torch side stream made to wait for both,
    both closed with their events unread.  Every library call returns QRL_OK (the wrappers raise on anything else) and the last round's
    outputs are the first round's."""
    import torch
    import qradiolink_amd as q
    xr, xc = _noise(2 * RX_CHUNK, seed=11), _noise(2 * CH_CHUNK, seed=12)
    side = torch.cuda.Stream()
    rounds = []
    for r in range(20):
        dem = q.Demod(qrl_ctx, q.MODEM_GMSK10K, batch=B, max_chunk=RX_CHUNK, device_samp_rate=2000000)
        ch = q.Channelizer(qrl_ctx, CH_M, batch=B, max_chunk=CH_CHUNK)
        try:
            ch.enable_4fsk()
            dem.profile(True)
            ch.profile(True)
            _calls(dem, xr, RX_CHUNK, 2)
            _calls(ch, xc, CH_CHUNK, 2)
            if r & 1:
                dem.stream_wait(side.cuda_stream)
                ch.stream_wait(side.cuda_stream)
                side.synchronize()
            dem.sync()
            ch.sync()
            if r in (0, 19):
                rounds.append([t.cpu().numpy().copy() for t in (dem.bits_a, dem.bits_b, dem.counts, dem.filtered, ch.out, ch.counts, ch.dibits, ch.fsk_counts)])
        finally:
            dem.close()
            ch.close()
    for a, b in zip(*rounds):
        assert a.tobytes() == b.tobytes()
    assert rounds[0][2].any() and rounds[0][5].any()       # the calls delivered something
