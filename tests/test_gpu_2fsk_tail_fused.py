"""k_2fsk_tail, the FLL and the three FIR stages of the non-FM 2FSK chain in one kernel, against the CPU oracle on the whole stream, bit for
bit: call sizes around the kernel's 16-sample window and its 104-sample history (1, 15, 16, 17, 103, 104, 105, 0, 400 and 666 / 667
decimated samples per call), a full workgroup beside a nearly empty one, switching between the fused kernel and the unfused pair
(QRL_OPT_FLL_SLIM) from call to call -- both find their history in the r2l ring -- and the serial order of a call.

Both modes that run the kernel: 2FSK-1k (20 ksps behind the 1:50 first decimator, 10 samples per symbol) and 2FSK-2k (40 ksps behind the 1:25 one, the
same 41 / 41 / 25 tap counts with other taps, FLL band edges and clock-loop gains), the second with call sizes that give the same decimated counts."""
import numpy as np
import pytest

import orc
import sig

pytestmark = pytest.mark.gpu

RATE, OFFSET = 1000000, 1200.0
NS = 64   # streams per workgroup of k_2fsk_tail (QRL_TAIL_NS in kernels_2fsk_tail.hip)


class Case:
    """one mode that runs k_2fsk_tail: sig.MODES name, modem type, the oracle receiver's arguments, samples per call at 1 Msps"""

    def __init__(self, mode, modem, sps, filter_width, calls):
        self.mode, self.modem, self.sps, self.filter_width, self.calls = mode, modem, sps, filter_width, calls


CASES = [
    Case("2fsk1k", 18, 10, 2000, (50, 750, 800, 850, 5150, 5200, 5250, 2, 20000, 33334)),    # decimation 50
    Case("2fsk2k", 17, 5, 4000, (25, 375, 400, 425, 2575, 2600, 2625, 2, 10000, 16668)),     # decimation 25: the same decimated counts
]


@pytest.fixture(scope="module", params=CASES, ids=[c.mode for c in CASES])
def case(request):
    return request.param


@pytest.fixture(scope="module")
def stream(case):
    x, _ = sig.make_stream(case.mode, nframes=2, device_rate=RATE, rx_offset_hz=OFFSET, impair=sig.SPEC)
    return x[:x.size & ~1].astype(np.complex64)


@pytest.fixture(scope="module")
def refs(case, stream):
    """oracle output of stream b (the base stream shifted circularly by 3001 b samples), computed once per b"""
    cache = {}

    def get(b):
        if b not in cache:
            cache[b] = orc.demod_2fsk(orc.frontend(np.roll(stream, 3001 * b), RATE, OFFSET), sps=case.sps, filter_width=case.filter_width, fm=False)
        return cache[b]
    return get


def _batch(stream, B):
    return np.stack([np.roll(stream, 3001 * b) for b in range(B)])


def _run_calls(qrl_ctx, case, iq, options=(), slim_pattern=None):
    """iq [B, N] through one handle in calls of case.calls (cycled); slim_pattern: QRL_OPT_FLL_SLIM values set before successive calls"""
    import torch
    import qradiolink_amd as q
    CALLS = case.calls
    B, N = iq.shape
    dem = q.Demod(qrl_ctx, case.modem, batch=B, max_chunk=max(CALLS), device_samp_rate=RATE, carrier_offset_hz=OFFSET)
    for opt, val in options:
        dem.set_option(opt, val)
    dev = torch.from_numpy(iq).cuda()
    names = ("filtered", "constellation", "bits_a", "bits_b")
    parts = {k: [[] for _ in range(B)] for k in names}
    s = k = 0
    while s < N:
        n = min(CALLS[k % len(CALLS)], N - s)
        if slim_pattern is not None:
            dem.set_option(q.OPT_FLL_SLIM, slim_pattern[k % len(slim_pattern)])
        part = torch.zeros((B, n + (n & 1) + 2), dtype=dev.dtype, device=dev.device)   # a buffer of its own: even pitch, 16-byte aligned rows
        part[:, :n] = dev[:, s:s + n]
        out = dem.process(part[:, :n])
        cnt = out["counts"].cpu().numpy()
        for j, name in enumerate(names):
            host = out[name].cpu().numpy()
            for b in range(B):
                parts[name][b].append(host[b, :cnt[b, j]].copy())
        s += n
        k += 1
    dem.close()
    assert k > 2 * len(CALLS)   # every call size came up more than once
    return {name: [np.concatenate(v) for v in parts[name]] for name in names}


def _compare(out, refs, B):
    """all four counts (the sizes of the concatenated ports) and the ports themselves, as test_gpu_parity._compare"""
    for b in range(B):
        ref = refs(b)
        assert ref["bits_a"].size > 0
        for port in ("bits_a", "bits_b"):
            assert out[port][b].size == ref[port].size, (port, b, out[port][b].size, ref[port].size)
            assert np.array_equal(out[port][b], ref[port]), "%s stream %d differs" % (port, b)
        for port in ("filtered", "constellation"):
            got, want = out[port][b].view(np.float32) + np.float32(0), ref[port].view(np.float32) + np.float32(0)
            assert got.size == want.size, (port, b, got.size, want.size)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s stream %d not bit-identical" % (port, b)


@pytest.mark.parametrize("B", [1, 3, NS + 1])
def test_call_edges(qrl_ctx, case, stream, refs, B):
    out = _run_calls(qrl_ctx, case, _batch(stream, B))
    _compare(out, refs, B)


def test_switching_between_fused_and_unfused_kernels(qrl_ctx, case, stream, refs):
    out = _run_calls(qrl_ctx, case, _batch(stream, 3), slim_pattern=(1, 0))
    _compare(out, refs, 3)


def test_serial_order(qrl_ctx, case, stream, refs):
    import qradiolink_amd as q
    out = _run_calls(qrl_ctx, case, _batch(stream, 3), options=[(q.OPT_OVERLAP, 0)])
    _compare(out, refs, 3)
