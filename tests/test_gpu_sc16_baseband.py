"""16-bit integer IQ (sc16) into a receiver WITHOUT a device-rate front end (1 Msps, QRL_OPT_SC16_BASEBAND): qrl_demod_process_sc16 on int16
input v equals, bit for bit on every port, the oracle chain fed np.float32(v) * np.float32(scale) -- for every kernel that reads the
caller's buffer at 1 Msps, with a shared carrier offset and with per-stream offsets (the PS instantiations), in the ragged calls of
tests/sc16_baseband.py: a call with n % 4 != 0, a 2-sample call, a call shorter than the stage's look-back, a row pitch larger than n, a scale
set between two calls, cf32 and int16 calls alternating on one handle.  tests/test_sc16_baseband_plan.py shows on the CPU that under
this schedule most outputs of the 1:50 stage come from the streaming kernel's 4-byte path, the rest from the staged edge unit and the
per-output kernel.  Inputs, receivers and oracle runs (with the conditions that keep a comparison from passing on dead air) are shared:
tests/sc16_baseband.py."""
import ctypes as C

import numpy as np
import pytest

import orc
import sc16_baseband as sb

pytestmark = pytest.mark.gpu

QRL_ERR_ARG = -1
COUNT_INDEX = {"filtered": 0, "constellation": 1, "audio": 1, "bits_a": 2, "bits_b": 3}


def _open(qrl_ctx, name, per_stream, max_chunk, **kw):
    import qradiolink_amd as q
    c = sb.case(name)
    _, offsets = sb.inputs(name, per_stream)
    dem = q.Demod(qrl_ctx, c["modem"], batch=sb.B, max_chunk=max_chunk, carrier_offset_hz=offsets[0], **kw)
    if per_stream:
        dem.set_carrier_offsets(list(offsets))
    for opt, val in c["options"]:
        dem.set_option(getattr(q, opt), val)
    if c["squelch"] is not None:
        dem.set_squelch(c["squelch"])
    return dem


class _Feed:
    """the device tensors of one receiver's input: the int16 stream, its copy shifted by two samples, the converted floats"""
    def __init__(self, v):
        import torch
        self.n = v.shape[1] // 2
        self.plain = torch.from_numpy(np.array(v)).cuda()          # (a writable copy: the shared input is read-only)
        self.shifted = torch.zeros((sb.B, 2 * (self.n + 4)), dtype=torch.int16, device="cuda")
        self.shifted[:, 4:4 + 2 * self.n] = self.plain
        self.floats = torch.from_numpy(sb.converted(v)).cuda()
        torch.cuda.current_stream().synchronize()
        assert self.plain.data_ptr() % 16 == 0 and self.shifted.data_ptr() % 16 == 0 and self.floats.data_ptr() % 16 == 0

    def call(self, dem, start, k, fmt, asynchronous=False):
        """one call of the schedule; returns the call's ports"""
        if fmt == sb.CF32:
            part = self.floats[:, start:start + k]
            dem.process_async(part)
        else:
            which, first, pitch, base16 = sb.placement(self.n, start, fmt)
            t = self.plain if which == "plain" else self.shifted
            part = t[:, 2 * first:2 * (first + k)]
            assert part.stride(0) == 2 * pitch and part.data_ptr() % 16 == base16 == 0 and pitch > k
            dem.process_sc16_async(part)
        if not asynchronous:
            dem.sync()
        return dem._ports()


def _run(dem, feed, ports, calls=None, fmt_of=lambda fmt: fmt, scope=False):
    """the schedule through dem; returns ({port: [stream arrays]}, per-call counts [calls, B, 4])"""
    got = {p: [[] for _ in range(sb.B)] for p in ports}
    if scope:
        got["scope"] = [[] for _ in range(sb.B)]
    counts, scale = [], None
    for start, k, fmt, sc in (calls or sb.calls(feed.n)):
        if scale is None or float(sc) != scale:
            scale = float(sc)
            dem.set_sc16_scale(scale)
        out = feed.call(dem, start, k, fmt_of(fmt))
        cnt = out["counts"].cpu().numpy()
        counts.append(cnt.copy())
        for p in ports:
            host = out[p].cpu().numpy()
            for b in range(sb.B):
                got[p][b].append(host[b, :cnt[b, COUNT_INDEX[p]]].copy())
        if scope:
            sc_cnt, sc_host = dem.scope_counts.cpu().numpy(), dem.scope.cpu().numpy()
            for b in range(sb.B):
                got["scope"][b].append(sc_host[b, :sc_cnt[b]].copy())
    return {p: [np.concatenate(x) for x in got[p]] for p in got}, np.stack(counts)


def _same(got, want, what):
    """bit-identical: bits byte for byte, float ports word for word (the sign of a zero included)"""
    assert got.size == want.size, (what, got.size, want.size)
    if got.dtype == np.uint8:
        assert np.array_equal(got, want), what
    else:
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), what


def _same_as_oracle(got, name, per_stream):
    want = sb.refs(name, per_stream)
    for p in sb.case(name)["ports"]:
        for b in range(sb.B):
            _same(got[p][b], want[b][p], (name, p, b))


@pytest.mark.parametrize("per_stream", [False, True], ids=["shared_offset", "per_stream_offsets"])
@pytest.mark.parametrize("name", sorted(sb.CASES))
def test_sc16_at_1_msps_bit_exact_for_every_reader_of_the_callers_buffer(qrl_ctx, name, per_stream):
    v, _ = sb.inputs(name, per_stream)
    sb.refs(name, per_stream)                                   # the oracle's conditions first
    feed = _Feed(v)
    dem = _open(qrl_ctx, name, per_stream, max(k for _, k, _, _ in sb.calls(feed.n)))
    dem.enable_sc16_baseband()
    got, _ = _run(dem, feed, sb.case(name)["ports"])
    dem.close()
    _same_as_oracle(got, name, per_stream)


def test_counts_of_every_call_are_those_of_the_cf32_run(qrl_ctx):
    """2FSK-1k: the same schedule fed as floats throughout gives the same four counts in every call (and both runs give the oracle's ports)"""
    name = "2fsk1k"
    v, _ = sb.inputs(name, False)
    feed = _Feed(v)
    runs = []
    for only_cf32 in (False, True):
        dem = _open(qrl_ctx, name, False, feed.n)
        dem.enable_sc16_baseband()
        runs.append(_run(dem, feed, sb.case(name)["ports"], fmt_of=(lambda f: sb.CF32) if only_cf32 else (lambda f: f)))
        dem.close()
    assert np.array_equal(runs[0][1], runs[1][1])
    assert runs[0][1][:, :, 2].sum() > 0
    for got, _ in runs:
        _same_as_oracle(got, name, False)


@pytest.mark.parametrize("name", ["2fsk1k", "qpsk250k"])
def test_scope_tap_under_int16_calls(qrl_ctx, name):
    """enable_time_domain: the 1:10 decimator of the scope tap reads the caller's int16 buffer too"""
    v, offsets = sb.inputs(name, False)
    feed = _Feed(v)
    dem = _open(qrl_ctx, name, False, feed.n)
    dem.enable_sc16_baseband()
    dem.enable_time_domain()
    got, _ = _run(dem, feed, sb.case(name)["ports"], scope=True)
    dem.close()
    _same_as_oracle(got, name, False)
    taps = orc.low_pass(1, 1000000, 50000, 25000)
    x = sb.converted(v)
    for b in range(sb.B):
        want = orc.decim_auto(orc.frontend(x[b], 1000000, offsets[b]), taps, 10)
        assert want.size > 10000
        _same(got["scope"][b], want, ("scope", b))


@pytest.mark.parametrize("resident", [True, False], ids=["helper_stream", "in_line"])
def test_edge_staging_with_and_without_input_resident(qrl_ctx, resident):
    """2FSK-1k: QRL_OPT_INPUT_RESIDENT = 1 stages the edge scratch (k_pl_edge_stage_sc16) and keeps the history (k_hist_sc16) on the helper
    stream, a call ahead; the calls are queued without a sync in between, each with its own output tensors"""
    import qradiolink_amd as q
    name = "2fsk1k"
    v, _ = sb.inputs(name, False)
    feed = _Feed(v)
    dem = _open(qrl_ctx, name, False, feed.n, input_resident=False)
    dem.set_option(q.OPT_INPUT_RESIDENT, 1 if resident else 0)
    dem.enable_sc16_baseband()
    outs, scale = [], None
    for start, k, fmt, sc in sb.calls(feed.n):
        if scale is None or float(sc) != scale:
            scale = float(sc)
            dem.set_sc16_scale(scale)
        dem.new_outputs()
        outs.append(feed.call(dem, start, k, fmt, asynchronous=True))
    dem.sync()
    ports = sb.case(name)["ports"]
    got = {p: [[] for _ in range(sb.B)] for p in ports}
    for out in outs:
        cnt = out["counts"].cpu().numpy()
        for p in ports:
            host = out[p].cpu().numpy()
            for b in range(sb.B):
                got[p][b].append(host[b, :cnt[b, COUNT_INDEX[p]]].copy())
    dem.close()
    _same_as_oracle({p: [np.concatenate(x) for x in got[p]] for p in ports}, name, False)


def test_host_entry_point_at_1_msps(qrl_ctx):
    """qrl_demod_process_sc16_host on a 1 Msps handle with the option on: the stream in two calls whose lengths are 2 (mod 4), 4-byte samples
    uploaded from a host pitch of n; the bits of the two calls together are the oracle's for the default scale"""
    name = "gmsk10k"
    c = sb.case(name)
    v, offsets = sb.inputs(name, False)
    v = np.ascontiguousarray(v)
    n = v.shape[1] // 2
    n1 = (n // 2) // 4 * 4 + 2
    assert n1 % 4 == 2 and (n - n1) % 4 == 2
    x = (v.astype(np.float32) * sb.SCALE0).view(np.complex64)
    want = [c["oracle"](orc.frontend(x[b], 1000000, offsets[b])) for b in range(sb.B)]
    assert all(w["bits_a"].size >= 80 and w["bits_b"].size >= 80 for w in want)
    dem = _open(qrl_ctx, name, False, n)
    cap = dem.caps[2]
    a, b_, cnt = np.zeros((sb.B, cap), np.uint8), np.zeros((sb.B, cap), np.uint8), np.zeros((sb.B, 4), np.uint32)
    fn = dem.lib.qrl_demod_process_sc16_host
    assert fn(dem.h, v.ctypes.data, n, n1, a.ctypes.data, b_.ctypes.data, cap, cnt.ctypes.data) == QRL_ERR_ARG     # the default: refused
    assert "1 Msps" in dem.lib.qrl_last_error().decode()
    dem.enable_sc16_baseband()
    got_a, got_b = [[] for _ in range(sb.B)], [[] for _ in range(sb.B)]
    for start, count in ((0, n1), (n1, n - n1)):
        rc = fn(dem.h, v.ctypes.data + 4 * start, n, count, a.ctypes.data, b_.ctypes.data, cap, cnt.ctypes.data)
        assert rc == 0, dem.lib.qrl_last_error().decode()
        for s in range(sb.B):
            got_a[s].append(a[s, :cnt[s, 2]].copy())
            got_b[s].append(b_[s, :cnt[s, 3]].copy())
    dem.close()
    for s in range(sb.B):
        assert np.array_equal(np.concatenate(got_a[s]), want[s]["bits_a"]), "bits A stream %d" % s
        assert np.array_equal(np.concatenate(got_b[s]), want[s]["bits_b"]), "bits B stream %d" % s


def test_option_back_to_0_refuses_again_and_the_stream_goes_on_in_cf32(qrl_ctx):
    """int16 calls up to the fifth call of the schedule, then QRL_OPT_SC16_BASEBAND = 0: the next int16 call is QRL_ERR_ARG with the text of a
    handle that never had the option, nothing has moved, and the rest of the schedule fed as floats completes the oracle's stream"""
    import qradiolink_amd as q
    name = "2fsk1k"
    v, _ = sb.inputs(name, False)
    feed = _Feed(v)
    calls = sb.calls(feed.n)
    dem = _open(qrl_ctx, name, False, feed.n)
    dem.enable_sc16_baseband()
    ports = sb.case(name)["ports"]
    head, _ = _run(dem, feed, ports, calls=calls[:5])
    dem.enable_sc16_baseband(False)
    start, k = calls[5][0], calls[5][1]
    part = feed.plain[:, 2 * start:2 * (start + k)]
    assert dem.lib.qrl_demod_process_sc16(dem.h, part.data_ptr(), feed.n, k, C.byref(dem._out)) == QRL_ERR_ARG
    err = dem.lib.qrl_last_error().decode()
    assert "1 Msps" in err and "front end" in err, err
    with pytest.raises(q.QrlError):
        dem.process_sc16(part)
    tail, _ = _run(dem, feed, ports, calls=calls[5:], fmt_of=lambda f: sb.CF32)
    dem.close()
    _same_as_oracle({p: [np.concatenate([head[p][b], tail[p][b]]) for b in range(sb.B)] for p in ports}, name, False)


@pytest.mark.parametrize("name", ["2fsk1k", "gmsk10k"])
def test_reset_after_int16_calls_gives_a_fresh_handles_output(qrl_ctx, name):
    """a few int16 calls from the middle of the stream, qrl_demod_reset, then the whole schedule: the oracle's stream from its first sample
    (the option, like every option, is kept across a reset)"""
    v, _ = sb.inputs(name, False)
    feed = _Feed(v)
    dem = _open(qrl_ctx, name, False, feed.n)
    dem.enable_sc16_baseband()
    dem.set_sc16_scale(float(sb.SCALE1))
    for start, k in ((40000, 30000), (70000, 10004), (80004, 2)):
        feed.call(dem, start, k, sb.SC16)
    dem.reset()
    got, _ = _run(dem, feed, sb.case(name)["ports"])
    dem.close()
    _same_as_oracle(got, name, False)
