"""8-bit IQ (sc8, cu8) into a receiver WITHOUT a device-rate front end (1 Msps, QRL_OPT_IQ8_BASEBAND): qrl_demod_process_sc8 / _cu8 on the
bytes equal, bit for bit on every port, the oracle chain fed x = (float32(byte ^ mask) - bias) * scale -- for every kernel that reads the
caller's buffer at 1 Msps, with a shared carrier offset and with per-stream offsets (the PS instantiations), in the ragged calls of
tests/iq8_baseband.py: both formats, calls with n % 8 != 0, a 2-sample and a 100-sample call, starts at 4 and 6 (mod 8) from shifted copies, a
row pitch larger than n, a scale that is no power of two and a cu8 bias of 127.4 set between two calls, cf32 and int16 calls in between on a
handle with both options on.  tests/test_iq8_baseband_plan.py shows on the CPU that under this schedule the 1:50 stage's outputs come from the
streaming kernel's 2-byte ring path (most of them), from its edge unit and from the per-output kernel; tests/test_iq8_baseband_conditions.py
that the oracle runs are alive at 8 bits.  Inputs, receivers and oracle runs are shared: tests/iq8_baseband.py."""
import ctypes as C

import numpy as np
import pytest

import iq8_baseband as ib
import orc

pytestmark = pytest.mark.gpu

QRL_ERR_ARG = -1
COUNT_INDEX = {"filtered": 0, "constellation": 1, "audio": 1, "bits_a": 2, "bits_b": 3}
REFUSAL_8 = ("%s: 8-bit input needs the device-rate front end (device_samp_rate >= 2000000); this handle runs at 1 Msps and its missing front "
             "end is what converts")
REFUSAL_16 = "qrl_demod_process_sc16: int16 input needs the device-rate front end (device_samp_rate >= 2000000); this handle runs at 1 Msps"


def _open(qrl_ctx, name, per_stream, max_chunk, **kw):
    import qradiolink_amd as q
    c = ib.case(name)
    offsets = ib.inputs(name, per_stream)[4]
    dem = q.Demod(qrl_ctx, c["modem"], batch=ib.B, max_chunk=max_chunk, carrier_offset_hz=offsets[0], **kw)
    if per_stream:
        dem.set_carrier_offsets(list(offsets))
    for opt, val in c["options"]:
        dem.set_option(getattr(q, opt), val)
    if c["squelch"] is not None:
        dem.set_squelch(c["squelch"])
    return dem


class _Feed:
    """the device tensors of one receiver's input: the sc8, cu8 and int16 streams, copies of the 8-bit ones shifted by 2 and 4 samples, the
    converted floats"""
    def __init__(self, name, per_stream):
        import torch
        v8, u8, v16, conv, _ = ib.inputs(name, per_stream)
        self.name, self.per_stream = name, per_stream
        self.n = n = v8.shape[1] // 2
        self.t = {(ib.SC8, "plain"): torch.from_numpy(np.array(v8)).cuda(), (ib.CU8, "plain"): torch.from_numpy(np.array(u8)).cuda(),
                  (ib.SC16, "plain"): torch.from_numpy(np.array(v16)).cuda(), (ib.CF32, "plain"): torch.from_numpy(np.array(conv)).cuda()}
        for fmt in (ib.SC8, ib.CU8):
            for shift in (2, 4):
                t = torch.zeros((ib.B, 2 * (n + 8)), dtype=self.t[(fmt, "plain")].dtype, device="cuda")
                t[:, 2 * shift:2 * (shift + n)] = self.t[(fmt, "plain")]
                self.t[(fmt, "shift%d" % shift)] = t
        torch.cuda.current_stream().synchronize()
        assert all(t.data_ptr() % 16 == 0 for t in self.t.values())

    def call(self, dem, start, k, fmt, asynchronous=False):
        """one call of the schedule; returns the call's ports"""
        if fmt == ib.CF32:
            part = self.t[(fmt, "plain")][:, start:start + k]
            dem.process_async(part)
        else:
            which, first, pitch, base16 = ib.placement(self.n, start, fmt)
            part = self.t[(fmt, which)][:, 2 * first:2 * (first + k)]
            assert part.stride(0) == 2 * pitch and part.data_ptr() % 16 == base16 == 0 and pitch > k
            {ib.SC8: dem.process_sc8_async, ib.CU8: dem.process_cu8_async, ib.SC16: dem.process_sc16_async}[fmt](part)
        if not asynchronous:
            dem.sync()
        return dem._ports()

    def settings(self, dem, step):
        scale, bias, scale16 = ib.step_settings(self.name, self.per_stream, step)
        dem.set_sc8_scale(scale)
        dem.set_cu8_scale(scale, bias)
        dem.set_sc16_scale(scale16)


def _collect(out, ports, got):
    cnt = out["counts"].cpu().numpy()
    for p in ports:
        host = out[p].cpu().numpy()
        for b in range(ib.B):
            got[p][b].append(host[b, :cnt[b, COUNT_INDEX[p]]].copy())
    return cnt


def _run(dem, feed, ports, calls=None, fmt_of=lambda fmt: fmt, scope=False):
    """the schedule through dem; returns ({port: [stream arrays]}, per-call counts [calls, B, 4])"""
    got = {p: [[] for _ in range(ib.B)] for p in ports}
    if scope:
        got["scope"] = [[] for _ in range(ib.B)]
    counts, cur = [], None
    for start, k, fmt, step in (calls or ib.calls(feed.n)):
        if step != cur:
            cur = step
            feed.settings(dem, step)
        out = feed.call(dem, start, k, fmt_of(fmt))
        counts.append(_collect(out, ports, got).copy())
        if scope:
            sc_cnt, sc_host = dem.scope_counts.cpu().numpy(), dem.scope.cpu().numpy()
            for b in range(ib.B):
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
    want = ib.refs(name, per_stream)
    for p in ib.case(name)["ports"]:
        for b in range(ib.B):
            _same(got[p][b], want[b][p], (name, p, b))


def _both_on(dem):
    dem.enable_iq8_baseband()
    dem.enable_sc16_baseband()


@pytest.mark.parametrize("per_stream", [False, True], ids=["shared_offset", "per_stream_offsets"])
@pytest.mark.parametrize("name", sorted(ib.CASES))
def test_8_bit_at_1_msps_bit_exact_for_every_reader_of_the_callers_buffer(qrl_ctx, name, per_stream):
    ib.refs(name, per_stream)                                   # the oracle's conditions first
    feed = _Feed(name, per_stream)
    dem = _open(qrl_ctx, name, per_stream, max(k for _, k, _, _ in ib.calls(feed.n)))
    _both_on(dem)
    got, _ = _run(dem, feed, ib.case(name)["ports"])
    dem.close()
    _same_as_oracle(got, name, per_stream)


def test_counts_of_every_call_are_those_of_the_cf32_run(qrl_ctx):
    """2FSK-1k: the same schedule fed as floats throughout gives the same four counts in every call (and both runs give the oracle's ports)"""
    name = "2fsk1k"
    feed = _Feed(name, False)
    runs = []
    for only_cf32 in (False, True):
        dem = _open(qrl_ctx, name, False, feed.n)
        _both_on(dem)
        runs.append(_run(dem, feed, ib.case(name)["ports"], fmt_of=(lambda f: ib.CF32) if only_cf32 else (lambda f: f)))
        dem.close()
    assert np.array_equal(runs[0][1], runs[1][1])
    assert runs[0][1][:, :, 2].sum() > 0
    for got, _ in runs:
        _same_as_oracle(got, name, False)


@pytest.mark.parametrize("name", ["2fsk1k", "qpsk250k"])
def test_scope_tap_under_8_bit_calls(qrl_ctx, name):
    """enable_time_domain: the 1:10 decimator of the scope tap reads the caller's 8-bit buffer too"""
    feed = _Feed(name, False)
    conv, offsets = ib.inputs(name, False)[3:]
    dem = _open(qrl_ctx, name, False, feed.n)
    _both_on(dem)
    dem.enable_time_domain()
    got, _ = _run(dem, feed, ib.case(name)["ports"], scope=True)
    dem.close()
    _same_as_oracle(got, name, False)
    taps = orc.low_pass(1, 1000000, 50000, 25000)
    for b in range(ib.B):
        want = orc.decim_auto(orc.frontend(conv[b], 1000000, offsets[b]), taps, 10)
        assert want.size > 10000
        _same(got["scope"][b], want, ("scope", b))


@pytest.mark.parametrize("resident", [True, False], ids=["helper_stream", "in_line"])
def test_edge_staging_with_and_without_input_resident(qrl_ctx, resident):
    """2FSK-1k: QRL_OPT_INPUT_RESIDENT = 1 stages the edge scratch (k_pl_edge_stage_iq8) and keeps the history (k_hist_iq8) on the helper
    stream, a call ahead; the calls are queued without a sync in between, each with its own output tensors"""
    import qradiolink_amd as q
    name = "2fsk1k"
    feed = _Feed(name, False)
    dem = _open(qrl_ctx, name, False, feed.n, input_resident=False)
    dem.set_option(q.OPT_INPUT_RESIDENT, 1 if resident else 0)
    _both_on(dem)
    outs, cur = [], None
    for start, k, fmt, step in ib.calls(feed.n):
        if step != cur:
            cur = step
            feed.settings(dem, step)
        dem.new_outputs()
        outs.append(feed.call(dem, start, k, fmt, asynchronous=True))
    dem.sync()
    ports = ib.case(name)["ports"]
    got = {p: [[] for _ in range(ib.B)] for p in ports}
    for out in outs:
        _collect(out, ports, got)
    dem.close()
    _same_as_oracle({p: [np.concatenate(x) for x in got[p]] for p in ports}, name, False)


@pytest.mark.parametrize("fmt", [ib.SC8, ib.CU8])
def test_host_entry_points_at_1_msps(qrl_ctx, fmt):
    """qrl_demod_process_sc8_host / _cu8_host on a 1 Msps handle: refused by default, and with the option on the stream in two calls whose
    lengths are 2 and 6 (mod 8), 2-byte samples uploaded from a host pitch of n; the bits of the two calls together are the oracle's"""
    name = "gmsk10k"
    c = ib.case(name)
    v8, u8, scale, offsets = ib.whole(name)
    raw = np.ascontiguousarray(v8 if fmt == ib.SC8 else u8)
    n = raw.shape[1] // 2
    n1 = (n // 2) // 8 * 8 + 2
    assert n1 % 8 == 2 and (n - n1) % 8 == 6
    x = ib.whole_converted(name, fmt)
    want = [c["oracle"](orc.frontend(x[b], 1000000, offsets[b])) for b in range(ib.B)]
    assert all(w["bits_a"].size >= 80 and w["bits_b"].size >= 80 for w in want)
    dem = _open(qrl_ctx, name, False, n)
    dem.set_sc8_scale(float(scale))
    dem.set_cu8_scale(float(scale), float(ib.BIAS1))
    cap = dem.caps[2]
    a, b_, cnt = np.zeros((ib.B, cap), np.uint8), np.zeros((ib.B, cap), np.uint8), np.zeros((ib.B, 4), np.uint32)
    fn = getattr(dem.lib, "qrl_demod_process_%s_host" % fmt)
    assert fn(dem.h, raw.ctypes.data, n, n1, a.ctypes.data, b_.ctypes.data, cap, cnt.ctypes.data) == QRL_ERR_ARG     # the default: refused
    assert dem.lib.qrl_last_error().decode() == REFUSAL_8 % ("qrl_demod_process_" + fmt)
    dem.enable_iq8_baseband()
    got_a, got_b = [[] for _ in range(ib.B)], [[] for _ in range(ib.B)]
    for start, count in ((0, n1), (n1, n - n1)):
        rc = fn(dem.h, raw.ctypes.data + 2 * start, n, count, a.ctypes.data, b_.ctypes.data, cap, cnt.ctypes.data)
        assert rc == 0, dem.lib.qrl_last_error().decode()
        for s in range(ib.B):
            got_a[s].append(a[s, :cnt[s, 2]].copy())
            got_b[s].append(b_[s, :cnt[s, 3]].copy())
    dem.close()
    for s in range(ib.B):
        assert np.array_equal(np.concatenate(got_a[s]), want[s]["bits_a"]), "bits A stream %d" % s
        assert np.array_equal(np.concatenate(got_b[s]), want[s]["bits_b"]), "bits B stream %d" % s


def test_option_back_to_0_refuses_again_and_the_stream_goes_on_in_cf32(qrl_ctx):
    """8-bit calls up to the fifth call of the schedule, then QRL_OPT_IQ8_BASEBAND = 0: the next 8-bit call is QRL_ERR_ARG with the text of a
    handle that never had the option, nothing has moved, and the rest of the schedule fed as floats completes the oracle's stream"""
    import qradiolink_amd as q
    name = "2fsk1k"
    feed = _Feed(name, False)
    calls = ib.calls(feed.n)
    dem = _open(qrl_ctx, name, False, feed.n)
    _both_on(dem)
    ports = ib.case(name)["ports"]
    head, _ = _run(dem, feed, ports, calls=calls[:5])
    dem.enable_iq8_baseband(False)
    start, k, fmt = calls[5][:3]
    assert fmt == ib.CU8 and start % 8 == 0
    for f, entry in ((ib.CU8, dem.lib.qrl_demod_process_cu8), (ib.SC8, dem.lib.qrl_demod_process_sc8)):
        part = feed.t[(f, "plain")][:, 2 * start:2 * (start + k)]
        assert entry(dem.h, part.data_ptr(), feed.n, k, C.byref(dem._out)) == QRL_ERR_ARG
        assert dem.lib.qrl_last_error().decode() == REFUSAL_8 % ("qrl_demod_process_" + f)
    with pytest.raises(q.QrlError):
        dem.process_cu8(feed.t[(ib.CU8, "plain")][:, 2 * start:2 * (start + k)])
    tail, _ = _run(dem, feed, ports, calls=calls[5:], fmt_of=lambda f: ib.CF32)
    dem.close()
    _same_as_oracle({p: [np.concatenate([head[p][b], tail[p][b]]) for b in range(ib.B)] for p in ports}, name, False)


def test_the_two_options_are_independent(qrl_ctx):
    """QRL_OPT_IQ8_BASEBAND alone refuses int16, QRL_OPT_SC16_BASEBAND alone refuses 8-bit input, each with the text of a handle without any
    option; the refusals move nothing: the whole schedule afterwards gives the oracle's stream"""
    name = "gmsk10k"
    feed = _Feed(name, False)
    dem = _open(qrl_ctx, name, False, feed.n)
    k = 8000
    p8s, p8u, p16 = (feed.t[(f, "plain")][:, :2 * k] for f in (ib.SC8, ib.CU8, ib.SC16))

    def rc16():
        return dem.lib.qrl_demod_process_sc16(dem.h, p16.data_ptr(), feed.n, k, C.byref(dem._out))

    def rc8(f):
        t = p8s if f == ib.SC8 else p8u
        return getattr(dem.lib, "qrl_demod_process_" + f)(dem.h, t.data_ptr(), feed.n, k, C.byref(dem._out))

    dem.enable_iq8_baseband()                                   # option 7 alone
    assert rc16() == QRL_ERR_ARG and dem.lib.qrl_last_error().decode() == REFUSAL_16
    dem.enable_iq8_baseband(False)
    dem.enable_sc16_baseband()                                  # option 6 alone
    for f in (ib.SC8, ib.CU8):
        assert rc8(f) == QRL_ERR_ARG and dem.lib.qrl_last_error().decode() == REFUSAL_8 % ("qrl_demod_process_" + f)
    dem.enable_iq8_baseband()
    got, _ = _run(dem, feed, ib.case(name)["ports"])
    dem.close()
    _same_as_oracle(got, name, False)


@pytest.mark.parametrize("name", ["2fsk1k", "gmsk10k"])
def test_reset_after_8_bit_calls_gives_a_fresh_handles_output(qrl_ctx, name):
    """a few 8-bit calls from the middle of the stream, qrl_demod_reset, then the whole schedule: the oracle's stream from its first sample
    (the option, like every option, is kept across a reset)"""
    feed = _Feed(name, False)
    dem = _open(qrl_ctx, name, False, feed.n)
    _both_on(dem)
    feed.settings(dem, 1)
    for start, k, fmt in ((40000, 30000, ib.CU8), (70000, 10004, ib.SC8), (80004, 2, ib.CU8)):
        feed.call(dem, start, k, fmt)
    dem.reset()
    got, _ = _run(dem, feed, ib.case(name)["ports"])
    dem.close()
    _same_as_oracle(got, name, False)
