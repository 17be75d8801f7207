"""Reset on every handle type gives a fresh handle's output: the handle is dirtied with a stream A, reset, and fed a DIFFERENT stream B in
ragged calls; every output of the B calls equals the oracle's output for B alone, bit for bit (floats up to the sign of an exact zero, as in
test_gpu_parity._compare).  In the code a reset is a hand-kept list per handle type (qrl_demod::init_state, AnalogChain::init_state,
qrl_mod::init_state, TxBackEnd::reset, qrl_chan::reset_state, ...): whatever is added to a handle and not to its list survives silently, and
feeding the SAME signal on both sides of a reset hides it -- what is left in a ring is then what is about to be written there again.

A is about eight times B's level, a few hundred Hz beside it, of another seed, fed in three calls, the last one queued and the reset (or the
setter that restarts the chain) called with no sync in between, and ends off every grid of the chain; tests/reset_streams.py builds the streams
and tests/test_reset_conditions.py shows on the oracle alone that each A changes what B gives when nothing is reset.  What a reset keeps --
carrier offsets, squelch, AGC, CTCSS, filter width, SSB gain, int16 scale, scope and DMO registrations, options, gains, levels, clip-count
pointers -- is asserted by the same comparisons, because the oracle for B runs with those settings."""
import numpy as np
import pytest

import orc
import reset_streams as rs

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.name for c in cases]


def _host(x):
    """a writable, contiguous copy (the shared streams are read-only; torch.from_numpy wants to own what it wraps)"""
    return np.array(x, order="C")


# ---------------------------------------------------------------- receivers
def _receive(dem, x, cuts, ports, sc16_scale=None, scope=False, queue_last=False):
    """x [B, n] complex64 through dem in the given calls (sc16_scale: as int16 IQ at that scale).  ports: {name: column of counts}.
    queue_last: the last call is only queued (nothing is collected from it).  -> {port: [array per stream]}"""
    import torch
    nb = x.shape[0]
    if sc16_scale is None:
        d = torch.from_numpy(_host(x)).cuda()
    else:
        v = rs.quantise(x, sc16_scale)
        assert np.array_equal(rs.converted(v, sc16_scale), x)          # the oracle was fed exactly what the kernel converts
        d = torch.from_numpy(v).cuda()
    got = {k: [[] for _ in range(nb)] for k in list(ports) + (["scope"] if scope else [])}
    pos = 0
    for i, c in enumerate(cuts):
        part = d[:, pos:pos + c] if sc16_scale is None else d[:, 2 * pos:2 * (pos + c)]
        pos += c
        if queue_last and i == len(cuts) - 1:
            dem.process_async(part) if sc16_scale is None else dem.process_sc16_async(part)
            break
        out = dem.process(part) if sc16_scale is None else dem.process_sc16(part)
        cnt = out["counts"].cpu().numpy()
        for name, j in ports.items():
            host = out[name].cpu().numpy()
            for b in range(nb):
                got[name][b].append(host[b, :cnt[b, j]].copy())
        if scope:
            sc, n = dem.scope.cpu().numpy(), dem.scope_counts.cpu().numpy()
            for b in range(nb):
                got["scope"][b].append(sc[b, :n[b]].copy())
    assert pos == x.shape[1]
    return {k: [np.concatenate(v) if v else np.zeros(0) for v in got[k]] for k in got}


def _same_as_refs(case, got):
    for b, ref in enumerate(case.refs()):
        for port in case.PORTS:
            rs.assert_same(got[port][b], ref[port], "%s: port %s, stream %d" % (case, port, b))


@pytest.mark.parametrize("case", rs.RX_CASES, ids=_ids(rs.RX_CASES))
def test_demod_reset_then_another_stream(qrl_ctx, case):
    import qradiolink_amd as q
    A, B = case.streams()
    cuts_a, cuts_b = case.cuts()
    dem = q.Demod(qrl_ctx, case.modem, batch=rs.NB, max_chunk=max(cuts_a + cuts_b), device_samp_rate=case.rate, carrier_offset_hz=case.offset,
                  input_resident=case.resident)
    try:
        for opt, val in case.pre:
            dem.set_option(opt, val)
        if case.scope:
            dem.enable_time_domain()
        if case.sc16_scale is not None:
            dem.set_sc16_scale(float(case.sc16_scale))
        ports = {"filtered": 0, "constellation": 1, "bits_a": 2, "bits_b": 3}
        _receive(dem, A, cuts_a, ports, case.sc16_scale if case.a_sc16 else None, case.scope, queue_last=True)
        dem.reset()                                   # no sync behind the queued call: the reset's own wait is part of its contract
        for opt, val in case.post:                    # legal only before the first sample of a stream: a reset counts as such
            dem.set_option(opt, val)
        got = _receive(dem, B, cuts_b, ports, case.sc16_scale if case.b_sc16 else None, case.scope)
    finally:
        dem.close()
    _same_as_refs(case, got)
    assert all(r["bits_a"].size >= 80 for r in case.refs()) or "bits_a" in case.SILENT


@pytest.mark.parametrize("case", rs.ANALOG_CASES, ids=_ids(rs.ANALOG_CASES))
def test_analog_reset_or_restarting_setter_then_another_stream(qrl_ctx, case):
    """The analogue receivers with their controls off the defaults; the `mid` cases call qrl_demod_set_filter_width / qrl_demod_set_ctcss between
    A and B and NO reset (test_analog_set_filter_width_bit_exact resets behind the setter, so it never sees the setter's own restart)."""
    import qradiolink_amd as q
    A, B = case.streams()
    cuts_a, cuts_b = case.cuts()
    c = case.controls
    dem = q.Demod(qrl_ctx, case.R["modem"], batch=rs.NB, max_chunk=max(cuts_a + cuts_b))
    try:
        dem.set_squelch(c["squelch"])
        if "agc" in c:
            dem.set_agc(*c["agc"])
        if "gain" in c:
            dem.set_gain(c["gain"])
        if "ctcss" in c and case.mid != "ctcss":
            dem.set_ctcss(c["ctcss"])
        ports = {"filtered": 0, "audio": 1}
        _receive(dem, A, cuts_a, ports, queue_last=True)
        if case.mid == "set_width":
            dem.set_filter_width(c["set_width"])
        elif case.mid == "ctcss":
            dem.set_ctcss(c["ctcss"])
        else:
            dem.reset()
        got = _receive(dem, B, cuts_b, ports)
    finally:
        dem.close()
    _same_as_refs(case, got)


# ---------------------------------------------------------------- transmitters
def _same_iq(case, got):
    for b, ref in enumerate(case.refs()):
        rs.assert_same(got[b], ref["iq"], "%s: stream %d" % (case, b))


@pytest.mark.parametrize("case", rs.MOD_CASES, ids=_ids(rs.MOD_CASES))
def test_mod_reset_then_another_payload(qrl_ctx, case):
    """Mod.reset behind a queued call; the DMR case has queued a zero run that starts beyond the end of A: a reset drops it, it does not fire in B"""
    import torch
    import qradiolink_amd as q
    A, B = case.streams()
    cuts_a, cuts_b = case.cuts()
    mod = q.Mod(qrl_ctx, case.modem, batch=rs.NB, max_bytes=max(cuts_a + cuts_b), bb_gain=case.bb_gain, device_samp_rate=case.rate, carrier_offset_hz=case.offset)
    clip = None
    try:
        if case.sc16:
            clip = torch.zeros(rs.NB, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            mod.set_sc16_scale(case.sc16)
            mod.set_sc16_clip_counts(clip)
        send = mod.process_sc16_async if case.sc16 else mod.process_async
        if case.zero_run:
            mod.add_zero_runs(case.queued_runs())
        d, pos, keep = torch.from_numpy(_host(A)).cuda(), 0, []
        for c in cuts_a:
            keep.append(send(d[:, pos:pos + c].contiguous()))        # the last one still queued when the reset comes
            pos += c
            if pos < A.shape[1]:
                mod.sync()
        mod.reset()
        d, pos, parts = torch.from_numpy(_host(B)).cuda(), 0, []
        for c in cuts_b:
            out = send(d[:, pos:pos + c].contiguous())
            mod.sync()
            parts.append(out.cpu().numpy().reshape(rs.NB, -1))
            pos += c
    finally:
        mod.close()
    got = np.concatenate(parts, axis=1)
    if not case.sc16:
        _same_iq(case, got.view(np.complex64))
        return
    clips = []
    for b, ref in enumerate(case.refs()):
        want, n_b = rs.to_sc16(ref["iq"], case.sc16)
        rs.assert_same(got[b], want, "%s: stream %d" % (case, b))
        clips.append(rs.to_sc16(case.oracle(A[b], b)["iq"], case.sc16)[1] + n_b)
    assert min(clips) > 0 and clip.cpu().numpy().tolist() == clips        # the registration survives the reset: the counts keep adding


@pytest.mark.parametrize("case", rs.AMOD_CASES, ids=_ids(rs.AMOD_CASES))
def test_amod_reset_or_set_filter_width_then_other_audio(qrl_ctx, case):
    import torch
    import qradiolink_amd as q
    A, B = case.streams()
    cuts_a, cuts_b = case.cuts()
    mod = q.AMod(qrl_ctx, case.modem, batch=rs.NB, max_samples=max(cuts_a + cuts_b + [4]), bb_gain=case.bb_gain, device_samp_rate=case.rate, carrier_offset_hz=case.offset)
    try:
        if case.tone:
            mod.set_ctcss(case.tone)
        if case.mode == "cw":
            mod.set_cw_k(True)

        def send(x, pos, c):
            return mod.process_cw(c) if case.mode == "cw" else mod.process(torch.from_numpy(_host(x[:, pos:pos + c])).cuda())
        pos = 0
        for c in cuts_a:
            send(A, pos, c)
            pos += c
        if case.mid_width:
            mod.set_filter_width(case.mid_width)          # restarts the chain; the tone source runs on (amod.cpp: init_state(keep_tone_phase))
        else:
            mod.reset()
        pos, parts = 0, []
        for c in cuts_b:
            parts.append(send(B, pos, c).cpu().numpy())
            pos += c
    finally:
        mod.close()
    _same_iq(case, np.concatenate(parts, axis=1))


@pytest.mark.parametrize("case", rs.SYNTH_CASES, ids=_ids(rs.SYNTH_CASES))
def test_synth_reset_then_other_channels(qrl_ctx, case):
    import torch
    import qradiolink_amd as q
    A, B = case.streams()
    cuts_a, cuts_b = case.cuts()
    syn = q.Synth(qrl_ctx, case.N, batch=rs.NB, max_samples=max(cuts_a + cuts_b), bb_gain=case.bb_gain, single_carrier=case.single)
    try:
        if case.zero_run:
            syn.add_zero_runs(case.queued_runs())
        d, pos = torch.from_numpy(_host(A)).cuda(), 0
        for c in cuts_a:
            syn.process(d[:, :, pos:pos + c])
            pos += c
        syn.reset()
        d, pos, parts = torch.from_numpy(_host(B)).cuda(), 0, []
        for c in cuts_b:
            parts.append(syn.process(d[:, :, pos:pos + c]).cpu().numpy())
            pos += c
    finally:
        syn.close()
    _same_iq(case, np.concatenate(parts, axis=1))


# ---------------------------------------------------------------- wideband receivers
def _chan_feed(ch, case, x, cuts, sc16=False, queue_last=False):
    """x [streams, n] (form 3: [channels, n] channel samples) through ch in the given calls -> {port: [stream][channel] -> array}"""
    import torch
    f3 = case.form == 3
    ns, nc = (1, x.shape[0]) if f3 else (x.shape[0], ch.cc)
    d = torch.from_numpy(rs.quantise(x, case.sc16_scale) if sc16 else _host(x)).cuda()
    torch.cuda.synchronize()
    got = {p: [[[] for _ in range(nc)] for _ in range(ns)] for p in case.PORTS}
    pos = 0
    for i, c in enumerate(cuts):
        if f3:
            ch.process_channels_async(d[:, pos:pos + c], c)
        elif sc16:
            ch.process_sc16_async(d[:, 2 * pos:2 * (pos + c)])
        else:
            ch.process_async(d[:, pos:pos + c])
        pos += c
        if queue_last and i == len(cuts) - 1:
            break
        ch.sync()
        o, cnt = ch.out.cpu().numpy(), ch.counts.cpu().numpy()
        r, rc = ch.rssi.cpu().numpy(), ch.rssi_counts.cpu().numpy()
        if case.fsk:
            bits, fc = ch.dibits.cpu().numpy(), ch.fsk_counts.cpu().numpy()
        for s in range(ns):
            for k in range(nc):
                row = (k, 0) if f3 else (s, k)
                got["pcm"][s][k].append(o[row][:cnt[row]].copy())
                got["rssi"][s][k].append(r[row][:rc[row]].copy())
                if case.fsk:
                    got["dibits"][s][k].append(bits[row][:fc[row][2]].copy())
    assert pos == x.shape[1]
    return got


_CHAN_RUNS = {}


def _chan_run(qrl_ctx, case):
    """A, reset, B through a handle of the case's form; the B outputs, kept for the tests that share the run"""
    if case.name in _CHAN_RUNS:
        return _CHAN_RUNS[case.name]
    import qradiolink_amd as q
    A, B = case.streams()
    cuts_a, cuts_b = case.cuts()
    kw = {1: dict(form=1, decimation=10), 2: dict(form=2), 3: dict(form=3)}.get(case.form, {})
    ch = q.Channelizer(qrl_ctx, case.M, batch=6 if case.form == 3 else case.nb, max_chunk=max(cuts_a + cuts_b), **kw)
    try:
        ch.calibrate_rssi(case.CAL)
        if case.fsk:
            ch.enable_4fsk()
        if case.a_sc16:
            ch.set_sc16_scale(float(case.sc16_scale))
        xa, xb = (A[0], B[0]) if case.form == 3 else (A, B)
        _chan_feed(ch, case, xa, cuts_a, sc16=case.a_sc16, queue_last=True)
        ch.reset()
        for opt, val in case.post:                    # QRL_CHAN_OPT_LEGACY_TAIL: legal before the first samples or after a reset
            ch.set_option(opt, val)
        _CHAN_RUNS[case.name] = _chan_feed(ch, case, xb, cuts_b)
    finally:
        ch.close()
    return _CHAN_RUNS[case.name]


@pytest.mark.parametrize("case", rs.CHAN_CASES, ids=_ids(rs.CHAN_CASES))
def test_channelizer_reset_then_another_band(qrl_ctx, case):
    """Channelizer.reset behind a queued call, every form: the int16 samples and the 4FSK tail's dibits of every channel, with the counts of every
    call (calls of a few samples that deliver nothing among them), against the oracle for B"""
    got = _chan_run(qrl_ctx, case)
    for s, ref in enumerate(case.refs()):
        assert np.abs(np.stack(ref["pcm"])).max() > 1000          # the carriers are there
        for port in case.PORTS:
            if port == "rssi":
                continue
            for k, want in enumerate(ref[port]):
                rs.assert_same(np.concatenate(got[port][s][k]), want, "%s: port %s, stream %d, channel %d" % (case, port, s, k))


@pytest.mark.parametrize("case", rs.CHAN_CASES, ids=_ids(rs.CHAN_CASES))
def test_channelizer_reset_rssi_tags(qrl_ctx, case, capsys):
    """The RSSI tags of the same runs, bit for bit like every other output: the count of tags per channel and call, and the values.  A tag is
    10 log10f(level) + calibration; libm's log10f and the device library's differ in the last place (about a third of the tags, by up to
    1.5e-05 dB), so both the oracle and the kernels take the deterministic det_log10f (devmath.hpp / oracle/orc_side.c), as the RSSI block and
    the spectrum tap do with det_log2f.  The figures of every case are printed before the assertion."""
    got = _chan_run(qrl_ctx, case)
    worst, differing, total = 0.0, 0, 0
    for s, ref in enumerate(case.refs()):
        for k, want in enumerate(ref["rssi"]):
            g = np.concatenate(got["rssi"][s][k])
            assert g.size == want.size, (case, s, k, g.size, want.size)
            differing += int(np.count_nonzero(g.view(np.uint32) != want.view(np.uint32)))
            total += g.size
            if g.size:
                worst = max(worst, float(np.max(np.abs(g.astype(np.float64) - want.astype(np.float64)))))
    with capsys.disabled():
        print("\n[rssi tags] %s: %d of %d tags differ from the oracle's bits, largest difference %.3g dB" % (case, differing, total, worst))
    assert total > 0 and differing == 0, "%s: %d of %d RSSI tags differ, by at most %.3g dB" % (case, differing, total, worst)


# ---------------------------------------------------------------- bit-level blocks
@pytest.mark.parametrize("case", rs.BITS_CASES, ids=_ids(rs.BITS_CASES))
def test_deframer_and_framesync_reset_inside_a_frame(qrl_ctx, case):
    """A ends behind a sync word, 19 bits into its frame; after the reset B's records (and, for the frame synchroniser, its byte / frame counts and
    the per-call activity) are those of a fresh block"""
    import torch
    import qradiolink_amd as q
    A, B = case.streams()
    cuts_a, cuts_b = case.cuts()
    blk = q.Deframer(qrl_ctx, case.arg, rs.NB) if case.block == "deframer" else q.FrameSync(qrl_ctx, case.arg, rs.NB)
    refs = [None] * rs.NB
    try:
        d, pos = torch.from_numpy(_host(A)).cuda(), 0
        for c in cuts_a:
            blk.process(d[:, pos:pos + c].contiguous())
            pos += c
        blk.reset()
        d, pos, got = torch.from_numpy(_host(B)).cuda(), 0, [[] for _ in range(rs.NB)]
        for c in cuts_b:
            out, oc = blk.process(d[:, pos:pos + c].contiguous())
            out, oc = out.cpu().numpy(), oc.cpu().numpy()
            act = blk.activity.cpu().numpy() if case.block == "framesync" else None
            for b in range(rs.NB):
                want, collected, refs[b] = case.run(B[b, pos:pos + c], refs[b])          # the oracle from a fresh state, call by call
                n = int(oc[b, 0]) if case.block == "framesync" else int(oc[b])
                rs.assert_same(out[b, :n], want, "%s: records of stream %d, call at bit %d" % (case, b, pos))
                if case.block == "framesync":
                    assert int(oc[b, 1]) == len(orc.parse_frames(want)) and int(act[b]) == collected, (case, b, pos)
                got[b].append(out[b, :n].copy())
            pos += c
    finally:
        blk.close()
    for b, ref in enumerate(case.refs()):
        rs.assert_same(np.concatenate(got[b]), ref["records"], "%s: stream %d" % (case, b))
        assert ref["records"].size > 0


def test_rssi_reset_inside_a_block(qrl_ctx):
    """70 streams; A ends 500 items into a block of 2000 with the IIR charged 30 dB above B's level"""
    import torch
    import qradiolink_amd as q
    A, B = rs.rssi_streams()
    r = q.Rssi(qrl_ctx, rs.RSSI_STREAMS, level=rs.RSSI_LEVEL)
    try:
        d, pos = torch.from_numpy(_host(A)).cuda(), 0
        for c in rs.three_calls(rs.RSSI_DIRT, 1):
            r.process(d[:, pos:pos + c].contiguous())
            pos += c
        r.reset()
        d, pos, got = torch.from_numpy(_host(B)).cuda(), 0, []
        for c in [1, 63, 64, 65, 1999, 1, rs.RSSI_CLEAN - 2193]:
            out, last = r.process(d[:, pos:pos + c].contiguous())
            out, last = out.cpu().numpy()[:, :c].copy(), last.cpu().numpy()
            assert np.array_equal(last.view(np.uint32), out[:, -1].view(np.uint32))
            got.append(out)
            pos += c
        assert pos == rs.RSSI_CLEAN
    finally:
        r.close()
    got = np.concatenate(got, axis=1)
    for b in range(rs.RSSI_STREAMS):
        want = orc.rssi_block(B[b], level=rs.RSSI_LEVEL)
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), "stream %d" % b


def test_fft_set_fft_size_with_the_buffer_half_filled(qrl_ctx):
    """qrl_fft_set_fft_size restarts the fill: the frame behind it is the transform of the samples fed behind it.  The transform is hipFFT, so
    the comparison is test_rx_fft_spectrum_and_state_machine's: bins within 80 dB of the peak to 0.05 dB of the oracle's float64 FFT, same argmax."""
    import torch
    import qradiolink_amd as q
    A, B = rs.fft_streams()
    n = rs.FFT_SIZE // 2
    f = q.Fft(qrl_ctx, rs.NB, fftsize=rs.FFT_SIZE, wintype=rs.FFT_WINDOW)
    try:
        f.set_enabled(True)
        f.work(torch.from_numpy(_host(A)).cuda())            # half of the buffer of 1024
        f.set_fft_size(n)
        assert f.get_fft_size() == n and f.get_fft_data() is None
        d = torch.from_numpy(_host(B)).cuda()
        f.work(d[:, :n - 100].contiguous())
        f.work(d[:, n - 100:n].contiguous())
        assert f.get_fft_data() is None                                   # full; the transform runs when the next sample arrives
        f.work(d[:, n:].contiguous())
        got = f.get_fft_data()
        assert got is not None and got.shape == (rs.NB, n)
        got = got.cpu().numpy()
    finally:
        f.close()
    w = np.hamming(n).astype(np.float32)
    for b in range(rs.NB):
        want = orc.power_spectrum(B[b, :n], w)
        strong = want > want.max() - 80.0
        assert np.max(np.abs(got[b][strong] - want[strong])) < 0.05, b
        assert np.argmax(got[b]) == np.argmax(want), b
