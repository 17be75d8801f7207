"""The repeater-mode DMR burst sink on the GPU (k_dmr_sink through qrl_dmr_sink_process): the reference's recorded frame and slot records
(tests/golden/ref/dmr_sink.npz) are the expected values, byte for byte, call by call; the reference itself is not read here."""
import numpy as np
import pytest

import dmr_sink

pytestmark = pytest.mark.gpu
G = dmr_sink.load_golden()
N = dmr_sink.NSTREAMS
FILL = 0xEE


def _run(ctx, idx, stride, junk=0, cap=None):
    """the scenarios idx as the streams of one handle, call j of the handle = call j of every stream (counts 0 for a stream that has no call
    j left); a flush or reset before call j where a scenario has one (such a scenario runs alone).  Bytes behind a stream's count are 1s,
    which would show in the records if they were read; junk goes into the upper seven bits of every byte.  Every call's counts and records
    are compared with the reference's."""
    import torch
    import qradiolink_amd as q
    scn = [dmr_sink.scenario(G, k) for k in idx]
    B = len(scn)
    cap = max(x.cap for x, _ in scn) if cap is None else cap
    assert all(x.cap == cap for x, _ in scn) and (B == 1 or not any(x.ops for x, _ in scn))
    ncalls = max(len(x.cuts) for x, _ in scn)
    sink = q.DmrSink(ctx, B, cap_frames=cap)
    at, rec = [0] * B, [0] * B
    try:
        for j in range(ncalls):
            sizes = [x.cuts[j] if j < len(x.cuts) else 0 for x, _ in scn]
            assert max(sizes) <= stride
            op = scn[0][0].ops.get(j, 0)
            if op == dmr_sink.FLUSH:
                sink.flush()
            elif op == dmr_sink.RESET:
                sink.reset()
            host = np.full((B, stride), 1 | junk, np.uint8)
            for b, (x, _) in enumerate(scn):
                host[b, :sizes[b]] = x.bits[at[b]:at[b] + sizes[b]] | junk
                at[b] += sizes[b]
            sink.frames.fill_(FILL)
            sink.slot_info.fill_(FILL)
            counts = torch.from_numpy(np.array(sizes, np.int32)).cuda()
            frames, info, found = sink.process(torch.from_numpy(host).cuda(), counts, n=max(sizes))
            frames, info, found = frames.cpu().numpy(), info.cpu().numpy(), found.cpu().numpy()
            for b, (x, exp) in enumerate(scn):
                want = int(exp["counts"][j]) if j < len(x.cuts) else 0
                assert int(found[b]) == want, "stream %d (%s), call %d: %d bursts, the reference %d" % (b, x.name, j, found[b], want)
                w = min(want, cap)
                mine = np.nonzero(exp["call_of"] == j)[0][:w]
                assert np.array_equal(frames[b, :w], exp["frames"][mine]), "stream %d (%s), call %d: frame records" % (b, x.name, j)
                assert np.array_equal(info[b, :w], exp["info"][mine]), "stream %d (%s), call %d: slot records" % (b, x.name, j)
                assert (frames[b, w:] == FILL).all() and (info[b, w:] == FILL).all(), "stream %d (%s), call %d: written past the count or the cap" % (b, x.name, j)
                rec[b] += w
        for b, (x, exp) in enumerate(scn):
            assert rec[b] == len(dmr_sink.written(exp, cap)[0])
    finally:
        sink.close()


def _fits(idx, stride, cap=64):
    return [k for k in idx if max(dmr_sink.scenario(G, k)[0].cuts) <= stride and dmr_sink.scenario(G, k)[0].cap == cap]


def test_72_streams_against_the_golden(qrl_ctx):
    """a wave and a bit: every scenario that shares a handle, each stream another scenario or the same one behind another number of bits"""
    idx = _fits(range(N), 3360)
    assert len(idx) == N - 1    # all but cap_two, which has a mailbox of its own size
    _run(qrl_ctx, idx + [0], 3360)


@pytest.mark.parametrize("batch", [1, 64])
def test_batch_1_and_64(qrl_ctx, batch):
    _run(qrl_ctx, _fits(range(N), 3360)[:batch], 3360)


def test_stride_1000_and_junk_in_the_upper_bits(qrl_ctx):
    """a stride that is no multiple of the tile; only bit 0 of a byte counts (packFrame and findSync mask it)"""
    idx = _fits(range(N), 1000)
    assert len(idx) >= 64
    _run(qrl_ctx, idx, 1000, junk=0xA4)


def test_stride_1001_takes_the_byte_path(qrl_ctx):
    _run(qrl_ctx, _fits(range(N), 1000)[3:70], 1001)


def test_cap_two_writes_nothing_past_the_cap(qrl_ctx):
    k = list(G["names"]).index("cap_two")
    x, exp = dmr_sink.scenario(G, k)
    assert x.cap == 2 and int(exp["counts"][0]) == 5
    _run(qrl_ctx, [k], 1440)


@pytest.mark.parametrize("name", ["flush_mid_voice", "flush_in_search", "reset_mid_burst", "reset_remainder"])
def test_flush_and_reset(qrl_ctx, name):
    _run(qrl_ctx, [list(G["names"]).index(name)], 3360)


def test_long_quiet_run_one_call_and_many(qrl_ctx):
    """the trim argument: the same 3 x 288 + 300 sync-free bits and bursts as one call and as many give the same records"""
    names = list(G["names"])
    a, b = names.index("long_quiet_one_call"), names.index("long_quiet_many_calls")
    _run(qrl_ctx, [a], 3360)
    _run(qrl_ctx, [b], 3360)
    ea, eb = dmr_sink.scenario(G, a)[1], dmr_sink.scenario(G, b)[1]
    assert np.array_equal(ea["frames"], eb["frames"]) and np.array_equal(ea["info"], eb["info"]) and len(ea["frames"]) == 4


# ------------------------------------------------------------------------------------------------------------------ the call layer, repeater mode
def _tracker(ctx, config):
    import qradiolink_amd as q
    cc, prom, mode, ts = config
    rx = q.DmrRx(ctx, 1, colour_code=cc, promiscuous=bool(prom))
    rx.set_mode(mode, ts)
    return rx


@pytest.mark.parametrize("name", [str(n) for n in G["rx_names"]])
def test_call_layer_against_the_golden(qrl_ctx, name):
    """qrl_dmr_l2_decode -> qrl_dmr_rx_process_slots, the configuration switched between calls where the scenario says"""
    import torch
    import qradiolink_amd as q
    import dmr_rx
    x, want = dmr_sink.rx_scenario(G, name)
    rx = _tracker(qrl_ctx, x.config)
    cuts = [0] + [r[0] for r in x.reconfig] + [len(x.frames)]
    cfgs = [x.config] + [r[1:] for r in x.reconfig]
    try:
        for (a, b), (cc, prom, mode, ts) in zip(zip(cuts[:-1], cuts[1:]), cfgs):
            rx.set_config(cc, bool(prom))
            rx.set_mode(mode, ts)
            l2 = q.dmr_l2_decode(qrl_ctx, torch.from_numpy(np.ascontiguousarray(x.frames[None, a:b])).cuda(), audio_fec=bool(dmr_rx.AUDIO_FEC))
            got = rx.process_slots(l2, torch.from_numpy(np.ascontiguousarray(x.slots[None, a:b])).cuda()).cpu().numpy()[0]
            bad = np.nonzero((got != want[a:b]).any(axis=1))[0]
            assert not len(bad), "bursts %s differ; first: device %s, reference %s" % (a + bad[:8], got[bad[0], :16], want[a + bad[0], :16])
        assert int(rx.state().cpu().numpy()[0, 3]) == int(want[-1, 5])      # _timeslot_RX in the public state
    finally:
        rx.close()


def test_chain_sink_l2_call_layer_on_one_stream(qrl_ctx):
    """sink -> qrl_dmr_l2_decode -> qrl_dmr_rx_process_slots queued on one HIP stream, nothing waited for in between; every call's records
    against what the reference's DMRControl made of the reference sink's own bursts (chain_call of the golden)"""
    import ctypes as C
    import torch
    import qradiolink_amd as q
    import dmr_rx
    idx = _fits(range(N), 3360)
    scn = [dmr_sink.scenario(G, k) for k in idx]
    B, cap, stride = len(scn), 64, 3360
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    sink = q.DmrSink(qrl_ctx, B, cap_frames=cap, stream=s)
    cc, prom, mode, ts = dmr_sink.CHAIN_CONFIG
    rx = q.DmrRx(qrl_ctx, B, colour_code=cc, promiscuous=bool(prom))
    rx.set_mode(mode, ts)
    l2 = torch.zeros((B, cap, 80), dtype=torch.uint8, device="cuda")
    out = torch.zeros((B, cap, 128), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    at, seen = [0] * B, [0] * B
    try:
        for j in range(max(len(x.cuts) for x, _ in scn)):
            sizes = [x.cuts[j] if j < len(x.cuts) else 0 for x, _ in scn]
            host = np.ones((B, stride), np.uint8)
            for b, (x, _) in enumerate(scn):
                host[b, :sizes[b]] = x.bits[at[b]:at[b] + sizes[b]]
                at[b] += sizes[b]
            bits, counts = torch.from_numpy(host).cuda(), torch.from_numpy(np.array(sizes, np.int32)).cuda()
            torch.cuda.synchronize()
            frames, info, found = sink.process(bits, counts, n=max(sizes), sync=False)
            assert q.load_library().qrl_dmr_l2_decode(qrl_ctx.h, C.c_void_p(s), frames.data_ptr(), found.data_ptr(), B, cap, dmr_rx.AUDIO_FEC, l2.data_ptr()) == 0
            rx.process_slots(l2, info, found, out=out, stream=s)
            stream.synchronize()
            got, cnt = out.cpu().numpy(), found.cpu().numpy()
            for b, (x, exp) in enumerate(scn):
                c = int(cnt[b])
                assert c == (int(exp["counts"][j]) if j < len(x.cuts) else 0) <= cap
                want = G["chain_call"][idx[b], seen[b]:seen[b] + c]
                assert np.array_equal(got[b, :c], want), "stream %d (%s), call %d" % (b, x.name, j)
                assert not got[b, c:].any()
                seen[b] += c
        assert all(seen[b] == len(exp["frames"]) for b, (_, exp) in enumerate(scn)) and sum(seen) > 400
    finally:
        sink.close()
        rx.close()


def test_behind_the_demodulator(qrl_ctx, tmp_path):
    """a QRL_MODEM_DMR handle at 1 Msps, three streams of the downlink of scenario 1 from the project's DMR modulator; Demod.enable_dmr_sink
    with layer 2 and the call layer behind it, process() in three ragged calls.  The port-2 bits are the oracle chain's, and every call's
    bursts are those of the core header run on the oracle's bits under the same cuts."""
    import torch
    import orc
    import dmr_rx
    import qradiolink_amd as q
    core = dmr_sink.load_core(tmp_path)
    rows = dmr_sink.radio_rows(G)
    B, cap = rows.shape[0], 16
    mod = q.Mod(qrl_ctx, q.MODEM_DMR, batch=B, max_bytes=rows.shape[1])
    iq = (mod.process(torch.from_numpy(rows).cuda()) * dmr_sink.RADIO_LEVEL).contiguous()
    mod.close()
    n = iq.shape[1]
    dem = q.Demod(qrl_ctx, q.MODEM_DMR, batch=B, max_chunk=n)
    with pytest.raises(RuntimeError):
        dem.enable_dmr_sink_l2()
    dem.enable_dmr_sink(cap_frames=cap)
    with pytest.raises(RuntimeError):
        dem.enable_dmr_sink_call()
    dem.enable_dmr_sink_l2(audio_fec=False)
    dem.enable_dmr_sink_call(colour_code=1, promiscuous=True, timeslot=1)
    ref_bits = [orc.demod_dmr(orc.mod_dmr(rows[b]) * np.float32(dmr_sink.RADIO_LEVEL))["bits_a"] for b in range(B)]
    states = [np.zeros(dmr_sink.STATE_BYTES, np.uint8) for _ in range(B)]
    rx_state = [np.zeros(dmr_rx.STATE_BYTES, np.uint8) for _ in range(B)]
    at, total = [0] * B, [0] * B
    cuts = [0, (n // 5) & ~1, (3 * n // 5 + 1234) & ~1, n]
    try:
        for a, z in zip(cuts[:-1], cuts[1:]):
            out = dem.process(iq[:, a:z].contiguous())
            produced = out["counts"].cpu().numpy()[:, 2]
            bits = out["bits_a"].cpu().numpy()
            frames, info, found = dem.dmr_frames.cpu().numpy(), dem.dmr_slot_info.cpu().numpy(), dem.dmr_counts.cpu().numpy()
            call = dem.dmr_call.cpu().numpy()
            for b in range(B):
                k = int(produced[b])
                mine = ref_bits[b][at[b]:at[b] + k]
                assert np.array_equal(bits[b, :k], mine), "stream %d: port 2 differs from the oracle chain's" % b
                at[b] += k
                f, i, got = core.call(states[b], mine, cap)
                assert int(found[b]) == got <= cap, "stream %d: %d bursts, the core on the oracle's bits %d" % (b, found[b], got)
                assert np.array_equal(frames[b, :got], f[:got]) and np.array_equal(info[b, :got], i[:got]), "stream %d" % b
                x = dmr_sink.RxScenario("radio", (1, 1, dmr_sink.MODE_REPEATER, 1))
                x.frames, x.slots = f[:got], i[:got]
                l2, o = np.zeros((max(got, 1), 80), np.uint8), np.zeros((max(got, 1), 128), np.uint8)
                if got:
                    core.lib.core_dmr_rxs_run(1, 1, 1, 1, 0, dmr_sink._p(rx_state[b], dmr_sink.C.c_uint8), dmr_sink._p(np.ascontiguousarray(f[:got]), dmr_sink.C.c_uint8),
                                              dmr_sink._p(np.ascontiguousarray(i[:got]), dmr_sink.C.c_uint8), got, dmr_sink._p(l2, dmr_sink.C.c_uint8), dmr_sink._p(o, dmr_sink.C.c_uint8))
                    assert np.array_equal(call[b, :got], o[:got]), "stream %d: call records" % b
                assert not call[b, got:].any()
                total[b] += got
        assert all(at[b] == len(ref_bits[b]) for b in range(B)) and all(t >= 4 for t in total), (at, total)
        dem.reset()
        torch.cuda.synchronize()
    finally:
        dem.close()
