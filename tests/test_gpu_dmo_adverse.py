"""a37b on the GPU, the whole state machine: k_dmo_sink behind port 3 of the HIP gr_demod_dmr chain against the oracle
(orc.demod_dmr_port3 -> orc.DmoSink) on the named scenarios of tests/sig.py (what each scenario reaches is asserted on the CPU, from the
oracle's records and state, by tests/test_dmo_scenarios.py).  Every comparison is bit for bit: records as (type, fn, colour code, 33
bytes), the per-call counts, and the demodulator's own ports for a few streams, so that a chain that leaves the oracle under heavy noise
shows up as an upstream failure and not as a slicer failure.  There is no tolerance in this file."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import orc
import sig

pytestmark = pytest.mark.gpu

# BATCHES ABOVE 64: a full wave plus eight lanes, i.e. a second workgroup; every stream distinct, the lanes of one wave in different states.
BATCH = 72
# WINDOW WRAP: delays (IQ samples of carrier in front of the long voice call, seed = lane, carrier offset of the lane) found on the CPU
# with DmoSink.peek for which the first sync lands at ring slot 0, 1 and 1439: the `mn >= mx` arm of the re-sync window is taken at
# syncPtr 0 (window 1439, 0, 1) and 1439 (1438, 1439, 0), and slot 1 is the last one on the other arm (0, 1, 2).
SLOT_LANES = {0: (0, 34008), 1: (1, 34051), 2: (1439, 33970)}      # lane: (ring slot of the first sync, delay)
LOST_SYNC_LANES = (3, 40, 66)                                       # 1.3 M samples each: a handful, one of them in the second workgroup
_ROTA = ("data_call", "impaired2", "drifting_level", "after_reset", "impaired0", "long_voice_call", "data_call", "impaired3", "data_call", "impaired4",
         "drifting_level", "data_call", "impaired1", "impaired5", "after_reset", "impaired6", "impaired7")
SHORT_IQ = 260000       # VERY SHORT CALLS: stream length of the max_chunk = 2502 case (104 calls; the lead and the first three bursts)


def lane(b):
    """(scenario, seed, delay, carrier offset in Hz) of stream b"""
    cfo = -300.0 + 600.0 * ((b * 37) % BATCH) / (BATCH - 1)
    if b in SLOT_LANES:
        return "long_voice_call", b, SLOT_LANES[b][1], cfo
    return ("lost_sync" if b in LOST_SYNC_LANES else _ROTA[b % len(_ROTA)]), b, (b * 8329) % 60000, cfo


def lanes_of(name):
    return [b for b in range(BATCH) if lane(b)[0] == name and b not in SLOT_LANES]


def first_sync_slot(port3):
    """ring slot (syncPtr) the oracle holds when it cuts its first record, and the slots it holds at every later record of the call"""
    snk, slots = orc.DmoSink(), []
    for s in range(0, port3.size, 60):
        if snk.process(port3[s:s + 60]) and snk.peek("state") != 0:
            slots.append(snk.peek("syncPtr"))
    return slots[0], slots


class Air:
    """the batch, built once: ragged host IQ (every stream as long as its scenario), the oracle's port 3 and records of every stream
    continued to the common length by repeating the stream from its start (a new call with a phase step, at another ring position)"""

    def __init__(self):
        with ThreadPoolExecutor(8) as pool:
            self.x = list(pool.map(lambda b: sig.dmo_iq(lane(b)[0], seed=lane(b)[1], delay=lane(b)[2], cfo=lane(b)[3])[1], range(BATCH)))
            self.n = max(x.size for x in self.x)
            self.port3 = list(pool.map(lambda b: orc.demod_dmr_port3(self.row(b)), range(BATCH)))
        self.want = [orc.DmoSink().process(p, cap=256) for p in self.port3]
        self._dev = None

    def row(self, b, n=None):
        return np.resize(self.x[b], n or self.n)

    def device(self):
        import torch
        if self._dev is None:
            self._dev = torch.empty((BATCH, self.n), dtype=torch.complex64, device="cuda")
            for b, x in enumerate(self.x):
                d = torch.from_numpy(x).cuda()
                self._dev[b] = d.repeat(-(-self.n // x.size))[:self.n]
        return self._dev


@pytest.fixture(scope="module")
def air():
    return Air()


def _chain_equals_oracle(out, iq, streams):
    """ports 2 and 1 of the demodulator itself against orc.demod_dmr"""
    for b in streams:
        ref = orc.demod_dmr(iq(b))
        assert np.array_equal(out["bits_a"][b], ref["bits_a"]) and ref["bits_a"].size > 500, "stream %d: the chain's dibits differ from the oracle (upstream of the slicer)" % b
        assert np.array_equal(out["constellation"][b].view(np.uint32), ref["constellation"].view(np.uint32)), "stream %d: constellation (upstream of the slicer)" % b


def _collect_ports(dem, out, ports, streams):
    cnt = out["counts"].cpu().numpy()
    for k, j in (("constellation", 1), ("bits_a", 2)):
        host = out[k].cpu().numpy()
        for b in streams:
            ports[k].setdefault(b, []).append(host[b, :cnt[b, j]].copy())


def test_slot_lanes_sit_where_the_window_wraps(air):
    """WINDOW WRAP, the condition: the oracle's own state says that lanes 0, 1, 2 acquire at ring slots 0, 1 and 1439 and hold them (+- 1)"""
    for b, (slot, _) in SLOT_LANES.items():
        first, slots = first_sync_slot(air.port3[b][:16000])
        assert first == slot, (b, first)
        assert len(slots) >= 9 and all((s - slot + 1) % 1440 <= 2 for s in slots), (b, slots)


@pytest.mark.parametrize("chunk", [1 << 19, 33334])
def test_every_scenario_in_one_wave_and_a_bit(qrl_ctx, air, chunk):
    """72 distinct streams -- data continuation, the terminator in the wrong state, the frame number wrap, lost sync and re-acquisition,
    unequal averages, refused syncs under noise and fades, the window wrap -- each at its own delay, carrier offset and noise"""
    import qradiolink_amd as q
    d = air.device()
    dem = q.Demod(qrl_ctx, q.MODEM_DMR, batch=BATCH, max_chunk=chunk)
    dem.enable_dmo_sink(cap_frames=32)
    got, counts = [[] for _ in range(BATCH)], []
    # watched upstream: a slot lane each way, lost sync in both workgroups, sigma 0.7 (impaired1), a fade (impaired7), the last lane
    watch = (0, 2, LOST_SYNC_LANES[0], lanes_of("impaired1")[0], LOST_SYNC_LANES[2], lanes_of("impaired7")[-1], BATCH - 1)
    ports = {"constellation": {}, "bits_a": {}}
    for s in range(0, air.n, chunk):
        out = dem.process(d[:, s:s + chunk].contiguous())
        _collect_ports(dem, out, ports, watch)
        counts.append(dem.dmo_counts.cpu().numpy().copy())
        for b, recs in enumerate(dem.dmo_records()):
            got[b].extend(recs)
    dem.close()
    _chain_equals_oracle({k: {b: np.concatenate(v) for b, v in ports[k].items()} for k in ports}, air.row, watch)
    counts = np.stack(counts)
    for b in range(BATCH):
        assert got[b] == air.want[b], "stream %d (%s): records differ from the oracle" % (b, lane(b)[0])
        # per-call counts: what a fresh oracle finds in the port-3 samples of each call (125 IQ samples are 3 port-3 samples)
        snk, edges = orc.DmoSink(), [orc.lib.orc_decim_count(min(s + chunk, air.n), 3, 125) for s in range(0, air.n, chunk)]
        want_counts = [len(snk.process(air.port3[b][a:e], cap=256)) for a, e in zip([0] + edges[:-1], edges)]
        assert list(counts[:, b]) == want_counts, "stream %d: per-call counts" % b
    assert min(len(w) for w in air.want) >= 5 and len({tuple(w) for w in air.want}) == BATCH


def test_very_short_calls(qrl_ctx, air):
    """VERY SHORT CALLS: max_chunk = 2502 is about 60 port-3 samples a call: one burst (660 samples) spans eleven launches, the sync
    correlation, the frame cut and the look-back of 1439 samples all reach into earlier calls"""
    import torch
    import qradiolink_amd as q
    lanes = (lanes_of("data_call")[1], lanes_of("long_voice_call")[0], lanes_of("impaired3")[0])     # (impaired3: a fade that takes the header)
    iq = np.stack([air.x[b][:SHORT_IQ] for b in lanes])
    d = torch.from_numpy(iq).cuda()
    dem = q.Demod(qrl_ctx, q.MODEM_DMR, batch=3, max_chunk=2502)
    dem.enable_dmo_sink(cap_frames=4)
    got = [[] for _ in lanes]
    ports = {"constellation": {}, "bits_a": {}}
    for s in range(0, SHORT_IQ, 2502):
        out = dem.process(d[:, s:s + 2502].contiguous())
        _collect_ports(dem, out, ports, range(3))
        for b, recs in enumerate(dem.dmo_records()):
            got[b].extend(recs)
    dem.close()
    _chain_equals_oracle({k: {b: np.concatenate(v) for b, v in ports[k].items()} for k in ports}, lambda b: iq[b], range(3))
    for b in range(3):
        want = orc.DmoSink().process(orc.demod_dmr_port3(iq[b]))
        assert got[b] == want, "stream %d" % b
        assert len(want) >= 2


def _records(frames, counts):
    """host view of one mailbox: per stream the (type, fn, colour code, 33 bytes) of the records that were written"""
    f, c = frames.cpu().numpy(), counts.cpu().numpy()
    return [[(int(f[b, i, 0]), int(f[b, i, 1]), int(f[b, i, 2]), f[b, i, 4:37].tobytes()) for i in range(min(int(c[b]), f.shape[1]))] for b in range(f.shape[0])]


def test_mailbox_overflow_drops_records_and_reports_them(qrl_ctx, air):
    """MAILBOX OVERFLOW: cap_frames = 4 and a call that holds the ten bursts of the long voice call: counts[b] says 10 (> cap: "lost"), the
    four records written are the oracle's first four, nothing is written beyond them -- stream 1, whose mailbox lies right behind stream 0's
    in the buffer, is plain carrier in that call and its mailbox keeps the pattern it was filled with -- and the next call goes on correctly"""
    import torch
    import qradiolink_amd as q
    cap = 4
    voice, data = air.x[lanes_of("long_voice_call")[0]], air.x[lanes_of("data_call")[0]]
    n = voice.size
    carrier = sig.make_4fsk(levels=np.zeros(n // 208 + 2), seed=77)[0][:n]
    iq = np.stack([np.concatenate([voice, voice]), np.concatenate([carrier, np.resize(data, n)])])
    d = torch.from_numpy(iq).cuda()
    dem = q.Demod(qrl_ctx, q.MODEM_DMR, batch=2, max_chunk=n)
    dem.enable_dmo_sink(cap_frames=cap)
    edge = orc.lib.orc_decim_count(n, 3, 125)
    want = []
    for b in range(2):
        snk, p3 = orc.DmoSink(), orc.demod_dmr_port3(iq[b])
        want.append([snk.process(p3[:edge]), snk.process(p3[edge:])])
    assert len(want[0][0]) == 10 and want[1][0] == [] and len(want[0][1]) >= 7 and len(want[1][1]) >= 5      # (cap = 4: each of them overflows)
    ports = {"constellation": {}, "bits_a": {}}
    for call in range(2):
        dem.dmo_frames.fill_(0xA5)
        dem.dmo_counts.fill_(-1)
        torch.cuda.synchronize()
        out = dem.process(d[:, call * n:(call + 1) * n].contiguous())
        _collect_ports(dem, out, ports, range(2))
        raw, counts = dem.dmo_frames.cpu().numpy(), dem.dmo_counts.cpu().numpy()
        for b in range(2):
            assert counts[b] == len(want[b][call]), (call, b, counts)
            written = min(len(want[b][call]), cap)
            assert dem.dmo_records()[b] == want[b][call][:cap], (call, b)
            assert np.all(raw[b, written:] == 0xA5), "call %d stream %d: bytes behind the records were written" % (call, b)
        assert counts.max() > cap
    dem.close()
    _chain_equals_oracle({k: {b: np.concatenate(v) for b, v in ports[k].items()} for k in ports}, lambda b: iq[b], range(2))


def test_reset_with_the_sink_enabled(qrl_ctx, air):
    """RESET: half a stream, qrl_demod_reset, then another stream from its start: the records are those of a fresh oracle on the second
    stream alone.  The cut lies where the machine is in RECV_VOICE with a live endPtr (asserted from the oracle's state), so a reset
    that left any of state, endPtr, the averages or the ring behind would cut a frame out of the new stream's lead"""
    import torch
    import qradiolink_amd as q
    first = [air.x[lanes_of("long_voice_call")[0]], air.x[lanes_of("drifting_level")[0]]]
    second = [air.x[lanes_of("data_call")[2]], air.x[lanes_of("long_voice_call")[1]]]
    chunk = 100000
    cut = 4 * chunk
    for x in first:
        snk = orc.DmoSink()
        assert len(snk.process(orc.demod_dmr_port3(x[:cut]))) >= 4
        assert snk.peek("state") == 3 and snk.peek("endPtr") < 1440 and snk.peek("syncCount") >= 1
    n = min(x.size for x in second)
    a, b2 = torch.from_numpy(np.stack([x[:cut] for x in first])).cuda(), torch.from_numpy(np.stack([x[:n] for x in second])).cuda()
    dem = q.Demod(qrl_ctx, q.MODEM_DMR, batch=2, max_chunk=chunk)
    dem.enable_dmo_sink(cap_frames=8)
    before, got = [[], []], [[], []]
    for s in range(0, cut, chunk):
        dem.process(a[:, s:s + chunk].contiguous())
        for b, recs in enumerate(dem.dmo_records()):
            before[b].extend(recs)
    dem.reset()
    ports = {"constellation": {}, "bits_a": {}}
    for s in range(0, n, chunk):
        out = dem.process(b2[:, s:s + chunk].contiguous())
        _collect_ports(dem, out, ports, range(2))
        for b, recs in enumerate(dem.dmo_records()):
            got[b].extend(recs)
    dem.close()
    _chain_equals_oracle({k: {b: np.concatenate(v) for b, v in ports[k].items()} for k in ports}, lambda b: second[b][:n], range(2))
    for b in range(2):
        assert before[b] == orc.DmoSink().process(orc.demod_dmr_port3(first[b][:cut]))
        want = orc.DmoSink().process(orc.demod_dmr_port3(second[b][:n]))
        assert got[b] == want and len(want) >= 5, "stream %d" % b


def test_back_to_back_calls_with_two_mailboxes(qrl_ctx, air):
    """ASYNC USE: the double-buffered mailboxes that the header of qrl_demod_set_dmo_output describes: before every process_async the output
    moves to the other (frames, counts) pair and the host waits only after every second call.  Same records as with a wait after every
    call, and as the oracle.  With two calls in flight the slicer of call k looks back 1439 samples into ring r3 while the filter of
    call k + 1 may already write that ring."""
    import torch
    import qradiolink_amd as q
    lanes = tuple(SLOT_LANES)                       # the three long voice calls at ring slots 0, 1, 1439
    chunk, cap = 33334, 4
    n = min(air.x[b].size for b in lanes)
    iq = np.stack([air.x[b][:n] for b in lanes])
    d = torch.from_numpy(iq).cuda()
    parts = [d[:, s:s + chunk].contiguous() for s in range(0, n, chunk)]
    boxes = [(torch.zeros((3, cap, 40), dtype=torch.uint8, device="cuda"), torch.zeros((3,), dtype=torch.int32, device="cuda")) for _ in range(2)]
    torch.cuda.synchronize()
    runs, ports = {}, {"constellation": {}, "bits_a": {}}
    for every in (2, 1):
        dem = q.Demod(qrl_ctx, q.MODEM_DMR, batch=3, max_chunk=chunk)
        got = [[] for _ in lanes]
        pending = []
        for k, part in enumerate(parts):
            frames, counts = boxes[k % 2]
            assert dem.lib.qrl_demod_set_dmo_output(dem.h, frames.data_ptr(), cap, counts.data_ptr()) == 0
            dem.process_async(part)
            pending.append(k)
            if len(pending) == every or k == len(parts) - 1:
                dem.sync()
                if every == 1:
                    _collect_ports(dem, dem._ports(), ports, range(3))
                for j in pending:
                    for b, recs in enumerate(_records(*boxes[j % 2])):
                        got[b].extend(recs)
                pending = []
        dem.close()
        runs[every] = got
    _chain_equals_oracle({k: {b: np.concatenate(v) for b, v in ports[k].items()} for k in ports}, lambda b: iq[b], range(3))
    assert runs[2] == runs[1]
    for i in range(3):
        want = orc.DmoSink().process(orc.demod_dmr_port3(iq[i]))
        assert runs[2][i] == want and len(want) == 10, "stream %d" % i
