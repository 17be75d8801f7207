#!/usr/bin/env python3
"""Times the repeater-mode DMR receive chain (docs/MEASUREMENT.md, "DMR repeater-mode receive", describes the measurement; the table this tool
prints goes there).

    python tools/dmr_sink_ab.py [--batch 16384] [--bursts 16] [--warmup 5] [--steps 100] [--cpu-streams 256] [--out table.md]

Shape: `batch` streams x `bursts` bursts of downlink bits, one bit per byte: every stream holds the recorded downlink of
tests/golden/ref/dmr_sink.npz (scenario voice_superframe: header, voice A..F and terminator on TS1, CSBKs on TS2) from a burst drawn per
stream, behind a sync-free run of its own length (0..287 bits), so the lanes of a wave stand at different places of a burst.  Two figures
on the device: qrl_dmr_sink_process alone, and the three-stage chain sink -> qrl_dmr_l2_decode -> qrl_dmr_rx_process_slots on one HIP stream
(HIP events around every single call or chain, warm-up first; median, min .. max; the sink is reset before each so that every pass walks the
same states).  Baseline: the same core header (dmr_sink_core.hpp through tests/host/dmr_sink_core_shim.cpp, g++ -O2) on one CPU core over
`cpu-streams` of the streams, scaled to the batch.  Before anything is timed the device's records of those streams are compared with the
core's, byte for byte.  No GPU: the tool fails."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--bursts", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--cpu-streams", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dmr_sink_ab.py needs a GPU")
    import dmr_sink
    import qradiolink_amd as q
    g = dmr_sink.load_golden()
    x, _ = dmr_sink.scenario(g, "voice_superframe")
    air = x.bits.reshape(-1, 288)                              # 16 bursts, TS1 and TS2 alternating
    B, nb = args.batch, args.bursts
    n = 288 * (nb + 1)
    rng = np.random.RandomState(16384)
    start, lead = rng.randint(0, air.shape[0], B), rng.randint(0, 288, B)
    quiet = dmr_sink.quiet(288, 7)
    bits = np.zeros((B, n), np.uint8)
    for b in range(B):
        row = np.concatenate([quiet[:lead[b]], air[(start[b] + np.arange(nb)) % air.shape[0]].reshape(-1)])
        bits[b, :row.size] = row
    counts = (lead + 288 * nb).astype(np.int32)
    ctx = q.Context(0)
    lib = ctx.lib
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    cap = nb + 1
    sink = q.DmrSink(ctx, B, cap_frames=cap, stream=s)
    rx = q.DmrRx(ctx, B, colour_code=1, promiscuous=True)
    rx.set_mode(q.DMR_MODE_REPEATER, 1)
    d_bits, d_counts = torch.from_numpy(bits).cuda(), torch.from_numpy(counts).cuda()
    d_l2 = torch.zeros((B, cap, 80), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((B, cap, 128), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def sink_call():
        sink.reset()
        sink.process(d_bits, d_counts, sync=False)
        return 0

    def chain_call():
        sink_call()
        rc = lib.qrl_dmr_l2_decode(ctx.h, C.c_void_p(s), sink.frames.data_ptr(), sink.counts.data_ptr(), B, cap, 1, d_l2.data_ptr())
        rx.reset(stream=s)
        rx.process_slots(d_l2, sink.slot_info, sink.counts, out=d_out, stream=s)
        return rc

    assert chain_call() == 0
    stream.synchronize()
    core = dmr_sink.load_core(tempfile.mkdtemp())
    frames, info, found = sink.frames.cpu().numpy(), sink.slot_info.cpu().numpy(), sink.counts.cpu().numpy()
    m = min(args.cpu_streams, B)
    pick = rng.choice(B, m, replace=False)
    for b in pick:
        f, i, got = core.call(np.zeros(dmr_sink.STATE_BYTES, np.uint8), bits[b, :counts[b]], cap)
        assert got == int(found[b]) and np.array_equal(f[:got], frames[b, :got]) and np.array_equal(i[:got], info[b, :got]), "stream %d differs from the core" % b

    def timed(call):
        for _ in range(args.warmup):
            call()
        stream.synchronize()
        ms = []
        for _ in range(args.steps):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            assert call() == 0
            z.record(stream)
            z.synchronize()
            ms.append(a.elapsed_time(z))
        return statistics.median(ms), min(ms), max(ms)

    rounds = [(timed(sink_call), timed(chain_call)) for _ in range(2)]
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        for b in pick:
            core.call(np.zeros(dmr_sink.STATE_BYTES, np.uint8), bits[b, :counts[b]], cap)
    cpu_s = (time.perf_counter() - t0) / (reps * m)
    fmt = lambda t: "%.4f ms (%.4f – %.4f)" % t
    lines = ["| call | device, median of %d (min – max), round 1 / round 2 | one CPU core, same core header |" % args.steps, "|---|---|---|",
             "| `qrl_dmr_sink_process`, %d streams × %d bursts (%d bits a stream), after a reset | **%s** / %s | %.1f ms (%.2f µs per stream) |"
             % (B, nb, 288 * nb, fmt(rounds[0][0]), fmt(rounds[1][0]), 1e3 * cpu_s * B, 1e6 * cpu_s),
             "| sink → `qrl_dmr_l2_decode` → `qrl_dmr_rx_process_slots`, one HIP stream | %s / %s | — |" % (fmt(rounds[0][1]), fmt(rounds[1][1])), "",
             "%d bursts found in all; %d of the streams compared with the core header before timing: equal." % (int(found.sum()), m)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    sink.close()
    rx.close()
    ctx.close()


if __name__ == "__main__":
    main()
