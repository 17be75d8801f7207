#!/usr/bin/env python3
"""Times the DMR receive call layer (docs/MEASUREMENT.md, "DMR receive call layer", describes the measurement; the table this tool prints goes there).

    python tools/dmr_rx_ab.py [--batch 16384] [--slots 16] [--warmup 5] [--steps 200] [--cpu-streams 512] [--out table.md]

Shape: `batch` streams x `slots` mailbox slots of a running voice call: every stream holds `slots` consecutive voice bursts of the recorded
whole call of tests/golden/ref/dmr_rx.npz (30 bursts: the call's LC, the alias header and blocks 1..3), from a start drawn per stream, so the
lanes of a wave sit at different places of the superframe and the alias.  The tracker is promiscuous (a call entered late), counts = NULL.
Three figures: qrl_dmr_l2_decode alone, qrl_dmr_rx_process alone (HIP events on the null stream around every single call, warm-up calls
first; median, min .. max), and the same scalar core (dmr_rx_core.hpp through tests/host/dmr_rx_core_shim.cpp, g++ -O2) on one CPU core over
`cpu-streams` of the streams, scaled to the batch.  Before anything is timed the device's records of the first call are compared with the
core's for those streams, byte for byte.  No GPU: the tool fails."""
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
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--cpu-streams", type=int, default=512)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dmr_rx_ab.py needs a GPU")
    import dmr_rx
    import qradiolink_amd as q
    g = dmr_rx.load_golden()
    _, inp, _, _, _, _ = dmr_rx.scenario(g, "whole_call")
    voice = inp[2:32]                                      # 30 voice bursts, five superframes
    B, n = args.batch, args.slots
    rng = np.random.RandomState(16384)
    start = rng.randint(0, 30, B)
    records = voice[(start[:, None] + np.arange(n)[None, :]) % 30]
    ctx = q.Context(0)
    lib = ctx.lib
    d_in = torch.from_numpy(np.ascontiguousarray(records)).cuda()
    d_l2 = torch.empty((B, n, 80), dtype=torch.uint8, device="cuda")
    d_out = torch.empty((B, n, 128), dtype=torch.uint8, device="cuda")
    rx = q.DmrRx(ctx, B, colour_code=1, promiscuous=True)
    torch.cuda.synchronize()
    l2_call = lambda: lib.qrl_dmr_l2_decode(ctx.h, None, d_in.data_ptr(), None, B, n, 1, d_l2.data_ptr())
    rx_call = lambda: lib.qrl_dmr_rx_process(rx.h, None, d_l2.data_ptr(), None, n, d_out.data_ptr())
    assert l2_call() == 0 and rx_call() == 0
    torch.cuda.synchronize()
    # correctness at the timed size: the first call of a fresh handle against the scalar core
    core = dmr_rx.load_core(tempfile.mkdtemp())
    l2_host, first = d_l2.cpu().numpy(), d_out.cpu().numpy()
    m = min(args.cpu_streams, B)
    pick = rng.choice(B, m, replace=False)
    for b in pick:
        want, l2_core, _, _ = core.run(records[b], 1, 1)
        assert np.array_equal(l2_core, l2_host[b]) and np.array_equal(want, first[b]), "stream %d differs from the scalar core" % b

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(torch.cuda.default_stream())
            assert call() == 0
            b.record(torch.cuda.default_stream())
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    rounds = [(timed(l2_call), timed(rx_call)) for _ in range(2)]
    # one CPU core: the same scalar core over the layer-2 records of `m` streams, state carried, repeated until about a second has passed
    l2_pick = np.ascontiguousarray(l2_host[pick])
    out = bytearray(128 * n)
    states = [bytearray(dmr_rx.STATE_BYTES) for _ in range(m)]
    bufs = [bytearray(l2_pick[i].tobytes()) for i in range(m)]
    u8 = lambda b: (C.c_uint8 * len(b)).from_buffer(b)
    args_c = [(u8(states[i]), u8(bufs[i])) for i in range(m)]
    o = u8(out)
    reps = 200
    t0 = time.perf_counter()
    for st, l2 in args_c:
        core.lib.core_dmr_rx_run_l2(1, 1, st, l2, n, o, reps)
    cpu_s = (time.perf_counter() - t0) / (reps * m * n)
    lines = ["| call | device, median of %d (min – max), round 1 / round 2 | one CPU core, same scalar code |" % args.steps, "|---|---|---|"]
    fmt = lambda t: "%.4f ms (%.4f – %.4f)" % t
    lines.append("| `qrl_dmr_l2_decode`, %d streams × %d voice bursts, `audio_fec = 1` | %s / %s | — |" % (B, n, fmt(rounds[0][0]), fmt(rounds[1][0])))
    lines.append("| `qrl_dmr_rx_process` on its records | **%s** / %s | %.1f ms (%.3f µs per burst) |" % (fmt(rounds[0][1]), fmt(rounds[1][1]), 1e3 * cpu_s * B * n, 1e6 * cpu_s))
    share = rounds[0][1][0] / (rounds[0][0][0] + rounds[0][1][0])
    lines.append("")
    lines.append("The tracker's share of layer 2 + tracker: %.0f %% (round 1 medians).  %d of the streams compared with the scalar core before timing: equal." % (100 * share, m))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    rx.close()
    ctx.close()


if __name__ == "__main__":
    main()
