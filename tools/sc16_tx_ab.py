#!/usr/bin/env python3
"""A/B of qrl_mod_process (cf32 out) against qrl_mod_process_sc16 (int16 out) on one handle shape (docs/MEASUREMENT.md, "sc16 output", describes the measurement; the table this tool prints goes there).

    python tools/sc16_tx_ab.py [--batch 256] [--nbytes 4096] [--rate 25000000] [--warmup 5] [--steps 20] [--out table.md]

Shape: QPSK-250k behind the gr_mod_base back end (rotator at 1 Msps, interpolator to the device rate): `batch` streams x `nbytes` bytes per call,
32 x rate / 1e6 samples per byte.  Two handles see the same bytes, one per format, calls interleaved format by format.  Timing: HIP events on the
handle's own stream around every call (warm-up calls first); reported: ms per call (median, min .. max) for both formats, and the time of ONE
device -> host copy of a call's output into pinned memory for both formats (8 / 4 bytes per sample).  No thresholds: the interpolator is a
thread-per-output FIR of about 209 taps per sample, so the halved store is not expected to shorten the kernel; what the format halves is the
output buffer and the download.  The int16 output is checked against the converted cf32 output before anything is timed.  No GPU: the tool fails."""
import argparse
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--nbytes", type=int, default=4096)
    ap.add_argument("--rate", type=int, default=25000000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sc16_tx_ab.py needs a GPU")
    import qradiolink_amd as q
    ctx = q.Context(0)
    B, n = args.batch, args.nbytes
    count = n * 32 * (args.rate // 1000000)
    data = torch.randint(0, 256, (B, n), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    mk = lambda: q.Mod(ctx, q.MODEM_QPSK250K, batch=B, max_bytes=n, device_samp_rate=args.rate, carrier_offset_hz=25000.0)
    m32, m16 = mk(), mk()
    o32 = torch.empty((B, count), dtype=torch.complex64, device="cuda")
    o16 = torch.empty((B, count, 2), dtype=torch.int16, device="cuda")
    clip = torch.zeros(B, dtype=torch.int32, device="cuda")
    m16.set_sc16_clip_counts(clip)
    torch.cuda.synchronize()
    streams = {32: torch.cuda.ExternalStream(m32.lib.qrl_mod_stream(m32.h)), 16: torch.cuda.ExternalStream(m16.lib.qrl_mod_stream(m16.h))}
    call = {32: lambda: m32.process_async(data, out=o32), 16: lambda: m16.process_sc16_async(data, out=o16)}
    sync = {32: m32.sync, 16: m16.sync}
    # first call of both: the int16 output is the converted cf32 output (row by row: the whole batch as floats would double the footprint)
    call[32](); call[16](); sync[32](); sync[16]()
    for b in range(0, B, max(1, B // 8)):
        r = torch.view_as_real(o32[b]).mul(32767.0).round_().clamp_(-32768, 32767).to(torch.int16)
        assert torch.equal(r, o16[b]), "stream %d: int16 output differs from the converted cf32 output" % b
    assert int(clip.sum()) == 0
    ms = {32: [], 16: []}
    for k in range(args.warmup + args.steps):
        for fmt in ((32, 16) if k % 2 == 0 else (16, 32)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(streams[fmt])
            call[fmt]()
            e1.record(streams[fmt])
            sync[fmt]()
            e1.synchronize()
            if k >= args.warmup:
                ms[fmt].append(e0.elapsed_time(e1))
    # one download of a call's output, pinned host memory, both formats
    d2h = {}
    for fmt, dev in ((32, o32), (16, o16)):
        host = torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True)
        host.copy_(dev)                                               # touches the pages once
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        host.copy_(dev, non_blocking=True)
        e1.record()
        e1.synchronize()
        d2h[fmt] = (e0.elapsed_time(e1), dev.numel() * dev.element_size())
        del host
    box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    med = statistics.median
    lines = ["box: %s; QPSK-250k, %d streams x %d bytes per call at %d Msps (%d samples per stream and call), %d warm-up + %d timed calls per format, interleaved"
             % (box, B, n, args.rate // 1000000, count, args.warmup, args.steps), "",
             "| output format | ms per call median (min .. max) | vs cf32 | output bytes per call | device -> host copy of one call's output, ms | GB/s |",
             "|---|---|---|---|---|---|"]
    for fmt, name in ((32, "cf32 (qrl_mod_process)"), (16, "sc16 (qrl_mod_process_sc16)")):
        t, nb = d2h[fmt]
        lines.append("| %s | %.3f (%.3f .. %.3f) | %.4f | %d | %.3f | %.1f |" % (name, med(ms[fmt]), min(ms[fmt]), max(ms[fmt]), med(ms[fmt]) / med(ms[32]), nb, t, nb / t / 1e6))
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps({"box": box, "batch": B, "nbytes": n, "rate": args.rate, "ms_cf32": ms[32], "ms_sc16": ms[16],
                      "d2h_ms_cf32": d2h[32][0], "d2h_ms_sc16": d2h[16][0]}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    m32.close(); m16.close(); ctx.close()


if __name__ == "__main__":
    main()
