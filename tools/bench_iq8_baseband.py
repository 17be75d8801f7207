#!/usr/bin/env python3
"""The headline shape fed cf32, int16, sc8 and cu8, one process, one GPU, the formats alternating (docs/MEASUREMENT.md, "8-bit at 1 Msps").

    python tools/bench_iq8_baseband.py [--rounds 7] [--steps 30] [--warmup 5] [--rotate K] [--out table.md]

Shape: C1 of bench.py -- 2FSK-1k at 1 Msps, 16384 streams x 262 144 samples, the handle as bench.py opens it (side outputs on, the library's
default options).  Five handles on one context: two are fed the complex64 batch through qrl_demod_process (an A/A pair: what separates them
is what this box and this process cannot resolve), one -- with QRL_OPT_SC16_BASEBAND = 1 -- int16 pairs through qrl_demod_process_sc16, two
-- with QRL_OPT_IQ8_BASEBAND = 1 -- signed and unsigned bytes through qrl_demod_process_sc8 / _cu8.  All see the SAME samples: bench.py's
synthetic batch quantised to 8 bits with a power-of-two gain (the largest that keeps the peak at or below 127 counts); sc8 is v, cu8 is
v + 128 with the bias 128, int16 is 256 v with the scale / 256, cf32 is float(v) * scale.  After the last round the outputs of all five are
compared bit for bit.

A round runs each handle once (the order rotates from round to round): warm-up calls, then `steps` calls queued back to back between two
synchronisations.  Measured per round: the step time from the host clock over the whole queue, the intervals between step completions from
events on the handle's internal streams (bench.py's StepMarks: they order nothing), and the first-stage kernel alone (k_decim_pm) from
qrl_demod_profile's event pair around its launch.  Reported: the median over the rounds with min .. max, the kernel's algorithmic bytes (8, 4
or 2 B of input per sample + 8 B per 50 samples of output ring) and the share of the 8 TB/s HBM roof they make at the kernel's time; the A/A
spread of the cf32 pair; and whether the 8-bit steps beat the int16 step of the same run by more than that spread.  Nothing is asserted
about the times: the exit status is 1 only if the outputs differ.  --rotate K creates the five handles in an order rotated by K: one
handle of several in a process may run slower whatever it is fed (docs/MEASUREMENT.md, "8-bit input"), and a second run with another K tells
a format from a place.  No GPU: the tool fails."""
import argparse
import json
import math
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D = 50                      # the first stage decimates 1:50 onto a cf32 ring
IN_BYTES = {"cf32": 8.0, "cf32 (A/A)": 8.0, "sc16": 4.0, "sc8": 2.0, "cu8": 2.0}


def quantise(iq, torch, rows=1024):
    """[B, n] complex64 -> (sc8 [B, 2 n] int8, cu8 [B, 2 n] uint8, int16 [B, 2 n], [B, n] complex64 = float(v) * scale, scale), a block of
    rows at a time; iq becomes the converted floats in place"""
    B, n = iq.shape
    peak = float(torch.view_as_real(iq).abs().max())
    gain = 2.0 ** math.floor(math.log2(127.0 / peak))
    scale = 1.0 / gain
    v8 = torch.empty((B, 2 * n), dtype=torch.int8, device=iq.device)
    u8 = torch.empty((B, 2 * n), dtype=torch.uint8, device=iq.device)
    v16 = torch.empty((B, 2 * n), dtype=torch.int16, device=iq.device)
    for r in range(0, B, rows):
        f = torch.view_as_real(iq[r:r + rows]).reshape(-1, 2 * n)
        q = f.mul(gain).round_().clamp_(-127, 127)
        v8[r:r + rows] = q.to(torch.int8)
        u8[r:r + rows] = (q + 128.0).to(torch.uint8)
        v16[r:r + rows] = (q * 256.0).to(torch.int16)
        f.copy_(q.mul_(scale))
    return v8, u8, v16, iq, scale, peak * gain


def run_case(bench, torch, dem, call, data, warmup, steps):
    for _ in range(warmup):
        call(data)
    dem.sync()
    torch.cuda.synchronize()
    dem.profile(True)
    marks = bench.StepMarks(torch, dem.internal_streams)
    marks.mark()
    t0 = time.perf_counter()
    for _ in range(steps):
        call(data)
        marks.mark()
    dem.sync()
    dt = time.perf_counter() - t0
    kms, launches, kname = dem.profile_read()
    dem.profile(False)
    assert launches == steps
    return dt / steps * 1e3, marks.spread()["median"], kms / launches, kname


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="streams (default: C1's 16384; smaller values are rehearsals, not the measurement)")
    ap.add_argument("--rotate", type=int, default=0, help="create the handles in the order cf32, sc16, sc8, cf32 (A/A), cu8 rotated by this many places")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_iq8_baseband.py needs a GPU")
    import bench
    import qradiolink_amd as q
    label, mode, modem, rate, offset, dbatch, nsamp, _, abytes = bench.WORKLOADS["c1"]
    batch = args.batch or dbatch
    dev = torch.device("cuda:0")
    ctx = q.Context(0)
    v8, u8, v16, x, scale, peak_counts = quantise(bench.synth(mode, rate, offset, batch, nsamp, 1234, torch, dev), torch)
    torch.cuda.synchronize()
    mk = lambda: q.Demod(ctx, modem, batch=batch, max_chunk=nsamp, device_samp_rate=rate, carrier_offset_hz=offset, side_outputs=True)
    names = ["cf32", "sc16", "sc8", "cf32 (A/A)", "cu8"]
    made = {name: mk() for name in names[args.rotate % 5:] + names[:args.rotate % 5]}      # (dicts keep the order of insertion = of creation)
    d_a, d_16, d_s8, d_b, d_u8 = (made[name] for name in names)
    d_16.enable_sc16_baseband()
    d_16.set_sc16_scale(scale / 256.0)
    for d in (d_s8, d_u8):
        d.enable_iq8_baseband()
    d_s8.set_sc8_scale(scale)
    d_u8.set_cu8_scale(scale, 128.0)
    cases = [("cf32", d_a, d_a.process_async, x), ("sc16", d_16, d_16.process_sc16_async, v16), ("sc8", d_s8, d_s8.process_sc8_async, v8),
             ("cf32 (A/A)", d_b, d_b.process_async, x), ("cu8", d_u8, d_u8.process_cu8_async, u8)]
    rec = {name: {"step": [], "interval": [], "kernel": [], "kname": ""} for name, _, _, _ in cases}
    for r in range(args.rounds):
        for k in range(len(cases)):
            name, dem, call, data = cases[(k + r) % len(cases)]
            step, interval, kern, kname = run_case(bench, torch, dem, call, data, args.warmup, args.steps)
            rec[name]["step"].append(step); rec[name]["interval"].append(interval); rec[name]["kernel"].append(kern); rec[name]["kname"] = kname
    ref = d_a._ports()      # the same samples the same number of times: the last calls agree bit for bit
    same = True
    for name, dem, _, _ in cases[1:]:
        got = dem._ports()
        for port in ("bits_a", "bits_b", "counts", "filtered", "constellation"):
            if not torch.equal(ref[port], got[port]):
                same = False
                sys.stderr.write("port %s: %s and cf32 differ\n" % (port, name))
    assert int(ref["counts"][:, 2].sum()) > 0
    for _, dem, _, _ in cases:
        dem.close()
    med = statistics.median
    box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    samples = float(batch) * nsamp
    lines = ["box: %s; %s, %d x %d samples, peak %.0f counts at scale 1 / %d; %d rounds x %d steps per handle, handles alternating in one process; "
             "handles created in the order %s" % (box, label, batch, nsamp, peak_counts, round(1.0 / scale), args.rounds, args.steps, ", ".join(made)), "",
             "| input | step ms, host clock: median (min .. max) | step interval ms, stream events: median | kernel | kernel alone ms: median (min .. max) | "
             "algorithmic bytes per sample | GB per launch | share of the 8 TB/s roof |", "|---|---|---|---|---|---|---|---|"]
    for name, _, _, _ in cases:
        c = rec[name]
        bps = IN_BYTES[name] + 8.0 / D
        gb = samples * bps / 1e9
        lines.append("| %s | %.3f (%.3f .. %.3f) | %.3f | %s | %.3f (%.3f .. %.3f) | %.2f | %.2f | %.3f |" % (
            name, med(c["step"]), min(c["step"]), max(c["step"]), med(c["interval"]), c["kname"], med(c["kernel"]), min(c["kernel"]), max(c["kernel"]),
            bps, gb, gb / (med(c["kernel"]) * 1e-3) / bench.HBM_PEAK_GBPS))
    s = {name: med(rec[name]["step"]) for name in rec}
    kk = {name: med(rec[name]["kernel"]) for name in rec}
    aa = abs(s["cf32"] - s["cf32 (A/A)"])
    aak = abs(kk["cf32"] - kk["cf32 (A/A)"])
    lines += ["", "A/A spread of the cf32 pair: step %.3f ms (%.2f %%), kernel alone %.3f ms" % (aa, 100.0 * aa / s["cf32"], aak)]
    verdict = {}
    for name in ("sc8", "cu8"):
        gain_ms = s["sc16"] - s[name]
        verdict[name] = gain_ms > aa
        lines.append("%s: step %.3f ms against %.3f ms for int16 (%+.3f ms), kernel alone %.3f against %.3f ms: %s the A/A spread" % (
            name, s[name], s["sc16"], -gain_ms, kk[name], kk["sc16"], "faster than int16 by more than" if verdict[name] else "not faster than int16 by more than"))
    lines.append("outputs of the five handles: %s" % ("bit-identical" if same else "DIFFER"))
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps({"box": box, "batch": batch, "nsamp": nsamp, "rounds": args.rounds, "steps": args.steps, "cases": rec, "aa_step_ms": aa,
                      "aa_kernel_ms": aak, "faster_than_sc16": verdict, "same": same, "default_shape": batch == dbatch}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    ctx.close()
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
