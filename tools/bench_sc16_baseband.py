#!/usr/bin/env python3
"""The headline shape fed cf32 and fed int16, one process, one GPU, the two formats alternating (docs/MEASUREMENT.md, "sc16 at 1 Msps").

    python tools/bench_sc16_baseband.py [--rounds 7] [--steps 30] [--warmup 5] [--out table.md]

Shape: C1 of bench.py -- 2FSK-1k at 1 Msps, 16384 streams x 262 144 samples, the handle as bench.py opens it (side outputs on, the library's
default options).  Two handles on one context: one is fed the complex64 batch through qrl_demod_process, the other -- with
QRL_OPT_SC16_BASEBAND = 1 -- the same samples as int16 pairs through qrl_demod_process_sc16.  Both see the SAME samples: bench.py's
synthetic batch quantised to int16 at 1 / 32768, the cf32 handle its converted floats, and after the last round their outputs are
compared bit for bit.

A round runs each format once (the order alternates from round to round): warm-up calls, then `steps` calls queued back to back between
two synchronisations.  Measured per round: the step time from the host clock over the whole queue, the intervals between step completions
from events on the handle's internal streams (bench.py's StepMarks: they order nothing), and the first-stage kernel alone (k_decim_pm) from
qrl_demod_profile's event pair around its launch.  Reported: the median over the rounds with min .. max, the kernel's algorithmic bytes
(8 B resp. 4 B of input per sample + 8 B per 50 samples of output ring) and the share of the 8 TB/s HBM roof they make at the kernel's time.

Condition: the int16 step (median) is not slower than the cf32 step of the same run by more than the 1 % that the same-box A/Bs of README.md
resolve.  PASS / FAIL is printed, the exit status is 1 on FAIL (the table is written first either way).  No GPU: the tool fails."""
import argparse
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MARGIN = 1.01               # README.md: same-box A/B resolution 1 %
D = 50                      # the first stage decimates 1:50 onto a cf32 ring
IN_BYTES = {"cf32": 8.0, "sc16": 4.0}


def quantise(iq, torch, rows=1024):
    """[B, n] complex64 -> ([B, 2 n] int16 at 32768 counts per unit, [B, n] complex64 = float(v) / 32768), a block of rows at a time"""
    B, n = iq.shape
    v = torch.empty((B, 2 * n), dtype=torch.int16, device=iq.device)
    for r in range(0, B, rows):
        f = torch.view_as_real(iq[r:r + rows]).reshape(-1, 2 * n)
        v[r:r + rows] = f.mul(32768.0).round_().clamp_(-32768, 32767).to(torch.int16)
        f.copy_(v[r:r + rows].to(torch.float32).mul_(1.0 / 32768.0))      # in place: iq becomes the converted floats
    return v, iq


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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sc16_baseband.py needs a GPU")
    import bench
    import qradiolink_amd as q
    label, mode, modem, rate, offset, dbatch, nsamp, _, abytes = bench.WORKLOADS["c1"]
    batch = args.batch or dbatch
    dev = torch.device("cuda:0")
    ctx = q.Context(0)
    v, x = quantise(bench.synth(mode, rate, offset, batch, nsamp, 1234, torch, dev), torch)
    torch.cuda.synchronize()
    mk = lambda: q.Demod(ctx, modem, batch=batch, max_chunk=nsamp, device_samp_rate=rate, carrier_offset_hz=offset, side_outputs=True)
    d_cf, d_sc = mk(), mk()
    d_sc.enable_sc16_baseband()
    cases = [("cf32", d_cf, d_cf.process_async, x), ("sc16", d_sc, d_sc.process_sc16_async, v)]
    rec = {name: {"step": [], "interval": [], "kernel": [], "kname": ""} for name, _, _, _ in cases}
    for r in range(args.rounds):
        for k in range(len(cases)):
            name, dem, call, data = cases[(k + r) % len(cases)]
            step, interval, kern, kname = run_case(bench, torch, dem, call, data, args.warmup, args.steps)
            rec[name]["step"].append(step); rec[name]["interval"].append(interval); rec[name]["kernel"].append(kern); rec[name]["kname"] = kname
    ref, got = d_cf._ports(), d_sc._ports()      # the same samples the same number of times: the last calls agree bit for bit
    for port in ("bits_a", "bits_b", "counts", "filtered", "constellation"):
        assert torch.equal(ref[port], got[port]), "port %s: int16 and cf32 differ" % port
    assert int(ref["counts"][:, 2].sum()) > 0
    for _, dem, _, _ in cases:
        dem.close()
    med = statistics.median
    box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    samples = float(batch) * nsamp
    lines = ["box: %s; %s, %d x %d samples; %d rounds x %d steps per format, formats alternating in one process" % (box, label, batch, nsamp, args.rounds, args.steps), "",
             "| input | step ms, host clock: median (min .. max) | step interval ms, stream events: median | kernel | kernel alone ms: median (min .. max) | "
             "algorithmic bytes per sample | GB per launch | share of the 8 TB/s roof |", "|---|---|---|---|---|---|---|---|"]
    for name, _, _, _ in cases:
        c = rec[name]
        bps = IN_BYTES[name] + 8.0 / D
        gb = samples * bps / 1e9
        lines.append("| %s | %.3f (%.3f .. %.3f) | %.3f | %s | %.3f (%.3f .. %.3f) | %.2f | %.2f | %.3f |" % (
            name, med(c["step"]), min(c["step"]), max(c["step"]), med(c["interval"]), c["kname"], med(c["kernel"]), min(c["kernel"]), max(c["kernel"]),
            bps, gb, gb / (med(c["kernel"]) * 1e-3) / bench.HBM_PEAK_GBPS))
    ratio = med(rec["sc16"]["step"]) / med(rec["cf32"]["step"])
    kratio = med(rec["sc16"]["kernel"]) / med(rec["cf32"]["kernel"])
    ok = ratio <= MARGIN
    lines += ["", "int16 / cf32: step %.4f, kernel alone %.4f" % (ratio, kratio),
              "%s: the int16 step is not slower than the cf32 step of the same run by more than 1 %% (ratio <= %.2f)" % ("PASS" if ok else "FAIL", MARGIN)]
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps({"box": box, "batch": batch, "nsamp": nsamp, "rounds": args.rounds, "steps": args.steps, "margin": MARGIN, "cases": rec,
                      "step_ratio": ratio, "kernel_ratio": kratio, "ok": ok, "default_shape": batch == dbatch}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    ctx.close()
    if not ok:
        sys.stderr.write("bench_sc16_baseband: the int16 step is slower than the cf32 step (ratio %.4f)\n" % ratio)
        sys.exit(1)


if __name__ == "__main__":
    main()
