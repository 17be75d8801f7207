#!/usr/bin/env python3
"""The four input formats of the front end side by side, one process, one GPU, cases interleaved (docs/MEASUREMENT.md, "8-bit input").

    python tools/iq8_ab.py [--rounds 7] [--steps 100] [--out table.md]

Shapes: C2's (384 streams x 1 638 400 samples at 25 Msps, GMSK-10k behind the 25:1 front end, D = 25) and a 50 Msps 2FSK-1k shape (256 x 2 000 000,
D = 50).  Per shape five cases on five handles of this library: cf32, sc16, sc8, cu8, and a second cf32 handle as the A/A control.  All see the
SAME samples: the synthetic batch of bench.py quantised to 8 bits at 1 / 128; the int16 case carries the codes at set_sc16_scale(1 / 128), the cu8
case the codes + 128 at set_cu8_scale(1 / 128, 128), the cf32 cases the converted floats.  A round runs every case once (order rotated from round
to round): warm-up steps, then `steps` timed calls between two synchronisations (step time, host clock) with qrl_demod_profile on (front-end
kernel time, HIP events).  Reported: median over the rounds, min .. max, the ratio of the medians to the sc16 case's (the reference point of the
8-bit kernel: the sc16 kernel of the same run) and to the first cf32 case's; the A/A spread is the second cf32 case's ratio to the first.

There is no speed gate: the tool reports.  The last calls of the five handles must agree bit for bit (asserted).  No GPU: the tool fails, it never
falls back."""
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

SHAPES = [
    # name, sig mode, modem type, device rate, offset, batch, samples per stream
    ("C2 25 Msps GMSK-10k 384 x 1638400", "gmsk10k", 22, 25000000, 25000.0, 384, 25 * (1 << 16)),
    ("50 Msps 2FSK-1k 256 x 2000000", "2fsk1k", 18, 50000000, 25000.0, 256, 2000000),
]


def run_case(dem, call, data, warmup, steps):
    for _ in range(warmup):
        call(data)
    dem.sync()
    dem.profile(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        call(data)
    dem.sync()
    dt = time.perf_counter() - t0
    kms, launches, kname = dem.profile_read()
    dem.profile(False)
    assert launches == steps
    return dt / steps * 1e3, kms / launches, kname


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", type=int, default=-1, help="index into SHAPES (default: all)")
    ap.add_argument("--scale-down", type=int, default=1, help="divide batch by this (rehearsals)")
    ap.add_argument("--swap-8bit-handles", action="store_true", help="create the cu8 handle before the sc8 one (tells an effect of where a handle's buffers lie from an effect of the format)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("iq8_ab.py needs a GPU")
    import bench
    import qradiolink_amd as q
    dev = torch.device("cuda:0")
    ctx = q.Context(0)
    box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    lines = ["box: %s; rounds %d x %d steps per case, cases interleaved in one process" % (box, args.rounds, args.steps), "",
             "| shape | case | bytes / sample | kernel | kernel ms median (min .. max) | vs sc16 | vs cf32 | step ms median (min .. max) | vs sc16 | vs cf32 |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    results = []
    for si, (label, mode, modem, rate, offset, batch, nsamp) in enumerate(SHAPES):
        if args.shape >= 0 and si != args.shape:
            continue
        batch = max(1, batch // args.scale_down)
        assert nsamp % 8 == 0
        iq = bench.synth(mode, rate, offset, batch, nsamp, 1234, torch, dev)
        peak = float(torch.view_as_real(iq).abs().max())
        gain = 100.0 / (128.0 * peak) if peak * 128.0 > 100.0 or peak * 128.0 < 30.0 else 1.0      # the codes use the 8 bits: peak at about 100 counts
        v8 = torch.view_as_real(iq).mul(128.0 * gain).round_().clamp_(-128, 127).to(torch.int8).reshape(batch, 2 * nsamp).contiguous()
        del iq
        v16 = v8.to(torch.int16)
        u8 = (v16 + 128).to(torch.uint8)
        x = torch.view_as_complex((v8.to(torch.float32) * (1.0 / 128.0)).reshape(batch, nsamp, 2).contiguous())
        torch.cuda.synchronize()
        mk = lambda: q.Demod(ctx, modem, batch=batch, max_chunk=nsamp, device_samp_rate=rate, carrier_offset_hz=offset, side_outputs=True)
        d_cf, d_16, d_s8, d_u8, d_aa = mk(), mk(), mk(), mk(), mk()
        if args.swap_8bit_handles:
            d_s8, d_u8 = d_u8, d_s8
        d_16.set_sc16_scale(1.0 / 128.0)
        d_u8.set_cu8_scale(1.0 / 128.0, 128.0)
        cases = [("cf32", 8, d_cf, d_cf.process_async, x), ("sc16", 4, d_16, d_16.process_sc16_async, v16), ("sc8", 2, d_s8, d_s8.process_sc8_async, v8),
                 ("cu8", 2, d_u8, d_u8.process_cu8_async, u8), ("cf32 again (A/A)", 8, d_aa, d_aa.process_async, x)]
        rec = {c[0]: {"step": [], "kernel": [], "kname": ""} for c in cases}
        for r in range(args.rounds):
            for k in range(len(cases)):
                name, _, dem, call, data = cases[(k + r) % len(cases)]
                step, kern, kname = run_case(dem, call, data, args.warmup, args.steps)
                rec[name]["step"].append(step); rec[name]["kernel"].append(kern); rec[name]["kname"] = kname
        # the five handles saw the same samples the same number of times: their last calls must agree bit for bit
        ref = d_cf._ports()
        for name, _, dem, _, _ in cases[1:]:
            got = dem._ports()
            for port in ("bits_a", "bits_b", "counts", "filtered"):
                assert torch.equal(ref[port], got[port]), "%s: port %s differs from the cf32 handle's" % (name, port)
        med = statistics.median
        b16, bcf = rec["sc16"], rec["cf32"]
        for name, bps, _, _, _ in cases:
            c = rec[name]
            lines.append("| %s | %s | %d | %s | %.3f (%.3f .. %.3f) | %.4f | %.4f | %.3f (%.3f .. %.3f) | %.4f | %.4f |" % (
                label if batch == SHAPES[si][5] else "%s (batch %d)" % (label, batch), name, bps, c["kname"],
                med(c["kernel"]), min(c["kernel"]), max(c["kernel"]), med(c["kernel"]) / med(b16["kernel"]), med(c["kernel"]) / med(bcf["kernel"]),
                med(c["step"]), min(c["step"]), max(c["step"]), med(c["step"]) / med(b16["step"]), med(c["step"]) / med(bcf["step"])))
        aa = rec["cf32 again (A/A)"]
        lines.append("| | A/A spread (cf32 again / cf32) | | | %.4f | | | %.4f | | |" % (med(aa["kernel"]) / med(bcf["kernel"]), med(aa["step"]) / med(bcf["step"])))
        results.append({"shape": label, "batch": batch, "nsamp": nsamp, "cases": rec})
        for _, _, dem, _, _ in cases:
            dem.close()
        del v8, v16, u8, x
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps({"box": box, "rounds": args.rounds, "steps": args.steps, "results": results}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
