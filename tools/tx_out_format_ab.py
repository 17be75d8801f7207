#!/usr/bin/env python3
"""A/B of the transmitters' three output formats (cf32, sc16, sc8) and of this tree's cf32 and sc16 calls against the parent commit's: one process,
one GPU, both libraries loaded, cases interleaved (the method of tools/tx_back_end_ab.py; docs/MEASUREMENT.md, "sc8 output" and "sc16 output", hold
the table this tool prints).

    python tools/tx_out_format_ab.py --parent-lib /path/to/parent/libqrl_hip.so [--rates 1,8,25,183] [--rounds 5] [--out table.md]

--parent-lib is libqrl_hip.so built from the parent commit (a second work tree: `git worktree add ../parent HEAD~1 && make -C
../parent/qradiolink_amd/csrc`).  It is loaded beside this tree's library; both get their own qrl_ctx on device 0.

Shape: QPSK-250k, 256 streams x 4096 bytes per call, 32 x rate / 1e6 samples per byte.  Rate 1: no back end, k_tx_interp_sym stores to the caller's
buffer.  The other rates: the gr_mod_base back end at +25 kHz, and the batch is cut so that one call's cf32 output stays under 8 GB (the streams used
are printed).  Per rate seven cases: cf32 and sc16 on the parent's library; cf32, sc16 and sc8 on this tree; and this tree's cf32 and sc16 a second
time on handles of their own -- the A/A pair, whose ratio of medians is the spread a ratio of this run can be read against.  A round runs every
case of a rate once, order rotated from round to round: warm-up calls, then timed calls, each between two HIP events on the handle's own stream.
Reported per case: median and p10 .. p90 of the timed calls of all rounds, the ratio of the medians to the parent's same-format median, to this
tree's cf32 and to this tree's sc16, and GS/s of device-rate samples.  Before anything is timed, one call of a fresh handle of both libraries must
give the same bits in cf32 and in sc16 at every rate.

Condition: this tree's cf32 and sc16 medians are not above the parent's same-format medians by more than 2 % (the margin docs/MEASUREMENT.md, "TX
back end rates", derives for one call).  sc8 against sc16 and cf32 is recorded, no bound is set.  Every check is printed as PASS / FAIL and the exit
status is 1 when any fails (the table is written first either way).  No GPU: the tool fails, it never falls back."""
import argparse
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tx_back_end_ab import open_parent, mfma_min_interp   # noqa: E402

MARGIN = 1.02
OUT_BYTES_MAX = 8e9


def pct(v, p):
    s = sorted(v)
    return s[min(len(s) - 1, int(round(p / 100.0 * (len(s) - 1))))]


def kernel_of(I, thr):
    return "k_tx_interp_sym" if I == 1 else "k_tx_interp_mfma" if I >= thr else "k_tx_interp_c"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--rates", default="1,8,25,183", help="device rates in Msps; 1 = no back end")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--nbytes", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tx_out_format_ab.py needs a GPU")
    import qradiolink_amd as q
    ctx_new = q.Context(0)
    ctx_old = open_parent(q, args.parent_lib)
    thr = mfma_min_interp()
    box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    n = args.nbytes
    lines = ["box: %s; QPSK-250k, up to %d streams x %d bytes per call (rate 1: no back end; above: back end at +25 kHz); %d rounds x (%d warm-up + %d "
             "timed calls) per case, cases interleaved in one process" % (box, args.batch, n, args.rounds, args.warmup, args.steps), "",
             "| rate, Msps | streams | samples per stream and call | terminal kernel | library | output | ms per call median (p10 .. p90) | vs parent, same format | vs this cf32 | vs this sc16 | GS/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    results, checks, spreads = [], [], []
    med = statistics.median
    for I in [int(r) for r in args.rates.split(",")]:
        rate = I * 1000000
        count = n * 32 * I
        B = max(1, min(args.batch, int(OUT_BYTES_MAX // (count * 8))))
        data = torch.randint(0, 256, (B, n), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(I))
        out = {"cf32": torch.empty((B, count), dtype=torch.complex64, device="cuda"), "sc16": torch.empty((B, count, 2), dtype=torch.int16, device="cuda"),
               "sc8": torch.empty((B, count, 2), dtype=torch.int8, device="cuda")}
        mk = lambda ctx: q.Mod(ctx, q.MODEM_QPSK250K, batch=B, max_bytes=n, device_samp_rate=0 if I == 1 else rate, carrier_offset_hz=0.0 if I == 1 else 25000.0)
        run = {"cf32": lambda m: m.process_async(data, out=out["cf32"]), "sc16": lambda m: m.process_sc16_async(data, out=out["sc16"]),
               "sc8": lambda m: m.process_sc8_async(data, out=out["sc8"])}
        print("rate %d Msps: %d streams x %d samples per call" % (I, B, count), flush=True)
        # one call of fresh handles: the same bits from both libraries, cf32 and sc16
        ref32, ref16 = torch.empty_like(out["cf32"]), torch.empty_like(out["sc16"])
        for ctx, a, b in ((ctx_old, ref32, ref16), (ctx_new, out["cf32"], out["sc16"])):
            m32, m16 = mk(ctx), mk(ctx)
            m32.process_async(data, out=a); m16.process_sc16_async(data, out=b)
            m32.sync(); m16.sync()
            m32.close(); m16.close()
        assert torch.equal(torch.view_as_real(ref32).view(torch.int32), torch.view_as_real(out["cf32"]).view(torch.int32)), "%d Msps: cf32 output differs from the parent's" % I
        assert torch.equal(ref16, out["sc16"]), "%d Msps: sc16 output differs from the parent's" % I
        del ref32, ref16
        torch.cuda.empty_cache()
        print("rate %d Msps: both libraries give the same bits (cf32 and sc16)" % I, flush=True)
        cases = []
        for lname, ctx, fmts in (("parent", ctx_old, ("cf32", "sc16")), ("this commit", ctx_new, ("cf32", "sc16", "sc8")), ("this commit (A/A)", ctx_new, ("cf32", "sc16"))):
            for fmt in fmts:
                m = mk(ctx)
                cases.append({"lib": lname, "fmt": fmt, "mod": m, "call": (lambda m=m, fmt=fmt: run[fmt](m)),
                              "stream": torch.cuda.ExternalStream(m.lib.qrl_mod_stream(m.h)), "ms": []})
        for r in range(args.rounds):
            for k in range(len(cases)):
                c = cases[(k + r) % len(cases)]
                for step in range(args.warmup + args.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(c["stream"])
                    c["call"]()
                    e1.record(c["stream"])
                    c["mod"].sync()
                    e1.synchronize()
                    if step >= args.warmup:
                        c["ms"].append(e0.elapsed_time(e1))
        t = {(c["lib"], c["fmt"]): med(c["ms"]) for c in cases}
        for c in cases:
            tc = t[(c["lib"], c["fmt"])]
            vs_parent = tc / t[("parent", c["fmt"])] if c["fmt"] != "sc8" and c["lib"] != "parent" else None
            lines.append("| %d | %d | %d | %s | %s | %s | %.3f (%.3f .. %.3f) | %s | %.4f | %.4f | %.1f |" % (
                I, B, count, kernel_of(I, thr), c["lib"], c["fmt"], tc, pct(c["ms"], 10), pct(c["ms"], 90),
                "%.4f" % vs_parent if vs_parent is not None else "-", tc / t[("this commit", "cf32")], tc / t[("this commit", "sc16")], B * count / tc / 1e6))
            results.append({"rate": rate, "streams": B, "count": count, "lib": c["lib"], "fmt": c["fmt"], "ms": c["ms"]})
            if c["lib"] == "this commit" and vs_parent is not None:
                checks.append(("%d Msps %s: not above the parent by more than 2 %%" % (I, c["fmt"]), vs_parent, vs_parent <= MARGIN))
        for fmt in ("cf32", "sc16"):
            spreads.append((I, fmt, t[("this commit (A/A)", fmt)] / t[("this commit", fmt)]))
        for c in cases:
            c["mod"].close()
        del cases, out, data, run
        torch.cuda.empty_cache()
    lines += ["", "A/A of this run (median of a second handle of the same case / the first's):", ""]
    lines += ["- %d Msps %s: %.4f" % s for s in spreads]
    lines += ["", "conditions (median / the parent's median of the same format):", ""]
    for label, ratio, ok in checks:
        lines.append("- %s: %s: %.4f" % ("PASS" if ok else "FAIL", label, ratio))
    failed = [c for c in checks if not c[2]]
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps({"box": box, "rounds": args.rounds, "warmup": args.warmup, "steps": args.steps, "results": results,
                      "aa": [dict(rate=s[0], fmt=s[1], ratio=s[2]) for s in spreads], "checks": [dict(check=c[0], ratio=c[1], ok=c[2]) for c in checks]}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    ctx_old.lib.qrl_shutdown(ctx_old.h)
    ctx_new.close()
    if failed:
        sys.stderr.write("tx_out_format_ab: %d of %d conditions FAILED\n" % (len(failed), len(checks)))
        sys.exit(1)


if __name__ == "__main__":
    main()
