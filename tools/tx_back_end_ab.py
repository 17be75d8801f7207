#!/usr/bin/env python3
"""A/B of the transmitters' back-end interpolator against the parent commit, one process, one GPU, both libraries loaded, cases interleaved
(docs/MEASUREMENT.md, "TX back end rates"; the table this tool prints goes there).

    python tools/tx_back_end_ab.py --parent-lib /path/to/parent/libqrl_hip.so [--rates 4,10,25,64,100,183] [--rounds 5] [--out table.md]

--parent-lib is libqrl_hip.so built from the parent commit (a second work tree: `git worktree add ../parent HEAD~1 && make -C
../parent/qradiolink_amd/csrc`).  It is loaded beside this tree's library; both get their own qrl_ctx on device 0.

Shape: QPSK-250k behind the gr_mod_base back end, 256 streams x 4096 bytes per call (the shape of tools/sc16_tx_ab.py), 32 x rate / 1e6 samples per
byte; at every rate the batch is cut so that one call's cf32 output stays under 8 GB (the streams used are printed).  Rates up to 64 Msps run
through both libraries, the rates above through this one only (the parent refuses them).  Per rate and library two cases, cf32 and sc16 output.  A
round runs every case of a rate once, order rotated from round to round: warm-up calls, then timed calls, each between two HIP events on the
handle's own stream.  Reported per case: median, min .. max of the timed calls of all rounds, the ratio of the medians to the parent's, GS/s of
device-rate samples, and above 64 Msps the fraction of the contract's arithmetic floor (418 fmaf = 836 flop per output sample over the 157.3 TF
f32 peak = 188 GS/s).  Before anything is timed, one call of a fresh handle of both libraries must give the same bits at every shared rate.

Conditions, against the parent's median of the same format: (1) at every shared rate that this tree runs on k_tx_interp_mfma (kTxMfmaMinInterp of
qradiolink_amd/csrc/tx_common.hpp) the median is not above the parent's by more than 2 % (the 1 % same-box resolution of README.md, doubled: one
call, not a whole step); (2) at 25 and 64 Msps it is below the parent's.  Every check is printed as PASS / FAIL and the exit status is 1 when any
fails (the table is written first either way).  No GPU: the tool fails, it never falls back."""
import argparse
import ctypes as C
import json
import os
import re
import socket
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGIN = 1.02
FLOOR_GSPS = 157.3e12 / 836 / 1e9
PARENT_MAX_RATE = 64
OUT_BYTES_MAX = 8e9


def open_parent(q, path):
    """the parent's library with this binding's prototypes for every symbol it has, and a context on it"""
    here = q.load_library()
    lib = C.CDLL(path)
    for name in q.EXPORTED_SYMBOLS:
        if hasattr(lib, name):
            fn, mine = getattr(lib, name), getattr(here, name)
            fn.argtypes, fn.restype = mine.argtypes, mine.restype
    ctx = types.SimpleNamespace(lib=lib, h=C.c_void_p(), device=0)
    rc = lib.qrl_init(0, C.byref(ctx.h))
    if rc != 0:
        raise SystemExit("qrl_init on the parent library failed: %d" % rc)
    return ctx


def mfma_min_interp():
    text = open(os.path.join(ROOT, "qradiolink_amd", "csrc", "tx_common.hpp")).read()
    return int(re.search(r"kTxMfmaMinInterp\s*=\s*(\d+)", text).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--rates", default="4,10,25,64,100,183", help="device rates in Msps")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--nbytes", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tx_back_end_ab.py needs a GPU")
    import qradiolink_amd as q
    ctx_new = q.Context(0)
    ctx_old = open_parent(q, args.parent_lib)
    thr = mfma_min_interp()
    box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    n = args.nbytes
    lines = ["box: %s; QPSK-250k, up to %d streams x %d bytes per call, offset +25 kHz; %d rounds x (%d warm-up + %d timed calls) per case, cases "
             "interleaved in one process; k_tx_interp_mfma from %d Msps up" % (box, args.batch, n, args.rounds, args.warmup, args.steps, thr), "",
             "| rate, Msps | streams | samples per stream and call | library | kernel | output | ms per call median (min .. max) | vs parent | GS/s | of the 188 GS/s floor |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    results, checks = [], []
    for I in [int(r) for r in args.rates.split(",")]:
        rate = I * 1000000
        count = n * 32 * I
        B = max(1, min(args.batch, int(OUT_BYTES_MAX // (count * 8))))
        shared = I <= PARENT_MAX_RATE
        data = torch.randint(0, 256, (B, n), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(I))
        o32 = torch.empty((B, count), dtype=torch.complex64, device="cuda")
        o16 = torch.empty((B, count, 2), dtype=torch.int16, device="cuda")
        mk = lambda ctx: q.Mod(ctx, q.MODEM_QPSK250K, batch=B, max_bytes=n, device_samp_rate=rate, carrier_offset_hz=25000.0)
        print("rate %d Msps: %d streams x %d samples per call" % (I, B, count), flush=True)
        if shared:   # one call of fresh handles: the same bits from both libraries, both formats
            ref32, ref16 = torch.empty_like(o32), torch.empty_like(o16)
            for ctx, a, b in ((ctx_old, ref32, ref16), (ctx_new, o32, o16)):
                m32, m16 = mk(ctx), mk(ctx)
                m32.process_async(data, out=a); m16.process_sc16_async(data, out=b)
                m32.sync(); m16.sync()
                m32.close(); m16.close()
            assert torch.equal(torch.view_as_real(ref32).view(torch.int32), torch.view_as_real(o32).view(torch.int32)), "%d Msps: cf32 output differs from the parent's" % I
            assert torch.equal(ref16, o16), "%d Msps: sc16 output differs from the parent's" % I
            del ref32, ref16
            torch.cuda.empty_cache()
            print("rate %d Msps: both libraries give the same bits (cf32 and sc16)" % I, flush=True)
        cases = []
        for lname, ctx in (("parent", ctx_old), ("this commit", ctx_new)):
            if lname == "parent" and not shared:
                continue
            for fmt in ("cf32", "sc16"):
                m = mk(ctx)
                call = (lambda m=m: m.process_async(data, out=o32)) if fmt == "cf32" else (lambda m=m: m.process_sc16_async(data, out=o16))
                cases.append({"lib": lname, "fmt": fmt, "mod": m, "call": call, "stream": torch.cuda.ExternalStream(m.lib.qrl_mod_stream(m.h)), "ms": []})
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
        med = statistics.median
        base = {c["fmt"]: med(c["ms"]) for c in cases if c["lib"] == "parent"}
        for c in cases:
            t = med(c["ms"])
            gsps = B * count / t / 1e6
            kern = "k_tx_interp_mfma" if c["lib"] == "this commit" and I >= thr else "k_tx_interp_c"
            ratio = t / base[c["fmt"]] if shared else None
            lines.append("| %d | %d | %d | %s | %s | %s | %.3f (%.3f .. %.3f) | %s | %.1f | %s |" % (
                I, B, count, c["lib"], kern, c["fmt"], t, min(c["ms"]), max(c["ms"]), "%.4f" % ratio if shared else "-", gsps,
                "%.3f" % (gsps / FLOOR_GSPS) if not shared else "-"))
            results.append({"rate": rate, "streams": B, "count": count, "lib": c["lib"], "kernel": kern, "fmt": c["fmt"], "ms": c["ms"]})
            if shared and c["lib"] == "this commit" and I >= thr:
                checks.append(("%d Msps %s: not above the parent by more than 2 %%" % (I, c["fmt"]), ratio, ratio <= MARGIN))
                if I in (25, 64):
                    checks.append(("%d Msps %s: faster than the parent" % (I, c["fmt"]), ratio, ratio < 1.0))
        for c in cases:
            c["mod"].close()
        del cases, o32, o16, data
        torch.cuda.empty_cache()
    lines += ["", "conditions (median / the parent's median of the same format):", ""]
    for label, ratio, ok in checks:
        lines.append("- %s: %s: %.4f" % ("PASS" if ok else "FAIL", label, ratio))
    failed = [c for c in checks if not c[2]]
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps({"box": box, "rounds": args.rounds, "warmup": args.warmup, "steps": args.steps, "mfma_min_interp": thr, "results": results,
                      "checks": [dict(check=c[0], ratio=c[1], ok=c[2]) for c in checks]}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    ctx_old.lib.qrl_shutdown(ctx_old.h)
    ctx_new.close()
    if failed:
        sys.stderr.write("tx_back_end_ab: %d of %d conditions FAILED\n" % (len(failed), len(checks)))
        sys.exit(1)


if __name__ == "__main__":
    main()
