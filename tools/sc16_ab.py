#!/usr/bin/env python3
"""A/B of the int16 input path against the parent commit, one process, one GPU, cases interleaved (docs/MEASUREMENT.md, "sc16 input").

    python tools/sc16_ab.py --parent-lib /path/to/parent/libqrl_hip.so [--rounds 7] [--steps 100] [--out table.md]

--parent-lib is libqrl_hip.so built from the parent commit (a second work tree: `git worktree add ../parent HEAD~1 && make -C
../parent/qradiolink_amd/csrc`).  It is loaded beside this tree's library; both get their own qrl_ctx on device 0.

Shapes: C2's (384 streams x 1 638 400 samples at 25 Msps, GMSK-10k behind the 25:1 front end) and a 50 Msps 2FSK-1k shape of about 4 GB of
cf32 (256 x 2 000 000).  Per shape three cases: cf32 through the parent's library, cf32 through this one, sc16 through this one.  All three
see the SAME samples: the synthetic batch of bench.py quantised to int16 at 1 / 32768, the cf32 cases its converted floats.  A round runs
every case once (order rotated from round to round): warm-up steps, then `steps` timed calls between two synchronisations (step time, host
clock) with qrl_demod_profile on (front-end kernel time, HIP events).  Reported: median over the rounds, min .. max, and the ratio of the
medians to the parent's.

Two conditions per shape, each for the kernel time and for the step time, against the PARENT's cf32 medians with the same-box A/B resolution of
README.md (1 %) as the margin: cf32 on this commit is not slower (ratio <= 1.01) and sc16 on this commit is not slower (ratio <= 1.01).  Every check is
printed as PASS / FAIL and the exit status is 1 when any fails (the table is written first either way).  No GPU: the tool fails, it never falls back."""
import argparse
import ctypes as C
import json
import os
import socket
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MARGIN = 1.01          # README.md: same-box A/B resolution 1 %

SHAPES = [
    # name, sig mode, modem type, device rate, offset, batch, samples per stream
    ("C2 25 Msps GMSK-10k 384 x 1638400", "gmsk10k", 22, 25000000, 25000.0, 384, 25 * (1 << 16)),
    ("50 Msps 2FSK-1k 256 x 2000000", "2fsk1k", 18, 50000000, 25000.0, 256, 2000000),
]


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
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", type=int, default=-1, help="index into SHAPES (default: all)")
    ap.add_argument("--scale-down", type=int, default=1, help="divide batch by this (rehearsals)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sc16_ab.py needs a GPU")
    import bench
    import qradiolink_amd as q
    dev = torch.device("cuda:0")
    ctx_new = q.Context(0)
    ctx_old = open_parent(q, args.parent_lib)
    box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    lines = ["box: %s; rounds %d x %d steps per case, cases interleaved in one process" % (box, args.rounds, args.steps), "",
             "| shape | case | kernel | kernel ms median (min .. max) | vs parent | step ms median (min .. max) | vs parent |",
             "|---|---|---|---|---|---|---|"]
    results, checks = [], []
    for si, (label, mode, modem, rate, offset, batch, nsamp) in enumerate(SHAPES):
        if args.shape >= 0 and si != args.shape:
            continue
        batch = max(1, batch // args.scale_down)
        iq = bench.synth(mode, rate, offset, batch, nsamp, 1234, torch, dev)
        v = torch.view_as_real(iq).mul(32768.0).round_().clamp_(-32768, 32767).to(torch.int16).reshape(batch, 2 * nsamp).contiguous()
        del iq
        x = torch.view_as_complex((v.to(torch.float32) * (1.0 / 32768.0)).reshape(batch, nsamp, 2).contiguous())
        torch.cuda.synchronize()
        mk = lambda ctx: q.Demod(ctx, modem, batch=batch, max_chunk=nsamp, device_samp_rate=rate, carrier_offset_hz=offset, side_outputs=True)
        d_old, d_new, d_sc = mk(ctx_old), mk(ctx_new), mk(ctx_new)
        cases = [("cf32 parent", d_old, d_old.process_async, x), ("cf32 this commit", d_new, d_new.process_async, x),
                 ("sc16 this commit", d_sc, d_sc.process_sc16_async, v)]
        rec = {name: {"step": [], "kernel": [], "kname": ""} for name, _, _, _ in cases}
        for r in range(args.rounds):
            for k in range(len(cases)):
                name, dem, call, data = cases[(k + r) % len(cases)]
                step, kern, kname = run_case(dem, call, data, args.warmup, args.steps)
                rec[name]["step"].append(step); rec[name]["kernel"].append(kern); rec[name]["kname"] = kname
        # the three handles saw the same samples the same number of times: their last calls must agree bit for bit
        ref = d_old._ports()
        for name, dem, _, _ in cases[1:]:
            got = dem._ports()
            for port in ("bits_a", "bits_b", "counts", "filtered"):
                assert torch.equal(ref[port], got[port]), "%s: port %s differs from the parent's" % (name, port)
        med = lambda a: statistics.median(a)
        base = rec["cf32 parent"]
        for name, _, _, _ in cases:
            c = rec[name]
            lines.append("| %s | %s | %s | %.3f (%.3f .. %.3f) | %.4f | %.3f (%.3f .. %.3f) | %.4f |" % (
                label if batch == SHAPES[si][5] else "%s (batch %d)" % (label, batch), name, c["kname"],
                med(c["kernel"]), min(c["kernel"]), max(c["kernel"]), med(c["kernel"]) / med(base["kernel"]),
                med(c["step"]), min(c["step"]), max(c["step"]), med(c["step"]) / med(base["step"])))
        for name in ("cf32 this commit", "sc16 this commit"):
            for what in ("kernel", "step"):
                ratio = med(rec[name][what]) / med(base[what])
                checks.append((label, name, what, ratio, ratio <= MARGIN))
        results.append({"shape": label, "batch": batch, "nsamp": nsamp, "cases": rec})
        for _, dem, _, _ in cases:
            dem.close()
        del v, x
        torch.cuda.empty_cache()
    lines += ["", "conditions (median / parent's cf32 median <= %.2f):" % MARGIN, ""]
    for label, name, what, ratio, ok in checks:
        lines.append("- %s: %s, %s, %s time: %.4f" % ("PASS" if ok else "FAIL", label, name, what, ratio))
    failed = [c for c in checks if not c[4]]
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps({"box": box, "rounds": args.rounds, "steps": args.steps, "margin": MARGIN, "results": results,
                      "checks": [dict(shape=c[0], case=c[1], time=c[2], ratio=c[3], ok=c[4]) for c in checks]}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    ctx_old.lib.qrl_shutdown(ctx_old.h)
    ctx_new.close()
    if failed:
        sys.stderr.write("sc16_ab: %d of %d conditions FAILED\n" % (len(failed), len(checks)))
        sys.exit(1)


if __name__ == "__main__":
    main()
