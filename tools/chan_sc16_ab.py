#!/usr/bin/env python3
"""A/B of the int16 input path of the wideband receiver against the parent commit, one process, one GPU, cases interleaved
(docs/MEASUREMENT.md, "sc16 wideband input").

    python tools/chan_sc16_ab.py --parent-lib /path/to/parent/libqrl_hip.so [--rounds 7] [--steps 30] [--out table.md]

--parent-lib is libqrl_hip.so built from the parent commit (a second work tree: `git worktree add ../parent HEAD~1 && make -C
../parent/qradiolink_amd/csrc`).  It is loaded beside this tree's library; both get their own qrl_ctx on device 0.

Shape: C4's of bench.py -- 64 wideband streams x 2 097 152 samples at 1.6 Msps, 64 channels, PFB form, RSSI tags and the 4FSK symbol tail on.
Four cases: cf32 through the parent's library TWICE (two handles: the A/A pair, whose spread is what the box resolves), cf32 through this
library, sc16 through this library.  All see the SAME samples: bench.py's C4 input quantised to int16 at 1 / 32768 (peak scaled to about 30 000
counts), the cf32 cases its converted floats.  A round runs every case once (order rotated from round to round): warm-up steps, then `steps`
timed calls between two synchronisations (step time, host clock) with qrl_chan_profile on (HIP events: the channelizer, the fused per-channel
kernel and the symbol synchroniser, qrl_chan_profile_read_kernels).  Reported: median over the rounds, min .. max, the ratio of the medians to
parent A's, and whether this tree's cf32 step lies within the A/A spread (the min .. max of both parent handles): the device code is the parent's,
so it must.  The sc16 figures are recorded as measured; there is no speed condition on them.  After the last round the int16 outputs, counts,
RSSI tags and dibits of all four handles must agree bit for bit.  No GPU: the tool fails, it never falls back."""
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

KERNELS = ("channelizer", "k_chan_tail", "k_symsync_ff")


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


def run_case(ch, call, data, warmup, steps):
    for _ in range(warmup):
        call(data)
    ch.sync()
    ch.profile(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        call(data)
    ch.sync()
    dt = time.perf_counter() - t0
    kern = ch.profile_read_kernels()
    ch.profile(False)
    assert all(n == steps for _, _, n in kern)
    return dt / steps * 1e3, [ms / n for _, ms, n in kern]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--nsamp", type=int, default=1 << 21)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("chan_sc16_ab.py needs a GPU")
    import bench
    import qradiolink_amd as q
    dev = torch.device("cuda:0")
    ctx_new = q.Context(0)
    ctx_old = open_parent(q, args.parent_lib)
    box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    M, B, n = 64, args.batch, args.nsamp // 64 * 64
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    iq = bench.c4_add_4fsk(torch.view_as_complex(torch.randn((B, n, 2), generator=g, device=dev, dtype=torch.float32) * 0.05), torch, 40)
    f = torch.view_as_real(iq)
    v = f.mul(30000.0 / float(f.abs().max())).round_().clamp_(-32768, 32767).to(torch.int16).reshape(B, 2 * n).contiguous()
    del iq, f
    x = torch.view_as_complex((v.to(torch.float32) * (1.0 / 32768.0)).reshape(B, n, 2).contiguous())
    torch.cuda.synchronize()

    def mk(ctx):
        ch = q.Channelizer(ctx, M, batch=B, max_chunk=n)
        ch.enable_4fsk()
        return ch

    a, a2, new, sc = mk(ctx_old), mk(ctx_old), mk(ctx_new), mk(ctx_new)
    cases = [("cf32 parent A", a, a.process_async, x), ("cf32 parent A'", a2, a2.process_async, x),
             ("cf32 this commit", new, new.process_async, x), ("sc16 this commit", sc, sc.process_sc16_async, v)]
    rec = {name: {"step": [], "kernels": []} for name, _, _, _ in cases}
    for r in range(args.rounds):
        for k in range(len(cases)):
            name, ch, call, data = cases[(k + r) % len(cases)]
            step, kern = run_case(ch, call, data, args.warmup, args.steps)
            rec[name]["step"].append(step); rec[name]["kernels"].append(kern)
    # the four handles saw the same samples the same number of times: their last calls must agree bit for bit
    for name, ch, _, _ in cases[1:]:
        for attr in ("out", "counts", "rssi", "rssi_counts", "dibits", "fsk_counts"):
            assert torch.equal(getattr(a, attr), getattr(ch, attr)), "%s: %s differs from the parent's" % (name, attr)
    med = statistics.median
    base = rec["cf32 parent A"]
    lines = ["box: %s; C4 shape %d x %d, 64 channels, RSSI + 4FSK tail; rounds %d x %d steps per case, cases interleaved in one process" % (box, B, n, args.rounds, args.steps), "",
             "| case | step ms median (min .. max) | vs parent A | " + " | ".join("%s ms median (min .. max)" % k for k in KERNELS) + " |",
             "|---|---|---|" + "---|" * len(KERNELS)]
    for name, _, _, _ in cases:
        c = rec[name]
        cols = []
        for i in range(len(KERNELS)):
            ks = [kk[i] for kk in c["kernels"]]
            cols.append("%.3f (%.3f .. %.3f)" % (med(ks), min(ks), max(ks)))
        lines.append("| %s | %.3f (%.3f .. %.3f) | %.4f | %s |" % (name, med(c["step"]), min(c["step"]), max(c["step"]), med(c["step"]) / med(base["step"]), " | ".join(cols)))
    aa = rec["cf32 parent A"]["step"] + rec["cf32 parent A'"]["step"]
    lo, hi = min(aa), max(aa)
    m_new = med(rec["cf32 this commit"]["step"])
    inside = lo <= m_new <= hi
    lines += ["", "A/A spread of the parent's cf32 step (both handles, every round): %.3f .. %.3f ms; medians %.3f and %.3f" % (lo, hi, med(rec["cf32 parent A"]["step"]), med(rec["cf32 parent A'"]["step"])),
              "%s: this commit's cf32 step median %.3f ms lies %s that spread" % ("PASS" if inside else "FAIL", m_new, "within" if inside else "OUTSIDE"),
              "sc16 this commit (convert on landing): step %.4f of parent A's, channelizer kernel %.4f of parent A's (recorded as measured; no condition)" % (
                  med(rec["sc16 this commit"]["step"]) / med(base["step"]),
                  med([k[0] for k in rec["sc16 this commit"]["kernels"]]) / med([k[0] for k in base["kernels"]]))]
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps({"box": box, "rounds": args.rounds, "steps": args.steps, "batch": B, "nsamp": n, "cases": rec, "aa_spread_ms": [lo, hi], "cf32_within_aa": inside}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)
    for _, ch, _, _ in cases:
        ch.close()
    ctx_old.lib.qrl_shutdown(ctx_old.h)
    ctx_new.close()
    if not inside:
        sys.stderr.write("chan_sc16_ab: this commit's cf32 step lies outside the parent's A/A spread\n")
        sys.exit(1)


if __name__ == "__main__":
    main()
