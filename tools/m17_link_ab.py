#!/usr/bin/env python3
"""Times the M17 link layer on receive (docs/MEASUREMENT.md, "M17 link layer", describes the measurement; the table this tool prints goes there).

    python tools/m17_link_ab.py [--batch 16384] [--slots 16] [--warmup 5] [--steps 100] [--cpu-streams 256] [--out table.md]

Shape: `batch` streams x `slots` stream frames of a running call: every stream holds `slots` consecutive stream frames of one call (a bank of
96 frames, 16 LICH rounds), from a start drawn per stream, so the lanes of a wave sit at different places of the LICH round.  The frames lie
on the device as the frame synchroniser writes them (56-byte records, counts = slots).
Figures:
  the new chain    qrl_m17_rx_process (decode stage + walk), HIP events on the null stream around every single call, warm-up calls first;
                   median, min .. max, two rounds
  its FEC alone    qrl_m17_decode_frames on the same frames as [n][48]: the Viterbi work the chain shares with the parent
  the parent path  m17_frame_decoder_hip::decodeFrames (host/m17_frame_decoder_hip.cpp) on the same frames from host memory: copy up,
                   qrl_m17_decode_frames, blocking copy down, the scalar LICH reassembly; wall clock per call, a process of its own
                   (tools/m17_link_ab_host, built by `make -C qradiolink_amd/csrc m17_link_ab`)
  one CPU core     the reference's own M17FrameDecoder::decodeFrame (oracle/_ref/libqrl_ref.so, ref_m17_decode_sequence) over `cpu-streams`
                   of the streams, scaled to the batch; it is the decoder alone, without gr_modem's callsign and CAN work, so a lower bound
                   of the reference's path.  Left out where the library is absent.
Before anything is timed the device's records of the first call are compared with the scalar core's (m17_link_core.hpp on the oracle's decode)
for `cpu-streams` of the streams, byte for byte.  No GPU: the tool fails."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--cpu-streams", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("m17_link_ab.py needs a GPU")
    import m17_link as M
    import qradiolink_amd as q
    B, n = args.batch, args.slots
    bank = np.stack([M.stream_frame(M.A_LSF, k) for k in range(96)])
    rng = np.random.RandomState(16384)
    start = rng.randint(0, 96, B)
    frames = bank[(start[:, None] + np.arange(n)[None, :]) % 96]                      # [B, n, 48]
    records = np.zeros((B, n, M.FS_REC), np.uint8)
    records[:, :, 0:8] = np.array([M.FT_STREAM, 46 | (8 << 16)], "<u4").view(np.uint8)
    records[:, :, 8:54] = frames[:, :, 2:]
    ctx = q.Context(0)
    lib = ctx.lib
    d_fs = torch.from_numpy(records.reshape(B, n * M.FS_REC)).cuda()
    d_cnt = torch.from_numpy(np.tile(np.array([[n * M.FS_REC, n]], np.int32), (B, 1))).cuda()
    d_out = torch.empty((B, n, M.REC), dtype=torch.uint8, device="cuda")
    d_frames = torch.from_numpy(np.ascontiguousarray(frames.reshape(B * n, 48))).cuda()
    d_rec = torch.empty((B * n, 40), dtype=torch.uint8, device="cuda")
    rx = q.M17Rx(ctx, B, can_rx=0, decode_all_can=True)
    torch.cuda.synchronize()
    chain = lambda: lib.qrl_m17_rx_process(rx.h, None, d_fs.data_ptr(), n * M.FS_REC, d_cnt.data_ptr(), n, d_out.data_ptr())
    fec = lambda: lib.qrl_m17_decode_frames(ctx.h, None, d_frames.data_ptr(), B * n, d_rec.data_ptr())
    assert chain() == 0 and fec() == 0
    torch.cuda.synchronize()
    # correctness at the timed size: the first call of a fresh handle against the scalar core
    core = M.load_core(tempfile.mkdtemp())
    first = d_out.cpu().numpy()
    m = min(args.cpu_streams, B)
    pick = rng.choice(B, m, replace=False)
    for b in pick:
        want, _ = core.run(records[b], 0, 1)
        assert np.array_equal(want, first[b]), "stream %d differs from the scalar core" % b
    assert (M.flags(first)[:, 6:] & M.AUDIO).all()          # every stream has locked by its sixth frame

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

    rounds = [(timed(chain), timed(fec)) for _ in range(2)]
    # the parent's path, a process of its own
    host = os.path.join(ROOT, "tools", "m17_link_ab_host")
    parent = None
    if os.path.exists(host):
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "frames.bin")
            frames.tofile(path)
            env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(filter(None, [os.path.join(ROOT, "qradiolink_amd"), os.environ.get("LD_LIBRARY_PATH")])))
            r = subprocess.run([host, path, str(B), str(n), "3", "15"], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr
        v = [float(x) for x in r.stdout.split()]
        parent = (statistics.median(v), min(v), max(v))
    # the reference's decoder on one CPU core
    cpu_s = None
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libqrl_ref.so")
    if os.path.exists(ref_so):
        ref = C.CDLL(ref_so)
        seqs = [np.ascontiguousarray(frames[b]) for b in pick]
        lsf, st = np.zeros(30, np.uint8), np.zeros(18, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        t0 = time.perf_counter()
        for s in seqs:
            ref.ref_m17_decode_sequence(p(s), n, p(lsf), p(st))
        cpu_s = (time.perf_counter() - t0) / (m * n)
    fmt = lambda t: "%.3f ms (%.3f – %.3f)" % t
    lines = ["| what | %d streams × %d stream frames |" % (B, n), "|---|---|"]
    lines.append("| `qrl_m17_rx_process` (decode stage + walk), device, median of %d (min – max), round 1 / round 2 | **%s** / %s |" % (args.steps, fmt(rounds[0][0]), fmt(rounds[1][0])))
    lines.append("| `qrl_m17_decode_frames` alone on the same frames | %s / %s |" % (fmt(rounds[0][1]), fmt(rounds[1][1])))
    lines.append("| the parent's path: `m17_frame_decoder_hip::decodeFrames` from host memory, wall clock, median of 15 | %s |" % (fmt(parent) if parent else "not built"))
    lines.append("| the reference's `M17FrameDecoder::decodeFrame` on one CPU core, %d streams scaled to the batch | %s |" % (
        m, "%.0f ms (%.2f µs per frame)" % (1e3 * cpu_s * B * n, 1e6 * cpu_s) if cpu_s else "library absent"))
    lines.append("")
    lines.append("Chain / FEC alone: %.2f (round 1 medians).  %d of the streams compared with the scalar core before timing: equal." % (rounds[0][0][0] / rounds[0][1][0], m))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    rx.close()
    ctx.close()


if __name__ == "__main__":
    main()
