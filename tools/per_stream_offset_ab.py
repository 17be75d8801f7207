"""Cost of per-stream carrier offsets (qrl_demod_set_carrier_offsets) at the C1 and C2 shapes, in one process on one device.

Two handles on the same synthetic input (bench.py's synth): A with the shared offset of the workload, B with all-distinct per-stream offsets
(the workload's offset + 0.37 Hz x stream index).  Rounds alternate A and B; each round times `--steps` steps after `--warmup` steps with
device events around the steps on the handle's stream and keeps the mean step time.  Prints one JSON line per shape (median over rounds, ratio
B / A) and appends it to --out.

    python tools/per_stream_offset_ab.py [--shapes c1,c2] [--rounds 5] [--steps 10] [--warmup 3] [--out profiles/per_stream_offset_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {   # workload of bench.py: (sig mode, modem type, device rate, offset, batch, samples per stream)
    "c1": ("2fsk1k", 18, 1000000, 1200.0, 16384, 1 << 18),
    "c2": ("gmsk10k", 22, 25000000, 25000.0, 384, 25 * (1 << 16)),
}


def _time_steps(dem, iq, torch, steps, warmup):
    for _ in range(warmup):
        dem.process_async(iq)
    dem.sync()
    s = torch.cuda.ExternalStream(dem.lib.qrl_demod_stream(dem.h)) if hasattr(torch.cuda, "ExternalStream") else None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s) if s is not None else e0.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        dem.process_async(iq)
    dem.sync()
    e1.record(s) if s is not None else e1.record()
    e1.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    return e0.elapsed_time(e1) / steps, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import bench
    import qradiolink_amd as q
    dev = torch.device("cuda:0")
    ctx = q.Context(0)
    for name in a.shapes.split(","):
        mode, modem, rate, offset, batch, nsamp = SHAPES[name]
        iq = bench.synth(mode, rate, offset, batch, nsamp, 1234, torch, dev)
        hs = {}
        for kind in ("shared", "per_stream"):
            dem = q.Demod(ctx, modem, batch=batch, max_chunk=nsamp, device_samp_rate=rate, carrier_offset_hz=offset, side_outputs=True)
            if kind == "per_stream":
                dem.set_carrier_offsets([offset + 0.37 * b for b in range(batch)])
            hs[kind] = dem
        ms = {k: [] for k in hs}
        wall = {k: [] for k in hs}
        for r in range(a.rounds):
            for k in (("shared", "per_stream") if r % 2 == 0 else ("per_stream", "shared")):
                ev, w = _time_steps(hs[k], iq, torch, a.steps, a.warmup)
                ms[k].append(ev)
                wall[k].append(w)
        for dem in hs.values():
            dem.close()
        del iq
        torch.cuda.empty_cache()
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = dict(tool="per_stream_offset_ab", shape=name, mode=mode, rate=rate, batch=batch, nsamp=nsamp, steps=a.steps, warmup=a.warmup,
                   rounds=a.rounds, ms_shared=med["shared"], ms_per_stream=med["per_stream"], ratio=med["per_stream"] / med["shared"],
                   ms_shared_all=ms["shared"], ms_per_stream_all=ms["per_stream"],
                   wall_ms_shared=statistics.median(wall["shared"]), wall_ms_per_stream=statistics.median(wall["per_stream"]),
                   device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
