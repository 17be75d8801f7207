#!/usr/bin/env python3
"""The ordering workload: four small profiled calls on every receiver and channelizer configuration whose host code orders streams
differently, with one stream_wait (channelizers: and one wait_for), one reset and one read of the profile each.  Run it under a HIP API
trace at two commits and compare what the library asked of the runtime:

    rocprofv3 --hip-trace -f json -d OUT -o trace -- python tools/order_trace.py
    python tools/order_trace.py --digest OUT/trace_results.json [SEQUENCE.txt]    (at both commits; equal digests = the same calls in the same order)

The digest covers, in order, every hipEventRecord, hipStreamWaitEvent, kernel-launch entry point, hipMemsetAsync and hipStreamSynchronize
of the process (torch's own among them: the same in both runs).  The json form of the trace carries the calls' arguments: streams, events
and kernel addresses go into the digest numbered by first appearance (anew after a destroy), the launch geometry as it is.  The csv form (..._hip_api_trace.csv)
has names only; the digest line says which was compared."""
import csv
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERED = re.compile(r"^(hipEventRecord\w*|hipStreamWaitEvent\w*|hipMemsetAsync\w*|hipStreamSynchronize\w*|hip\w*Launch\w*Kernel\w*)$")


def _rows(path):
    """(start, name, args) of every HIP API call of a trace: args is None for the csv form, which has no argument column, and the list of
    {name, value} of the json form"""
    if path.endswith(".csv"):
        with open(path, newline="") as f:
            return [(int(r["Start_Timestamp"]), r["Function"], None) for r in csv.DictReader(f)]
    with open(path) as f:
        tool = json.load(f)["rocprofiler-sdk-tool"][0]
    kinds = tool["strings"]["buffer_records"]
    return [(r["start_timestamp"], kinds[r["kind"]]["operations"][r["operation"]], r.get("args", [])) for r in tool["buffer_records"]["hip_api"]]


def digest(path):
    ids, seq, per_name, with_args = {}, [], {}, False
    for _, name, args in sorted(_rows(path), key=lambda r: r[0]):
        if name in ("hipEventDestroy", "hipStreamDestroy"):   # the runtime hands the address out again: what comes after is another object
            for a in args or []:
                ids.pop(a["value"], None)
        if not ORDERED.match(name):
            continue
        per_name[name] = per_name.get(name, 0) + 1
        if args is not None:   # streams, events and kernels numbered by first appearance; launch geometry as it is
            with_args = True
            parts = []
            for a in args:
                if a["name"] in ("stream", "hStream", "event", "function_address", "f"):
                    if a["value"] not in ids:
                        ids[a["value"]] = ids["next"] = ids.get("next", -1) + 1
                    parts.append("%s=#%d" % (a["name"], ids[a["value"]]))
                elif a["name"] in ("numBlocks", "dimBlocks", "sharedMemBytes"):
                    parts.append("%s=%s" % (a["name"], a["value"]))
            name += "(" + ", ".join(parts) + ")"
        seq.append(name)
    text = "\n".join(seq) + "\n"
    print("%s  %d calls, %s" % (hashlib.sha256(text.encode()).hexdigest(), len(seq),
                                "names, stream / event / kernel identities, launch geometry" if with_args else "names only"))
    for name in sorted(per_name):
        print("  %-36s %d" % (name, per_name[name]))
    return text


def workload():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import qradiolink_amd as q

    ctx = q.Context(0)
    side = torch.cuda.Stream()
    rng = np.random.default_rng(5)

    def noise(rows, n):
        x = 0.05 * (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n)))
        return torch.from_numpy(x.astype(np.complex64)).cuda()

    def receiver(modem, B=2, n=4096, rate=1000000, setup=None, between=None):
        dem = q.Demod(ctx, modem, batch=B, max_chunk=n, device_samp_rate=rate)
        if setup:
            setup(dem)
        dem.profile(True)
        x = noise(B, 4 * n)
        for k in range(4):
            if between:
                between(dem, k)
            dem.process_async(x[:, k * n:(k + 1) * n])
            if k == 1:
                dem.stream_wait(side.cuda_stream)
            if k == 2:
                dem.reset()
        print(modem, rate, dem.profile_read())
        dem.close()

    def channelizer(M, B=2, n1=100, setup=None, **kw):
        form3 = kw.get("form") == 3
        n = n1 * (1 if form3 else M)
        ch = q.Channelizer(ctx, M, batch=B, max_chunk=n, **kw)
        if setup:
            setup(ch)
        ch.profile(True)
        x = noise(B, 4 * n)
        for k in range(4):
            part = x[:, k * n:(k + 1) * n]
            if k == 1:
                ch.wait_for(side.cuda_stream)
            if form3:
                ch.process_channels_async(part, n)
            else:
                ch.process_async(part)
            if k == 1:
                ch.stream_wait(side.cuda_stream)
            if k == 2:
                ch.reset()
        print(M, kw, ch.profile_read_kernels(), ch.profile_read())
        ch.close()

    receiver(q.MODEM_2FSK1K, setup=lambda d: d.set_option(q.OPT_OVERLAP, 1))
    receiver(q.MODEM_2FSK1K, setup=lambda d: d.set_option(q.OPT_OVERLAP, 0))
    receiver(q.MODEM_QPSK20K, B=3, setup=lambda d: d.set_option(q.OPT_GROUPED, 1))
    receiver(q.MODEM_QPSK20K, B=3, setup=lambda d: d.set_option(q.OPT_GROUPED, 0))
    receiver(q.MODEM_QPSK20K, B=3, setup=lambda d: d.set_option(q.OPT_GROUPED, 1), between=lambda d, k: d.set_option(q.OPT_GROUPED, k & 1))
    receiver(q.MODEM_BPSK1K)
    receiver(q.MODEM_DMR, setup=lambda d: d.enable_dmo_sink())
    receiver(q.MODEM_NBFM5000)
    receiver(q.MODEM_GMSK10K, B=4, n=8 * 4096, rate=8000000, setup=lambda d: d.set_option(q.OPT_INPUT_RESIDENT, 1))
    channelizer(10, setup=lambda c: c.enable_4fsk())
    channelizer(1, n1=2000)
    channelizer(1, B=4, form=3)
    torch.cuda.synchronize()
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--digest":
        text = digest(sys.argv[2])
        if len(sys.argv) == 4:
            with open(sys.argv[3], "w") as f:
                f.write(text)
    else:
        workload()
