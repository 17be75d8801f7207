"""Measurement plumbing of bench.py that can be checked without a GPU: the PMC traffic figure is tied to the kernel sources it was taken
on, the CPU baseline carries SURVEY 8(d)'s thread-per-block variant, and the committed traffic file belongs to the committed sources."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench   # noqa: E402


def test_committed_pmc_traffic_belongs_to_the_committed_kernel_sources():
    """profiles/pmc_traffic.json is only meaningful for the kernels it was measured on: its source id must be the id of
    qradiolink_amd/csrc + include as they are committed (re-run tools/profile_round.sh + tools/collect_round.py after a kernel change)."""
    d = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    if d["_source_id"] != bench.source_id():      # kernels changed since the pass: bench.py must then report no traffic, with the reason
        t, why = bench.pmc_traffic("c1", "k_decim_pm")
        assert t is None and d["_source_id"] in why
        pytest.skip("profiles/pmc_traffic.json is stale for these kernel sources: re-run tools/profile_round.sh + tools/collect_round.py")
    cal = d["_calibration"]["applied"]
    assert cal["FETCH_SIZE"] == 0.5 and cal["WRITE_SIZE"] == 1.0      # measured in the same pass: tools/pmc_calibrate.py
    for cfg in ("c1", "c2", "c3", "c4", "c5"):
        assert d[cfg]["fetch_bytes"] > 0 and d[cfg]["write_bytes"] > 0 and d[cfg]["kernel"].startswith("qrl::k_")


def test_traffic_is_reported_only_for_matching_sources(monkeypatch):
    d = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    monkeypatch.setattr(bench, "source_id", lambda: d["_source_id"])          # as if run on the sources of the pass
    t, src = bench.pmc_traffic("c1", "k_decim_pm")
    import re
    assert t and t > 35e9 and re.fullmatch(r"profiles/r\d\d_pmc_summary\.txt", src)   # 35.1 GB of algorithmic bytes per launch
    assert bench.pmc_traffic("c1", "k_decim_pm", default_shape=False) == (None, None)
    assert bench.pmc_traffic("c1", "k_some_other_kernel") == (None, None)
    monkeypatch.setattr(bench, "source_id", lambda: "000000000000")
    t, why = bench.pmc_traffic("c1", "k_decim_pm")
    assert t is None and "000000000000" in why


def test_issue_bound_of_the_qpsk_receivers(monkeypatch):
    """round 4: C3 and C5 carry roofline.issue -- VALU wave instructions of one receiver call from the SQ_INSTS_* pass of the same round,
    tied to the same source id, over the RX-alone time measured in the bench."""
    d = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    monkeypatch.setattr(bench, "source_id", lambda: d["_source_id"])
    for cfg, secs in (("c3", 1.93e-3), ("c5", 3.4e-3)):
        r = bench.issue_roofline(cfg, secs)
        top = bench.promote_issue(dict(bound="hbm", achieved=1.0, peak=8000.0, unit="GB/s", frac=0.1, kernel="k_x"), r, "k_qpsk_pipe4", "why")
        assert top["bound"] == "issue" and top["frac"] == r["frac"] and top["kernel"] == "k_qpsk_pipe4" and top["hbm"]["kernel"] == "k_x"   # round 5: the issue side is the headline of these sub-lines
        assert r["bound"] == "issue" and r["peak"] == bench.VALU_ISSUE_PEAK_G and 0.05 < r["frac"] < 1.0
        assert r["valu_wave_instr_per_rx_call"] > 1e8 and "all_classes_frac" not in r and r["all_wave_instr_per_rx_call"] > r["valu_wave_instr_per_rx_call"]   # round 6: no figure that can exceed 1
        assert any("k_fec" in k for k in r["by_kernel"]) and any("k_qpsk_pipe4" in k for k in r["by_kernel"])
        assert not any("k_tx_" in k for k in r["by_kernel"])          # the modulator's kernels are not part of a receiver call
    assert bench.issue_roofline("c5", 3.4e-3, default_shape=False) is None
    monkeypatch.setattr(bench, "source_id", lambda: "000000000000")
    assert bench.issue_roofline("c5", 3.4e-3)["frac"] is None


def test_traffic_close_to_the_algorithmic_bytes_for_the_streaming_front_ends():
    d = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    alg = {"c1": 16384 * 262144 * 8.178, "c2": 384 * 1638400 * 8.033, "c3": 384 * 1638400 * 8.0625}
    for cfg, a in alg.items():
        ratio = (d[cfg]["fetch_bytes"] + d[cfg]["write_bytes"]) / a
        assert 0.98 < ratio < 1.10, (cfg, ratio)
    # C4 (round 5: the record carries the whole chain): the streaming channelizer reads the wideband input once and writes the 64 channel rings once
    # (8 + 8 B per sample); the per-channel kernel re-reads the ring with its 20 % halo and writes int16 + the RRC ring; the chain's sum is what
    # bench.py reports as `traffic` -- two ring hand-offs above the algorithmic 10.3 B per sample
    if "chain_by_kernel" in d["c4"]:
        n = 64 * (1 << 21)
        pfb = [v for k, v in d["c4"]["chain_by_kernel"].items() if k.startswith("k_pfb_stream64")]
        assert pfb and 0.98 < pfb[0] / (n * 16.0) < 1.06
        assert abs(sum(d["c4"]["chain_by_kernel"].values()) - d["c4"]["chain_bytes"]) < 1.0
        assert 3.0 < d["c4"]["chain_bytes"] / (n * bench.C4_BYTES) < 4.5


def test_cpu_baseline_has_the_thread_per_block_variant():
    r = bench.cpu_baseline("c1", 2, budget_s=0.4)
    assert r["kind"] == "port" and r["cores"] == 2 and r["value"] > 0 and r["single_thread"] > 0
    tpb = r["thread_per_block_model"]
    assert tpb["blocks"] >= 10 and tpb["value"] > r["single_thread"] and 0 < tpb["slowest_block_share"] <= 1


def test_source_id_changes_with_the_kernel_sources(tmp_path, monkeypatch):
    a = bench.source_id()
    assert len(a) == 12 and a == bench.source_id()
    # a copy of the tree with one byte appended to a kernel file gives another id
    import shutil
    for d in ("qradiolink_amd/csrc", "include"):
        dst = tmp_path / d
        dst.mkdir(parents=True)
        for fn in os.listdir(os.path.join(ROOT, d)):
            if fn.endswith((".hip", ".cpp", ".hpp", ".h")):
                shutil.copy(os.path.join(ROOT, d, fn), dst / fn)
    with open(tmp_path / "qradiolink_amd/csrc/kernels_ff.hip", "a") as f:
        f.write("\n")
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.source_id() != a


def test_front_end_flop_roofline_on_the_committed_default_line():
    """c1 / c2 / c3 carry the f32 flop roofline of their front-end kernel beside the HBM one (C2 / C3 are compute bound: profiles/r05_sq_front_end_counters.txt);
    on c3 it sits with the HBM figures under roofline.hbm (the issue roofline is that line's headline)"""
    import json
    import os
    import bench
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r05_bench_default_with_traffic.json")
    d = json.loads(open(path).read().strip().splitlines()[-1])
    f1, f2, f3 = d["roofline"]["flops"], d["c2"]["roofline"]["flops"], d["c3"]["roofline"]["hbm"]["flops"]
    for f, name in ((f1, "c1"), (f2, "c2"), (f3, "c3")):
        assert f["bound"] == "f32" and f["peak"] == bench.F32_PEAK_TFLOPS and abs(f["algorithmic_flop_per_sample"] - bench.FRONT_END_FLOP[name]) < 0.06
        assert abs(f["frac"] - f["achieved"] / f["peak"]) < 1e-3
    assert 0.35 < f2["frac"] < 0.55 and 0.33 < f3["frac"] < 0.55 and f1["frac"] < 0.2
    assert abs(bench.FRONT_END_FLOP["c2"] - (4 * 1045 / 25 + 6)) < 1e-9


def test_dump_outputs_are_a_fixed_sample_cut_at_the_valid_lengths(tmp_path):
    """--dump-outputs: the same seeded sample of streams on every run, every port cut at its stream's valid length (the rest zero), float32,
    counts of every stream, and at most bench.DUMP_MAX_BYTES in all"""
    import torch
    B = 1000
    g = torch.Generator().manual_seed(1)
    ports = dict(filtered=torch.randn((B, 50), dtype=torch.complex64, generator=g), constellation=None,
                 bits_a=torch.randint(0, 2, (B, 30), dtype=torch.uint8, generator=g), bits_b=torch.randint(0, 2, (B, 30), dtype=torch.uint8, generator=g),
                 counts=torch.randint(0, 60, (B, 4), dtype=torch.int32, generator=g))

    class Dem:
        def _ports(self):
            return ports
    a = bench.snapshot_outputs(bench.demod_ports(Dem()), torch)
    b = bench.snapshot_outputs(bench.demod_ports(Dem()), torch)
    assert sorted(a) == ["bits_a", "bits_b", "counts", "filtered", "streams"] and all(np.array_equal(a[k], b[k]) for k in a)
    s = a["streams"].astype(np.int64)
    assert s.size == 256 and np.all(np.diff(s) > 0) and a["counts"].shape == (B, 4) and a["filtered"].shape == (256, 50, 2)
    c = ports["counts"].numpy()[s]
    for i in (0, 7, 255):
        want = torch.view_as_real(ports["filtered"][s[i], :c[i, 0]]).numpy()
        assert np.array_equal(a["filtered"][i, :c[i, 0]], want) and not a["filtered"][i, c[i, 0]:].any()
        assert np.array_equal(a["bits_b"][i, :c[i, 3]], ports["bits_b"][s[i], :c[i, 3]].numpy()) and not a["bits_b"][i, c[i, 3]:].any()
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    bench.write_outputs(str(tmp_path / "out"), a)
    assert np.array_equal(np.load(tmp_path / "out" / "filtered.npy"), a["filtered"])
    old = bench.DUMP_MAX_BYTES
    try:
        bench.DUMP_MAX_BYTES = 100000
        small = bench.snapshot_outputs(bench.demod_ports(Dem()), torch)
        assert 1 <= small["streams"].size < 256 and sum(v.nbytes for v in small.values()) <= 100000
    finally:
        bench.DUMP_MAX_BYTES = old


def test_dump_outputs_budget_covers_ports_without_valid_lengths(monkeypatch):
    """a port without valid lengths that is larger than a quarter of the budget (C5's modulator output: [16384, 16384] complex64 at the
    default shape) is sampled with the streams like the others, never written whole: the arrays stay within bench.DUMP_MAX_BYTES"""
    import torch
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 20)
    B = 1024
    g = torch.Generator().manual_seed(2)
    big = torch.randn((B, 1024), dtype=torch.complex64, generator=g)                      # 8 MiB as float32: 8 x the budget
    counts = torch.randint(0, 64, (B, 4), dtype=torch.int32, generator=g)
    bits = torch.randint(0, 2, (B, 64), dtype=torch.uint8, generator=g)
    o = bench.snapshot_outputs({"tx": (big, None), "counts": (counts, None), "bits_a": (bits, counts[:, 2])}, torch)
    s = o["streams"].astype(np.int64)
    assert sum(v.nbytes for v in o.values()) <= 1 << 20
    assert o["counts"].shape == (B, 4) and o["tx"].shape == (s.size, 1024, 2) and 1 <= s.size < B
    assert np.array_equal(o["tx"], torch.view_as_real(big[torch.as_tensor(s)]).numpy())
    # C5 hands its modulator output with a full valid length per stream: the same sample
    o2 = bench.snapshot_outputs({"tx": (big, torch.full((B,), 1024)), "counts": (counts, None), "bits_a": (bits, counts[:, 2])}, torch)
    assert all(np.array_equal(o[k], o2[k]) for k in o)
    # one stream larger than the whole budget: refused, not written past it
    with pytest.raises(SystemExit):
        bench.snapshot_outputs({"tx": (torch.zeros((4, 1 << 18), dtype=torch.complex64), None)}, torch)


def test_dump_outputs_refused_up_front_where_not_covered():
    """C4's channel-sharded path has no dump: refused while the arguments are parsed (every rank, before any setup), not after the timed steps"""
    import subprocess
    for extra in (["--cluster"], ["--gpus", "2"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c4", "--dump-outputs", "unused"] + extra,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--dump-outputs covers the single-GPU C4 path only" in r.stderr


def test_command_line_has_full_and_dump_outputs():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
