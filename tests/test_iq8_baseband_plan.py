"""The conditions of tests/test_gpu_iq8_baseband.py, on the CPU: under the launcher's own rule (qradiolink_amd/csrc/decim_plan.hpp:
decim_pm_streamable -> decim_pm_split -> pm_segments, with CallInput::iq8 set for the 8-bit calls) the cut schedule of tests/iq8_baseband.py
sends the 8-bit outputs of the 1:50 / 419-tap first stage (one lag tile) through all three routes -- the streaming kernel, its edge unit, the
per-output kernel -- and the last call streams at least SEGMENTS_WANTED segments per stream: the GPU test is a test of the streaming kernel's
2-byte ring path at one lag tile, not of the exact fallback.  tests/host/test_iq8_baseband_plan.cpp is a stand-alone program with its own main,
built here from decim_plan.hpp alone with the address and undefined-behaviour sanitizers and run directly; per segment it also checks the
ring arithmetic the kernel relies on (a group of 1600 bytes in a ring of 8 KiB)."""
import os
import subprocess

import pytest

import iq8_baseband as ib
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NT, WAVE_SLOTS = ib.PM_D, ib.PM_NT, ib.WAVE_SLOTS
FMT_CODE = {ib.CF32: 0, ib.SC16: 1, ib.SC8: 2, ib.CU8: 2}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("iq8_baseband_plan") / "test_iq8_baseband_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_iq8_baseband_plan.cpp"), "-o", path])
    return path


def _plan(exe, n, batch=ib.B):
    lines = ["stage %d %d %d %d\n" % (D, NT, batch, WAVE_SLOTS)]
    calls = ib.calls(n)
    for start, k, fmt, _ in calls:
        _, _, pitch, base16 = ib.placement(n, start, fmt)
        lines.append("call %d %d %d %d\n" % (k, FMT_CODE[fmt], pitch, base16))
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = [l.split() for l in r.stdout.splitlines()]
    assert out[-1] == ["ok", str(len(calls))], r.stdout[-2000:]
    per_call = [dict(zip(("n", "fmt", "streamable", "gen", "edge", "main", "S", "nseg", "turns100", "pieces"), map(int, l[2:]))) for l in out[:-2]]
    assert out[-2][0] == "total" and len(per_call) == len(calls)
    return calls, per_call, tuple(int(v) for v in out[-2][1:])


def test_the_schedule_holds_what_the_issue_lists_and_the_header_sees_it_so(exe):
    assert int(orc.low_pass(1, 1e6, 10e3, 10e3, orc.WIN_BH).size) == NT and orc.lib.orc_decim_uses_pm(NT, D)      # the one-tile stage (the program checks pm_tiles == 1)
    assert ib.N_PM % 8 == 0
    calls, per_call, _ = _plan(exe, ib.N_PM)
    assert [c["n"] for c in per_call] == [k for _, k, _, _ in calls]
    iq8 = [(f, k, c) for (_, k, f, _), c in zip(calls, per_call) if f in (ib.SC8, ib.CU8)]
    assert {f for f, _, _ in iq8} == {ib.SC8, ib.CU8}                                     # both 8-bit formats
    for fmt in (ib.SC8, ib.CU8):
        assert any(f == fmt and c["main"] > 0 for f, _, c in iq8), fmt                    # ... each in a call that streams
    assert any(k % 8 and k > 100 and not c["streamable"] for _, k, c in iq8)              # n % 8 != 0
    assert any(k == 2 and not c["streamable"] for _, k, c in iq8)                         # a 2-sample call
    assert any(k == 100 and c["main"] == 0 for _, k, c in iq8)                            # 100 samples: shorter than every look-back (k_dec2_fir: 130), no segment fits
    assert all(ib.placement(ib.N_PM, s, f)[2] > k for s, k, f, _ in calls)                # the row pitch is larger than n in every call
    assert all(ib.placement(ib.N_PM, s, f)[3] == 0 for s, k, f, _ in calls)               # every call starts on a 16-byte piece
    assert {ib.placement(ib.N_PM, s, f)[0] for s, _, f, _ in calls} >= {"plain", "shift2", "shift4"}      # ... starts 4 and 6 (mod 8) from shifted copies
    assert [st for _, _, _, st in calls] == sorted(st for _, _, _, st in calls) and {st for _, _, _, st in calls} == {0, 1}
    assert any(f == ib.CU8 and st == 1 for _, _, f, st in calls) and float(ib.BIAS1) != 127.5                # a cu8 bias other than 127.5
    fmts = [f for _, _, f, _ in calls]
    assert ib.CF32 in fmts[1:-1] and ib.SC16 in fmts[1:-1]                                # cf32 and int16 calls in between


def test_stream_length_comes_from_the_headers_pm_segments(exe):
    """ib.pm_segments (tests/sc16_baseband.py's) restates decim_plan.hpp's for every streamed call of the schedule; at N_PM the real split of
    the last call gives SEGMENTS_WANTED segments per stream, and at one segment's samples less it does not"""
    assert ib.SEGMENTS_WANTED >= 10
    for n, enough in ((ib.N_PM, True), (ib.N_PM - 128 * D, False)):
        _, per_call, _ = _plan(exe, n)
        for c in per_call:
            if c["main"]:
                assert ib.pm_segments(c["main"], ib.B, WAVE_SLOTS, ib.PM_LAGS) == (c["S"], c["nseg"]), c
        last = per_call[-1]
        assert (last["nseg"] >= ib.SEGMENTS_WANTED) == enough and last["nseg"] <= ib.SEGMENTS_WANTED, (n, last)


@pytest.mark.parametrize("n", [ib.N_PM, 400000])
def test_8_bit_outputs_take_all_three_routes_and_the_last_call_streams(exe, n):
    calls, per_call, (total, gen, edge, main) = _plan(exe, n)
    assert total == gen + edge + main and total > 0.75 * (n // D)
    assert gen > 100 and edge > 20 and main > 1000, (gen, edge, main)      # the per-output kernel, the edge unit, the streaming kernel
    assert 2 * main > total, (gen, edge, main)                              # the streamed range carries the majority of the 8-bit outputs
    for (start, k, fmt, _), c in zip(calls, per_call):
        if fmt in (ib.SC8, ib.CU8):
            assert c["fmt"] == 2 and c["streamable"] == (k % 8 == 0), (start, k)
            assert (c["main"] > 0) == (k % 8 == 0 and k > 5000), (start, k, c)
            if c["main"]:
                assert 2 <= c["pieces"] <= 3, c                             # a group of 1600 bytes: two or three of the ring's eight pieces
        if k % 8 and fmt in (ib.SC8, ib.CU8):                               # n % 8 != 0: the per-output kernel, every output
            assert c["edge"] == c["main"] == 0 and (c["gen"] > 0) == (k >= D), (start, k, c)
    last = per_call[-1]
    assert last["fmt"] == 2 and last["nseg"] >= ib.SEGMENTS_WANTED and last["S"] >= 64 and last["edge"] > 0, last
    assert last["turns100"] >= 100, last                                    # each segment more than a whole turn of a wave's 8 KiB ring at 2 bytes per sample
    first = per_call[0]
    assert first["fmt"] == 2 and first["nseg"] >= 2 and first["edge"] > 0, first
