"""The conditions of tests/test_gpu_sc16_baseband.py, on the CPU: under the launcher's own rule (qradiolink_amd/csrc/decim_plan.hpp:
decim_pm_streamable -> decim_pm_split -> pm_segments) the cut schedule of tests/sc16_baseband.py sends the int16 outputs of the 1:50 / 419-tap
first stage (one lag tile) through all three routes -- the streamed range, the staged edge unit, the per-output kernel -- and the streamed
range carries most of them: the GPU test is a test of the streaming kernel's 4-byte path, not of the exact fallback.
tests/host/test_sc16_baseband_plan.cpp is built with the address and undefined-behaviour sanitizers, as tests/test_decim_plan_host.py
builds its program, and checks per segment what the kernel relies on."""
import os
import subprocess

import pytest

import orc
import sc16_baseband as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NT, WAVE_SLOTS = sb.PM_D, sb.PM_NT, sb.WAVE_SLOTS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("sc16_baseband_plan") / "test_sc16_baseband_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_sc16_baseband_plan.cpp"), "-o", path])
    return path


def _plan(exe, n, batch=sb.B):
    lines = ["stage %d %d %d %d\n" % (D, NT, batch, WAVE_SLOTS)]
    calls = sb.calls(n)
    for start, k, fmt, _ in calls:
        _, _, pitch, base16 = sb.placement(n, start, fmt)
        lines.append("call %d %d %d %d\n" % (k, fmt == sb.SC16, pitch, base16))
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = [l.split() for l in r.stdout.splitlines()]
    assert out[-1] == ["ok", str(len(calls))], r.stdout[-2000:]
    per_call = [dict(zip(("n", "sc16", "streamable", "gen", "edge", "main", "S", "nseg", "turns100"), map(int, l[2:]))) for l in out[:-2]]
    assert out[-2][0] == "total" and len(per_call) == len(calls)
    return calls, per_call, tuple(int(v) for v in out[-2][1:])


def test_the_schedule_holds_what_the_issue_lists_and_the_header_sees_it_so(exe):
    """the cases of the issue are in the schedule, and decim_plan.hpp's rule treats each as the GPU test's docstring says"""
    assert int(orc.low_pass(1, 1e6, 10e3, 10e3, orc.WIN_BH).size) == NT and orc.lib.orc_decim_uses_pm(NT, D)      # the one-tile stage (the program checks pm_tiles == 1)
    calls, per_call, _ = _plan(exe, sb.N_PM)
    assert [c["n"] for c in per_call] == [k for _, k, _, _ in calls]
    sc = [(k, c) for (_, k, f, _), c in zip(calls, per_call) if f == sb.SC16]
    assert any(k % 4 and k > 2 and not c["streamable"] for k, c in sc)               # n % 4 != 0
    assert any(k == 2 and not c["streamable"] for k, c in sc)                        # a 2-sample call
    assert any(2 < k < 130 and c["streamable"] and c["main"] == 0 for k, c in sc)    # shorter than the shortest look-back (k_dec2_fir: 130 samples): no segment fits
    assert all(sb.placement(sb.N_PM, s, f)[2] > k for s, k, f, _ in calls)           # the row pitch is larger than n in every call
    assert all(sb.placement(sb.N_PM, s, f)[3] == 0 for s, k, f, _ in calls)          # every call starts on a 16-byte piece
    assert len({float(x) for _, _, _, x in calls}) == 2 and float(calls[0][3]) == float(sb.SCALE0) != float(calls[-1][3])
    fmts = [f for _, _, f, _ in calls]
    assert any(a == sb.SC16 and b == sb.CF32 for a, b in zip(fmts, fmts[1:])) and any(a == sb.CF32 and b == sb.SC16 for a, b in zip(fmts, fmts[1:]))
    # the receiver added for the register kernel: the 837-tap 1:100 first stage of the 4FSK sps = 10 modes is k_decim_plx's, QPSK-2k's 3 621 taps are not
    nt100 = int(orc.low_pass(1, 1e6, 5e3, 5e3, orc.WIN_BH).size)
    assert nt100 == 837 and orc.lib.orc_decim_uses_pl(nt100, 100) and not orc.lib.orc_decim_uses_pm(nt100, 100) and orc.lib.orc_decim_uses_pm(3621, 100)
    assert "k_decim_plx" in sb.case("4fsk1kfm")["reader"]


def test_stream_length_comes_from_the_headers_pm_segments(exe):
    """sb.pm_segments restates decim_plan.hpp's for every streamed call of the schedule; at N_PM the real split of the last call gives
    SEGMENTS_WANTED segments per stream (sb derives the length with a bound on the outputs in front of the first segment, so it may
    overshoot by less than one segment), and at one segment's samples less it does not"""
    for n, enough in ((sb.N_PM, True), (sb.N_PM - 128 * D, False)):
        _, per_call, _ = _plan(exe, n)
        for c in per_call:
            if c["main"]:
                assert sb.pm_segments(c["main"], sb.B, WAVE_SLOTS, sb.PM_LAGS) == (c["S"], c["nseg"]), c
        last = per_call[-1]
        assert (last["nseg"] >= sb.SEGMENTS_WANTED) == enough and last["nseg"] <= sb.SEGMENTS_WANTED, (n, last)


@pytest.mark.parametrize("n", [sb.N_PM, 400000])
def test_int16_outputs_take_all_three_routes_and_most_are_streamed(exe, n):
    calls, per_call, (total, gen, edge, main) = _plan(exe, n)
    assert total == gen + edge + main and total > 0.75 * (n // D)
    assert gen > 100 and edge > 20 and main > 1000, (gen, edge, main)
    assert 2 * main > total, (gen, edge, main)                     # the streamed range carries the majority of the int16 outputs
    for (start, k, fmt, _), c in zip(calls, per_call):
        if fmt == sb.SC16:
            assert c["streamable"] == (k % 4 == 0), (start, k)
            assert (c["main"] > 0) == (k % 4 == 0 and k > 5000), (start, k, c)
        if k % 4:                                                       # n % 4 != 0: the per-output kernel, every output
            assert c["edge"] == c["main"] == 0 and (c["gen"] > 0) == (k >= D), (start, k, c)
    # the last call: several streamed segments per stream, each several turns of a wave's 8 KiB ring at 4 bytes per sample
    last = per_call[-1]
    assert last["sc16"] and last["nseg"] >= 4 and last["S"] >= 64 and last["turns100"] >= 200, last
    first = per_call[0]
    assert first["sc16"] and first["nseg"] >= 2 and first["edge"] > 0, first
