"""The front end's host-side arithmetic (qradiolink_amd/csrc/decim_plan.hpp: which kernel a geometry gets, how a call's outputs are split
between the streaming kernel, the staged edge scratch and the per-output kernel, the segments of a launch) on the CPU:
tests/host/test_decim_plan.cpp, built with the address and undefined-behaviour sanitizers and fed the geometries from here."""
import os
import subprocess

import pytest

import front_end_rates as fer
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BH = orc.WIN_BH
NAMES = {"pm": fer.PM, "pl": fer.PL, "m16": fer.M16, "generic": fer.GENERIC}
# first stages of the modes at 1 Msps (engine.cpp: low_pass(1, 1e6, target / 2, target / 2)): D and the output rate
MODE_STAGES = [(25, 40000), (50, 20000), (100, 10000), (125, 8000)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("decim_plan") / "test_decim_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_decim_plan.cpp"), "-o", path])
    return path


def _run(exe, lines):
    r = subprocess.run([exe], input="".join("%s %d %d\n" % l for l in lines), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert out[-1].startswith("ok "), r.stdout[-2000:]
    return [l.split() for l in out[:-1]], int(out[-1].split()[1])


def _oracle_class(nt, D):
    """the oracle's rules in orc_decim_auto's order"""
    u = orc.lib
    return fer.PM if u.orc_decim_uses_pm(nt, D) else fer.PL if u.orc_decim_uses_pl(nt, D) else fer.M16 if u.orc_decim_uses_m16(nt, D) else fer.GENERIC


def _front_end_nt(D):
    return int(orc.frontend_taps(D * 1000000).size)


def test_library_partition_follows_the_table_and_the_oracle(exe):
    """decim_choose, the rule DecimStage::plan runs, for the front-end filter of every D = 2 .. 183 against front_end_rates (and so against
    the oracle's rules, which test_oracle.py pins to the same table), and for the 1:50 / 419-tap stage and the modes' first stages
    against the oracle's rules."""
    rates = [(D, _front_end_nt(D)) for D in range(fer.FIRST_D, fer.LAST_D + 1)]
    stages = [(50, 419)] + [(D, int(orc.low_pass(1, 1e6, rate / 2, rate / 2, BH).size)) for D, rate in MODE_STAGES]
    assert int(orc.low_pass(1, 1e6, 10e3, 10e3, BH).size) == 419
    got, _ = _run(exe, [("class", D, nt) for D, nt in rates + stages])
    assert len(got) == len(rates) + len(stages)
    wrong = []
    for (D, nt), line in zip(rates + stages, got):
        assert line[:3] == ["class", str(D), str(nt)], line
        lib = NAMES.get(line[3], line[3])
        want = {_oracle_class(nt, D)} | ({fer.front_end_class(D)} if (D, nt) in rates else set())
        if {lib} != want:
            wrong.append((D, nt, line[3], sorted(want)))
    assert not wrong, wrong
    assert NAMES[got[len(rates)][3]] == fer.PM   # the C1 front end


def test_call_plans_keep_every_cut_on_the_streaming_path(exe):
    """Every pm and every pl geometry of the front-end filter, and the 1:50 / 419-tap stage: random streams cut into calls of 2 samples up
    to 6000 D; the contracts of tests/host/test_decim_plan.cpp hold for every call and no geometry is left out."""
    pm = [D for D in range(fer.FIRST_D, fer.LAST_D + 1) if fer.front_end_class(D) == fer.PM]
    pl = [D for D in range(fer.FIRST_D, fer.LAST_D + 1) if fer.front_end_class(D) == fer.PL]
    assert len(pm) == 20 and len(pl) == 30
    cases = [(D, _front_end_nt(D), "pm") for D in pm] + [(50, 419, "pm")] + [(D, _front_end_nt(D), "pl") for D in pl]
    got, total = _run(exe, [("plan", D, nt) for D, nt, _ in cases])
    assert len(got) == len(cases)
    for (D, nt, contract), line in zip(cases, got):
        assert line[:4] == ["plan", str(D), str(nt), contract], line
        calls, staged, streamed = (int(v) for v in line[4:7])
        assert calls > 5000 and staged > 1000 and streamed > 1000, line   # the geometry contributed: calls, staged edges, streamed ranges
    print("calls checked: pm %d, pl %d" % (sum(int(l[4]) for l in got if l[3] == "pm"), sum(int(l[4]) for l in got if l[3] == "pl")))
    assert total == sum(int(l[4]) for l in got)
