"""The plan of an 8-bit call, on the CPU: tests/host/test_iq8_plan.cpp is a stand-alone program over qradiolink_amd/csrc/decim_plan.hpp, built here with
the address and undefined-behaviour sanitizers (host code, no Python in the process).  For D in {9, 18, 25, 27, 50, 98, 100} and calls whose
length, row pitch and base are and are not whole 16-byte pieces of 2-byte samples it checks that decim_pm_streamable says what the rule says
and, for the streamable calls, that every segment's first piece is 16-byte aligned inside the row and that the last byte any lane may fetch lies
inside row + row_bytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("iq8_plan") / "test_iq8_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_iq8_plan.cpp"), "-o", path])
    return path


def test_the_plan_of_8_bit_calls_holds_what_the_kernel_relies_on(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    word, calls, streamable, segments = r.stdout.split()
    assert word == "ok"
    # 7 rates x 5 stream positions x 14 lengths x 5 pitches x 3 bases; of the calls whose length is a multiple of 8, two pitches in five and one base in three are streamable; segments were walked
    assert int(calls) == 7 * 5 * 14 * 5 * 3
    assert int(streamable) == 7 * 5 * 7 * 2 * 1
    assert int(segments) > 1000


def test_the_older_seven_field_initialiser_still_compiles():
    """tests/host/test_sc16_baseband_plan.cpp brace-initialises CallInput with seven positional fields: the new field has a default"""
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "tests", "host", "test_sc16_baseband_plan.cpp")])
