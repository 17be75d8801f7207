"""The run list of gr_zero_idle_bursts (qradiolink_amd/csrc/zero_runs.hpp: what qrl_mod_add_zero_runs and qrl_synth_add_zero_runs keep
between calls) on the CPU: tests/host/test_zero_runs.cpp, built with the address and undefined-behaviour sanitizers, checks add() and split()
against the block's rule over a few hundred random tag sets and call cuts."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_zero_run_list_follows_the_block_rule(tmp_path):
    exe = str(tmp_path / "test_zero_runs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_zero_runs.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
