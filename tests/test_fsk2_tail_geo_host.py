"""The host-side arithmetic of k_2fsk_tail (qradiolink_amd/csrc/fsk2_tail_geo.hpp: LDS layout and bank mapping, the windows and ring slots of a
call of any length, the y windows that go back to the history ring, which calls get the kernel) on the CPU: tests/host/test_fsk2_tail_geo.cpp,
built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_fsk2_tail_geo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_fsk2_tail_geo.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100000, r.stdout[-2000:]
