"""The launch plans of the three-step pass (exastencils_amd/csrc/ts3_plan.h) are host-only arithmetic: tests/ts3_plan_check.cpp, a
stand-alone program, walks every box with 1 .. 600 tile columns, {20, 63, 129, 255, 511, 1023} planes and {8, 12, 104, 256, 304} CUs
and checks that every (column, plane) lies in exactly one chunk of exactly one segment, that chunk lengths are multiples of four
except a segment's last, that block indices are dense, that no segment is empty and that a forced chunk length gives the uniform
grid the pass had before plans (same ntz and zc)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plans_cover_every_box_once(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile tests/ts3_plan_check.cpp")
    exe = str(tmp_path / "ts3_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "exastencils_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ts3_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK "), r.stdout[-2000:]
    assert int(r.stdout.split()[1]) >= 600 * 6 * 5 * 6       # at least the forced-zc plans of every box
