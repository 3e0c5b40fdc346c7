"""The covisibility handle's memory plan and scratch state (csrc/covis_plan.h) on the CPU: tests/cpp/covis_plan_test.cpp
crosses K 1 / 2 / 64 / 65 / 500 / 4096, n_mp 0 / 1 / 4094 / 4095 / 4096 / 100000, n_obs 0 / 1 / 63 / 600000, n_q 0 / 1 / K,
batch 1 / 2 / 3, recent_cap 0 / 1 / 255 / 256 / 257, n_features 0 / 1 / 2000, without and with a bird side, and checks that
every region is 256-byte aligned inside its part, that nothing overlaps, that the parts of a call follow each other with the
tail at the index's end, that every fb_covis_reserve* total is the one the size formulas gave before the plan, and that the
window's key-frame offsets do not depend on the point counts.  Then eight state sequences (window kept by a reuse, dropped by
an index at offset 0, growth, another map, a failed build, the guard of a host-pointer call, the bird window's kept index, an
editing call) with no device."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_sweep_reserve_totals_and_state_sequences():
    exe = os.path.join(tempfile.mkdtemp(), "covis_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "covis_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    m = re.search(r"cases=(\d+) failures=(\d+)", r.stdout)
    assert m, r.stdout
    assert r.returncode == 0 and int(m.group(2)) == 0, r.stdout
    assert int(m.group(1)) == 6 * 6 * 4 * 3 * 3 * 5 * 3 * 2 + 8, r.stdout
