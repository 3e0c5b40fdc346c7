"""The matchers' LDS plan (csrc/match_plan.h) on the CPU: tests/cpp/match_plan_test.cpp crosses target strides 1 / 63 / 64 /
65 / 1023 / 1024 / 1025 / 2064 / 2900 / 3400 / 4000 / 8000 / 65535, query strides 0 / 1 / 1024 / 2400 / 5000 / 50000, the front
grid (64 x 48 cells), the bird grid (32 x 32) and one cell, with the M3 cache on and off, and checks for every kernel family
that each region is aligned for its element, inside the launch's bytes and disjoint from what lives with it, that the
overlays are the documented ones, and that variant and bytes are those of the launchers' formulas before the plan (restated
in the test) outside the two windows the plan closes.  Then 21 named cases: one shape per variant -- the four M3 rungs, the
tails with the items and the camera copy in and out of LDS, both sides of descInLds for BoW, triangulation, k_sim3,
k_init_match and fuse -- and one per window."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_sweep_layouts_variants_and_named_shapes():
    exe = os.path.join(tempfile.mkdtemp(), "match_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "match_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    m = re.search(r"cases=(\d+) failures=(\d+)", r.stdout)
    assert m, r.stdout
    assert r.returncode == 0 and int(m.group(2)) == 0, r.stdout
    assert int(m.group(1)) == 13 * 6 * 3 * 2 + 21, r.stdout
