"""The frame handle's memory plan (csrc/track_plan.h) on the CPU: tests/cpp/track_plan_test.cpp runs plan_frame() over
batch 1 / 2 / 3 / 256, 50..2000 features at 1..8 levels and map / list capacities 1 / 7 / 2000 / 4096, and checks that every
region is 256-byte aligned inside its arena, that nothing overlaps but the two declared aliases, that front-side scratch never
meets bird-side scratch, that the byte counts are those of the separate buffers the handle used to own, the member and BoW
lists, the initial fills, that a refusal leaves the plan alone, and that a handle's device memory did not grow."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_sweep_aliases_sizes_and_granted_bytes():
    exe = os.path.join(tempfile.mkdtemp(), "track_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "track_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    m = re.search(r"cases=(\d+) failures=(\d+)", r.stdout)
    assert m, r.stdout
    assert r.returncode == 0 and int(m.group(2)) == 0, r.stdout
    assert int(m.group(1)) == 4 * 4 * 8 * 64, r.stdout
    assert len(re.findall(r"granted bytes per handle", r.stdout)) == 4, r.stdout
