"""The plan of the bundle adjustment (csrc/ba_plan.h) on the CPU: tests/cpp/ba_plan_test.cpp crosses 10 counts of free key
frames with 7 point counts, 6 odometry edge counts, world 1 / 2 and a workgroup cap of 2 / 256 and checks every figure of the
plan, the exchange block's offsets and each scratch slot's size against the driver's formulas before the plan (restated in the
test), and the invariants launcher and kernels rely on (chunk rounding, accumulator tiles of the chosen Schur variant, dynamic
+ static LDS within 160 KiB, aligned slots that do not overlap); then which Schur variants are reachable over every count of
free key frames (683 rows + 1), the odometry rule at every edge count up to 1000, the hand derivation of
ba_cases.NWG_CAP_FOR_CHUNKS and the schedule's slot counts."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_sweep_against_the_driver_before_the_plan():
    exe = os.path.join(tempfile.mkdtemp(), "ba_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "ba_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    m = re.search(r"cases=(\d+) failures=(\d+)", r.stdout)
    assert m, r.stdout
    assert r.returncode == 0 and int(m.group(2)) == 0, r.stdout
    assert int(m.group(1)) == 10 * 7 * 6 * 2 * 2 + 683 + 1 + 1001 + 1 + 1, r.stdout
