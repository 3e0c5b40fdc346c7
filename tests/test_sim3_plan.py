"""The plan of the two Sim3 stages (csrc/sim3_plan.h) on the CPU: tests/cpp/sim3_plan_test.cpp crosses KF1 strides 1 / 63 / 64 /
65 / 2363 / 2364 / 3402 / 3403 / 65535 with 1 / 12 / 64 candidates for the solver and for OptimizeSim3 and checks variant,
dynamic LDS bytes and workspace bytes against the launchers' formulas before the plan (restated in the test) and against the
160 KiB of a workgroup; then the keep rule on a table with one row per skip clause and the row just inside each bound
(25 rows), and the four outcomes of the workspace refusal."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_sweep_keep_rule_and_workspace_refusal():
    exe = os.path.join(tempfile.mkdtemp(), "sim3_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "sim3_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    m = re.search(r"cases=(\d+) failures=(\d+)", r.stdout)
    assert m, r.stdout
    assert r.returncode == 0 and int(m.group(2)) == 0, r.stdout
    assert int(m.group(1)) == 9 * 3 * 2 + 25 + 4, r.stdout
