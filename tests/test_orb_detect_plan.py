"""The host path of fb_orb_detect (csrc/orb_detect_plan.h) on the CPU: tests/cpp/orb_detect_plan_test.cpp, a stand-alone program
built with -fsanitize=address,undefined, runs the workspace and tile grid laid on the extractor's plan, the candidate bound,
the LDS layout of the selection kernel, the argument checks of both entry points (missing arrays, fast_threshold out of range,
kp_stride <= 0, a mask stride below the width, batch = 0 as a no-op) and the bytes the host entry point stages of each array."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_bound_argument_checks_and_staged_sizes_under_the_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(), "orb_detect_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "orb_detect_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    m = re.search(r"cases=(\d+) failures=(\d+)", r.stdout)
    assert m, r.stdout
    assert r.returncode == 0 and int(m.group(2)) == 0, r.stdout
    assert int(m.group(1)) >= 1000, r.stdout
