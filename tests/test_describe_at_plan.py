"""The host path of fb_orb_describe (csrc/orb_describe_at_plan.h) on the CPU: tests/cpp/describe_at_plan_test.cpp, a stand-alone
program built with -fsanitize=address,undefined, runs the LDS layout shared by launcher and kernel, the argument checks of both
entry points (never extracted, batch above the last batch, IC mode without images, strides, missing arrays, empty calls) and
the bytes the host entry point stages of each array."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_argument_checks_and_staged_sizes_under_the_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(), "describe_at_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "describe_at_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    m = re.search(r"cases=(\d+) failures=(\d+)", r.stdout)
    assert m, r.stdout
    assert r.returncode == 0 and int(m.group(2)) == 0, r.stdout
    assert int(m.group(1)) >= 40, r.stdout
