"""The extractor's workspace plan (csrc/orb_plan.h) on the CPU: tests/cpp/orb_plan_test.cpp runs plan_orb() over the image
sizes and pyramids of the GPU tests and a sweep of 45..700 px at scale 1.1 / 1.2 / 1.5 / 2.0 with 1..8 levels, and checks
that the regions of one image are disjoint and inside their strides, that the grid bases and LDS carves add up, that a
refusal returns its code and leaves a filled plan byte for byte unchanged, and the 640x480 known answers."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_sweep_refusals_and_known_answers():
    exe = os.path.join(tempfile.mkdtemp(), "orb_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "orb_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    m = re.search(r"cases=(\d+) refused=(\d+) failures=(\d+)", r.stdout)
    assert m, r.stdout
    assert r.returncode == 0 and int(m.group(3)) == 0, r.stdout
    assert int(m.group(1)) > 5000 and 0 < int(m.group(2)) < int(m.group(1)), r.stdout
