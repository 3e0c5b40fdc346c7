"""fb::ldlt<N> (csrc/fb_se3.h) compiled for the host: tests/cpp/ldlt7_test.cpp checks the dense solver's failure rule, which
no finite OptimizeSim3 problem reaches on the device (H = J^T W J is positive semi-definite and lambda >= 0)."""
import os
import subprocess
import tempfile

from fishbirdeyevisualslam_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ldlt_failure_rule_on_the_host():
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "include")
    exe = os.path.join(tempfile.mkdtemp(), "ldlt7_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", rocm_include,
                           "-I", os.path.join(ROOT, "fishbirdeyevisualslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "ldlt7_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "ldlt7_test ok" in r.stdout, r.stdout
