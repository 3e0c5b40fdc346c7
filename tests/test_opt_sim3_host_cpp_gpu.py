"""tests/cpp/opt_sim3_host_test.cpp drives the header-only fishbird::Optimizer::OptimizeSim3 (host/fishbird_host.hpp) in a
fresh child process against the C entry point on the same arrays."""
import os
import subprocess
import tempfile

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_header_optimize_sim3():
    import fishbirdeyevisualslam_amd as fb
    pkg = os.path.dirname(fb.LIB_PATH)
    exe = os.path.join(tempfile.mkdtemp(), "opt_sim3_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"),
                           os.path.join(ROOT, "tests", "cpp", "opt_sim3_host_test.cpp"), "-o", exe, "-L", pkg, "-lfishbird_hip",
                           "-Wl,-rpath," + pkg])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"opt_sim3_host_test ok" in r.stdout
