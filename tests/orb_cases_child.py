"""Child process of test_orb_cases_gpu.py: every extractor case with the 256-thread instantiation of k_octree.

    python orb_cases_child.py OUT.npz

The caller sets FB_OCT_WIDE_MAX=0 (no launch is small enough for the 1024-thread instantiation); the variable is read
once per process, hence the process.  Everything is written to OUT.npz and judged by the caller.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import orb_cases_hip as G  # noqa: E402

if __name__ == "__main__":
    assert os.environ.get("FB_OCT_WIDE_MAX") == "0"
    np.savez(sys.argv[1], **G.collect())
