"""Builds the HIP library (libfishbird_hip.so) in-tree for gfx950.

    python -m fishbirdeyevisualslam_amd.build [--force]

hipcc cross-compiles without a GPU.  -ffp-contract=off is part of the parity contract:
float expressions are evaluated exactly as written (see csrc/fb_detmath.h).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libfishbird_hip.so")
SOURCES = ["runtime.hip", "match.hip", "match_bow.hip", "frame.hip", "track.hip", "bow.hip", "orb.hip", "pose.hip", "ba.hip", "mapping.hip", "kfdb.hip", "sim3_solver.hip", "opt_sim3.hip", "covis.hip"]
# Files whose results are held to a floating-point tolerance (poses: 1e-4 relative), not to bit equality with the
# oracle: fused multiply-adds are allowed there.  An LM evaluation of k_pose_opt is ~75 % fp64 edge arithmetic that one
# wave per SIMD issues back to back; mul + add pairs instead of fma made it a quarter longer.
FMA_OK = {"pose.hip", "opt_sim3.hip"}
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fgpu-rdc=0" if False else "-Wall", "-Wno-unused-function"]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def needs_build():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "fishbird.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    srcs = [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    if not force and not needs_build():
        return OUT
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for s in srcs:
        o = os.path.join(HERE, "build", os.path.basename(s) + ".o")
        objs.append(o)
        if not force and os.path.exists(o) and os.path.getmtime(o) > max(
                os.path.getmtime(s), *(os.path.getmtime(os.path.join(CSRC, h)) for h in os.listdir(CSRC) if h.endswith((".h", ".inc"))),
                os.path.getmtime(os.path.join(HERE, "..", "include", "fishbird.h"))):
            continue
        flags = FLAGS
        if os.path.basename(s) in FMA_OK:
            # fast-honor-pragmas, not fast: "fast" lets the backend fuse everything and ignores the
            # `#pragma clang fp contract(off)` that keeps the inlier / outlier decision of k_pose_opt unfused
            flags = [("-ffp-contract=fast-honor-pragmas" if f == "-ffp-contract=off" else f) for f in FLAGS]
        # FB_BUILD_DEFS="-DFB_POSE_STAMPS ...": diagnostic variants for the probes under profiles/probes/ (never the product build)
        cmd = [hipcc()] + flags + os.environ.get("FB_BUILD_DEFS", "").split() + ["-c", s, "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((s, subprocess.Popen(cmd)))
    for s, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed on " + s)
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
