"""Generates tests/golden/kfdb_score_ref.npz from the REFERENCE's own L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp)
and BowVector (BowVector.cpp), compiled where they lie into a temporary directory behind the few lines of C shim below.
ScoringObject.cpp includes the vocabulary header, which needs OpenCV: predefining that header's include guard leaves it empty,
and ScoringObject.h + <cmath> are force-included in its place.  The fixture is data: for a dozen vector pairs the input
(word id, weight) streams, the BowVectors the reference's addWeight + normalize(L1) made of them, and the double its score
returned in both argument orders.

    python tests/golden/make_kfdb_ref_golden.py [reference root]
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "kfdb_score_ref.npz")
DEFAULT_REF = os.environ.get("FB_REFERENCE_ROOT", "/root/reference")

SHIM = r"""
#include <cmath>
#include "BowVector.h"
#include "ScoringObject.h"
static DBoW2::BowVector make(int n, const unsigned *word, const double *w) {
  DBoW2::BowVector v;
  for (int i = 0; i < n; i++) v.addWeight(word[i], w[i]);
  if (!v.empty()) v.normalize(DBoW2::L1);
  return v;
}
extern "C" int shim_bow(int n, const unsigned *word, const double *w, unsigned *ids, double *vals) {
  DBoW2::BowVector v = make(n, word, w);
  int k = 0;
  for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it, ++k) { ids[k] = it->first; vals[k] = it->second; }
  return k;
}
extern "C" double shim_score(int na, const unsigned *aw, const double *av, int nb, const unsigned *bw, const double *bv) {
  DBoW2::L1Scoring s;
  return s.score(make(na, aw, av), make(nb, bw, bv));
}
"""


def dbow2_dir(ref_root=DEFAULT_REF):
    return os.path.join(ref_root, "Thirdparty", "DBoW2", "DBoW2")


def build(ref_root=DEFAULT_REF):
    """-> ctypes library of the reference's score behind the shim (built in a temporary directory)"""
    d, src = tempfile.mkdtemp(), dbow2_dir(ref_root)
    open(os.path.join(d, "shim.cpp"), "w").write(SHIM)
    cxx = ["g++", "-std=c++11", "-O2", "-fPIC", "-I" + src]
    subprocess.check_call(cxx + ["-D__D_T_TEMPLATED_VOCABULARY__", "-include", "cmath", "-include", "ScoringObject.h", "-c",
                                 os.path.join(src, "ScoringObject.cpp"), "-o", os.path.join(d, "score.o")])
    subprocess.check_call(cxx + ["-c", os.path.join(src, "BowVector.cpp"), "-o", os.path.join(d, "bow.o")])
    subprocess.check_call(cxx + ["-c", os.path.join(d, "shim.cpp"), "-o", os.path.join(d, "shim.o")])
    so = os.path.join(d, "libkfdb_score_ref.so")
    subprocess.check_call(["g++", "-shared", "-o", so] + [os.path.join(d, x) for x in ("shim.o", "score.o", "bow.o")])
    lib = C.CDLL(so)
    lib.shim_score.restype = C.c_double
    return lib


def pairs():
    """The dozen (word, weight) stream pairs (streams may repeat a word: addWeight accumulates)."""
    g = np.random.Generator(np.random.PCG64(4242))

    def stream(n, vocab, lo=0):
        return (g.integers(0, vocab, n).astype(np.uint64) + lo).astype(np.uint32), g.uniform(0.01, 9.0, n)
    out = []
    for n, vocab in ((1, 1), (40, 60), (1500, 4000)):  # sizes 1 / 40 / 1500, overlapping
        out.append(stream(n, vocab) + stream(n, vocab))
    a = stream(300, 1000)
    out.append(a + ((a[0] + np.uint32(5000)), a[1]))                     # disjoint
    out.append(a + a)                                                    # identical
    out.append((np.zeros(0, np.uint32), np.zeros(0)) + stream(40, 60))   # one empty
    out.append(stream(40, 60) + (np.zeros(0, np.uint32), np.zeros(0)))
    b = stream(400, 2000)
    keep = np.isin(b[0], np.unique(b[0])[::3])
    out.append((b[0][keep], b[1][keep]) + b)                             # a strict subset (same weights, other norm)
    out.append(b + (b[0][keep], b[1][keep]))
    out.append(stream(200, 300, lo=2 ** 32 - 300) + stream(200, 300, lo=2 ** 32 - 300))  # ids near 2^32
    out.append(stream(1500, 100000) + stream(1500, 100000))              # sparse overlap
    out.append(stream(40, 45) + stream(1500, 2000))                      # very different sizes
    return out


def generate(ref_root=DEFAULT_REF):
    lib = build(ref_root)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    rec = {"n_pairs": np.int32(0)}
    for i, (aw, av, bw, bv) in enumerate(pairs()):
        aw, bw = np.ascontiguousarray(aw, np.uint32), np.ascontiguousarray(bw, np.uint32)
        av, bv = np.ascontiguousarray(av, np.float64), np.ascontiguousarray(bv, np.float64)
        for tag, w, v in (("a", aw, av), ("b", bw, bv)):
            ids, vals = np.zeros(max(len(w), 1), np.uint32), np.zeros(max(len(w), 1), np.float64)
            k = lib.shim_bow(len(w), vp(w), vp(v), vp(ids), vp(vals))
            rec.update({"p%d_%s_word" % (i, tag): w, "p%d_%s_w" % (i, tag): v, "p%d_%s_ids" % (i, tag): ids[:k].copy(),
                        "p%d_%s_vals" % (i, tag): vals[:k].copy()})
        rec["p%d_score" % i] = np.float64(lib.shim_score(len(aw), vp(aw), vp(av), len(bw), vp(bw), vp(bv)))
        rec["p%d_score_ba" % i] = np.float64(lib.shim_score(len(bw), vp(bw), vp(bv), len(aw), vp(aw), vp(av)))
        rec["n_pairs"] = np.int32(i + 1)
    return rec


if __name__ == "__main__":
    r = generate(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_REF)
    np.savez_compressed(OUT, **r)
    print("wrote %s (%d pairs)" % (OUT, int(r["n_pairs"])))
    for i in range(int(r["n_pairs"])):
        print(i, len(r["p%d_a_ids" % i]), len(r["p%d_b_ids" % i]), repr(float(r["p%d_score" % i])), repr(float(r["p%d_score_ba" % i])))
