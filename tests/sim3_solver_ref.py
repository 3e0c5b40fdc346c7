"""CPU restatement of the reference's Sim3Solver (src/Sim3Solver.cc) -- TEST INFRASTRUCTURE.

The literal serial class lives in tests/cpp/sim3_solver_ref.cpp (g++ -O2 -ffp-contract=off, no dependencies): constructor loop,
SetRansacParameters, iterate() with persistent state, ComputeSim3 through atan2 / Rodrigues with libm, CheckInliers.  This
module builds it, wraps one solver per candidate and turns its per-iteration log into the table the device call fills."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from fishbirdeyevisualslam_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
MAXH = cabi.FB_SIM3_MAX_HYP
RAZOR_ERR, RAZOR_GAP = 1e-4, 1e-3  # the razor condition: |err - thr| / thr and (l0 - l1) / l0


def lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp()
        so = os.path.join(d, "libsim3_solver_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                               os.path.join(ROOT, "tests", "cpp", "sim3_solver_ref.cpp"), "-o", so])
        _LIB = C.CDLL(so)
        _LIB.s3r_create.restype = C.c_void_p
    return _LIB


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def eigen4(N):
    N = np.ascontiguousarray(N, np.float32).reshape(16)
    ev = np.zeros(4, np.float32)
    evec = np.zeros((4, 4), np.float32)
    lib().s3r_eigen4(_p(N), _p(ev), _p(evec))
    return ev, evec


def compute_sim3(P1, P2, fix_scale=0):
    """P1, P2: 3x3, samples as columns -> s, R[3][3], t"""
    a = np.ascontiguousarray(P1, np.float32)
    b = np.ascontiguousarray(P2, np.float32)
    o = np.zeros(13, np.float32)
    lib().s3r_compute_sim3(_p(a), _p(b), int(fix_scale), _p(o))
    return o[0], o[1:10].reshape(3, 3).copy(), o[10:].copy()


class Solver:
    """Sim3Solver for candidate c of a sim3_problem problem, with the reference's method names."""

    def __init__(self, p, c, with_index=True):
        cd = p["cands"][c]
        self.n1 = p["n1"]
        self._keep = [np.ascontiguousarray(cd["matches12"], np.int32), np.ascontiguousarray(p["valid1"]), np.ascontiguousarray(cd["valid2"]),
                      np.ascontiguousarray(p["index1"], np.int32) if with_index else None,
                      np.ascontiguousarray(cd["index2"], np.int32) if with_index else None,
                      np.ascontiguousarray(p["kps1"]["octave"], np.int32), np.ascontiguousarray(cd["kps2"]["octave"], np.int32),
                      np.ascontiguousarray(p["xw1"], np.float32), np.ascontiguousarray(cd["xw2"], np.float32),
                      np.ascontiguousarray(p["T1"], np.float32), np.ascontiguousarray(cd["T2"], np.float32),
                      np.ascontiguousarray(p["level_sigma2"], np.float32),
                      np.array([p["fx"], p["fy"], p["cx"], p["cy"]], np.float32), np.array([p["fx"], p["fy"], p["cx"], p["cy"]], np.float32)]
        self.h = C.c_void_p(lib().s3r_create(self.n1, *[_p(x) for x in self._keep], int(p["fix_scale"])))
        self.N = lib().s3r_N(self.h)
        self.rand = np.ascontiguousarray(p["rand_idx"][c], np.int32)
        self.max_its = None

    def __del__(self):
        if getattr(self, "h", None):
            lib().s3r_destroy(self.h)
            self.h = None

    def correspondences(self):
        idx = np.zeros(self.N, np.int32)
        corr = np.zeros(self.N, cabi.SIM3_CORR_DTYPE)
        lib().s3r_correspondences(self.h, _p(idx), _p(corr))
        return idx, corr

    def SetRansacParameters(self, probability=0.99, minInliers=20, maxIterations=300):
        self.min_inliers = minInliers
        self.max_its = lib().s3r_set_ransac(self.h, C.c_double(probability), minInliers, maxIterations)
        return self.max_its

    def iterations(self):
        return lib().s3r_iterations(self.h)

    def iterate(self, n, accept_above=None):
        """-> (returned, bNoMore, vbInliers[n1], nInliers, (s, R, t) or None)"""
        nm = C.c_int32(0)
        ni = C.c_int32(0)
        vb = np.zeros(self.n1, np.uint8)
        srt = np.zeros(13, np.float32)
        r = lib().s3r_iterate(self.h, n, _p(self.rand), self.min_inliers if accept_above is None else accept_above, C.byref(nm), _p(vb),
                              C.byref(ni), _p(srt))
        return bool(r), bool(nm.value), vb, ni.value, ((srt[0], srt[1:10].copy(), srt[10:].copy()) if r else None)

    def log(self, mask_words):
        n = lib().s3r_log_size(self.h)
        o = dict(s=np.zeros(n, np.float32), R=np.zeros((n, 9), np.float32), t=np.zeros((n, 3), np.float32), n_inliers=np.zeros(n, np.int32),
                 is_best=np.zeros(n, np.uint8), accept=np.zeros(n, np.uint8), razor=np.zeros(n, np.float64), gap=np.zeros(n, np.float64), n_razor=np.zeros(n, np.int32),
                 inlier_mask=np.zeros((n, mask_words), np.uint32), band_mask=np.zeros((n, mask_words), np.uint32))
        lib().s3r_log(self.h, _p(o["s"]), _p(o["R"]), _p(o["t"]), _p(o["n_inliers"]), _p(o["is_best"]), _p(o["accept"]), _p(o["razor"]),
                      _p(o["gap"]), _p(o["n_razor"]), _p(o["inlier_mask"]), _p(o["band_mask"]), mask_words)
        return o


def full_table(p, accept_above=None, with_index=True):
    """Every iteration of every candidate: iterate(1) until bNoMore, going on after each return as LoopClosing does after a
    failed OptimizeSim3.  -> list of dicts per candidate with the fields of the device outputs + razor / gap per row."""
    mw = (p["n1"] + 31) // 32
    out = []
    for c in range(p["C"]):
        S = Solver(p, c, with_index)
        mi = S.SetRansacParameters(p["ransac_prob"], p["min_inliers"], p["max_iterations"])
        above = None if accept_above is None else int(accept_above[c])
        first = -1
        while True:
            ret, nm, _, _, _ = S.iterate(1, above)
            if ret and first < 0:
                first = S.iterations() - 1
            if nm:
                break
        idx, corr = S.correspondences()
        lg = S.log(mw)
        done = len(lg["s"])
        assert done == (0 if S.N < p["min_inliers"] else mi)
        lg.update(N=S.N, indices1=idx, corr=corr, max_its=(mi if S.N >= p["min_inliers"] else 0), n_hyp_done=done, first_accept=first,
                  no_more=int(first < 0), razor_row=(lg["razor"] < RAZOR_ERR) | (lg["gap"] < RAZOR_GAP))
        out.append(lg)
    return out


def accept_rule(n_inliers, above):
    """The accept scan in Python: is_best[k] = n_k >= max_{j<k} n_j (mnBestInliers starts at 0), accept = is_best & n_k > above."""
    best = 0
    acc = np.zeros(len(n_inliers), np.uint8)
    for k, n in enumerate(n_inliers):
        if n >= best:
            best = n
            acc[k] = n > above
    return acc


def razor_shares(p, table):
    """-> (share of (hypothesis, correspondence) decisions excluded, share of hypotheses excluded) of one problem"""
    dec = sum(t["n_hyp_done"] * t["N"] for t in table)
    exc = sum(int(t["n_razor"].sum()) for t in table)
    hyp = sum(t["n_hyp_done"] for t in table)
    return (exc / dec if dec else 0.0), (sum(int(t["razor_row"].sum()) for t in table) / hyp if hyp else 0.0)


# the problems of tests/test_sim3_solver_gpu.py (the CPU suite asserts the razor caps on the same list):
# (seed, kept correspondences per candidate, make_problem arguments)
PARITY_PROBLEMS = [
    (201, [300], dict(n1=600, n2=640, outlier_share=0.0, pixel_noise=0.1)),
    (202, [800, 12, 20, 1500], dict(n1=2000, n2=2000, outlier_share=0.3, pixel_noise=0.1)),
    (203, [60, 45, 90, 33, 64, 21, 120, 75, 50, 28, 66, 40], dict(n1=1000, n2=900, outlier_share=0.6, pixel_noise=0.3)),
    (204, [1500], dict(n1=2000, n2=1800, outlier_share=0.2, pixel_noise=0.2, fix_scale=1, scale=1.0)),
    (205, [400, 35, 100, 250], dict(n1=1200, n2=1200, outlier_share=0.45, pixel_noise=0.2, fix_scale=1, scale=1.0)),
    (206, [700, 19, 333, 20, 64, 65, 128, 500, 31, 257, 1000, 23], dict(n1=1500, n2=1300, outlier_share=0.1, pixel_noise=0.15)),
]
RAZOR_DECISION_CAP, RAZOR_HYPOTHESIS_CAP = 1e-3, 2e-2

# kept counts at the workgroup size of k_sim3_prepare (256 threads) and its neighbours: the seams of the compaction
SEAM_PROBLEM = (220, [255, 256, 257], dict(n1=700, n2=640, outlier_share=0.3, pixel_noise=0.2))
# the last KF1 stride whose correspondences k_sim3_hypotheses stages in LDS and the first it reads from the workspace
LDS_BOUNDARY_STRIDES = (3402, 3403)
UNSAFE_CLAUSES = ("match = s2", "index1 = s1", "index2 = s2", "octave1 = -1", "octave1 = FB_MAX_LEVELS", "octave2 = -1",
                  "octave2 = FB_MAX_LEVELS")


def skip_clause_problem(seed=221, n_corr=90, n1=300, n2=280):
    """One candidate in which every skip clause of the walk occurs.  make_problem plants the reference's own (no match, NULL /
    bad pMP1, bad pMP2, GetIndexInKeyFrame = -1 on either side); here seven otherwise kept pairs get the values that the
    project skips for memory safety (UNSAFE_CLAUSES), one each.  The reference, and so the restatement, would index out of
    bounds with them, so the restatement gets the same problem with those seven matches removed: skipping them is the
    specification.  -> (problem for the device, problem for the restatement, N both must find)"""
    import copy
    from fishbirdeyevisualslam_amd import sim3_problem as SP
    p = SP.make_problem(seed, [n_corr], n1=n1, n2=n2, pixel_noise=0.2, n_outliers=[0])
    cd, tr = p["cands"][0], p["truth"][0]
    i1 = [int(v) for v in tr["i1"][:len(UNSAFE_CLAUSES)]]
    j = [int(cd["matches12"][i]) for i in i1]
    assert len(set(j)) == len(j) and all(p["index1"][i] == i for i in i1) and all(cd["index2"][v] == v for v in j)
    cd["matches12"][i1[0]] = n2
    p["index1"][i1[1]] = n1
    cd["index2"][j[2]] = n2
    p["kps1"]["octave"][i1[3]] = -1
    p["kps1"]["octave"][i1[4]] = cabi.FB_MAX_LEVELS
    cd["kps2"]["octave"][j[5]] = -1
    cd["kps2"]["octave"][j[6]] = cabi.FB_MAX_LEVELS
    N = n_corr - len(UNSAFE_CLAUSES)
    p["rand_idx"] = SP.random_int_table(np.random.default_rng(seed + 1), N)[None]
    ref = copy.deepcopy(p)
    ref["cands"][0]["matches12"][i1] = -1
    return p, ref, N
