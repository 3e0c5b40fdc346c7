"""CPU restatement of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:231-476, monocular) -- TEST INFRASTRUCTURE.

The literal serial loop of the reference: for each neighbour in order the baseline gate, F12, SearchForTriangulation (the
oracle's orc_match_triangulation, run with the CURRENT has_mp1 / has_mp2), then every match in ascending idx1 is triangulated
and checked, and a new point immediately marks both slots.  The arithmetic of one neighbour / one match is in
tests/cpp/new_points_ref.cpp (g++ -ffp-contract=off).  Independent of the device's per-feature claim formulation."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from fishbirdeyevisualslam_amd import bow_problem as BP, cabi
from fishbirdeyevisualslam_amd.cabi import fill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
REASONS = {0: "ok", 1: "parallax", 2: "w0", 3: "behind", 4: "chi2", 5: "dist0", 6: "scale"}


def lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp()
        so = os.path.join(d, "libnew_points_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                               os.path.join(ROOT, "tests", "cpp", "new_points_ref.cpp"), "-o", so])
        _LIB = C.CDLL(so)
    return _LIB


def _p(a):
    return C.c_void_p(a.ctypes.data)


def null_vector(A):
    A = np.ascontiguousarray(A, np.float32).reshape(16)
    v = np.zeros(4, np.float64)
    lib().npr_null_vector(_p(A), _p(v))
    return v


def neighbour(T1, T2, mp_xw, fx, fy, cx, cy):
    F = np.zeros(9, np.float32)
    O1 = np.zeros(3, np.float32)
    O2 = np.zeros(3, np.float32)
    med = np.zeros(1, np.float32)
    xw = np.ascontiguousarray(mp_xw, np.float32)
    gated = lib().npr_neighbour(_p(T1), _p(T2), _p(xw), len(xw), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
                                _p(F), _p(O1), _p(O2), _p(med))
    return bool(gated), F, O1, O2, float(med[0])


def triangulate(kp1, kp2, T1, T2, O1, O2, prob):
    k1 = np.array([kp1], cabi.KP_DTYPE)
    k2 = np.array([kp2], cabi.KP_DTYPE)
    X = np.zeros(3, np.float32)
    sf = np.ascontiguousarray(prob["scale_factors"], np.float32)
    s2 = np.ascontiguousarray(prob["level_sigma2"], np.float32)
    r = lib().npr_triangulate(_p(k1), _p(k2), _p(T1), _p(T2), _p(O1), _p(O2), C.c_float(prob["fx"]), C.c_float(prob["fy"]),
                              C.c_float(prob["cx"]), C.c_float(prob["cy"]), _p(sf), _p(s2), C.c_float(prob["scale_factor"]), _p(X))
    return r, X


def _m7(prob, nb, has1, has2, F, O1):
    """orc_match_triangulation for KF1 vs neighbour nb with the current has_mp arrays."""
    from oracle import pyoracle as O
    n1, n2 = len(prob["kps1"]), len(nb["kps"])
    fv1, k1 = BP._fv_struct([BP.feature_vector(prob["desc1"])], 100, max(n1, 1))
    fv2, k2 = BP._fv_struct([BP.feature_vector(nb["desc"])], 100, max(n2, 1))
    T2 = np.asarray(nb["T"])
    keep = dict(n1=np.array([n1], np.int32), kps1=np.ascontiguousarray(prob["kps1"]), desc1=np.ascontiguousarray(prob["desc1"]),
                has_mp1=np.ascontiguousarray(has1), n2=np.array([n2], np.int32), kps2=np.ascontiguousarray(nb["kps"]),
                desc2=np.ascontiguousarray(nb["desc"]), has_mp2=np.ascontiguousarray(has2),
                F12=np.ascontiguousarray(F, np.float32), Cw1=np.ascontiguousarray(O1, np.float32),
                R2w=np.ascontiguousarray(T2[:3, :3], np.float32).reshape(9), t2w=np.ascontiguousarray(T2[:3, 3], np.float32))
    out = dict(matches12=np.full((1, max(n1, 1)), -7, np.int32), nmatches=np.zeros(1, np.int32))
    a = cabi.TriangulationArgs()
    fill(a, batch=1, kf1_stride=max(n1, 1), kf2_stride=max(n2, 1), fx=prob["fx"], fy=prob["fy"], cx=prob["cx"], cy=prob["cy"],
         scale_factors=[float(x) for x in prob["scale_factors"]], level_sigma2=[float(x) for x in prob["level_sigma2"]], **keep, **out)
    a.fv1, a.fv2 = fv1, fv2
    fill(a.matcher, nnratio=0.6, check_orientation=0)
    O.call("orc_match_triangulation", a)
    return out["matches12"][0, :n1].copy(), int(out["nmatches"][0])


def create_new_map_points(prob, n_nb=None, has_mp1=None):
    """-> dict with the same fields as fb_create_new_map_points' outputs (rows cut to n_new) + `reasons`:
    {(nb, idx1): reason} for every match that was tried."""
    nbs = prob["nbs"][: (len(prob["nbs"]) if n_nb is None else n_nb)]
    B = len(nbs)
    n1 = len(prob["kps1"])
    T1 = np.ascontiguousarray(prob["Tcw1"], np.float32)
    has1 = (prob["has_mp1"] if has_mp1 is None else has_mp1).copy()
    has2 = [x["has_mp"].copy() for x in nbs]
    kf1_new = np.full(n1, -1, np.int32)
    kf2_new = [np.full(len(x["kps"]), -1, np.int32) for x in nbs]
    rows = dict(xw=[], normal=[], max_dist=[], min_dist=[], desc=[], idx1=[], nb=[], idx2=[])
    nb_matches = np.zeros(B, np.int32)
    nb_new = np.zeros(B, np.int32)
    nb_skipped = np.zeros(B, np.int32)
    reasons = {}
    sf = prob["scale_factors"]
    for b, nb in enumerate(nbs):
        T2 = np.ascontiguousarray(synth_to12(nb["T"]))
        gated, F, O1, O2, _ = neighbour(T1, T2, nb["mp_xw"], prob["fx"], prob["fy"], prob["cx"], prob["cy"])
        if gated:
            nb_skipped[b] = 1
            continue
        m12, nm = _m7(prob, nb, has1, has2[b], F, O1)
        nb_matches[b] = nm
        for i1 in np.nonzero(m12 >= 0)[0]:
            i2 = int(m12[i1])
            r, X = triangulate(prob["kps1"][i1], nb["kps"][i2], T1, T2, O1, O2, prob)
            reasons[(b, int(i1))] = REASONS[r]
            if r != 0:
                continue
            row = len(rows["idx1"])
            nrm = np.zeros(3, np.float32)
            mx = np.zeros(1, np.float32)
            mn = np.zeros(1, np.float32)
            lib().npr_normal_depth(_p(X), _p(O1), _p(O2), C.c_float(sf[prob["kps1"]["octave"][i1]]), C.c_float(sf[prob["n_levels"] - 1]),
                                   _p(nrm), _p(mx), _p(mn))
            rows["xw"].append(X)
            rows["normal"].append(nrm)
            rows["max_dist"].append(mx[0])
            rows["min_dist"].append(mn[0])
            rows["desc"].append(nb["desc"][i2] if nb["before"] else prob["desc1"][i1])
            rows["idx1"].append(int(i1))
            rows["nb"].append(b)
            rows["idx2"].append(i2)
            has1[i1] = 1
            has2[b][i2] = 1
            kf1_new[i1] = row
            kf2_new[b][i2] = row
            nb_new[b] += 1
    n = len(rows["idx1"])
    out = dict(n_new=n, xw=np.array(rows["xw"], np.float32).reshape(n, 3), normal=np.array(rows["normal"], np.float32).reshape(n, 3),
               max_dist=np.array(rows["max_dist"], np.float32), min_dist=np.array(rows["min_dist"], np.float32),
               desc=np.array(rows["desc"], np.uint8).reshape(n, 32), idx1=np.array(rows["idx1"], np.int32),
               nb=np.array(rows["nb"], np.int32), idx2=np.array(rows["idx2"], np.int32), has_mp1=has1, has_mp2=has2,
               kf1_new=kf1_new, kf2_new=kf2_new, nb_matches=nb_matches, nb_new=nb_new, nb_skipped=nb_skipped, reasons=reasons)
    return out


def synth_to12(T):
    return np.ascontiguousarray(np.asarray(T)[:3, :4].astype(np.float32).reshape(12))
