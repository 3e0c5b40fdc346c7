"""Synthetic problems + C-ABI argument builder for Optimizer::OptimizeSim3 (fb_optimize_sim3*).

The scene is sim3_problem.make_problem's (one KF1, C candidates whose maps are similarity-transformed copies), without its
3-D noise.  OptimizeSim3 reads key points, so here the key points of every kept pair ARE the projections of the two map
points into their own key frames plus Gaussian pixel noise; a wrong match keeps the random key point of the slot it points
at (a gross outlier, hundreds of pixels).  The input Sim3 is the true one, perturbed like a RANSAC hypothesis and rounded
to float.  Planted skips, each on a pair that would otherwise be kept: NULL / bad pMP1, bad pMP2, GetIndexInKeyFrame < 0,
an index or a match beyond the stride, an octave outside the level table."""
import numpy as np

from . import cabi, sim3_problem as SP, synth
from .cabi import fill

PLANTS = ("null1", "bad2", "noindex2", "bigindex2", "octave1", "octave2", "bigmatch")

# The parity set of the tests: (seed, kept per candidate, keywords).  Kept counts 0, 1, 9, 10, 11; 63, 64, 65 around the
# wave; 257 above the workgroup; == the stride; an empty candidate in the middle; strides that are no multiple of 64; every
# skip clause; nBad == 0 and > 0; the < 10 gate after round-1 nulls (11 kept, 3 wrong); fix_scale 0 and 1.
PARITY = [
    (11, [150], dict(n1=333, n2=301, n_outliers=[12], plants=PLANTS)),
    (12, [64, 0, 65], dict(n1=333, n2=301, n_outliers=[5, 0, 0])),
    (13, [1, 9, 10], dict(n1=150, n2=170)),
    (14, [11, 63, 11], dict(n1=150, n2=170, n_outliers=[0, 0, 3])),
    (15, [257], dict(n1=500, n2=450, n_outliers=[20])),
    (16, [97], dict(n1=97, n2=97)),
    (17, [150, 40], dict(n1=333, n2=301, n_outliers=[10, 0], fix_scale=1)),
    (18, [120], dict(n1=333, n2=301, pixel_noise=0.0)),
]
# a decision closer to th2 than this (relative) is a razor pair; derived in tests/test_opt_sim3_gpu.py from the measured
# device-to-model difference.  At most RAZOR_SHARE_CAP of the parity candidates may hold one.
RAZOR_GAP = 1e-3
RAZOR_SHARE_CAP = 0.02


def _project(T12, xw, fx, fy, cx, cy):
    T = np.asarray(T12, np.float64).reshape(3, 4)
    pc = xw.astype(np.float64) @ T[:, :3].T + T[:, 3]
    return np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], 1)


def make_problem(seed, n_corr, n1=400, n2=400, pixel_noise=0.7, n_outliers=None, outlier_px=None, fix_scale=0, plants=(),
                 init=(0.01, 0.05, 0.02), th2=10.0, scale=1.08):
    """n_corr: kept correspondences per candidate (exact).  n_outliers: wrong matches per candidate among them.  outlier_px:
    instead of a wrong match, displace obs1 of that many pairs by this many pixels (a planted outlier of known size).
    plants: names from PLANTS, one skipped pair each per candidate.  init: (rotation sigma, translation sigma, relative scale
    error) of the input Sim3 around the truth."""
    C = len(n_corr)
    n_outliers = [0] * C if n_outliers is None else list(n_outliers)
    p = SP.make_problem(seed, n_corr, n1=n1, n2=n2, pixel_noise=0.0, fix_scale=fix_scale, scale=1.0 if fix_scale else scale,
                        plants=False, n_outliers=[0] * C if outlier_px else n_outliers)
    g = synth.rng(seed + 77)
    fx, fy, cx, cy = p["fx"], p["fy"], p["cx"], p["cy"]
    kps1 = p["kps1"]
    uv1 = _project(p["T1"], p["xw1"], fx, fy, cx, cy) + g.normal(0, pixel_noise, (n1, 2))
    kps1["x"], kps1["y"] = uv1[:, 0].astype(np.float32), uv1[:, 1].astype(np.float32)
    planted = []
    # KF1 features no candidate matches: the planted pairs take theirs from here (KF1's flags and key points are shared)
    free_all = np.nonzero(np.all(np.stack([cd["matches12"] for cd in p["cands"]]) < 0, axis=0))[0]
    for c, cd in enumerate(p["cands"]):
        tr = p["truth"][c]
        good = ~tr["outlier"]
        j = tr["j2"][good]
        uv2 = _project(cd["T2"], cd["xw2"][j], fx, fy, cx, cy) + g.normal(0, pixel_noise, (len(j), 2))
        cd["kps2"]["x"][j], cd["kps2"]["y"][j] = uv2[:, 0].astype(np.float32), uv2[:, 1].astype(np.float32)
        tr["shifted"] = np.zeros(0, np.int64)
        if outlier_px:
            k = np.arange(int(n_outliers[c]))
            ang = g.uniform(0, 2 * np.pi, len(k))
            i1 = tr["i1"][k]
            cd["kps1_shift"] = (i1, np.stack([np.cos(ang), np.sin(ang)], 1) * outlier_px)
            tr["shifted"] = i1
        # planted skips on pairs of their own: free KF1 features matched to free KF2 slots, true geometry, valid flags
        m12 = cd["matches12"]
        used2 = set(m12[m12 >= 0].tolist())
        free2 = np.array([x for x in range(n2) if x not in used2], np.int64)
        pl = {}
        for q, name in enumerate(plants):
            i1, j2 = int(free_all[-1 - q - len(plants) * c]), int(free2[-1 - q])
            m12[i1] = j2
            pl[name] = (i1, j2)
            if name == "null1":
                p["valid1"][i1] = 0
            elif name == "bad2":
                cd["valid2"][j2] = 0
            elif name == "noindex2":
                cd["index2"][j2] = -1
            elif name == "bigindex2":
                cd["index2"][j2] = n2 + 7
            elif name == "octave1":
                kps1["octave"][i1] = cabi.FB_MAX_LEVELS
            elif name == "octave2":
                cd["kps2"]["octave"][j2] = -1
            elif name == "bigmatch":
                m12[i1] = n2 + 3
        planted.append(pl)
        # the input Sim3: the truth perturbed, as floats
        dT = synth.perturb_pose(g, np.eye(4), rot_sigma=init[0], t_sigma=init[1])
        cd["R12"] = (dT[:3, :3] @ tr["R"]).astype(np.float32).reshape(9)
        cd["t12"] = (tr["t"] + dT[:3, 3]).astype(np.float32)
        cd["s12"] = np.float32(1.0 if fix_scale else tr["s"] * (1.0 + init[2] * g.normal()))
    if outlier_px:  # (KF1's key points are shared: only meaningful with one candidate or disjoint pairs)
        for cd in p["cands"]:
            i1, d = cd.pop("kps1_shift")
            kps1["x"][i1] += d[:, 0].astype(np.float32)
            kps1["y"][i1] += d[:, 1].astype(np.float32)
    p["planted"] = planted
    p["th2"] = float(th2)
    p["inv_level_sigma2"] = np.asarray(synth.scale_tables()[3], np.float32)
    return p


def optimize_args(p, with_index=True, hyp_stride=1):
    """-> (cabi.OptimizeSim3Args on host arrays, outputs dict (matches12 is in/out), keepalive dict)"""
    C, n1, n2 = p["C"], p["n1"], p["n2"]
    cs = p["cands"]
    hs = max(1, hyp_stride)

    def strided(key, w):
        a = np.zeros(((C - 1) * hs + 1, w), np.float32)
        for c in range(C):
            a[c * hs] = np.asarray(cs[c][key], np.float32).reshape(w)
        return a
    keep = dict(n_kf1=np.array([n1], np.int32), kps1=np.ascontiguousarray(p["kps1"]),
                kps2=np.ascontiguousarray(np.stack([c["kps2"] for c in cs])),
                valid1=np.ascontiguousarray(p["valid1"]), xw1=np.ascontiguousarray(p["xw1"]),
                valid2=np.ascontiguousarray(np.stack([c["valid2"] for c in cs])),
                xw2=np.ascontiguousarray(np.stack([c["xw2"] for c in cs])),
                T1w=np.ascontiguousarray(p["T1"], np.float32), T2w=np.ascontiguousarray(np.stack([c["T2"] for c in cs]), np.float32),
                kf2_index=np.ascontiguousarray(np.stack([c["index2"] for c in cs])),
                s12=strided("s12", 1), R12=strided("R12", 9), t12=strided("t12", 3))
    out = dict(matches12=np.ascontiguousarray(np.stack([c["matches12"] for c in cs])).copy(),
               n_inliers=np.full(C, -7, np.int32), n_correspondences=np.full(C, -7, np.int32), n_bad=np.full(C, -7, np.int32),
               q=np.full((C, 4), -7.0), t=np.full((C, 3), -7.0), s=np.full(C, -7.0),
               scw_q=np.full((C, 4), -7.0), scw_t=np.full((C, 3), -7.0), scw_s=np.full(C, -7.0), Scw=np.full((C, 12), -7.0, np.float32))
    a = cabi.OptimizeSim3Args()
    fill(a, n_cand=C, T1w=keep["T1w"], T2w=keep["T2w"], s12=keep["s12"], R12=keep["R12"], t12=keep["t12"], hyp_stride=hyp_stride,
         inv_level_sigma2=[float(x) for x in p["inv_level_sigma2"]], th2=p["th2"], fix_scale=p["fix_scale"], **out)
    if with_index:
        fill(a, kf2_index=keep["kf2_index"])
    fill(a.kf1, kf_stride=n1, n_kf=keep["n_kf1"], kf_kps=keep["kps1"])
    fill(a.kf2, kf_stride=n2, kf_kps=keep["kps2"])
    for k in (a.kf1, a.kf2):
        fill(k.cam, fx=p["fx"], fy=p["fy"], cx=p["cx"], cy=p["cy"], min_x=0.0, min_y=0.0, max_x=float(SP.W), max_y=float(SP.H))
    fill(a.mp1, mp_stride=n1, mp_valid=keep["valid1"], mp_xw=keep["xw1"])
    fill(a.mp2, mp_stride=n2, mp_valid=keep["valid2"], mp_xw=keep["xw2"])
    return a, out, keep


INPUT_FIELDS = [("kf1", "n_kf", "n_kf1"), ("kf1", "kf_kps", "kps1"), ("kf2", "kf_kps", "kps2"), ("mp1", "mp_valid", "valid1"),
                ("mp1", "mp_xw", "xw1"), ("mp2", "mp_valid", "valid2"), ("mp2", "mp_xw", "xw2"), (None, "T1w", "T1w"), (None, "T2w", "T2w"),
                (None, "kf2_index", "kf2_index"), (None, "s12", "s12"), (None, "R12", "R12"), (None, "t12", "t12")]
OUTPUT_FIELDS = ["matches12", "n_inliers", "n_correspondences", "n_bad", "q", "t", "s", "scw_q", "scw_t", "scw_s", "Scw"]


def optimize_dev(a, stream):
    """fb_optimize_sim3_dev on an OptimizeSim3Args of device pointers (raises on a non-zero return code)"""
    import ctypes as C
    from . import check, lib
    check(lib().fb_optimize_sim3_dev(C.byref(a), C.c_void_p(stream)), "fb_optimize_sim3_dev")


def optimize(a):
    """fb_optimize_sim3 on an OptimizeSim3Args of host pointers"""
    import ctypes as C
    from . import check, lib
    check(lib().fb_optimize_sim3(C.byref(a)), "fb_optimize_sim3")
