"""Pose-optimisation frames that synth.make_pose_problem never produces: each case starts from its output and edits the
arrays, so that a branch of Optimizer::PoseOptimization / PoseOptimizationWithBird / BirdOptimization is taken that the
generator leaves alone.  tests/test_pose_cases.py proves every case on the CPU (oracle against tests/pose_ref.py, and from
the oracle's trace that the branch was taken) before tests/test_pose_gpu.py sends it through the kernels.

A case is dict(id, doc = the Optimizer.cc line it pins, prob, kw = the keyword arguments of problems.pose_args, expect =
names of checks in EXPECT).  Every input is finite and every front point has |z_cam| >= 0.1 at the start pose.
"""
import ctypes as C
import math
import re

import numpy as np

from fishbirdeyevisualslam_amd import cabi, synth

FRONT, FRONT_BIRD, BIRD = cabi.FB_POSE_FRONT, cabi.FB_POSE_FRONT_BIRD, cabi.FB_POSE_BIRD
MODE_NAME = {FRONT: "front", FRONT_BIRD: "front_bird", BIRD: "bird"}
CHI2_BIRD = 5.991
PREFILL = 9                # value of mask slots that hold no edge; must come back untouched


# ---- edits over a problem dict ------------------------------------------------------------------------------------------
def _base(seed, n_front, n_bird, **kw):
    p = synth.make_pose_problem(seed, n_front=n_front, n_bird=n_bird, **kw)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}


def _gate_distance(p):
    """|d| at which inv_sigma2 * |d|^2 reaches 5.991, per bird edge (about 2.45 m at level 0, growing with the level's sigma)"""
    return np.sqrt(CHI2_BIRD / p["bird_inv_sigma2"].astype(np.float64))


def _displace_bird(p, g, which, lo, hi):
    """Move the measured camera point of the bird edges `which` by lo..hi times the gate distance, in a random direction."""
    which = np.asarray(which)
    d = g.normal(0, 1, (len(which), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= (g.uniform(lo, hi, len(which)) * _gate_distance(p)[which])[:, None]
    p["bird_xc"][which] = (p["bird_xc"][which].astype(np.float64) + d).astype(np.float32)
    p["bird_displaced"] = which


def _bad_start(p, g, rot_sigma, t_sigma):
    p["Tcw0"] = synth.to12(synth.perturb_pose(g, p["T_true"], rot_sigma=rot_sigma, t_sigma=t_sigma))


def _behind_camera(p, which):
    """Mirror the front points `which` through the camera centre: same pixel, negative depth."""
    T = p["T_true"]
    R, t = T[:3, :3], T[:3, 3]
    Xc = (R @ p["front_xw"][which].astype(np.float64).T).T + t
    p["front_xw"][which] = (R.T @ (-Xc - t).T).T.astype(np.float32)
    p["front_behind"] = np.asarray(which)


def spread_valid(n, n_invalid):
    """n slots of which n_invalid, spread evenly over the whole range, hold no edge."""
    v = np.ones(n, np.uint8)
    v[np.round(np.linspace(0, n - 1, n_invalid)).astype(np.int64)] = 0
    assert int(v.sum()) == n - n_invalid
    return v


def min_abs_depth_at_start(p):
    T = p["Tcw0"].astype(np.float64).reshape(3, 4)
    if len(p["front_xw"]) == 0:
        return math.inf
    return float(np.abs((T[:, :3] @ p["front_xw"].astype(np.float64).T).T[:, 2] + T[2, 3]).min())


# ---- the cases ----------------------------------------------------------------------------------------------------------
def _case(id, doc, prob, expect, **kw):
    kw.setdefault("mode", FRONT_BIRD)
    return dict(id=id, doc=doc, prob=prob, kw=kw, expect=tuple(expect))


def _bird_cross(seed, lo, hi, n_front=80, n_bird=80):
    p = _base(seed, n_front, n_bird)
    _displace_bird(p, synth.rng(seed + 1), np.nonzero(p["bird_is_outlier"])[0], lo, hi)
    return p


def bird_cross_all(seed, mode):
    """Optimizer.cc:673/:805 chi2 > chi2Bad flags every bird edge displaced past the gate"""
    return _case("bird_cross_all_" + MODE_NAME[mode], bird_cross_all.__doc__, _bird_cross(seed, 1.3, 3.0),
                 ["bird_flagged", "displaced_all_flagged"], mode=mode)


def bird_cross_some(seed, mode):
    """Optimizer.cc:673/:805 chi2Bad separates bird edges displaced to either side of the gate"""
    return _case("bird_cross_some_" + MODE_NAME[mode], bird_cross_some.__doc__, _bird_cross(seed, 0.3, 2.0),
                 ["bird_flagged", "displaced_mixed"], mode=mode)


def readmit(seed, mode, which=None, n_other=12, **kw):
    """Optimizer.cc:423-427, :651-655, :679-683, :811-815 an edge flagged after round 1 is back at level 0 after round 2: a
    third of the edges are gross outliers that all pull one way, so round 1 ends off the pose and flags good edges that
    lean the other way; round 2, without the gross ones, clears them"""
    g = synth.rng(seed + 1)
    which = which or MODE_NAME[mode]                         # the sensor whose edges are biased and re-admitted
    p = _base(seed, 90 if which == "front" else n_other, 90 if which == "bird" else 0, outlier_frac=0.0)
    expect = []
    if which == "front":
        n = len(p["front_xw"])
        sig = 1.0 / np.sqrt(p["front_inv_sigma2"].astype(np.float64))
        gross, other = np.arange(0, n, 3), np.arange(1, n, 3)
        p["front_obs"][gross, 0] += (g.uniform(25, 40, len(gross)) * sig[gross]).astype(np.float32)
        p["front_obs"][other, 0] -= (g.uniform(0.5, 2.2, len(other)) * sig[other]).astype(np.float32)
        expect.append("front_readmitted")
    else:
        n = len(p["bird_xw"])
        gd = _gate_distance(p)
        gross, other = np.arange(0, n, 3), np.arange(1, n, 3)
        p["bird_xc"][gross, 0] += (g.uniform(1.4, 1.8, len(gross)) * gd[gross]).astype(np.float32)
        p["bird_xc"][other, 0] -= (g.uniform(0.5, 0.95, len(other)) * gd[other]).astype(np.float32)
        expect.append("bird_readmitted")
    return _case("readmit_%s_in_%s" % (which, MODE_NAME[mode]), "Optimizer.cc:423-427, :651-655, :679-683, :811-815 a flagged edge goes back to level 0",
                 p, expect, mode=mode, **kw)


def bird_flag_on_entry(seed, mode):
    """Optimizer.cc:668/:800 mvBirdOutlier set on entry (it is not reset as mvbOutlier is, :297/:531): computeError at the
    round's pose, then decided like any other edge; some such edges end inliers and some outliers"""
    p = _bird_cross(seed, 1.5, 3.0)
    good, gross = np.nonzero(~p["bird_is_outlier"])[0], p["bird_displaced"]
    bo = np.zeros(len(p["bird_xw"]), np.uint8)
    bo[good[::7]] = 1
    bo[gross[::2]] = 1
    p["entry_flagged"] = np.nonzero(bo)[0]
    return _case("bird_flag_on_entry_" + MODE_NAME[mode], "Optimizer.cc:668/:800 mvBirdOutlier set on entry: computeError, then decided",
                 p, ["entry_flag_both_ways"], mode=mode, bird_outlier_in=[bo])


def weights(seed, mode, wF, wB):
    """Optimizer.cc:645 chi2 > chi2Mono * (wF + 1e-9), :672/:804 chi2Bad = chi2Bird * (wB + 1e-9): some edge's chi2 lies
    between the gate at weight 1 and the scaled gate"""
    p = _bird_cross(seed, 0.3, 2.0, n_front=80 if mode != BIRD else 20, n_bird=120)
    if mode == BIRD:
        return _case("weights_bird_wB%g" % wB, "Optimizer.cc:804 chi2Bird * (wB + 1e-9)", p, ["bird_flagged", "bird_between_gates"],
                     mode=BIRD, wB=wB)
    return _case("weights_wF%g_wB%g" % (wF, wB), "Optimizer.cc:645 chi2Mono * (wF + 1e-9), :672 chi2Bird * (wB + 1e-9)", p,
                 ["front_flagged", "bird_flagged", "front_between_gates", "bird_between_gates"], mode=FRONT_BIRD, wF=wF, wB=wB)


def count(seed, mode, nf, nb):
    """Optimizer.cc:379/:606/:776 fewer than 3 correspondences; :462/:690/:822 fewer than 10 edges"""
    counted = nb if mode == BIRD else nf                     # the edges the < 3 gate looks at
    total = {FRONT: nf, FRONT_BIRD: nf + nb, BIRD: nb}[mode]  # the edges of the graph
    rounds = 0 if counted < 3 else (1 if total < 10 else 4)
    doc = ("Optimizer.cc:379/:606/:776 fewer than 3 correspondences return 0" if rounds == 0 else
           "Optimizer.cc:462/:690/:822 edges().size() < 10 stops after one round" if rounds == 1 else
           "Optimizer.cc:462/:690/:822 ten edges run all four rounds")
    return _case("count_%s_%d_%d" % (MODE_NAME[mode], nf, nb), doc, _base(seed, nf, nb, outlier_frac=0.0), ["rounds_%d" % rounds],
                 mode=mode)


def no_active(seed, mode):
    """Optimizer.cc:394-396, :788-790 optimize() with every edge at level 1 returns at once (sparse_optimizer.cpp:356-359):
    every edge is a gross outlier after round 1, rounds 2 to 4 decide at the start pose"""
    g = synth.rng(seed + 1)
    if mode == BIRD:
        p = _base(seed, 0, 12)
        p["bird_xc"] = (p["bird_xc"] + g.uniform(-40, 40, (12, 3))).astype(np.float32)
    else:
        p = _base(seed, 14, 0)
        sign = np.where(g.random((14, 2)) < 0.5, -1.0, 1.0)
        p["front_obs"] = (p["front_obs"] + sign * g.uniform(200, 500, (14, 2))).astype(np.float32)
    return _case("no_active_" + MODE_NAME[mode], "Optimizer.cc:394-396/:788-790 optimize() with every edge at level 1", p,
                 ["no_active"], mode=mode)


def far_start(seed, mode, rot_sigma=0.5, t_sigma=1.5):
    """optimization_algorithm_levenberg.cpp:143-147 a step rejected before convergence (lambda *= ni), from a start pose far
    from the solution"""
    p = _base(seed, 120, 60 if mode == FRONT_BIRD else 0)
    _bad_start(p, synth.rng(seed + 1), rot_sigma, t_sigma)
    return _case("far_start_" + MODE_NAME[mode], "optimization_algorithm_levenberg.cpp:143-147 a rejected step before convergence", p,
                 ["early_reject"], mode=mode)


def behind_camera(seed, mode):
    """types_six_dof_expmap.cpp:266-296 projection and Jacobian at negative depth: PoseOptimization has no depth check, a
    point mirrored through the camera centre projects to the same pixel and stays an inlier"""
    p = _base(seed, 100, 60 if mode == FRONT_BIRD else 0)
    _behind_camera(p, np.arange(5, 100, 17))
    return _case("behind_camera_" + MODE_NAME[mode], "types_six_dof_expmap.cpp:266-296 projection and Jacobian at negative depth", p,
                 ["behind_camera_inliers"], mode=mode)


def bird_mask_holes(seed):
    """Optimizer.cc:666 idx = vnIndexEdgeBird[iB]: flags go back through the slot index, not the edge index; slots without
    an edge keep what they held"""
    p = _bird_cross(seed, 1.3, 3.0, n_front=60, n_bird=150)
    bv = spread_valid(150, 40)
    bo = np.where(bv == 0, PREFILL, 0).astype(np.uint8)
    return _case("bird_mask_holes", "Optimizer.cc:666 idx = vnIndexEdgeBird[iB]: flags go back through the slot index", p,
                 ["bird_flagged", "flags_both_sides_of_holes", "bird_prefill_kept"], mode=FRONT_BIRD, bird_valid=[bv],
                 bird_outlier_in=[bo])


# (constructor, seed, further arguments).  The seeds are chosen so that the oracle's margin is at least 1e-3 and the case's
# branch is taken; tests/test_pose_cases.py asserts both.
SPEC = (
    [(bird_cross_all, 4100, FRONT_BIRD), (bird_cross_all, 4100, BIRD), (bird_cross_some, 4101, FRONT_BIRD), (bird_cross_some, 5101, BIRD),
     (readmit, 4110, FRONT), (readmit, 4111, FRONT_BIRD, "front"), (readmit, 4113, FRONT_BIRD, "bird", 3), (readmit, 4112, BIRD),
     (bird_flag_on_entry, 5120, FRONT_BIRD), (bird_flag_on_entry, 4120, BIRD),
     (weights, 4130, FRONT_BIRD, 0.5, 4.0), (weights, 4131, FRONT_BIRD, 2.0, 0.5), (weights, 4134, BIRD, 1.0, 0.5), (weights, 4135, BIRD, 1.0, 4.0)]
    + [(count, 4140 + i, FRONT_BIRD, nf, nb) for i, (nf, nb) in enumerate(((2, 300), (3, 0), (3, 6), (3, 7), (6, 3), (6, 4)))]
    + [(count, 4150 + i, BIRD, 20, nb) for i, nb in enumerate((2, 3, 9, 10))]
    + [(count, 4160 + i, FRONT, nf, 5) for i, nf in enumerate((2, 3, 9, 10))]
    + [(no_active, 4300, FRONT), (no_active, 4302, BIRD), (far_start, 8310, FRONT), (far_start, 77311, FRONT_BIRD),
       (behind_camera, 4330, FRONT), (behind_camera, 4331, FRONT_BIRD), (bird_mask_holes, 4340)])

_CASES = None


def cases():
    """the cases, built once and shared; do not edit the arrays"""
    global _CASES
    if _CASES is None:
        _CASES = [s[0](s[1], *s[2:]) for s in SPEC]
    return _CASES


# ---- running a case -----------------------------------------------------------------------------------------------------
COUNTERS = ("accepted", "rejected", "exit_qmax", "exit_rho0", "exit_nbad", "failed_solve", "no_active", "rounds")
ROUND_COUNTERS = ("front_flagged", "bird_flagged", "front_readmitted", "bird_readmitted")


def oracle_trace_reset(lib):
    lib.orc_lm_trace_reset()
    lib.orc_pose_margin_reset()


def oracle_trace(lib):
    """dict of the oracle's counters since the last reset (per-round ones as lists of four), events and margin"""
    cnt = (C.c_long * 24)()
    buf = C.create_string_buffer(1 << 16)
    lib.orc_lm_trace_get.restype = C.c_long
    n = lib.orc_lm_trace_get(cnt, buf, C.c_long(len(buf)))
    assert n < len(buf)
    margin, decisions = C.c_double(), C.c_long()
    lib.orc_pose_margin_get(C.byref(margin), C.byref(decisions))
    t = {k: int(cnt[i]) for i, k in enumerate(COUNTERS)}
    for j, k in enumerate(ROUND_COUNTERS):
        t[k] = [int(cnt[8 + 4 * r + j]) for r in range(4)]
    t.update(events=buf.value.decode(), margin=margin.value, decisions=decisions.value)
    return t


def run_oracle(case, lib, call, pose_args):
    """the case through orc_pose_opt -> (outputs of frame 0, trace)"""
    a, out, keep = pose_args([case["prob"]], **case["kw"])
    oracle_trace_reset(lib)
    call("orc_pose_opt", a)
    return {k: v[0] for k, v in out.items()}, oracle_trace(lib)


def run_model(case):
    import pose_ref
    kw = {k: (v[0] if isinstance(v, list) else v) for k, v in case["kw"].items()}
    return pose_ref.pose_opt(case["prob"], front_prefill=PREFILL, **kw)


# ---- the branch each case is about, from the oracle's outputs and trace -------------------------------------------------
def _valid(case, which):
    v = case["kw"].get(which)
    n = len(case["prob"]["front_xw" if which == "front_valid" else "bird_xw"])
    return np.ones(n, bool) if v is None else np.asarray(v[0], bool)


def _displaced_flags(case, out):
    d = case["prob"]["bird_displaced"]
    d = d[_valid(case, "bird_valid")[d]]
    return out["bird_outlier"][d]


def _entry_flag_both_ways(case, out, tr, model):
    e = case["prob"]["entry_flagged"]
    return 0 < int(out["bird_outlier"][e].sum()) < len(e)


def _between(chi2, gate, gate1):
    lo, hi = min(gate, gate1), max(gate, gate1)
    return bool(((chi2 > lo) & (chi2 <= hi)).any())


def _flags_both_sides(case, out, tr, model):
    bv = _valid(case, "bird_valid")
    holes = np.nonzero(~bv)[0]
    flagged = np.nonzero(bv & (out["bird_outlier"] == 1))[0]
    # slot index minus edge index of every flagged edge: different from one flagged edge to another, flags before and after
    # most of the holes
    offsets = {int((holes < f).sum()) for f in flagged}
    return len(offsets) >= 4 and max(offsets) - min(offsets) >= len(holes) // 2


def _behind_inliers(case, out, tr, model):
    b = case["prob"]["front_behind"]
    T = out["Tcw"].astype(np.float64).reshape(3, 4)
    z = (T[:, :3] @ case["prob"]["front_xw"][b].astype(np.float64).T).T[:, 2] + T[2, 3]
    return bool((z < 0).all()) and bool((out["front_outlier"][b] == 0).any())


EXPECT = {
    "bird_flagged": lambda c, o, t, m: t["bird_flagged"][t["rounds"] - 1] > 0 and int((o["bird_outlier"] == 1).sum()) > 0,
    "front_flagged": lambda c, o, t, m: 0 < t["front_flagged"][t["rounds"] - 1] < len(c["prob"]["front_xw"]),
    "displaced_all_flagged": lambda c, o, t, m: bool((_displaced_flags(c, o) == 1).all()),
    "displaced_mixed": lambda c, o, t, m: 0 < int(_displaced_flags(c, o).sum()) < len(_displaced_flags(c, o)),
    "front_readmitted": lambda c, o, t, m: sum(t["front_readmitted"]) > 0,
    "bird_readmitted": lambda c, o, t, m: sum(t["bird_readmitted"]) > 0,
    "entry_flag_both_ways": _entry_flag_both_ways,
    # an edge whose chi2 lies between the gate at weight 1 and the scaled gate: ignoring the weight in the gate flips its flag
    "front_between_gates": lambda c, o, t, m: _between(m["front_chi2"], m["front_gate"], 1.5 * (1.0 + 1e-9)),
    "bird_between_gates": lambda c, o, t, m: _between(m["bird_chi2"], m["bird_gate"], float(np.float32(5.991 * (1.0 + 1e-9)))),
    "rounds_0": lambda c, o, t, m: t["rounds"] == 0 and o["ninliers"] == 0 and np.array_equal(o["Tcw"], c["prob"]["Tcw0"]),
    "rounds_1": lambda c, o, t, m: t["rounds"] == 1,
    "rounds_4": lambda c, o, t, m: t["rounds"] == 4,
    "no_active": lambda c, o, t, m: t["no_active"] > 0 and t["rounds"] == 4,
    # a rejection that is not rounding noise at convergence: in round 1, before the third accepted step
    "early_reject": lambda c, o, t, m: re.match(r"/([A.]{0,4})R", t["events"]) is not None,
    "behind_camera_inliers": _behind_inliers,
    "flags_both_sides_of_holes": _flags_both_sides,
    "bird_prefill_kept": lambda c, o, t, m: bool((o["bird_outlier"][~_valid(c, "bird_valid")] == PREFILL).all()),
}
