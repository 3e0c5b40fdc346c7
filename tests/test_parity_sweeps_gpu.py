"""Wide HIP-vs-oracle sweeps, bounded so that they run inside `pytest -m gpu`:
  * 240 pose-optimisation problems x 3 modes: outlier masks and inlier counts identical, poses within 1e-4; the test PRINTS
    the smallest |chi2 - threshold| / threshold over every inlier/outlier decision the oracle took, i.e. the margin behind
    "identical masks" for an implementation that rounds differently (k_pose_opt evaluates the LM passes with fused
    multiply-adds and wave-order sums; its decision arithmetic is unfused and operation-for-operation the oracle's).
  * ~300 random-parameter cases of ORB extraction (odd sizes, level counts, scale factors, thresholds, white noise) and of
    the windowed matchers (odd counts, thresholds, contention), bit-exact.
Both were probes under profiles/probes/ in round 1."""
import ctypes as C

import numpy as np
import pytest

import hip_lib as H
import oracle_lib as O
from fishbirdeyevisualslam_amd import cabi, kf_problems as KP, more_problems as M, problems as P, synth

pytestmark = pytest.mark.gpu


def test_pose_mask_sweep_240_problems(capsys):
    n = 240
    worst = 0.0
    O.lib().orc_pose_margin_reset()
    for mode in (cabi.FB_POSE_FRONT_BIRD, cabi.FB_POSE_FRONT, cabi.FB_POSE_BIRD):
        for s0 in range(0, n, 8):
            probs = [synth.make_pose_problem(7000 + s0 + i, n_front=500 + 37 * ((s0 + i) % 40), n_bird=200 + 19 * ((s0 + i) % 40)) for i in range(8)]
            a, oo, k = P.pose_args(probs, mode=mode)
            O.call("orc_pose_opt", a)
            a2, oh, k2 = P.pose_args(probs, mode=mode)
            H.call("fb_pose_opt", a2)
            To, Th = oo["Tcw"].reshape(-1, 3, 4), oh["Tcw"].reshape(-1, 3, 4)
            rel = (np.abs(Th - To) / np.maximum(1.0, np.abs(To).max(axis=(1, 2), keepdims=True))).max()
            worst = max(worst, rel)
            assert rel <= 1e-4, (mode, s0, rel)
            np.testing.assert_array_equal(oh["ninliers"], oo["ninliers"], err_msg="mode %d seeds %d.." % (mode, 7000 + s0))
            np.testing.assert_array_equal(oh["front_outlier"], oo["front_outlier"], err_msg="mode %d seeds %d.." % (mode, 7000 + s0))
            np.testing.assert_array_equal(oh["bird_outlier"], oo["bird_outlier"], err_msg="mode %d seeds %d.." % (mode, 7000 + s0))
    margin, decisions = C.c_double(0), C.c_long(0)
    O.lib().orc_pose_margin_get(C.byref(margin), C.byref(decisions))
    with capsys.disabled():
        print("\n[pose sweep] %d problems x 3 modes, %d inlier/outlier decisions: masks identical; worst relative pose difference %.3g; "
              "smallest |chi2 - threshold| / threshold = %.3g" % (n, decisions.value, worst, margin.value))
    assert decisions.value > 1000000


def test_local_ba_gate_sweep_60_problems(capsys):
    """60 LocalBundleAdjustmentWithOdom problems (6-20 key frames): outlier flags identical, poses / landmarks within 1e-4 per
    element (each pose by max(1, max|T_k|) of its own 3x4, each landmark by max(1, ||x||): ba_cases.pose_rel / point_rel);
    PRINTS the smallest |chi2 - 5.991| / 5.991 over every decision of the chi2 gate between the two optimisations and of the
    final outlier collection (Optimizer.cc:2534-2565, 2579-2610), front and bird edges: the margin behind 'identical flags'."""
    import ba_cases as BC
    from fishbirdeyevisualslam_amd import ba_problem
    O.lib().orc_ba_margin_reset()
    worst_pose = worst_pt = 0.0
    n = 60
    for i in range(n):
        nkf = 6 + (i * 7) % 15
        p = synth.make_ba_problem(8000 + i, n_kf=nkf, n_mp=300 + 53 * (i % 11), n_mpb=80 + 17 * (i % 7), outlier_frac=0.03 + 0.01 * (i % 4))
        a, oo, k = ba_problem.local_ba_args(p, with_odom=1)
        O.call("orc_local_ba", a)
        a2, oh, k2 = ba_problem.local_ba_args(p, with_odom=1)
        H.call("fb_local_ba", a2)
        worst_pose = max(worst_pose, BC.worst_pose_rel(oh["kf_Tcw"], oo["kf_Tcw"]))
        worst_pt = max(worst_pt, BC.worst_point_rel(oh["mp_xw"], oo["mp_xw"]), BC.worst_point_rel(oh["mpb_xw"], oo["mpb_xw"]))
        assert worst_pose <= 1e-4 and worst_pt <= 1e-4, (i, worst_pose, worst_pt)
        np.testing.assert_array_equal(oh["obs_outlier"], oo["obs_outlier"], err_msg="problem %d front flags" % i)
        nb = len(p["bobs_kf"])
        np.testing.assert_array_equal(oh["bobs_outlier"][:nb], oo["bobs_outlier"][:nb], err_msg="problem %d bird flags" % i)
    margin, decisions = C.c_double(0), C.c_long(0)
    O.lib().orc_ba_margin_get(C.byref(margin), C.byref(decisions))
    with capsys.disabled():
        print("\n[local BA sweep] %d problems (6-20 key frames), %d chi2-gate decisions: outlier flags identical; worst per-element relative "
              "difference poses %.3g, landmarks %.3g; smallest |chi2 - 5.991| / 5.991 = %.3g" % (n, decisions.value, worst_pose, worst_pt, margin.value))
    assert decisions.value > 100000


def _both(build, on, hn, keys):
    a, oo, k = build()
    O.call(on, a)
    a2, oh, k2 = build()
    H.call(hn, a2)
    return all(np.array_equal(oh[x], oo[x]) for x in keys)


def test_fuzz_parity_300_cases(capsys):
    g = np.random.default_rng(12345)
    n_cases, bad, skipped = 0, [], 0
    geomF = P.grid_geom(synth.front_grid_geom(1280, 720))
    geomB = P.grid_geom(synth.bird_grid_geom(512, 512))
    while n_cases < 300:
        kind = int(g.integers(0, 6))
        seed = int(g.integers(0, 1 << 30))
        desc = "?"
        try:
            if kind == 0:      # ORB extraction
                w, h = int(g.integers(60, 900)), int(g.integers(60, 700))
                p = O.orb_params(nfeatures=int(g.integers(50, 3000)), nlevels=int(g.integers(1, 9)),
                                 scale_factor=float(np.float32(g.uniform(1.05, 2.2))), ini_th_fast=int(g.integers(8, 40)),
                                 min_th_fast=int(g.integers(2, 8)))
                img = synth.synth_image(seed, w, h) if g.random() < 0.8 else g.integers(0, 256, (h, w), dtype=np.uint8)
                desc = "orb %dx%d nf=%d nl=%d sf=%.3f ini=%d min=%d" % (w, h, p.nfeatures, p.nlevels, p.scale_factor, p.ini_th_fast, p.min_th_fast)
                orb = H.Orb(p)
                try:
                    kh, dh = orb.extract(img)
                finally:
                    orb.close()
                ko, do = O.orb_extract(p, img)
                ok = len(kh) == len(ko) and np.array_equal(kh, ko) and np.array_equal(dh, do)
            else:
                ncur, nq = int(g.integers(0, 2600)), int(g.integers(0, 2600))
                B = int(g.integers(1, 4))
                if kind == 1:
                    probs = [synth.make_proj_frame_problem(seed + i, max(ncur, 1), nq, dup_frac=float(g.uniform(0, 0.5))) for i in range(B)]
                    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], geomF, O.grid_build, max(ncur, 1))
                    th = float(g.choice([7.0, 15.0, 30.0, 60.0]))
                    desc = "m3 ncur=%d nlast=%d B=%d th=%g" % (ncur, nq, B, th)
                    ok = _both(lambda: P.proj_frame_args(probs, cs, ci, th=th, check_ori=1), "orc_match_projection_frame", "fb_match_projection_frame", ["match_cur_to_last", "nmatches"])
                elif kind == 2:
                    probs = [synth.make_proj_points_problem(seed + i, max(ncur, 1), max(nq, 1)) for i in range(B)]
                    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], geomF, O.grid_build, max(ncur, 1))
                    th = float(g.choice([1.0, 3.0, 5.0]))
                    desc = "m2 ncur=%d nmp=%d B=%d th=%g" % (ncur, nq, B, th)
                    ok = _both(lambda: P.proj_points_args(probs, cs, ci, th=th), "orc_match_projection_points", "fb_match_projection_points", ["match_cur_to_mp", "nmatches"])
                elif kind == 3:
                    probs = [synth.make_bird_mp_problem(seed + i, max(ncur, 1), nq) for i in range(B)]
                    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], geomB, O.grid_build, max(ncur, 1))
                    desc = "m9 ncur=%d nref=%d B=%d" % (ncur, nq, B)
                    ok = _both(lambda: P.bird_mp_args(probs, cs, ci, prefill=-1), "orc_match_bird_mappoints", "fb_match_bird_mappoints", ["match_cur_to_ref", "ninliers"])
                elif kind == 4:
                    probs = [M.make_proj_kf_problem(seed + i, max(ncur, 1), nq) for i in range(B)]
                    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], geomF, O.grid_build, max(ncur, 1))
                    th = float(g.choice([3.0, 10.0, 40.0]))
                    desc = "m4 ncur=%d nkf=%d B=%d th=%g" % (ncur, nq, B, th)
                    ok = _both(lambda: M.proj_kf_args(probs, cs, ci, th=th), "orc_match_projection_keyframe", "fb_match_projection_keyframe", ["match_cur_to_kf", "nmatches"])
                else:
                    sim3 = bool(g.integers(0, 2))
                    probs = [KP.make_kf_points_problem(seed + i, max(ncur, 1), nq, sim3) for i in range(B)]
                    cs, ci = P.build_grid_host([p["kf_kps"] for p in probs], P.grid_geom(synth.front_grid_geom(KP.W, KP.H)), O.grid_build, max(ncur, 1))
                    thf, thi = float(g.choice([3.0, 8.0])), int(g.choice([5, 10, 40]))
                    desc = "fuse sim3=%s nkf=%d nmp=%d B=%d" % (sim3, ncur, nq, B)
                    ok = _both(lambda: KP.fuse_args(probs, cs, ci, th=thf), "orc_fuse_sim3_search" if sim3 else "orc_fuse_search",
                               "fb_fuse_sim3_search" if sim3 else "fb_fuse_search", ["best_idx"])
                    if sim3:
                        ok = ok and _both(lambda: KP.proj_sim3_args(probs, cs, ci, th=thi), "orc_match_projection_sim3", "fb_match_projection_sim3", ["match_kf_to_mp", "nmatches"])
        except Exception as e:  # a documented capacity / argument refusal (on either side) is a skipped case, anything else a failure
            msg = str(e)
            if isinstance(e, AssertionError) and msg == "-3":   # the oracle's own capacity error (orc_orb_extract)
                msg = "oracle capacity (-3)"
            if any(t in msg.lower() for t in ("capacity", "too large", "exceed", "bad argument", "is empty")):
                skipped += 1
                n_cases += 1
                continue
            ok = False
            desc += " EXC " + msg[:160]
        n_cases += 1
        if not ok:
            bad.append(desc)
    with capsys.disabled():
        print("\n[fuzz parity] %d cases (%d refused by a documented capacity / argument check), %d mismatches" % (n_cases, skipped, len(bad)))
    assert not bad, bad
    assert skipped < 60
