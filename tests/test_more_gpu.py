"""GPU parity (through the C-ABI) of M4 SearchByProjection(Frame, KeyFrame), M6 SearchByBoW(KF, KF), Frame::isInFrustum,
Frame::UndistortKeyPoints and Frame::ComputeImageBounds against the CPU oracle.  Match indices, masks, levels and the
float outputs are all required to be bit-identical (both sides evaluate the same IEEE expression sequence)."""
import os
import sys

import numpy as np
import pytest

import hip_lib as H
import oracle_lib as O
from fishbirdeyevisualslam_amd import bow_problem as BP, more_problems as M, problems as P, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("seed,ncur,nkf", [(7000, 2000, 2000), (7001, 2064, 1200), (7002, 300, 1500), (7003, 40, 0)])
def test_search_by_projection_keyframe(seed, ncur, nkf):
    probs = [M.make_proj_kf_problem(seed + 10 * i, ncur, nkf) for i in range(3)]
    geom = P.grid_geom(synth.front_grid_geom(1280, 720))
    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], geom, O.grid_build, ncur)
    for th, od, ori in ((10.0, 100, 1), (3.0, 64, 1), (10.0, 100, 0)):
        a, oo, k = M.proj_kf_args(probs, cs, ci, th=th, orb_dist=od, check_ori=ori)
        O.call("orc_match_projection_keyframe", a)
        a2, oh, k2 = M.proj_kf_args(probs, cs, ci, th=th, orb_dist=od, check_ori=ori)
        H.call("fb_match_projection_keyframe", a2)
        np.testing.assert_array_equal(oh["match_cur_to_kf"], oo["match_cur_to_kf"])
        np.testing.assert_array_equal(oh["nmatches"], oo["nmatches"])
    if nkf >= 1200:
        assert oo["nmatches"].min() > 50


def test_search_by_projection_keyframe_contention():
    """Many key-frame points compete for few free slots: the serial 'slot already has a MapPoint' rule."""
    probs = [M.make_proj_kf_problem(7500 + i, 150, 2000) for i in range(2)]
    geom = P.grid_geom(synth.front_grid_geom(1280, 720))
    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], geom, O.grid_build, 150)
    a, oo, k = M.proj_kf_args(probs, cs, ci, th=60.0)
    O.call("orc_match_projection_keyframe", a)
    a2, oh, k2 = M.proj_kf_args(probs, cs, ci, th=60.0)
    H.call("fb_match_projection_keyframe", a2)
    np.testing.assert_array_equal(oh["match_cur_to_kf"], oo["match_cur_to_kf"])
    np.testing.assert_array_equal(oh["nmatches"], oo["nmatches"])


@pytest.mark.parametrize("seed,n1,n2,share", [(7100, 1500, 1500, True), (7101, 2064, 700, True), (7102, 400, 2000, False), (7103, 30, 30, True)])
def test_search_by_bow_keyframes(seed, n1, n2, share):
    probs = [M.make_bow_kf_problem(seed + 10 * i, n1, n2, share) for i in range(3)]
    for ori in (1, 0):
        a, oo, k = M.bow_kf_args(probs, check_ori=ori)
        O.call("orc_match_bow_kf", a)
        a2, oh, k2 = M.bow_kf_args(probs, check_ori=ori)
        H.call("fb_match_bow_kf", a2)
        np.testing.assert_array_equal(oh["matches12"], oo["matches12"])
        np.testing.assert_array_equal(oh["nmatches"], oo["nmatches"])
    if share and n1 >= 400:
        assert oo["nmatches"].min() > 50


@pytest.mark.parametrize("above", [False, True])
def test_search_by_bow_keyframes_contention(above):
    """M6 under contention (see test_bow_gpu.test_search_by_bow_contention): the free candidates are the KF2 features that
    carry a MapPoint, and they limit the number of matches."""
    limit = BP.queries_kept_in_registers()
    n_q = limit + 104 if above else 2000
    assert (n_q > limit) == above
    probs = []
    for i in range(2):
        p = BP.make_contended_bow_problem(6500 + i, n_q, 150)
        probs.append(dict(kps1=p["kf_kps"], desc1=p["kf_desc"], has_mp1=p["kf_has_mp"], kps2=p["f_kps"], desc2=p["f_desc"],
                          has_mp2=(synth.rng(6600 + i).random(150) < 0.7).astype(np.uint8)))
    for ori in (1, 0):
        a, oo, k = M.bow_kf_args(probs, check_ori=ori)
        O.call("orc_match_bow_kf", a)
        a2, oh, k2 = M.bow_kf_args(probs, check_ori=ori)
        H.call("fb_match_bow_kf", a2)
        np.testing.assert_array_equal(oh["matches12"], oo["matches12"])
        np.testing.assert_array_equal(oh["nmatches"], oo["nmatches"])
        for b, p in enumerate(probs):
            assert 2 * oo["nmatches"][b] >= p["has_mp2"].sum()


@pytest.mark.parametrize("seed,n", [(7200, 5000), (7201, 257), (7202, 1), (7203, 0)])
def test_in_frustum(seed, n):
    probs = [M.make_frustum_problem(seed + 10 * i, max(n - 3 * i, 0)) for i in range(3)]
    if n == 0:
        probs = probs[:1]
    a, oo, k = M.frustum_args(probs)
    O.call("orc_in_frustum", a)
    a2, oh, k2 = M.frustum_args(probs)
    H.call("fb_in_frustum", a2)
    for b, p in enumerate(probs):
        m = len(p["mp_xw"])
        for key in ("in_view", "proj", "proj_xr", "level", "view_cos"):
            np.testing.assert_array_equal(oh[key][b, :m], oo[key][b, :m], err_msg=key)
    if n >= 257:
        assert (oo["in_view"] == 1).sum() > 50


def test_undistort_and_image_bounds():
    import fishbirdeyevisualslam_amd as fb
    g = synth.rng(7300)
    for n in (0, 1, 777, 2064):
        kps = synth.random_keypoints(g, n, 1280, 720)
        uo = M.undistort(O.lib(), "orc_", kps)
        uh = M.undistort(fb.lib(), "fb_", kps)
        np.testing.assert_array_equal(uh, uo)
        np.testing.assert_array_equal(M.undistort(fb.lib(), "fb_", kps, D4=np.zeros(4)), kps)
    for D in (M.FISHEYE_D, np.zeros(4)):
        np.testing.assert_array_equal(M.image_bounds(fb.lib(), "fb_", 1280, 720, D4=D), M.image_bounds(O.lib(), "orc_", 1280, 720, D4=D))


def test_hip_reproduces_more_golden():
    """tests/golden/{m4,m6,frustum,undistort}.npz through the HIP library."""
    import fishbirdeyevisualslam_amd as fb
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    got = make_golden.more_cases(fb, prefix="fb_", call=H.call, grid_fn=H.grid_build)
    for name, d in got.items():
        ref = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
        for key, v in d.items():
            np.testing.assert_array_equal(v, ref[key], err_msg="%s.%s" % (name, key))
