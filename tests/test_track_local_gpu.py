"""Discard outliers -> SearchLocalPoints on the device chain (csrc/track.hip: k_discard, k_local_points) against the literal
model of tests/track_local_ref.py and, bit-exact, against the oracle's granular steps: the controlled scenario of
tests/track_local_cases.py through fb_frame_pose_optimization_dev -> fb_frame_discard_outliers_dev ->
fb_frame_search_local_points_dev, and a short drive through fb_frame_track_dev / the granular entry points."""
import ctypes as C

import numpy as np
import pytest

import track_local_cases as TC
from fishbirdeyevisualslam_amd import cabi, track as T
from test_track_chain_gpu import _cmp_view

pytestmark = pytest.mark.gpu


def _chain(sc):
    seq = sc["seq"]
    return T.TrackChain(TC.B, TC.FRONT_WH, TC.BIRD_WH, K=seq.Kc, D=seq.D, use_lists=True)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_gpu(sc, two_stages):
    """tests/track_local_cases.run_oracle on the frame handle (after init_first the handle is tc.last)."""
    tc = _chain(sc)
    L, s = tc.L, tc._stream()
    f, b, c = (_up(x) for x in sc["imgs"])
    tc.extract(f, b, c, _up(sc["mask"]))
    tc.set_map(sc["M"], sc["MB"], sc["lm"], sc["lb"])
    tc.init_first(sc["mp0"], sc["mpb0"], sc["Tcw0"])
    h, A = tc.last, tc.targs
    out = {}

    def pose_and_discard(tag_pose, tag_discard):
        T.check(L.fb_frame_pose_optimization_dev(h, C.byref(A.map), C.byref(A.mpb), cabi.FB_POSE_FRONT_BIRD, C.c_float(1.0), C.c_float(1.0), 0, s), "pose")
        out[tag_pose] = tc.view("last")
        T.check(L.fb_frame_discard_outliers_dev(h, C.byref(A.map), s), "discard")
        out[tag_discard] = tc.view("last")
    pose_and_discard("pose", "discard")
    if two_stages:
        mp = _up(TC.second_stage_points(sc, out["discard"]["map_point"]))
        T.check(L.fb_frame_set_map_points_dev(h, C.c_void_p(mp.data_ptr()), None, s), "set_map_points")
        pose_and_discard("pose2", "discard2")
    tc.set_map(sc["M_after"], sc["MB"], sc["lm"], sc["lb"])     # (d): the points went bad after stage 1
    m08 = cabi.MatcherParams(0.8, 1)
    T.check(L.fb_frame_search_local_points_dev(h, C.byref(A.map), C.c_void_p(A.d_local_mp), C.c_void_p(A.d_n_local_mp), C.c_float(1.0), C.byref(m08), s), "local points")
    out["local"] = tc.view("last")
    tc.close()
    return out


@pytest.mark.parametrize("two_stages", [False, True], ids=["one discard", "two discards in one frame"])
def test_granular_steps_against_the_model_and_the_oracle(two_stages):
    sc = TC.scenario()
    ref = TC.run_oracle(sc, two_stages=two_stages)
    TC.check_discriminates(sc, ref, two_stages=two_stages)
    got = _run_gpu(sc, two_stages)
    for b in range(TC.B):
        e = TC.expected(sc, got, b, two_stages=two_stages)   # the model on the GPU frame's own flags, counters and pose
        for stage in ("discard", "discard2", "local") if two_stages else ("discard", "local"):
            TC.compare(got, e, b, stage, "gpu")
        N = int(got["local"]["n"][b])
        kept = {X for _, _, X in sc["kinds"][b]["c"]}
        assert not (e["marked"] - kept) & set(got["local"]["map_point"][b, :N].tolist())
    for stage in ref:
        _cmp_view(got[stage], ref[stage], "scenario, after " + stage)


def _drive_on_gpu(sc, ref, step, with_keyframe=False):
    """The drive of TC.fused_scenario on the device chain, every tracked frame compared with the oracle's (`ref`)."""
    tc = _chain(sc)
    mask = _up(sc["mask"])
    f, bd, c = (_up(x) for x in sc["imgs"][0])
    tc.extract(f, bd, c, mask)
    if with_keyframe:
        from fishbirdeyevisualslam_amd.bow_problem import make_vocabulary
        tc.set_vocabulary(make_vocabulary(TC.FUSED_SEED + 1, k=TC.VOC_K, L=TC.VOC_L)[1], TC.VOC_L)
    tc.set_map(sc["M"], sc["MB"], sc["lm"], sc["lb"])
    tc.init_first(sc["mp0"], sc["mpb0"], sc["Tcw0"])
    if with_keyframe:
        tc.make_keyframe("last")
    for k in range(1, TC.FUSED_FRAMES):
        f, bd, c = (_up(x) for x in sc["imgs"][k])
        step(tc, k, f, bd, c, mask)
        _cmp_view(tc.view(), ref[k - 1]["view"], "drive, frame %d" % k)
        assert np.array_equal(tc.bird_table_host()["n"], ref[k - 1]["table"]["n"])
    tc.close()


@pytest.mark.parametrize("granular", [False, True], ids=["fb_frame_track_dev", "granular entry points"])
def test_drive_with_points_the_first_stage_drops(granular):
    """Two tracked frames on a map with (a)-type edits of TC.FUSED_SHIFT_PX (what the drive contains and that it discriminates:
    test_track_local.py::test_drive_points_the_first_stage_drops_stay_out, on the oracle alone): device chain == oracle."""
    sc = TC.fused_scenario()

    def step(tc, k, f, bd, c, mask):
        tc.set_delta(sc["seq"].delta(k))
        (tc.track_granular if granular else tc.track)(f, bd, c, mask)
    _drive_on_gpu(sc, TC.run_oracle_drive(sc), step)


def test_fall_back_frame():
    """TrackWithMotionModel -> TrackReferenceKeyFrame -> TrackLocalMap in one frame (track_modes' "motion+reference"), sequence 0's
    motion-model stage failing after its discard loop in frame 1: the marks of both loops count (shown on the oracle and the
    model in test_track_local.py::test_fall_back_frame_marks_of_both_stages_count); device chain == oracle."""
    sc = TC.fused_scenario()
    ref = TC.run_oracle_drive(sc, TC.FALLBACK_MODES, TC.FALLBACK_YAW)
    c = ref[0]["stages"]["motion_discard"]["counts"]
    assert c[TC.CNT["PROJ_MATCHES"], 0] >= 20 and c[TC.CNT["MATCHES_MAP"], 0] < 10
    for fr in ref:   # the oracle's counter lies below what the marks of one loop alone give
        for b in range(TC.B):
            for only in ("motion", "reference"):
                assert int(fr["view"]["counts"][TC.CNT["TO_MATCH"], b]) < TC.model_drive_frame(sc, fr["stages"], b, marks=only)["TO_MATCH"]

    def step(tc, k, f, bd, c, mask):
        tc.set_delta(TC.drive_delta(sc, k, TC.FALLBACK_YAW))
        tc.set_delta_kf(sc["seq"].delta_between(0, k))
        tc.track_modes(f, bd, c, mask, mode=TC.FALLBACK_MODES[k])
    _drive_on_gpu(sc, ref, step, with_keyframe=True)
