"""CPU tests of SearchInNeighbors: the hand answers of tests/search_in_neighbors_cases.py on the literal model, the event
coverage of the generated scene, the two new entry points in the header and the library, and the host-side refusals that
come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import covis_ref as CR
import loop_fuse_ref as LR
import search_in_neighbors_cases as SC
import search_in_neighbors_ref as SR
from fishbirdeyevisualslam_amd import cabi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_model(d):
    c = d["c"]
    w, g = LR.World(c), CR.Graph(c["K"], c["kf_order"])
    out = SR.search_in_neighbors(w, g, c, d["cur"], d.get("n_features_arg", d["n_features"]), d["targets"], new_edge_cap=d.get("new_edge_cap"),
                                 cand_cap=d.get("cand_cap"))
    return w, g, out


@pytest.mark.parametrize("case", SC.FUSE_HAND, ids=lambda f: f.__name__)
def test_hand_answers_on_the_model(case):
    d = case()
    w, g, out = run_model(d)
    for key, got in (("n_fused", out.n_fused), ("added", [r[:3] for r in w.added_rows]), ("replaced", w.replaced_rows),
                     ("candidates", out.candidates), ("errors", w.errors)):
        if key in d:
            assert got == d[key], key


def test_replace_more_obs_skips_the_bad_snapshot_entry_at_later_targets():
    w, g, out = run_model(SC.replace_more_obs())
    assert w.mp_bad[0] and w.replaced[0] == 1 and w.stats["snapshot_bad_skipped"] == 2
    assert w.kf_mp[0, 0] == 1 and sorted(w.obs[1]) == [0, 1, 2, 3]


def test_two_win_one_feature_drops_the_second_points_edge():
    w, g, out = run_model(SC.two_win_one_feature())
    assert w.kf_mp[0].tolist() == [0, -1] and w.kf_mp[1, 0] == 0 and w.mp_bad[1] and sorted(w.obs[0]) == [0, 1]


def test_point_at_two_features_is_refused_on_the_live_map():
    w, g, out = run_model(SC.point_at_two_features_of_cur())
    assert w.stats["live_invalid"] == 1 and out.best_log[0] == [0, 0]


def test_candidate_order_sees_the_point_step_two_made_bad():
    w, g, out = run_model(SC.candidate_order())
    assert w.stats["candidate_bad_by_step2"] == 1 and w.stats["candidate_again"] == 1 and w.kf_mp[1, 2] == 3 and w.mp_bad[3]


def test_descriptor_moves_the_match():
    """the case cannot decay: with the descriptor it had at entry the point takes the other feature of target 2"""
    d = SC.descriptor_moves_the_match()
    c = d["c"]
    w, g, out = run_model(d)
    after = out.best_log[1][0]
    entry = SR.oracle_search(LR.World(c), c, 2, [0], [1], 3.0)[0]
    assert entry == 0 and after == 1
    assert not np.array_equal(w.desc[0], c["mp_desc"][0])
    assert w.stats["descriptor_changed_between_targets"] == 1


@pytest.mark.parametrize("case", SC.TARGET_CASES, ids=lambda f: f.__name__)
def test_target_lists_on_the_model(case):
    d = case()
    g = CR.Graph(d["K"], d["kf_order"])
    for a, b, wt in d["connections"]:
        g.add_connection(a, b, wt)
    t = SR.fuse_targets(g, d["cur"], d["kf_bad"], d["nn"], d["nn2"])
    assert len(t) == d.get("n_uncut", len(d["expected"])) and t[:len(d["expected"])] == d["expected"]


def test_second_twice_lists_the_key_frame_three_times():
    d = SC.second_twice()
    assert d["expected"].count(3) == 3


def test_generated_scene_shows_every_event():
    c, cur = SC.generated()
    w, g = LR.World(c), CR.Graph(c["K"], c["kf_order"])
    m = CR.Map(w.kf_n, w.kf_mp, w.kf_octave, w.mp_bad, w.obs_mp, w.obs_kf, w.obs_idx, w.kf_order)
    for s in sorted(range(c["K"]), key=g.key):
        g.update_connections(m, s)
    st = SR.new_stats()
    targets = SR.fuse_targets(g, cur, c["kf_bad"], 20, 5, st)
    w.stats.update(st)
    SR.search_in_neighbors(w, g, c, cur, int(c["kf_n"][cur]), targets, new_edge_cap=SC.GEN_NEW_EDGE_CAP)
    missing = [k for k in SR.EVENTS if not w.stats[k]]
    assert not missing, missing
    assert c["K"] == 12 and c["S"] == 64 and len(c["mp_bad"]) == 256


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
NEW = ("fb_covis_fuse_targets_dev", "fb_covis_fuse_targets", "fb_covis_search_in_neighbors_dev", "fb_covis_search_in_neighbors",
       "fb_covis_reserve_search_in_neighbors")


def test_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fishbird.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name + " is not declared"
        assert hasattr(lib(), name), name + " is not exported"
        assert name in cabi.EXPORTS


def host_call():
    d = SC.add_at_empty()
    c = d["c"]
    keys = ("kf_n", "kf_mp", "kf_octave", "mp_bad", "obs_mp", "obs_kf", "obs_idx", "kf_order")
    h = {k: np.ascontiguousarray(c[k]).copy() for k in keys + ("kf_bad", "kf_desc", "mp_desc", "mp_found", "mp_visible", "kf_Tcw", "mp_xw", "mp_normal",
                                                               "mp_min_dist", "mp_max_dist", "mp_ref_kf")}
    n_mp = len(c["mp_bad"])
    h["mp_replaced"] = np.full(n_mp, -1, np.int32)
    hm = cabi.fill(cabi.CovisMap(), max_keyframes=c["K"], kp_stride=c["S"], n_mp=n_mp, n_obs=len(c["obs_kf"]), **{k: h[k] for k in keys})
    o = dict(d_n_fused=np.zeros(2, np.int32), d_n_candidates=np.zeros(1, np.int32), d_candidates=np.zeros(4, np.int32), d_n_added=np.zeros(1, np.int32),
             d_added=np.zeros((4, 4), np.int32), d_n_counter=np.zeros(1, np.int32), d_front=np.zeros(1, np.int32), d_n_targets=np.array([1], np.int32),
             d_targets=np.array([1], np.int32), kf_keys_un=np.ascontiguousarray(c["kf_keys_un"]).view(np.uint8).reshape(-1).copy())
    fuse = cabi.fill(cabi.PointFuseArrays(), d_n_replaced=np.zeros(1, np.int32), replaced_cap=0,
                     **{k: h[k] for k in ("kf_mp", "mp_bad", "obs_mp", "obs_kf", "mp_found", "mp_visible", "mp_replaced", "kf_bad", "kf_desc", "mp_desc")})
    a = cabi.fill(cabi.SearchInNeighborsArgs(), cur_slot=0, n_features=2, n_targets=1, th=3.0, n_levels=8, obs_cap=len(h["obs_kf"]), obs_idx=h["obs_idx"],
                  new_edge_cap=0, cand_cap=4, added_cap=4, **{k: h[k] for k in ("kf_Tcw", "mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_ref_kf")},
                  **o)
    a.grid.cols, a.grid.rows = 64, 48
    a.map = fuse
    return hm, a, (h, o, fuse)


def test_refusals_come_before_any_device_work():
    """every one of these returns from the argument checks: the same answer with and without a device"""
    L = lib()
    g = C.c_void_p()
    assert L.fb_covis_create(3, C.byref(g)) == 0
    bad, n, t = np.zeros(3, np.uint8), np.zeros(1, np.int32), np.zeros(8, np.int32)
    p = lambda x: C.c_void_p(x.ctypes.data)
    for slot in (-1, 3):
        assert L.fb_covis_fuse_targets(g, slot, 20, 5, p(bad), 8, p(n), p(t)) == cabi.FB_ERR_ARG
        assert L.fb_covis_fuse_targets_dev(g, slot, 20, 5, p(bad), 8, p(n), p(t), None) == cabi.FB_ERR_ARG
    hm, a, keep = host_call()
    a.new_edge_cap = 1                                                                                 # n_obs + 1 > obs_cap
    assert L.fb_covis_search_in_neighbors(g, C.byref(hm), C.byref(a)) == cabi.FB_ERR_CAPACITY
    assert L.fb_covis_search_in_neighbors_dev(g, C.byref(hm), C.byref(a), None) == cabi.FB_ERR_CAPACITY
    assert b"obs_cap" in L.fb_last_error()
    a.new_edge_cap = 0
    for field, value in (("cur_slot", 3), ("cur_slot", -1), ("n_features", 5), ("n_targets", 4097), ("cand_cap", -1)):
        old = getattr(a, field)
        setattr(a, field, value)
        assert L.fb_covis_search_in_neighbors(g, C.byref(hm), C.byref(a)) == cabi.FB_ERR_ARG, field
        setattr(a, field, old)
    assert L.fb_covis_reserve_search_in_neighbors(g, 10, 10, 10, 0, 1, 1, 1) == cabi.FB_ERR_ARG
    L.fb_covis_destroy(g)
