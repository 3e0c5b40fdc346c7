"""The literal model of the per-point side of LocalMapping (tests/map_refresh_ref.py) on hand cases whose answers are worked
out here, against the oracle's ComputeDistinctiveDescriptors, and the declaration of the three calls.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import map_refresh_cases as MC
import map_refresh_ref as R
import oracle_lib as O
from fishbirdeyevisualslam_amd import cabi

f32 = np.float32
NEW = [p + s for p in ("fb_covis_refresh_points", "fb_covis_process_new_keyframe", "fb_covis_map_point_culling") for s in ("_dev", "")]
NEW += ["fb_covis_reserve_refresh_points", "fb_covis_reserve_process_new_keyframe", "fb_covis_reserve_map_point_culling"]


def test_the_calls_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fishbird.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in cabi.EXPORTS, name
    for struct in ("fb_point_refresh_args", "fb_new_keyframe_args", "fb_map_point_culling_args"):
        assert "} %s;" % struct in header


def test_median_tie_goes_to_the_smaller_kf_order():
    # three observers, pairwise distances 8, 8, 16: the sorted rows are [0 8 8], [0 8 16], [0 8 16], every median (index 1)
    # is 8, and `median < BestMedian` is strict: the first in std::map order wins.  That is slot 2, whose kf_order is least.
    c = MC.tiny(3, 2, [{0: 0, 1: 1, 2: 0}], kf_order=[30, 20, 10])
    c["kf_desc"][0, 0], c["kf_desc"][1, 1], c["kf_desc"][2, 0] = MC.bits(), MC.bits(*range(8)), MC.bits(*range(8, 16))
    w = R.World(c)
    R.refresh_points(w, what=R.DESCRIPTOR)
    assert np.array_equal(w.desc[0], MC.bits(*range(8, 16)))
    assert np.array_equal(w.normal, c["mp_normal"])                                                    # the other part was not asked for


def _axes_case(kf_bad):
    # the point at the origin, the centres on the negative axes at 3, 4, 5: the unit vectors are the axes, exactly
    c = MC.tiny(4, 2, [{0: 1, 1: 0, 2: 1}], centres=[[-3, 0, 0], [0, -4, 0], [0, 0, -5], [0, 0, -2]], kf_bad=kf_bad,
                octave=[[0, 2], [1, 1], [1, 1], [3, 1]])
    # slot 0's descriptor is the middle one: distances 0-1 = 4, 0-2 = 4, 1-2 = 8 -> medians 4, 4 (row [0 4 8]), 4: slot 0 first
    c["kf_desc"][0, 1], c["kf_desc"][1, 0], c["kf_desc"][2, 1] = MC.bits(0, 1, 2, 3), MC.bits(), MC.bits(*range(8))
    return c


def test_bad_key_frame_is_left_out_of_the_descriptor_but_not_of_the_normal():
    c = _axes_case(kf_bad=[0])
    w = R.World(c)
    R.refresh_points(w)
    # descriptor: slots 1 and 2 remain, N = 2, median index (int)(0.5 * 1) = 0 -> both medians 0 -> slot 1 (smaller kf_order)
    assert np.array_equal(w.desc[0], MC.bits())
    third = f32(1.0 / 3)
    assert np.array_equal(w.normal[0], np.array([third, third, third], f32))                          # (1, 1, 1) / 3, bad slot 0 included
    assert w.max_dist[0] == f32(3.0) * c["scale_factors"][2]                                           # ref = slot 0 at feature 1: octave 2
    assert w.min_dist[0] == f32(w.max_dist[0] / c["scale_factors"][3])


def test_all_observers_bad_keeps_the_descriptor():
    c = _axes_case(kf_bad=[0, 1, 2])
    w = R.World(c)
    R.refresh_points(w)
    assert np.array_equal(w.desc[0], c["mp_desc"][0])
    assert w.max_dist[0] == f32(3.0) * c["scale_factors"][2]


def test_reference_key_frame_that_is_no_observer_gives_feature_0():
    c = _axes_case(kf_bad=[])
    c["mp_ref_kf"][0] = 3                                                                              # centre (0, 0, -2), octave of feature 0 = 3
    w = R.World(c)
    R.refresh_points(w, points=[0, 0])
    assert w.max_dist[0] == f32(2.0) * c["scale_factors"][3]
    assert np.array_equal(w.desc[0], MC.bits(0, 1, 2, 3))                                              # nobody bad: slot 0, the middle descriptor


def test_bad_point_and_point_without_edges_keep_everything():
    c = _axes_case(kf_bad=[])
    c["mp_bad"][0] = 1
    w = R.World(c)
    R.refresh_points(w)
    c2 = MC.tiny(2, 2, [{}])
    w2 = R.World(c2)
    R.refresh_points(w2)
    for ww, cc in ((w, c), (w2, c2)):
        assert np.array_equal(ww.desc, cc["mp_desc"]) and np.array_equal(ww.normal, cc["mp_normal"]) and np.array_equal(ww.max_dist, cc["mp_max_dist"])


def test_model_choice_equals_the_oracle():
    g = np.random.default_rng(77)
    pool = g.integers(0, 256, (6, 32), dtype=np.uint8)
    sets = [pool[g.integers(0, 6, int(g.integers(1, 12)))] for _ in range(200)]
    start = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    desc = np.ascontiguousarray(np.concatenate(sets))
    best = np.full(200, -9, np.int32)
    assert O.lib().orc_distinctive_descriptors(C.c_void_p(start.ctypes.data), C.c_void_p(desc.ctypes.data), 200, C.c_void_p(best.ctypes.data)) == 0
    assert best.tolist() == [R.distinctive_choice(list(s)) for s in sets]


def test_culling_boundaries():
    c, lst = MC.culling_case(40)
    w = R.World(c)
    kept, culled, erased = R.map_point_culling(w, lst, MC.CUR_KF_ID, c["mp_first_kf_id"], c["mp_found"], c["mp_visible"])
    exp_kept, exp_culled = [], []
    for r in range(4):
        p = lst[10 * r:10 * r + 10].tolist()
        exp_kept += [p[2], p[3], p[5]] + ([] if r == 0 else [p[7]])                                    # 1/4 is not < 0.25; NaN compares false; age 2 with 3 observers
        exp_culled += [p[1], p[4]] + ([p[7]] if r == 0 else []) + [p[8]]                               # first id -1: age 11 with one observer
    assert kept == exp_kept and culled == exp_culled
    assert len(erased) == 4 * (2 + 2 + 2) + 1                                                          # the observers of the culled points
    for kf, mp, idx, e in erased:
        assert w.obs_kf[e] == -1 and c["obs_kf"][e] == kf and c["obs_mp"][e] == mp and w.kf_mp[kf, idx] == -1 and w.mp_bad[mp]
    assert all(not w.obs[mp] for mp in culled)


def test_process_new_keyframe_block_and_recent_list():
    c, slot, N = MC.new_keyframe_case()
    w = R.World(c)
    recent = []
    n_added = R.process_new_keyframe(w, slot, N, recent)
    base = len(c["obs_kf"])
    assert len(w.obs_kf) == base + N and w.errors == 1                                                 # the one out-of-range entry
    assert np.all(w.obs_kf[base:base + n_added] == slot) and np.all(w.obs_kf[base + n_added:] == -1)
    assert np.all(np.diff(w.obs_idx[base:base + n_added]) > 0)                                         # ascending i
    row = c["kf_mp"][slot]
    twice = [p for p in set(row[:N].tolist()) if 0 <= p < 150 and not c["mp_bad"][p] and (row[:N] == p).sum() == 2]
    assert len(twice) == 1 and recent.count(twice[0]) == 1 and twice[0] in w.obs_mp[base:base + n_added]
    w2 = R.World(c)
    assert R.process_new_keyframe(w2, slot, N - 1, []) == 0 and np.all(w2.obs_kf[base:] == -1) and w2.errors == 1
    assert np.array_equal(w2.desc, c["mp_desc"])
