"""MapPoint::Replace, the loop fusion and SearchAndFuse: the calls are declared and exported, and the literal model (tests/loop_fuse_ref.py)
gives the answers written out here on the hand cases of loop_fuse_cases.py.  No GPU."""
import os
import re

import numpy as np

import loop_fuse_cases as LC
import loop_fuse_ref as LR
from fishbirdeyevisualslam_amd import cabi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "fishbird.h")
CALLS = ("fb_covis_replace_points_dev", "fb_covis_replace_points", "fb_covis_reserve_replace_points", "fb_covis_loop_fuse_dev",
         "fb_covis_loop_fuse", "fb_covis_reserve_loop_fuse")


def run(case):
    c, op = case
    w = LR.World(c)
    if op[0] == "replace":
        LR.replace_points(w, op[1], op[2])
    else:
        LR.loop_fuse(w, op[1], len(op[2]), op[2])
    return c, w


def test_the_calls_are_declared_and_exported():
    text = open(HEADER).read()
    for name in CALLS:
        assert re.search(r"\bint %s\(fb_covis \*g" % name, text), name
        assert name in cabi.EXPORTS, name
    assert re.search(r"float \*d_set_Scw;[^\n]*\n\} fb_correct_loop_args;", text)                   # the last member
    assert cabi.CorrectLoopArgs._fields_[-1][0] == "d_set_Scw"


def test_to_already_observed_by_the_key_frame():
    c, w = run(LC.to_already_observed())
    assert w.kf_mp[0, 0] == 1 and w.kf_mp[1, 1] == -1 and w.kf_mp[1, 2] == 1                        # moved; nulled; to's own stays
    assert w.live_edges() == [(1, 0, 0), (1, 1, 2), (1, 2, 0)]
    assert w.mp_bad.tolist() == [1, 0] and w.replaced.tolist() == [1, -1]
    assert w.found.tolist() == [1, 3] and w.visible.tolist() == [10, 30]
    # to's observers are now (kf 0, 0), (kf 1, 2), (kf 2, 0); the model picked one of their descriptors
    assert any(np.array_equal(w.desc[1], c["kf_desc"][k, i]) for k, i in ((0, 0), (1, 2), (2, 0)))
    assert np.all(w.desc[0] == 0xAB)
    assert w.replaced_rows == [(0, 1)] and w.stats["moved"] == 1 and w.stats["dropped"] == 1


def test_the_same_from_in_two_pairs():
    c, w = run(LC.same_from_twice())
    assert w.live_edges() == [(1, 0, 0), (1, 1, 0), (2, 2, 0)]                                        # the second pair found no edges
    assert w.replaced.tolist() == [2, -1, -1]
    assert w.found.tolist() == [1, 2 + 1, 3 + 1] and w.visible.tolist() == [10, 30, 40]             # added twice
    assert w.replaced_rows == [(0, 1), (0, 2)] and w.stats["again"] == 1
    assert np.array_equal(w.desc[2], c["kf_desc"][2, 0])                                              # refreshed from its one observer


def test_from_equal_to_does_nothing():
    c, w = run(LC.from_is_to())
    assert w.mp_bad.tolist() == [0, 0] and w.replaced.tolist() == [-1, -1] and w.replaced_rows == []
    assert w.found.tolist() == [1, 2] and np.all(w.desc == 0xAB) and w.errors == 0
    assert np.array_equal(w.kf_mp, c["kf_mp"])


def test_a_chain():
    c, w = run(LC.chain())
    # a's slots: key frame 0 -> c; key frame 1, where c was already -> NULL.  b's own slot in key frame 2 -> c
    assert w.kf_mp[0, 0] == 2 and w.kf_mp[1, 0] == -1 and w.kf_mp[2, 0] == 2 and w.kf_mp[1, 1] == 2 and w.kf_mp[3, 0] == 2
    assert w.live_edges() == [(2, 0, 0), (2, 1, 1), (2, 2, 0), (2, 3, 0)]
    assert w.mp_bad.tolist() == [1, 1, 0] and w.replaced.tolist() == [1, 2, -1]
    assert w.found.tolist() == [1, 3, 6]
    # b was refreshed from (kf 0, 0), (kf 1, 0), (kf 2, 0) before it went bad, and keeps that descriptor
    assert any(np.array_equal(w.desc[1], c["kf_desc"][k, 0]) for k in (0, 1, 2))


def test_out_of_range_pairs_are_counted():
    c, w = run(LC.out_of_range())
    assert w.errors == 3 and w.replaced_rows == [(1, 0)]


def test_loop_fusion_with_the_loop_point_in_cur_already():
    c, w = run(LC.loop_point_already_in_cur())
    assert w.kf_mp[2].tolist() == [0, 1, 0, 1]                                                        # written at every matched feature
    assert w.added_rows == [(2, 1, 1, 3)] and w.stats["early_return"] == 2                          # one new edge, at index n_obs = 3
    assert w.live_edges() == [(0, 0, 0), (0, 2, 2), (1, 1, 0), (1, 2, 1)]
    assert w.obs_kf.tolist() == [0, 2, 1, 2, -1, -1, -1]                                              # packed, the rest tombstones
    assert w.mp_bad.tolist() == [0, 0] and w.replaced_rows == []


def test_loop_fusion_replaces_and_adds():
    c, w = run(LC.loop_replace_and_add())
    assert w.replaced_rows == [(0, 2), (1, 2)] and w.added_rows == [(1, 3, 1, 6)]                  # six edges came in
    assert w.kf_mp[1].tolist() == [2, 3, -1, -1] and w.kf_mp[0].tolist() == [2, -1, -1, -1] and w.kf_mp[2].tolist() == [3, 2, -1, -1]
    assert w.kf_mp[0, 1] == -1                                                                        # 0's slot in key frame 0, where 2 was
    assert w.mp_bad.tolist() == [1, 1, 0, 0]


def test_loop_fusion_with_the_wrong_feature_count_does_nothing():
    c, w = run(LC.loop_wrong_n())
    assert w.errors == 1 and np.array_equal(w.kf_mp, c["kf_mp"]) and w.added_rows == [] and np.all(w.obs_kf[-4:] == -1)


def test_the_generated_cases_exercise_every_branch():
    _, w = run(LC.generated_replace())
    assert w.stats["moved"] > 0 and w.stats["dropped"] > 0 and w.stats["again"] > 0 and w.errors == 2
    _, w = run(LC.generated_loop_fuse())
    assert len(w.added_rows) > 0 and len(w.replaced_rows) > 0 and w.stats["early_return"] > 0 and w.stats["dropped"] > 0
    assert w.errors == 1
    _, w = run(LC.more_than_a_wave())
    assert w.stats["moved"] > 64 and w.stats["dropped"] > 0


def test_to_cv_mat_casts_once():
    import map_correct_ref as MCR
    S = MCR.Sim3([0.0, 0.0, 0.0, 1.0], [1.0, 2.0, 3.0], 1.0 / 3.0)
    m = LR.to_cv_mat(S)
    assert m.dtype == np.float32 and m[0] == np.float32(1.0 / 3.0) and m[3] == 1.0 and m[1] == 0.0


def test_search_and_fuse_is_declared_and_exported():
    text = open(HEADER).read()
    for name in ("fb_covis_search_and_fuse_dev", "fb_covis_search_and_fuse", "fb_covis_reserve_search_and_fuse"):
        assert re.search(r"\bint %s\(fb_covis \*g" % name, text), name
        assert name in cabi.EXPORTS, name


def test_the_generated_scene_has_every_event_of_search_and_fuse():
    c, slots, scw, loop = LC.search_and_fuse_scene()
    w = LR.World(c)
    n_fused = LR.search_and_fuse(w, c, slots, scw, loop)
    print(n_fused, w.stats)
    assert min(n_fused) > 0 and sum(n_fused) == w.stats["add"] + w.stats["rep"] + w.stats["in_kf_bad"]
    assert w.stats["add"] > 0 and w.stats["rep"] > 0 and w.stats["collision"] > 0 and w.stats["in_kf_bad"] > 0
    assert w.stats["skipped_bad"] > 0                                                                  # made bad by an earlier key frame
    assert len(w.added_rows) > 0 and len(w.replaced_rows) == w.stats["rep"]


def _flat_search(table):
    """a search that returns what the test says: {(slot): [bestIdx per loop point]}"""
    return lambda w, c, slot, scw, loop_mp, valid, th: [b if v else -1 for b, v in zip(table[slot], valid)]


def test_two_loop_points_win_one_empty_feature():
    # key frame 1 feature 0 is empty; loop points 0 and 1 both get it: 0 adds, 1 replaces 0.  At key frame 2, 0 is bad: skipped.
    c = LC.described(LC.counted(LC.tiny(3, 4, [{0: 0}, {0: 1}, {2: 3}])))
    w = LR.World(c)
    n_fused = LR.search_and_fuse(w, c, [1, 2], np.zeros((2, 12), np.float32), [0, 1], search=_flat_search({1: [0, 0], 2: [1, 1]}))
    assert n_fused == [2, 1] and w.added_rows == [(1, 0, 0, 3), (2, 1, 1, 7)] and w.replaced_rows == [(0, 1)]
    assert w.kf_mp[1].tolist() == [1, -1, -1, -1] and w.kf_mp[2].tolist() == [-1, 1, -1, 2] and w.kf_mp[0].tolist() == [-1, 1, -1, -1]
    assert w.mp_bad.tolist() == [1, 0, 0] and w.stats["skipped_bad"] == 1 and w.stats["collision"] == 1
    # 1's descriptor was refreshed from its observers after the Replace: what key frame 2's search reads is the new one
    assert any(np.array_equal(w.desc[1], c["kf_desc"][k, i]) for k, i in ((0, 1), (1, 0)))


def test_a_bad_point_in_the_key_frame_counts_and_does_nothing_else():
    c = LC.described(LC.counted(LC.tiny(2, 2, [{0: 0}, {1: 1}])))
    c["mp_bad"][1] = 1
    w = LR.World(c)
    assert LR.search_and_fuse(w, c, [1], np.zeros((1, 12), np.float32), [0], search=_flat_search({1: [1]})) == [1]
    assert w.replaced_rows == [] and w.added_rows == [] and np.array_equal(w.kf_mp, c["kf_mp"]) and w.stats["in_kf_bad"] == 1
