"""The covisibility graph (fb_covis_*) without a device: hand-computed known answers of the literal model tests/covis_ref.py
(one per quirk of the reference), the C-ABI mirror, and the no-device / bad-argument answers of the new entry points."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import covis_ref as R
from fishbirdeyevisualslam_amd import cabi, covis_problem as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_FIELDS = ("kf_n", "kf_mp", "kf_octave", "mp_bad", "obs_mp", "obs_kf", "obs_idx", "kf_order")


def ref_map(arr):
    return R.Map(*[arr[k] for k in MAP_FIELDS])


def small(pairs, K=6, S=40, order=None, dup=None):
    """pairs: [(n, [kfs], [octaves] or None)]; dup: (pair index, point index, kf) held at a second feature"""
    b = P.MapBuilder(K, S, 0)
    made = [b.shared(n, kfs, octs) for n, kfs, octs in pairs]
    if dup:
        b.hold_again(made[dup[0]][dup[1]], dup[2])
    order = list(range(100, 100 + K)) if order is None else order
    return b.arrays(order, shuffle=False), made


def test_threshold_14_15_16_and_what_follows_from_the_kept_row():
    arr, _ = small([(14, [0, 1], None), (15, [0, 2], None), (16, [0, 3], None)], S=48)
    m, g = ref_map(arr), R.Graph(6, arr["kf_order"])
    assert g.update_connections(m, 0) == (3, 3)
    assert g.weights[0] == {1: 14, 2: 15, 3: 16}                       # the row keeps the entry below the threshold
    assert (g.ordered[0], g.ordered_w[0]) == ([3, 2], [16, 15])        # ... the ordered vector does not
    assert g.weights[1] == {} and g.weights[2] == {0: 15} and g.weights[3] == {0: 16}
    assert g.get_best_covisibility_keyframes(0, 1) == [3] and g.get_weight(0, 1) == 14 and g.get_weight(1, 0) == 0
    assert g.get_connected_keyframes(0) == [1, 2, 3]
    # GetCovisiblesByWeight: the prefix >= w, and EMPTY when every weight is >= w (upper_bound == end())
    assert g.get_covisibles_by_weight(0, 16) == [3]
    assert g.get_covisibles_by_weight(0, 15) == [] and g.get_covisibles_by_weight(0, 1) == []
    assert g.get_covisibles_by_weight(0, 17) == [] and g.get_covisibles_by_weight(4, 1) == []
    # AddConnection with the weight that is there: the ordered vector is left alone
    g.add_connection(0, 3, 16)
    assert g.ordered[0] == [3, 2]
    # a changed weight re-sorts from the whole row: the kept entry of 14 becomes a member
    g.add_connection(0, 3, 17)
    assert (g.ordered[0], g.ordered_w[0]) == ([3, 2, 1], [17, 15, 14])
    g.erase_connection(0, 5)                                            # no such entry: nothing
    assert g.ordered[0] == [3, 2, 1]
    g.erase_connection(0, 2)
    assert g.ordered[0] == [3, 1] and g.weights[0] == {1: 14, 3: 17}


def test_ties_smallest_order_is_pkfmax_largest_order_leads_the_vector():
    order = [100, 500, 300, 400, 200, 600]
    arr, _ = small([(7, [0, 1], None), (7, [0, 2], None), (3, [0, 3], None), (15, [4, 1], None), (15, [4, 2], None)], order=order)
    m, g = ref_map(arr), R.Graph(6, order)
    assert g.update_connections(m, 0) == (3, 2)                         # strict > in ascending order: slot 2 (300) beats slot 1 (500)
    assert g.ordered[0] == [2] and g.weights[0] == {1: 7, 2: 7, 3: 3}
    assert g.weights[2] == {0: 7} and g.weights[1] == {}
    assert g.update_connections(m, 4) == (2, 1)                         # sort + push_front: the larger pointer first
    assert (g.ordered[4], g.ordered_w[4]) == ([1, 2], [15, 15])
    assert g.get_connected_keyframes(4) == [2, 1]                       # std::set order
    g.erase_keyframe(4)
    assert g.weights[4] == {} and g.ordered[4] == [] and g.weights[1] == {} and g.weights[2] == {0: 7}


def test_empty_counter_leaves_the_graph_untouched():
    arr, _ = small([(15, [0, 1], None), (2, [2, 3], None)])
    arr["mp_bad"][15:] = 1                                              # the only points of slot 2 are bad
    m, g = ref_map(arr), R.Graph(6, arr["kf_order"])
    g.add_connection(2, 0, 5)
    before = ([dict(w) for w in g.weights], [list(o) for o in g.ordered])
    assert g.update_connections(m, 2) == (0, 0) and g.update_connections(m, 5) == (0, -1)
    assert ([dict(w) for w in g.weights], [list(o) for o in g.ordered]) == before


def test_a_point_held_at_two_features_counts_twice_and_makes_the_call_order_matter():
    arr, _ = small([(15, [0, 1], None)], dup=(0, 3, 0))
    m = ref_map(arr)
    g = R.Graph(6, arr["kf_order"])
    assert g.update_connections(m, 0) == (1, 1) and g.weights[0] == {1: 16} and g.weights[1] == {0: 16}
    assert g.update_connections(m, 1) == (1, 0) and g.weights[1] == {0: 15} and g.weights[0] == {1: 15}
    g2 = R.Graph(6, arr["kf_order"])
    g2.update_connections(m, 1)
    g2.update_connections(m, 0)
    assert g2.weights[0] == {1: 16} and g2.weights[1] == {0: 16}


def culling_map(not_erase=None):
    # cur 0; X1 = 1: 20 redundant points + 2 points of 3 observations shared with X2 = 2, which has 10 redundant points
    arr, made = small([(20, [1, 3, 4, 5], None), (10, [2, 3, 4, 5], None), (2, [1, 2, 3], None)], S=40)
    m, g = ref_map(arr), R.Graph(6, arr["kf_order"])
    g.add_connection(0, 1, 20)
    g.add_connection(0, 2, 18)
    return arr, made, m, g


def test_culling_first_removal_turns_points_bad_and_flips_the_second_decision():
    arr, made, m, g = culling_map()
    r = R.keyframe_culling(g, m, 0)
    assert r["slots"] == [1, 2] and r["n_redundant"] == [20, 10] and r["n_mps"] == [22, 10] and r["culled"] == [1, 1]
    assert np.nonzero(r["mp_bad_after"])[0].tolist() == made[2]
    r0 = R.keyframe_culling(g, m, 0, apply_effects=False)
    assert r0["n_mps"] == [22, 12] and r0["culled"] == [1, 0]           # 10 > 0.9 * 12 is false
    assert not arr["mp_bad"].any() and g.ordered[0] == [1, 2]           # neither the map nor the graph changed
    rid = R.keyframe_culling(g, m, 0, id0=1)
    assert rid["culled"] == [0, 0] and rid["n_mps"] == [0, 12]         # mnId == 0 is skipped


def test_culling_not_erase_suppresses_the_effects():
    arr, made, m, g = culling_map()
    ne = np.zeros(6, np.uint8)
    ne[1] = 1
    r = R.keyframe_culling(g, m, 0, not_erase=ne)
    assert r["culled"] == [1, 0] and r["n_mps"] == [22, 12] and not r["mp_bad_after"].any()


def test_culling_boundary_nine_of_ten_is_not_more_than_ninety_percent():
    arr, _ = small([(9, [1, 3, 4, 5], None), (1, [1], None), (10, [2, 3, 4, 5], None)], S=40)
    m, g = ref_map(arr), R.Graph(6, arr["kf_order"])
    g.add_connection(0, 1, 20)
    g.add_connection(0, 2, 18)
    r = R.keyframe_culling(g, m, 0)
    assert r["n_redundant"] == [9, 10] and r["n_mps"] == [10, 10] and r["culled"] == [0, 1]


def test_culling_counts_only_observations_at_the_same_or_a_finer_scale():
    # the point's feature in slot 1 is at octave 2: others at octave <= 3 count; one of the three is at octave 4
    arr, _ = small([(1, [1, 3, 4, 5], [2, 3, 3, 4]), (1, [1, 3, 4, 5], [2, 0, 3, 3])], S=40)
    m, g = ref_map(arr), R.Graph(6, arr["kf_order"])
    g.add_connection(0, 1, 20)
    r = R.keyframe_culling(g, m, 0)
    assert r["n_redundant"] == [1] and r["n_mps"] == [2] and r["culled"] == [0]


def test_planted_problem_has_what_the_gpu_tests_rely_on():
    p = P.make_covis_problem(1)
    assert p["kf_n"].max() == p["S"] and (p["kf_n"] == 0).sum() >= 3 and p["mp_bad"].sum() >= 5
    live = p["obs_kf"] >= 0
    assert 0.08 < (~live).mean() < 0.12 and 2000 < live.sum() < 3500
    assert len(set(int(x) for x in p["kf_order"][p["used"]])) == len(p["used"])
    m, g = ref_map(p), R.Graph(p["K"], p["kf_order"])
    for a in p["batch"]:
        g.update_connections(m, a)
    assert sorted(g.weights[0].values()) == [14, 15, 15, 16] and len(g.ordered[0]) == 4   # E2's update re-sorted E0's whole row
    g2 = R.Graph(p["K"], p["kf_order"])
    for a in reversed(p["batch"]):
        g2.update_connections(m, a)
    assert g2.weights != g.weights                                      # the batch is order-sensitive
    for a in p["used"]:
        g.update_connections(m, a)
    r, r0 = R.keyframe_culling(g, m, p["cur"]), R.keyframe_culling(g, m, p["cur"], apply_effects=False)
    at = [r["slots"].index(x) for x in p["X"]]
    assert at == sorted(at)
    assert [r["culled"][i] for i in at] == [1, 1, 1, 0] and [r0["culled"][i] for i in at] == [1, 0, 0, 1]


def test_struct_layout_matches_the_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fishbird.h"\nint main(void){printf("%zu %zu %zu %zu %d %d\\n", '
           'sizeof(fb_covis_map), offsetof(fb_covis_map, n_mp), offsetof(fb_covis_map, obs_mp), offsetof(fb_covis_map, kf_order), '
           'FB_COVIS_MAX_STRIDE, FB_COVIS_TH);return 0;}\n')
    d = tempfile.mkdtemp()
    open(os.path.join(d, "s.c"), "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
    got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    M = cabi.CovisMap
    assert got == [C.sizeof(M), M.n_mp.offset, M.obs_mp.offset, M.kf_order.offset, cabi.FB_COVIS_MAX_STRIDE, cabi.FB_COVIS_TH]
    assert R.TH == cabi.FB_COVIS_TH


def _host_map(arr):
    m = cabi.CovisMap()
    keep = {k: np.ascontiguousarray(arr[k]) for k in MAP_FIELDS}
    cabi.fill(m, max_keyframes=keep["kf_mp"].shape[0], kp_stride=keep["kf_mp"].shape[1], n_mp=len(keep["mp_bad"]),
              n_obs=len(keep["obs_kf"]), **keep)
    return m, keep


def test_no_device_no_answer():
    import fishbirdeyevisualslam_amd as fb
    L = fb.lib()
    arr, _ = small([(15, [0, 1], None), (16, [0, 2], None)])
    m, keep = _host_map(arr)
    h = C.c_void_p()
    assert L.fb_covis_create(6, C.byref(h)) == cabi.FB_OK               # host only
    K = 6
    vp = lambda x: C.c_void_p(x.ctypes.data)
    i32 = lambda n: np.zeros(n, np.int32)
    slots, ncnt, front, n, out, w = np.array([0], np.int32), i32(1), i32(1), i32(1), i32(K), i32(K)
    nred, nmps, culled, bad, rows = i32(K), i32(K), np.zeros(K, np.uint8), np.zeros(31, np.uint8), np.full((K, 10), -1, np.int32)
    cnt = C.c_int32(-1)
    host = [L.fb_covis_update_connections(h, C.byref(m), 1, vp(slots), vp(ncnt), vp(front)),
            L.fb_covis_ordered(h, 0, vp(n), vp(out), vp(w)), L.fb_covis_by_weight(h, 0, 16, vp(n), vp(out)),
            L.fb_covis_connected(h, 0, vp(n), vp(out)), L.fb_covis_weight(h, 0, 2, vp(w)),
            L.fb_covis_kfdb_rows(h, 0, None, vp(rows)),
            L.fb_covis_keyframe_culling(h, C.byref(m), 0, -1, None, vp(n), vp(out), vp(nred), vp(nmps), vp(culled), vp(bad)),
            L.fb_covis_error_count(h, C.byref(cnt), None), L.fb_covis_reserve(h, 31, 62, 1), L.fb_covis_clear(h, None)]
    if L.fb_device_count() > 0:
        assert host == [0] * len(host) and front[0] == 2 and w[0] == 16 and rows[0, :3].tolist() == [2, 1, -1] and cnt.value == 0
    else:
        assert host == [cabi.FB_ERR_NODEVICE] * len(host)
        assert b"no CPU fallback" in L.fb_last_error()
        # the _dev entry points: the arguments would be device pointers; without a device they are never looked at
        dev = [L.fb_covis_update_connections_dev(h, C.byref(m), 1, vp(slots), vp(ncnt), vp(front), None),
               L.fb_covis_set_order_dev(h, vp(keep["kf_order"]), None), L.fb_covis_add_connection_dev(h, 0, 1, 3, None),
               L.fb_covis_erase_connection_dev(h, 0, 1, None), L.fb_covis_erase_keyframe_dev(h, 0, None),
               L.fb_covis_ordered_dev(h, 0, vp(n), vp(out), vp(w), None), L.fb_covis_by_weight_dev(h, 0, 1, vp(n), vp(out), None),
               L.fb_covis_connected_dev(h, 0, vp(n), vp(out), None), L.fb_covis_weight_dev(h, 0, 1, vp(w), None),
               L.fb_covis_kfdb_rows_dev(h, 0, None, vp(rows), None),
               L.fb_covis_keyframe_culling_dev(h, C.byref(m), 0, -1, None, vp(n), vp(out), vp(nred), vp(nmps), vp(culled), vp(bad), None)]
        assert dev == [cabi.FB_ERR_NODEVICE] * len(dev)
    assert L.fb_covis_destroy(h) == 0 and L.fb_covis_destroy(None) == 0


def test_bad_arguments_are_refused_before_any_device_work():
    import fishbirdeyevisualslam_amd as fb
    L = fb.lib()
    E = cabi.FB_ERR_ARG
    h = C.c_void_p()
    assert L.fb_covis_create(0, C.byref(h)) == E and L.fb_covis_create(cabi.FB_KFDB_MAX_KEYFRAMES + 1, C.byref(h)) == E
    assert L.fb_covis_create(6, None) == E
    assert L.fb_covis_create(6, C.byref(h)) == 0
    arr, _ = small([(15, [0, 1], None)])
    vp = lambda x: C.c_void_p(x.ctypes.data)
    a = np.zeros(8, np.int32)
    b8 = np.zeros(64, np.uint8)

    def upd(**change):
        m, keep = _host_map(arr)
        for k, v in change.items():
            setattr(m, k, v)
        return (L.fb_covis_update_connections_dev(h, C.byref(m), 1, vp(a), vp(a), vp(a), None),
                L.fb_covis_update_connections(h, C.byref(m), 1, vp(a), vp(a), vp(a)),
                L.fb_covis_keyframe_culling_dev(h, C.byref(m), 0, -1, None, vp(a), vp(a), vp(a), vp(a), vp(b8), vp(b8), None),
                L.fb_covis_keyframe_culling(h, C.byref(m), 0, -1, None, vp(a), vp(a), vp(a), vp(a), vp(b8), vp(b8)))
    for change in (dict(max_keyframes=5), dict(kp_stride=0), dict(kp_stride=cabi.FB_COVIS_MAX_STRIDE + 1), dict(n_mp=-1), dict(n_obs=-1),
                   dict(kf_n=None), dict(kf_mp=None), dict(kf_octave=None), dict(kf_order=None), dict(mp_bad=None), dict(obs_kf=None),
                   dict(obs_mp=None), dict(obs_idx=None)):
        assert upd(**change) == (E, E, E, E), change
    m, keep = _host_map(arr)
    assert L.fb_covis_update_connections_dev(h, None, 1, vp(a), vp(a), vp(a), None) == E
    assert L.fb_covis_update_connections_dev(h, C.byref(m), 7, vp(a), vp(a), vp(a), None) == E
    assert L.fb_covis_update_connections_dev(h, C.byref(m), -1, vp(a), vp(a), vp(a), None) == E
    assert L.fb_covis_update_connections_dev(h, C.byref(m), 1, None, vp(a), vp(a), None) == E
    assert L.fb_covis_update_connections_dev(None, C.byref(m), 1, vp(a), vp(a), vp(a), None) == E
    assert L.fb_covis_keyframe_culling_dev(h, C.byref(m), 6, -1, None, vp(a), vp(a), vp(a), vp(a), vp(b8), vp(b8), None) == E
    assert L.fb_covis_keyframe_culling_dev(h, C.byref(m), 0, 6, None, vp(a), vp(a), vp(a), vp(a), vp(b8), vp(b8), None) == E
    assert L.fb_covis_keyframe_culling_dev(h, C.byref(m), 0, -1, None, vp(a), vp(a), vp(a), vp(a), vp(b8), None, None) == E
    assert L.fb_covis_add_connection_dev(h, 0, 6, 3, None) == E and L.fb_covis_add_connection_dev(h, -1, 1, 3, None) == E
    assert L.fb_covis_add_connection_dev(h, 0, 1, 0, None) == E and L.fb_covis_add_connection_dev(h, 0, 0, 3, None) == E
    assert L.fb_covis_add_connection_dev(h, 0, 1, cabi.FB_COVIS_MAX_STRIDE + 1, None) == E
    assert L.fb_covis_erase_connection_dev(h, 0, 6, None) == E and L.fb_covis_erase_keyframe_dev(h, 6, None) == E
    assert L.fb_covis_ordered_dev(h, 6, vp(a), vp(a), None, None) == E and L.fb_covis_ordered_dev(h, 0, None, vp(a), None, None) == E
    assert L.fb_covis_ordered(h, 0, vp(a), None, None) == E and L.fb_covis_by_weight(h, -1, 1, vp(a), vp(a)) == E
    assert L.fb_covis_connected_dev(h, 0, vp(a), None, None) == E and L.fb_covis_connected(h, 6, vp(a), vp(a)) == E
    assert L.fb_covis_weight_dev(h, 0, 6, vp(a), None) == E and L.fb_covis_weight(h, 0, 1, None) == E
    assert L.fb_covis_kfdb_rows_dev(h, 7, vp(a), vp(a), None) == E and L.fb_covis_kfdb_rows(h, 0, None, None) == E
    assert L.fb_covis_set_order_dev(h, None, None) == E and L.fb_covis_error_count(h, None, None) == E
    assert L.fb_covis_reserve(h, -1, 0, 0) == E and L.fb_covis_clear(None, None) == E
    assert b"bad argument" in L.fb_last_error()
    L.fb_covis_destroy(h)
