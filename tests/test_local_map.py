"""The spanning tree and Tracking::UpdateLocalMap without a device: hand-computed known answers of the literal model
tests/local_map_ref.py (one per quirk of the reference), the C-ABI mirror, and the no-device answers of the new entry points."""
import ctypes as C
import os
import subprocess

import numpy as np

import covis_ref as R
import local_map_cases as LC
import local_map_ref as LR
from fishbirdeyevisualslam_amd import cabi
from test_covis import _host_map, ref_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model_of(case):
    g = R.Graph(case["K"], case["order"])
    for a, b, w in case["conns"]:
        g.add_connection(a, b, w)
    t = LR.Tree(g)
    for c, p in case["parents"]:
        t.change_parent(c, p)
    return g, t, ref_map(case["arr"])


def run_model(case, **caps):
    g, t, m = model_of(case)
    mp = list(case["frame"])
    out = LR.update_local_map(t, m, len(mp), mp, case["kf_bad"], case["local_in"], case["ref_in"], **caps)
    out["map_point"] = mp
    return out


def test_update_local_map_known_answers():
    cases = LC.local_map_cases()
    assert len(cases) >= 8
    for name, case in cases.items():
        assert case["K"] <= 8 or name == "bad_neighbours_occupy_places"          # (ten places need more than eight key frames)
        out = run_model(case)
        for k, v in case["want"].items():
            assert out[k] == v, (name, k, out[k], v)
        assert out["n_local_kf"] == len(out["local_kf"]) and out["overflow"] == 0 and out["errors"] == 0, name


def test_the_81st_key_frame_ends_the_expansion():
    case = LC.expansion_limit_case()
    out = run_model(case)
    assert out["local_kf"] == case["want"]["local_kf"] and out["n_local_kf"] == 82 and out["ref_kf"] == 0
    out = run_model(LC.expansion_limit_case(81))                                    # 81 voters: the first test already fails
    assert out["local_kf"] == list(range(81))
    out = run_model(case, cap_kf=81, cap_mp=79)                                     # capacities: the prefix, the full lengths, the flag
    assert out["local_kf"] == case["want"]["local_kf"][:81] and out["n_local_kf"] == 82 and out["overflow"] == 1
    assert out["local_mp"] == list(range(79)) and out["n_local_mp"] == 80          # key frame 100 fitted and has no points; 125 did not fit


def _tree(K=8, order=None):
    g = R.Graph(K, order)
    return g, LR.Tree(g)


def test_first_connection_and_the_now_state4_search():
    from test_covis import small
    arr, _ = small([(15, [0, 1], None), (16, [0, 2], None), (2, [3, 4], None)], K=8)
    m = ref_map(arr)
    fid = [50, 10, 90, 0, 70, 30, 0, 0]
    in_map = [1, 1, 1, 1, 1, 0, 0, 0]
    g, t = _tree(8, arr["kf_order"])
    assert t.update_connections(m, 0) == (2, 2) and t.parent[0] == 2 and not t.first[0] and t.get_childs(2) == [0]
    assert t.update_connections(m, 5) == (0, -1) and t.first[5] and t.parent[5] == -1     # empty counter: mbFirstConnection stays
    assert t.update_connections(m, 1, id0=1) == (1, 0) and t.first[1] and t.parent[1] == -1   # mnId == 0
    t.change_parent(0, 1)                                                                    # a later update does not touch the parent
    assert t.update_connections(m, 0) == (2, 2) and t.parent[0] == 1
    # nowState == 4: the front (slot 2, frame 90) is newer than slot 0 (frame 50): the newest older key frame of the map is
    # slot 1 (frame 10); slot 5 (frame 30) is not in the map, slot 3 (frame 0) can never win
    g, t = _tree(8, arr["kf_order"])
    t.update_connections(m, 0, now_state4=True, frame_id=fid, in_map=in_map)
    assert t.parent[0] == 1 and t.get_childs(1) == [0]
    # nothing qualifies (only frame 0 and newer ones are in the map): the front stays
    g, t = _tree(8, arr["kf_order"])
    t.update_connections(m, 0, now_state4=True, frame_id=fid, in_map=[1, 0, 1, 1, 1, 0, 0, 0])
    assert t.parent[0] == 2
    # the front is older: no search
    g, t = _tree(8, arr["kf_order"])
    t.update_connections(m, 2, now_state4=True, frame_id=fid, in_map=in_map)
    assert t.parent[2] == 0
    # slot 3 (frame 0) looks at front 4 (frame 70): nothing lies strictly between 0 and 0
    g, t = _tree(8, arr["kf_order"])
    t.update_connections(m, 3, now_state4=True, frame_id=fid, in_map=in_map)
    assert t.parent[3] == 4


def set_bad_case():
    """slot 1 (parent 0) goes bad; its children are 2, 3, 4, 5, 6 (6 is bad).  3 and 4 both see 0 with weight 20: the tie goes to
    the first child in kf_order, which is 4 (order 130 < 140).  Then 3 (w 20 to 0), then 2 through the new candidate 4 (w 9);
    5 has no link to a candidate and falls back to 0, as does the bad 6 although it sees 0."""
    order = [100, 110, 120, 140, 130, 150, 160, 170]
    g, t = _tree(8, order)
    t.change_parent(1, 0)
    for c in (2, 3, 4, 5, 6):
        t.change_parent(c, 1)
    for a, b, w in ((3, 0, 20), (4, 0, 20), (2, 4, 9), (2, 1, 30), (6, 0, 50), (5, 7, 40)):
        g.add_connection(a, b, w)
    bad = np.zeros(8, np.uint8)
    bad[6] = 1
    return g, t, bad


def test_set_bad_flag_tie_order_fallback_and_the_kept_parent():
    g, t, bad = set_bad_case()
    seen = []
    orig = t.change_parent
    t.change_parent = lambda c, p: (seen.append((c, p)), orig(c, p))[1]
    t.set_bad_flag(1, bad)
    assert seen == [(4, 0), (3, 0), (2, 4), (5, 0), (6, 0)]
    parent, linked, first = t.state()
    assert parent.tolist() == [-1, 0, 4, 0, 0, 0, 0, -1]
    assert linked.tolist() == [0, 0, 1, 1, 1, 1, 1, 0]                                       # linked[1] cleared, parent[1] kept
    assert t.get_childs(0) == [4, 3, 5, 6] and t.get_childs(4) == [2]
    t.erase_child(0, 2)                                                                      # 2 is not a child of 0: nothing
    assert t.state()[1].tolist() == [0, 0, 1, 1, 1, 1, 1, 0]
    t.erase_child(4, 2)
    assert t.state()[1][2] == 0 and t.parent[2] == 4
    t.set_bad_flag(7, bad)                                                                   # no parent: nothing but the counter
    assert t.errors == 1 and t.state()[0].tolist() == [-1, 0, 4, 0, 0, 0, 0, -1]


def test_struct_layout_matches_the_header(tmp_path):
    A = cabi.LocalMapArgs
    names = [n for n, _ in A._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fishbird.h"\nint main(void){printf("%zu %d", sizeof(fb_local_map_args), '
           'FB_LOCAL_MAP_MAX_EXPAND);' + "".join('printf(" %%zu", offsetof(fb_local_map_args, %s));' % n for n in names) + 'return 0;}\n')
    d = str(tmp_path)
    with open(os.path.join(d, "s.c"), "w") as f:
        f.write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
    got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert got == [C.sizeof(A), cabi.FB_LOCAL_MAP_MAX_EXPAND] + [getattr(A, n).offset for n in names]
    assert LR.MAX_EXPAND == cabi.FB_LOCAL_MAP_MAX_EXPAND


def test_new_symbols_are_exported_and_give_no_answer_without_a_device():
    import fishbirdeyevisualslam_amd as fb
    L = fb.lib()
    new = ["fb_covis_tree_set_dev", "fb_covis_tree_get_dev", "fb_covis_tree_get", "fb_covis_change_parent_dev", "fb_covis_erase_child_dev",
           "fb_covis_children_dev", "fb_covis_children", "fb_covis_parent_dev", "fb_covis_first_connection_dev",
           "fb_covis_tree_erase_keyframe_dev", "fb_covis_local_map_dev", "fb_covis_local_map", "fb_covis_reserve_local_map",
           "fb_frame_update_local_map_dev", "fb_frame_track_graph_dev"]
    assert all(hasattr(L, s) for s in new) and set(new) <= set(cabi.EXPORTS)
    case = LC.local_map_cases()["parent_break"]
    m, keep = _host_map(case["arr"])
    K = case["K"]
    h = C.c_void_p()
    assert L.fb_covis_create(K, C.byref(h)) == cabi.FB_OK
    vp = lambda x: C.c_void_p(x.ctypes.data)
    i32 = lambda n, v=0: np.full(n, v, np.int32)
    t = dict(d_n=i32(1, 2), d_map_point=np.array([case["frame"]], np.int32), d_kf_bad=case["kf_bad"], d_local_kf=i32(16, -5), d_n_local_kf=i32(1),
             d_local_mp=i32(16, -5), d_n_local_mp=i32(1), d_ref_kf=i32(1, -1), d_n_voters=i32(1), d_overflow=i32(1))
    a = cabi.LocalMapArgs()
    cabi.fill(a, batch=1, kp_stride=2, cap_kf=16, cap_mp=16, **t)
    par, u8, n, out = i32(K), np.zeros(K, np.uint8), i32(1), i32(K)
    calls = [L.fb_covis_tree_get(h, vp(par), vp(u8), vp(u8.copy())), L.fb_covis_children(h, 0, vp(n), vp(out)),
             L.fb_covis_local_map(h, C.byref(m), C.byref(a)), L.fb_covis_reserve_local_map(h, 2, 2, 0, 1, 0)]
    if L.fb_device_count() > 0:
        assert calls == [0] * len(calls) and par.tolist() == [-1] * K and t["d_local_kf"][:2].tolist() == [0, 1]
    else:
        dev = [L.fb_covis_tree_set_dev(h, vp(par), vp(u8), vp(u8), None), L.fb_covis_tree_get_dev(h, vp(par), vp(u8), vp(u8), None),
               L.fb_covis_change_parent_dev(h, 0, 1, None), L.fb_covis_erase_child_dev(h, 1, 0, None),
               L.fb_covis_children_dev(h, 0, vp(n), vp(out), None), L.fb_covis_parent_dev(h, 0, vp(n), None),
               L.fb_covis_first_connection_dev(h, 1, vp(out), vp(out), vp(out), -1, 0, None, None, None),
               L.fb_covis_tree_erase_keyframe_dev(h, 0, vp(u8), None), L.fb_covis_local_map_dev(h, C.byref(m), C.byref(a), None),
               L.fb_frame_update_local_map_dev(None, h, C.byref(m), C.byref(a), None),
               L.fb_frame_track_graph_dev(None, None, None, h, C.byref(m), C.byref(a), None)]
        assert calls + dev == [cabi.FB_ERR_NODEVICE] * (len(calls) + len(dev))
        assert b"no CPU fallback" in L.fb_last_error()
    E = cabi.FB_ERR_ARG
    assert L.fb_covis_change_parent_dev(h, 0, 0, None) == E and L.fb_covis_change_parent_dev(h, 0, K, None) == E
    assert L.fb_covis_children_dev(h, K, vp(n), vp(out), None) == E and L.fb_covis_local_map_dev(h, C.byref(m), None, None) == E
    assert L.fb_covis_tree_erase_keyframe_dev(h, -1, vp(u8), None) == E
    L.fb_covis_destroy(h)
