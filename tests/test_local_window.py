"""The local-BA window without a GPU: hand-derived answers for the model tests/local_window_ref.py, the std::map restatement
tests/cpp/window_map_ref.cpp against it, and the new entry points in the header and the library."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import covis_ref as R
import local_window_ref as LW
from fishbirdeyevisualslam_amd import cabi, covis_problem as P
from test_covis import ref_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_SYMBOLS = ("fb_covis_reserve_window", "fb_covis_local_window_dev", "fb_covis_local_window_header", "fb_covis_local_window",
                  "fb_covis_window_scatter_dev")


def hand_map():
    """5 key frames, 8 points.  kf_order runs against the slot order.  cur = 0; its ordered list is [2, 1]; 1 is bad and
    observes the local point 1; 3 is a bad key frame outside the list that observes the local point 3; 4 is the fixed camera.
    Point 1 lies at two features of key frame 0, point 2 is bad, the edge (4, key frame 4) is erased."""
    K, S = 5, 8
    kf_mp = np.full((K, S), -1, np.int32)
    rows = {0: [0, 1, 2, 1, 5], 1: [1, 7], 2: [0, 3, 4, 5], 3: [3], 4: [0, 3, 6, 7, 2]}
    for kf, r in rows.items():
        kf_mp[kf, :len(r)] = r
    edges = [(0, 0, 0), (0, 2, 0), (0, 4, 0), (1, 0, 1), (1, 1, 0), (2, 0, 2), (2, 4, 4), (3, 2, 1), (3, 3, 0), (3, 4, 1), (4, 2, 2),
             (4, -1, 5), (5, 2, 3), (5, 0, 4), (6, 4, 2), (7, 1, 1), (7, 4, 3)]
    e = np.array(edges, np.int32)
    p = dict(K=K, S=S, kf_n=np.array([len(rows[k]) for k in range(K)], np.int32), kf_mp=kf_mp,
             kf_octave=(np.arange(K * S).reshape(K, S) % 8).astype(np.uint8), mp_bad=np.array([0, 0, 1, 0, 0, 0, 0, 0], np.uint8),
             obs_mp=e[:, 0].copy(), obs_kf=e[:, 1].copy(), obs_idx=e[:, 2].copy(),
             kf_order=np.array([500 - 100 * s for s in range(K)], np.uint64))
    p.update(P.window_tables(p, 1, kf_bad=[1, 3], kf_init=[2]))
    g = R.Graph(K, p["kf_order"])
    g.add_connection(0, 1, 20)
    g.add_connection(0, 2, 30)
    return p, g


def test_hand_derived_window():
    p, g = hand_map()
    assert g.get_vector_covisible_keyframes(0) == [2, 1]
    w = LW.local_window(g, p, 0, False)
    assert w["kf_slot"].tolist() == [0, 2, 4] and w["kf_fixed"].tolist() == [0, 1, 1] and (w["n_local"], w["n_fixed"]) == (2, 1)
    assert w["mp_index"].tolist() == [0, 1, 5, 3, 4]
    assert w["obs_kf"].tolist() == [2, 1, 0, 0, 1, 0, 2, 1, 1]
    assert w["obs_mp"].tolist() == [0, 0, 0, 1, 2, 2, 3, 3, 4]
    assert w["obs_src"].tolist() == [2, 1, 0, 3, 12, 13, 9, 7, 10]
    assert w["header"] == [2, 1, 5, 9, 0, 0, 0]
    kp = p["kf_keys_un"][4, 0]                                              # the first edge: point 0 in key frame 4, feature 0
    assert w["obs_uv"][0].tolist() == [kp["x"], kp["y"]] and w["obs_inv_sigma2"][0] == p["inv_level_sigma2"][kp["octave"]]
    np.testing.assert_array_equal(w["kf_Tcw"], p["kf_Tcw"][[0, 2, 4]])
    np.testing.assert_array_equal(w["mp_xw"], p["mp_xw"][[0, 1, 5, 3, 4]])
    # the write-back: local key frames and local points only, erase rows in edge order
    n_kf, n_mp = 3, 5
    out = LW.write_back(w, p, np.full((n_kf, 12), 7, np.float32), np.full((n_mp, 3), 8, np.float32), None,
                        np.array([0, 1, 0, 0, 0, 0, 1, 0, 0], np.uint8), np.zeros(0, np.uint8))
    assert out["erase"].tolist() == [[2, 0, 0, 1], [4, 3, 1, 9]]
    assert (out["kf_Tcw"][[0, 2]] == 7).all() and (out["kf_Tcw"][[1, 3, 4]] == p["kf_Tcw"][[1, 3, 4]]).all()
    assert (out["mp_xw"][[0, 1, 5, 3, 4]] == 8).all() and (out["mp_xw"][[2, 6, 7]] == p["mp_xw"][[2, 6, 7]]).all()


def test_std_map_restatement_equals_the_model():
    p = P.make_window_problem()
    g = R.Graph(p["K"], p["kf_order"])
    for a in p["used"]:
        g.update_connections(ref_map(p), a)
    d = tempfile.mkdtemp()
    exe, blob = os.path.join(d, "window_map_ref"), os.path.join(d, "map.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "window_map_ref.cpp"), "-o", exe])
    P.write_window_blob(p, g.get_vector_covisible_keyframes(p["cur"]), blob)
    for with_bird in (1, 0):
        w = LW.local_window(g, p, p["cur"], bool(with_bird))
        got = {}
        for line in subprocess.check_output([exe, blob, str(p["cur"]), str(with_bird)]).decode().splitlines():
            got[line.split()[0]] = [int(x) for x in line.split()[1:]] if line.split()[0] != "ms" else line.split()[1]
        assert got["local"] + got["fixed"] == w["kf_slot"].tolist() and len(got["local"]) == w["n_local"]
        assert got["mp"] == w["mp_index"].tolist() and got["mpb"] == w["mpb_index"].tolist()
        for k in ("obs_kf", "obs_mp", "obs_src", "bobs_kf", "bobs_mpb", "bobs_src"):
            assert got[k] == w[k].tolist(), k


def test_window_entry_points_are_declared_bound_and_exported():
    import fishbirdeyevisualslam_amd as fb
    header = open(os.path.join(ROOT, "include", "fishbird.h")).read()
    lib = fb.lib()
    for s in WINDOW_SYMBOLS:
        assert s + "(" in header and s in cabi.EXPORTS and hasattr(lib, s), s
    sizes = {"fb_covis_kf_tables": C.sizeof(cabi.CovisKfTables), "fb_covis_window": C.sizeof(cabi.CovisWindow),
             "fb_covis_window_header": C.sizeof(cabi.CovisWindowHeader)}
    src = '#include <stdio.h>\n#include "fishbird.h"\nint main(void){\n' + "".join(
        'printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in sizes) + "return 0;}\n"
    d = tempfile.mkdtemp()
    open(os.path.join(d, "s.c"), "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
    got = dict(l.split() for l in subprocess.check_output([os.path.join(d, "s")]).decode().splitlines())
    assert {k: int(v) for k, v in got.items()} == sizes
    # no device, no answer: the calls fail loudly instead of computing on the host
    if fb.lib().fb_device_count() == 0:
        h = C.c_void_p()
        assert lib.fb_covis_create(8, C.byref(h)) == 0
        assert lib.fb_covis_reserve_window(h, 10, 10, 0, 0) == cabi.FB_ERR_NODEVICE
        lib.fb_covis_destroy(h)


_COVIS_PROBLEM_SIZES = (620, 2696, 270)   # points, edges, erased edges of make_covis_problem() before MapBuilder had other users


def test_generators_of_existing_problems_are_unchanged():
    """the new MapBuilder users draw from generators of their own: a known digest of make_covis_problem's arrays"""
    q = P.make_covis_problem()
    assert (len(q["mp_bad"]), len(q["obs_kf"]), int((q["obs_kf"] < 0).sum())) == _COVIS_PROBLEM_SIZES

