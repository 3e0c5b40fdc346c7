"""CPU tests of the map correction calls (fb_covis_correct_loop*, fb_covis_propagate_gba*): known answers of the literal model
tests/map_correct_ref.py, one per quirk of the reference; identity checks; the ctypes mirrors; no CPU fallback."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import map_correct_cases as cases  # noqa: E402

import fishbirdeyevisualslam_amd as fb  # noqa: E402
from fishbirdeyevisualslam_amd import cabi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a float32 pose or point of magnitude <= 10 through a handful of double operations rounded once: a few ulp of 10
ROUND = 1e-5


def _check_ints(out, exp):
    assert out["n_set"] == exp["n_set"]
    assert out["set_slots"].tolist() == exp["set_slots"]
    assert out["mp_corrected_ref"].tolist() == exp["mp_corrected_ref"]
    assert out["errors"] == exp["errors"] and out["edge_errors"] == 0


def test_point_goes_to_the_smaller_kf_order_not_the_earlier_list_entry():
    c = cases.cl_first_claim()
    g, _, _ = cases.models(c)
    assert g.get_vector_covisible_keyframes(0) == [1, 2]          # 1 is earlier in the list
    out = cases.run_correct_loop(c)
    _check_ints(out, c["expect"])                                  # ... and 2 moves the point
    # the bad point, the point held outside the set: untouched, bit for bit
    assert out["mp_xw"][1].tobytes() == c["mp_xw"][1].tobytes() and out["mp_xw"][2].tobytes() == c["mp_xw"][2].tobytes()
    assert out["kf_Tcw"][3].tobytes() == c["kf_Tcw"][3].tobytes()


def test_centres_levels_and_bird_points_by_hand():
    c = cases.cl_centres()
    out, e = cases.run_correct_loop(c), c["expect"]
    _check_ints(out, e)
    np.testing.assert_allclose(out["mp_xw"], e["mp_xw"], atol=ROUND)
    np.testing.assert_allclose(out["kf_Tcw"].reshape(-1, 3, 4)[:, :, 3], e["kf_t"], atol=ROUND)
    np.testing.assert_allclose(out["kf_Tcw"].reshape(-1, 3, 4)[:, :, :3], np.tile(np.eye(3), (4, 1, 1)), atol=ROUND)
    # an observer outside the set, an earlier one (corrected centre) and the holder itself (old centre); the reference key
    # frame that is no observer (feature 0's octave); the point without an edge keeps its normal and distances
    np.testing.assert_allclose(out["mp_normal"], e["mp_normal"], atol=ROUND)
    np.testing.assert_allclose(out["mp_max_dist"], e["mp_max_dist"], rtol=ROUND)
    np.testing.assert_allclose(out["mp_min_dist"][:2], np.array(e["mp_max_dist"][:2]) / float(c["scale_factors"][-1]), rtol=ROUND)
    assert out["mp_normal"][2].tobytes() == c["mp_normal"][2].tobytes() and out["mp_min_dist"][2] == c["mp_min_dist"][2]
    # held by two members: moved twice; by one: once; bad: not at all
    np.testing.assert_allclose(out["mpb_xw"], e["mpb_xw"], atol=ROUND)
    assert out["mpb_xw"][2].tobytes() == c["mpb_xw"][2].tobytes()


def test_scale_two_halves_the_written_translation():
    c = cases.cl_scale2()
    out = cases.run_correct_loop(c)
    _check_ints(out, c["expect"])
    np.testing.assert_allclose(out["kf_Tcw"].reshape(-1, 3, 4)[:, :, 3], c["expect"]["kf_t"], atol=ROUND)
    assert out["kf_Tcw"][0].tobytes() == c["kf_Tcw"][0].tobytes()


def test_gba_tree_by_hand():
    c = cases.gba_tree()
    out, e = cases.run_propagate_gba(c), c["expect"]
    assert out["reached"].tolist() == e["reached"] and out["kf_gba"].tolist() == e["kf_gba"] and out["errors"] == e["errors"]
    for key, name in (("kf_t", "kf_Tcw"), ("gba_t", "kf_Tcw_gba"), ("bef_t", "kf_Tcw_bef")):
        np.testing.assert_allclose(out[name].reshape(-1, 3, 4)[:, :, 3], e[key], atol=ROUND, err_msg=name)
    np.testing.assert_allclose(out["mp_xw"], e["mp_xw"], atol=ROUND)
    np.testing.assert_allclose(out["mpb_xw"], e["mpb_xw"], atol=ROUND)
    assert out["mp_xw"][1].tobytes() == c["mp_xw"][1].tobytes()   # the bad point


def test_correct_loop_with_the_current_pose_is_the_identity():
    c = cases.cl_identity()
    out = cases.run_correct_loop(c)
    assert out["n_set"] >= 2 and (out["mp_corrected_ref"] >= 0).sum() >= 3
    # |x| up to ~15 here: float32 rounding of a pose product and of two maps
    np.testing.assert_allclose(out["kf_Tcw"], c["kf_Tcw"], atol=2e-5)
    np.testing.assert_allclose(out["mp_xw"], c["mp_xw"], atol=2e-5)
    np.testing.assert_allclose(out["mpb_xw"], c["mpb_xw"], atol=2e-5)


def test_gba_with_its_own_poses_is_the_identity():
    c = cases.gba_identity()
    out = cases.run_propagate_gba(c)
    assert out["reached"].sum() >= 2
    assert out["kf_Tcw"].tobytes() == c["kf_Tcw"].tobytes()
    moved = [i for i in range(len(c["mp_bad"])) if not c["mp_bad"][i] and out["reached"][c["mp_ref_kf"][i]]]
    assert moved
    np.testing.assert_allclose(out["mp_xw"], c["mp_xw"], atol=2e-5)
    np.testing.assert_allclose(out["mpb_xw"], c["mpb_xw"], atol=2e-5)


def test_random_cases_have_every_branch():
    """what the device tests rely on: the seeded cases reach the branches the hand cases pin"""
    twice, skipped, unreached_flag, counted = 0, 0, 0, 0
    for name, c in cases.all_cases():
        if not name.startswith(("random", "bad_entries")):
            continue
        cl, gba = cases.run_correct_loop(c), cases.run_propagate_gba(c)
        assert abs(c["s"] - 1.0) > 1e-3
        twice += int(((c["kf_mpb"][cl["set_slots"]][:, :, None] == np.arange(len(c["mpb_bad"]))).sum((0, 1)) >= 2).any())
        skipped += int(((cl["mp_corrected_ref"] < 0) & (c["mp_bad"] == 0)).any())
        unreached_flag += int(((gba["reached"] == 0) & (gba["kf_gba"] == 1)).any())
        counted += int(name.startswith("bad") and cl["errors"] >= 2 and gba["errors"] >= 3 and cl["edge_errors"] == 1)
    assert twice >= 5 and skipped >= 5 and unreached_flag >= 5 and counted == len(cases.BAD_ENTRY_SEEDS)


def test_ctypes_mirrors_match_the_header_layout():
    names = {"fb_correct_loop_args": C.sizeof(cabi.CorrectLoopArgs), "fb_propagate_gba_args": C.sizeof(cabi.PropagateGbaArgs)}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "fishbird.h"\nint main(void){\n' + "".join(
        'printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names)
    src += 'printf("cur_slot %zu\\n", offsetof(fb_correct_loop_args, cur_slot));\nprintf("origins %zu\\n", offsetof(fb_propagate_gba_args, origins));\n'
    src += "return 0;}\n"
    d = tempfile.mkdtemp()
    open(os.path.join(d, "s.c"), "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
    got = dict(l.split() for l in subprocess.check_output([os.path.join(d, "s")]).decode().splitlines())
    for n, sz in names.items():
        assert int(got[n]) == sz, (n, got[n], sz)
    assert int(got["cur_slot"]) == cabi.CorrectLoopArgs.cur_slot.offset and int(got["origins"]) == cabi.PropagateGbaArgs.origins.offset


def test_no_cpu_fallback_without_device():
    lib = fb.lib()
    for name in ("fb_covis_correct_loop_dev", "fb_covis_correct_loop", "fb_covis_propagate_gba_dev", "fb_covis_propagate_gba",
                 "fb_covis_reserve_correct_loop"):
        assert hasattr(lib, name), name
    if lib.fb_device_count() > 0:
        return  # on the GPU box this is covered by the gpu tests
    c = cases.cl_centres()
    K = c["K"]
    keep = {k: np.ascontiguousarray(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    m = cabi.CovisMap()
    cabi.fill(m, max_keyframes=K, kp_stride=c["S"], n_mp=len(c["mp_bad"]), n_obs=len(c["obs_kf"]),
              **{k: keep[k] for k in ("kf_n", "kf_mp", "kf_octave", "mp_bad", "obs_mp", "obs_kf", "obs_idx", "kf_order")})
    t = cabi.CovisKfTables()
    cabi.fill(t, n_levels=len(c["scale_factors"]), kf_Tcw=keep["kf_Tcw"], mp_xw=keep["mp_xw"])
    out = {k: np.zeros(16, np.int32) for k in ("d_mp_corrected_ref", "d_n_set", "d_set_slots")}
    a = cabi.CorrectLoopArgs()
    cabi.fill(a, q=[0.0, 0.0, 0.0, 1.0], t=[1.0, 0.0, 0.0], s=1.0, cur_slot=3, reuse_index=0,
              **{k: keep[k] for k in ("scale_factors", "mp_ref_kf", "mp_normal", "mp_min_dist", "mp_max_dist")}, **out)
    reached = np.zeros(K, np.uint8)
    b = cabi.PropagateGbaArgs()
    cabi.fill(b, n_origins=0, d_reached=reached, **{k: keep[k] for k in ("kf_gba", "kf_Tcw_gba", "kf_Tcw_bef", "mp_gba", "mp_pos_gba", "mp_ref_kf")})
    h = C.c_void_p()
    assert lib.fb_covis_create(K, C.byref(h)) == 0
    assert lib.fb_covis_correct_loop_dev(h, C.byref(m), C.byref(t), C.byref(a), None) == cabi.FB_ERR_NODEVICE
    assert lib.fb_covis_correct_loop(h, C.byref(m), C.byref(t), C.byref(a)) == cabi.FB_ERR_NODEVICE
    assert lib.fb_covis_propagate_gba_dev(h, C.byref(m), C.byref(t), C.byref(b), None) == cabi.FB_ERR_NODEVICE
    assert lib.fb_covis_propagate_gba(h, C.byref(m), C.byref(t), C.byref(b)) == cabi.FB_ERR_NODEVICE
    assert b"no CPU fallback" in lib.fb_last_error()
    assert lib.fb_covis_reserve_correct_loop(h, 3, 3, 0, 0, 0) == cabi.FB_ERR_NODEVICE
    assert keep["kf_Tcw"].tobytes() == c["kf_Tcw"].tobytes() and keep["mp_xw"].tobytes() == c["mp_xw"].tobytes()
    lib.fb_covis_destroy(h)
