"""GPU parity on the graphs of tests/ba_cases.py: HIP local bundle adjustment vs the CPU oracle through every path a case can
take -- fb_local_ba (device-resident LM), fb_local_ba with FB_BA_HOST_LM=1 (the same schedule host-paced, one slot per batch;
byte-equal), fb_local_ba_dev (graph built by kernels; byte-equal to fb_local_ba) and, with 24 free key frames, the HBM-resident
path of ba_big.inc (default and host-paced; byte-equal).

Asserted per path: outlier flags identical to the oracle AND to the flags the construction demands; the one-sided chi2 / depth
gate recomputed in numpy float64 on the HIP output; poses and landmarks within 1e-4 (BASELINE.json north_star) PER ELEMENT
(each pose by max(1, max|T_k|) of its own 3x4, each landmark by max(1, ||x||)); fixed key frames byte-identical.  The oracle's
answers come from ba_cases.oracle (computed once, shared with tests/test_ba_structure.py, which proves the constructions)."""
import ctypes as C

import numpy as np
import pytest

import ba_cases as BC
import hip_lib as H
from fishbirdeyevisualslam_amd import ba_problem, cabi

pytestmark = pytest.mark.gpu
OUT_KEYS = ("kf_Tcw", "mp_xw", "mpb_xw", "obs_outlier")


def _host(p, ex):
    a, out, keep = ba_problem.local_ba_args(p, with_odom=ex["with_odom"])
    H.call("fb_local_ba", a)
    return out


def _dev(p, ex):
    import torch
    import fishbirdeyevisualslam_amd as fb
    a, dev, keep = ba_problem.local_ba_args_dev(p, with_odom=ex["with_odom"])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc = fb.lib().fb_local_ba_dev(C.byref(a), C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in dev.items()}


def _check(p, ex, out_o, out_h, label, capsys):
    with_odom = ex["with_odom"]
    nb = len(p["bobs_kf"]) if with_odom else 0
    wp = BC.worst_pose_rel(out_h["kf_Tcw"], out_o["kf_Tcw"])
    wl = max(BC.worst_point_rel(out_h["mp_xw"], out_o["mp_xw"]), BC.worst_point_rel(out_h["mpb_xw"], out_o["mpb_xw"]) if with_odom else 0.0)
    with capsys.disabled():
        print("\n[ba structure gpu] %-50s worst per-element difference: poses %.3g, landmarks %.3g" % (label, wp, wl), end="")
    np.testing.assert_array_equal(out_h["obs_outlier"], out_o["obs_outlier"], err_msg=label + ": front flags")
    np.testing.assert_array_equal(out_h["bobs_outlier"][:nb], out_o["bobs_outlier"][:nb], err_msg=label + ": bird flags")
    BC.check_flags_by_construction(ex, out_h)
    bad, left_out = BC.gate_check(p, out_h, with_odom)
    assert len(bad) == 0, "%s: edges returned with flag 0 that fail the gate in float64: %s" % (label, bad[:10])
    assert left_out < 0.02
    assert wp <= BC.REL_TOL, "%s: poses %.3g" % (label, wp)
    assert wl <= BC.REL_TOL, "%s: landmarks %.3g" % (label, wl)
    fx = p["kf_fixed"] == 1
    assert out_h["kf_Tcw"][fx].tobytes() == np.ascontiguousarray(p["kf_Tcw"][fx], np.float32).tobytes(), label + ": fixed key frames"


def _paced(p, ex, monkeypatch):
    monkeypatch.setenv("FB_BA_HOST_LM", "1")
    out = _host(p, ex)
    monkeypatch.delenv("FB_BA_HOST_LM")
    return out


def _assert_same_bytes(out_a, out_b, label):
    for k in ("kf_Tcw", "mp_xw", "mpb_xw", "obs_outlier", "bobs_outlier"):
        assert out_a[k].tobytes() == out_b[k].tobytes(), "%s: %s differs" % (label, k)


def _lds_paths(cid, monkeypatch, capsys):
    """Up to 23 free key frames: device LM from host pointers, the same host-paced (byte-equal: the default take enqueues
    slots past the end of the schedule and the paced one does not, so equality also proves the kernels' `phase == 2` and
    `needInit` guards), device LM from device inputs (byte-equal)."""
    p, ex, out_o, _ = BC.oracle(cid)
    name = BC.case_name(cid)
    out_h = _host(p, ex)
    _check(p, ex, out_o, out_h, name + " / fb_local_ba", capsys)
    out_l = _paced(p, ex, monkeypatch)
    _check(p, ex, out_o, out_l, name + " / FB_BA_HOST_LM=1", capsys)
    _assert_same_bytes(out_l, out_h, name + ": FB_BA_HOST_LM=1 against the default take")
    rc, out_d = _dev(p, ex)
    assert rc == 0
    out_d = {k: out_d[k][: len(out_h[k])] for k in out_h}   # an empty host array travels as a one-element placeholder
    for k in OUT_KEYS[: 4 if ex["with_odom"] else 2] + ("obs_outlier",):
        assert out_d[k].tobytes() == out_h[k].tobytes(), "%s: fb_local_ba_dev differs from fb_local_ba in %s" % (name, k)
    nb = len(p["bobs_kf"]) if ex["with_odom"] else 0
    np.testing.assert_array_equal(out_d["bobs_outlier"][:nb], out_h["bobs_outlier"][:nb])
    _check(p, ex, out_o, out_d, name + " / fb_local_ba_dev", capsys)
    return p, ex, out_o, out_h


def _big_path(cid, monkeypatch, capsys):
    """24 free key frames (P6 = 144: three full panels of 48): the HBM-resident path from host pointers, the same host-paced
    (byte-equal: every kernel of ba_big.inc is a no-op in a slot that only linearises and after the schedule has finished),
    FB_ERR_CAPACITY from device inputs."""
    p, ex, out_o, _ = BC.oracle(cid)
    assert int((p["kf_fixed"] == 0).sum()) == 24
    out_h = _host(p, ex)
    _check(p, ex, out_o, out_h, BC.case_name(cid) + " / fb_local_ba (HBM-resident)", capsys)
    _assert_same_bytes(_paced(p, ex, monkeypatch), out_h, BC.case_name(cid) + " (HBM-resident): FB_BA_HOST_LM=1 against the default take")
    rc, _ = _dev(p, ex)
    assert rc == cabi.FB_ERR_CAPACITY
    return p, ex, out_o


def test_behind_camera(monkeypatch, capsys):
    """Pins `|| !(p[2] > 0.0)` of gate_edge (ba.hip): without it the special edges, which fit (chi2 < 3) from 6 m behind their
    camera, stay in round 2 and come back with flag 0 -- the flags differ from the oracle and from the construction."""
    p, ex, out_o, out_h = _lds_paths(("structural", "behind_camera", False), monkeypatch, capsys)
    r = BC.recompute(p, out_h, 1)
    assert (r["depth"][ex["special"]] < -1.0).all() and (r["chi2"][ex["special"]] < 3.0).all()
    assert (out_h["obs_outlier"][ex["special"]] == 1).all()


def test_landmark_fully_gated(monkeypatch, capsys):
    """Pins the `lvl != 0` branch of lin_edge (ba.hip): a landmark whose two edges both left at the gate must contribute
    nothing in round 2 (Hll = lambda I, bl = 0, W = 0) and stay where round 1 left it, as the vertex that leaves g2o's system.
    A gated edge that kept its terms would drag the landmark 80 px worth of residual away from the oracle's."""
    p, ex, out_o, out_h = _lds_paths(("structural", "landmark_fully_gated", False), monkeypatch, capsys)
    assert BC.worst_point_rel(out_h["mp_xw"][ex["special"]], out_o["mp_xw"][ex["special"]]) <= BC.REL_TOL


def test_keyframe_fully_gated(monkeypatch, capsys):
    """Pins `if (D.e_level[e] != 0) continue;` of pose_body (ba.hip) and the treatment of a free key frame without any active
    edge (Hpp block = lambda I, bp = 0: a zero step), both for the key frame gated after round 1 and for the one that never
    had an observation; an isolated landmark comes back byte-identical."""
    p, ex, out_o, out_h = _lds_paths(("structural", "keyframe_fully_gated", False), monkeypatch, capsys)
    kf_gated, kf_empty = ex["special"]
    np.testing.assert_allclose(out_h["kf_Tcw"][kf_empty], p["kf_Tcw"][kf_empty], rtol=0, atol=1e-6)
    lonely = BC.observers(p) == 0
    assert out_h["mp_xw"][lonely].tobytes() == np.ascontiguousarray(p["mp_xw"][lonely], np.float32).tobytes()


def test_single_observation_landmark(monkeypatch, capsys):
    """Pins the 3x3 inverse of Hll + lambda I in schur_body / k_ba_dinv on a rank-2 Hll: only lambda keeps it invertible."""
    _lds_paths(("structural", "single_observation_landmark", False), monkeypatch, capsys)


def test_landmark_seen_only_by_fixed(monkeypatch, capsys):
    """Pins the `pj < 0` filters of schur_body (scatter and clear) and update_body, and the `pj >= 0` branch of lin_edge: a
    landmark seen by fixed key frames only has Hll and bl, no W block and no row in the panels.  Indexing the panels with
    6 * pj for pj = -1 would write before the panel."""
    p, ex, out_o, out_h = _lds_paths(("structural", "landmark_seen_only_by_fixed", False), monkeypatch, capsys)
    assert np.abs(out_h["mp_xw"][ex["special"]] - p["mp_xw"][ex["special"]]).max() > 0


@pytest.mark.parametrize("name", list(BC.STRUCTURAL))
def test_structural_case_on_the_hbm_resident_path(name, monkeypatch, capsys):
    """The same five graphs with 24 free key frames: pins the e_level filters of k_ba_schur_gather / k_ba_rhs_gather, the pair
    lists of big_prepare for landmarks without a free observer, and k_ba_dinv on the degenerate Hll (ba_big.inc)."""
    _big_path(("structural", name, True), monkeypatch, capsys)


@pytest.mark.parametrize("f", BC.FREE_COUNTS[:-1])
def test_free_count(f, monkeypatch, capsys):
    """Every count of free key frames the LDS-resident system takes, 1...23: pins the NT = (6 f + 1 + 15) / 16 tile count and
    the MAXT = 9 / 20 / 34 dispatch of k_ba_schur_c / k_ba_solve_c, among them 2 and 5 (a tile boundary), 19-21 (NT = 8) and 22."""
    _lds_paths(("free_count", f), monkeypatch, capsys)


def test_free_count_24_takes_the_hbm_resident_path(monkeypatch, capsys):
    _big_path(("free_count", 24), monkeypatch, capsys)


@pytest.mark.parametrize("n", BC.POINT_COUNTS)
def test_point_count(n, monkeypatch, capsys):
    """npt = 1, 15, 16, 17, 33, 100: pins the `l < l1` guard of the tail chunk in schur_body, the `l < D.npt` guards of the
    linearisation / update lanes and the rounding of nWg / lmPerWg in plan()."""
    _lds_paths(("point_count", n), monkeypatch, capsys)


def test_point_count_several_chunks_per_workgroup(monkeypatch, capsys):
    """FB_BA_NWG=2 at 100 points: lmPerWg = 64, the second workgroup walks two full chunks and a tail of four -- the only way to
    the chunk loop's clear-after-MFMA traversal (stale panel entries would leak into the next chunk) at test size."""
    monkeypatch.setenv("FB_BA_NWG", str(BC.NWG_CAP_FOR_CHUNKS))
    _lds_paths(("point_count", 100), monkeypatch, capsys)
