"""Bundle adjustment beyond the LDS-resident limit (> 23 free key frames): the reduced pose system lives in HBM
(csrc/ba_big.inc: deterministic block gather of the Schur complement, blocked LDL^T over several kernels).  Same parity bar as
tests/test_ba_gpu.py: poses / landmarks within 1e-4 relative of the oracle per element (ba_cases.pose_rel / point_rel), outlier flags identical."""
import ctypes as C

import numpy as np
import pytest

import ba_cases as BC
import oracle_lib as O
from fishbirdeyevisualslam_amd import ba_problem, synth

pytestmark = pytest.mark.gpu
REL_TOL = 1e-4


def _assert_close(label, oh, oo, bird):
    wp, wl = BC.worst_pose_rel(oh["kf_Tcw"], oo["kf_Tcw"]), BC.worst_point_rel(oh["mp_xw"], oo["mp_xw"])
    wb = BC.worst_point_rel(oh["mpb_xw"], oo["mpb_xw"]) if bird else 0.0
    print("%s: worst per-element difference: poses %.3g, landmarks %.3g, bird landmarks %.3g" % (label, wp, wl, wb))
    assert wp <= REL_TOL
    assert wl <= REL_TOL
    assert wb <= REL_TOL


@pytest.mark.parametrize("seed,n_kf,n_fixed,n_mp,n_mpb,with_odom", [(4200, 32, 2, 6000, 1500, 1), (4201, 30, 3, 4000, 0, 0),
                                                                   (4202, 70, 2, 12000, 3000, 1)])
def test_local_ba_many_keyframes(seed, n_kf, n_fixed, n_mp, n_mpb, with_odom):
    import hip_lib as H
    p = synth.make_ba_problem(seed, n_kf=n_kf, n_fixed=n_fixed, n_mp=n_mp, n_mpb=n_mpb)
    a, oo, k = ba_problem.local_ba_args(p, with_odom=with_odom)
    O.call("orc_local_ba", a)
    a2, oh, k2 = ba_problem.local_ba_args(p, with_odom=with_odom)
    H.call("fb_local_ba", a2)
    _assert_close("local BA, %d key frames" % n_kf, oh, oo, bool(with_odom and n_mpb))
    np.testing.assert_array_equal(oh["obs_outlier"], oo["obs_outlier"])
    if with_odom:
        np.testing.assert_array_equal(oh["bobs_outlier"], oo["bobs_outlier"])


def test_global_ba_many_keyframes():
    import fishbirdeyevisualslam_amd as fb
    p = synth.make_ba_problem(4300, n_kf=100, n_fixed=1, n_mp=15000, n_mpb=3000)
    for key in ("odom_kf_i", "odom_kf_j", "odom_Tij", "odom_info"):
        p[key] = p[key][:0]
    a, oo, k = ba_problem.local_ba_args(p, with_odom=1)
    assert O.lib().orc_global_ba(C.byref(a), 10, 1) == 0
    a2, oh, k2 = ba_problem.local_ba_args(p, with_odom=1)
    fb.check(fb.lib().fb_global_ba(C.byref(a2), 10, 1), "fb_global_ba")
    _assert_close("global BA, 100 key frames", oh, oo, True)
