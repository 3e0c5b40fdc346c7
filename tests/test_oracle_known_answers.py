"""CPU tests: the oracle against hand-derivable known answers.  The reference ships no
test vectors, so these pin the restatement where an answer can be derived without OpenCV/Eigen."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib as O
from fishbirdeyevisualslam_amd import cabi, problems as P, synth


def test_extractor_tables():
    t = O.orb_tables(O.orb_params())
    assert list(t.features_per_level)[:8] == [434, 362, 302, 251, 209, 175, 145, 122]
    assert list(O.orb_tables(O.orb_params(nfeatures=4000)).features_per_level)[:8] == [869, 724, 603, 503, 419, 349, 291, 242]
    assert list(O.orb_tables(O.orb_params(nfeatures=1000)).features_per_level)[:8] == [217, 181, 151, 126, 105, 87, 73, 60]
    assert list(t.umax) == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    sf = np.array(t.scale_factor[:8], np.float32)
    np.testing.assert_array_equal(sf, np.array([1, 1.2000000477, 1.4400000572, 1.728000164, 2.0736002922, 2.4883203506,
                                                2.9859845638, 3.5831816196], np.float32))
    np.testing.assert_array_equal(np.array(t.level_sigma2[:8], np.float32), sf * sf)


def test_pyramid_level_sizes():
    p = O.orb_params()
    for (w, h), sizes in {(1280, 720): [(1280, 720), (1067, 600), (889, 500), (741, 417), (617, 347), (514, 289), (429, 241), (357, 201)],
                          (512, 512): [(512, 512), (427, 427), (356, 356), (296, 296), (247, 247), (206, 206), (171, 171), (143, 143)],
                          (640, 480): [(640, 480), (533, 400), (444, 333), (370, 278), (309, 231), (257, 193), (214, 161), (179, 134)]}.items():
        img = np.zeros((h, w), np.uint8)
        for l, (lw, lh) in enumerate(sizes):
            assert O.orb_level(p, img, l).shape == (lh, lw)


def test_orb_pattern_checksum():
    import hashlib, re, struct, os
    txt = open(os.path.join(O.ROOT, "oracle", "orb_pattern.inc")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    nums = [int(x) for x in re.findall(r"-?\d+", txt)]
    assert len(nums) == 1024 and nums[:8] == [8, -3, 9, 5, 4, 2, 7, -12] and nums[-4:] == [-1, -6, 0, -11]
    assert sum(nums) == -406 and sum(abs(n) for n in nums) == 6854
    assert hashlib.sha256(b"".join(struct.pack("<i", n) for n in nums)).hexdigest() == \
        "7e645581387b82784797e8adddb9b6f0c12611859fda09ca8a9bec96d767a05f"
    prod = open(os.path.join(O.ROOT, "fishbirdeyevisualslam_amd", "csrc", "orb_pattern.inc")).read()
    assert re.findall(r"-?\d+", re.sub(r"/\*.*?\*/", "", prod, flags=re.S)) == [str(n) for n in nums]


def test_descriptor_distance_known_answers():
    g = synth.rng(1)
    a = synth.random_descriptors(g, 300)
    b = synth.random_descriptors(g, 300)
    b[0] = a[0]
    a[1] = 0
    b[1] = 255
    b[2] = a[2]
    b[2, 31] ^= 0x80
    out = np.zeros(300, np.int32)
    O.lib().orc_descriptor_distance(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), 300, C.c_void_p(out.ctypes.data))
    np.testing.assert_array_equal(out, np.unpackbits(a ^ b, axis=1).sum(1))
    assert out[0] == 0 and out[1] == 256 and out[2] == 1


def _maxima(h):
    h = np.array(h, np.int32)
    ind = np.zeros(3, np.int32)
    O.lib().orc_three_maxima(C.c_void_p(h.ctypes.data), len(h), C.c_void_p(ind.ctypes.data))
    return list(ind)


def test_three_maxima():
    h = [0] * 30
    assert _maxima(h) == [-1, -1, -1]
    h[5], h[7], h[9] = 100, 50, 20
    assert _maxima(h) == [5, 7, 9]
    h[9] = 9          # < 10% of max1 -> third dropped
    assert _maxima(h) == [5, 7, -1]
    h[7] = 9          # second < 10% -> second and third dropped
    assert _maxima(h) == [5, -1, -1]
    h = [0] * 30
    h[3] = h[4] = h[8] = 40  # ties: strict '>' cascade keeps the earliest bin first
    assert _maxima(h) == [3, 4, 8]
    hist = lambda d: [d.get(i, 0) for i in range(30)]
    # on the rule (ORBmatcher.cc:1937,1942): 0.1f*(float)max1 rounds to the float max1/10 exactly (0.1f is 1.5e-8 too big,
    # half a float step at 1, 2, 3 is 6e-8 or more), and max2 < max1/10 is false when they are equal: the bin stays
    assert _maxima(hist({0: 10, 4: 1})) == [0, 4, -1]          # 1 < 1.0f false
    assert _maxima(hist({0: 20, 4: 2})) == [0, 4, -1]          # 2 < 2.0f false
    assert _maxima(hist({0: 30, 4: 3})) == [0, 4, -1]          # 3 < 3.0f false
    assert _maxima(hist({0: 11, 4: 1})) == [0, -1, -1]         # 1 < 1.1f
    assert _maxima(hist({0: 21, 4: 2})) == [0, -1, -1]         # 2 < 2.1f
    assert _maxima(hist({0: 10, 4: 5, 8: 1})) == [0, 4, 8]     # the same rule for the third
    assert _maxima(hist({0: 20, 4: 5, 8: 2})) == [0, 4, 8]
    assert _maxima(hist({0: 30, 4: 5, 8: 3})) == [0, 4, 8]
    assert _maxima(hist({0: 11, 4: 5, 8: 1})) == [0, 4, -1]
    assert _maxima(hist({0: 21, 4: 5, 8: 2})) == [0, 4, -1]
    # ties, strict '>' at :1914,:1923,:1930: a bin that only equals a place does not take it, so the earlier bin stays ahead
    assert _maxima(hist({1: 4, 3: 4, 6: 4, 9: 4})) == [1, 3, 6]        # a fourth bin equal to the third is dropped
    assert _maxima(hist({1: 5, 3: 4, 6: 4, 9: 4})) == [1, 3, 6]        # tie for second among three
    assert _maxima(hist({3: 4, 6: 4, 9: 4, 11: 5})) == [11, 3, 6]      # 11 takes first and pushes 3, 6 down; 9 falls out
    assert _maxima(hist({1: 5, 3: 4, 6: 2, 9: 2})) == [1, 3, 6]        # tie for third
    # 6 leads, 9 (equal) takes second; 10 then 11 push them down: 6 is third, 9 falls out although it equals 6
    assert _maxima(hist({6: 2, 9: 2, 10: 5, 11: 4})) == [10, 11, 6]
    assert _maxima(hist({3: 5})) == [3, -1, -1]
    assert _maxima(hist({2: 5, 7: 3})) == [2, 7, -1]


def test_huber_kernel():
    delta = math.sqrt(5.991)
    rho = (C.c_double * 2)()
    O.lib().orc_huber(C.c_double(delta * delta), C.c_double(delta), rho)
    assert rho[0] == delta * delta and rho[1] == 1.0
    e = 10.0
    O.lib().orc_huber(C.c_double(e), C.c_double(delta), rho)
    assert rho[0] == pytest.approx(2 * math.sqrt(e) * delta - delta * delta, rel=1e-15)
    assert rho[1] == pytest.approx(delta / math.sqrt(e), rel=1e-15)


def _exp(u):
    u = np.array(u, np.float64)
    o = np.zeros(7)
    O.lib().orc_se3_exp(C.c_void_p(u.ctypes.data), C.c_void_p(o.ctypes.data))
    return o


def _log(q):
    q = np.array(q, np.float64)
    o = np.zeros(6)
    O.lib().orc_se3_log(C.c_void_p(q.ctypes.data), C.c_void_p(o.ctypes.data))
    return o


def test_se3_exp_log():
    np.testing.assert_allclose(_exp([0] * 6), [0, 0, 0, 1, 0, 0, 0], atol=0)
    g = synth.rng(3)
    for _ in range(50):
        u = np.concatenate([g.normal(0, 0.5, 3), g.normal(0, 2.0, 3)])
        np.testing.assert_allclose(_log(_exp(u)), u, atol=1e-9)
    # rotation by pi/2 about z, no translation
    q = _exp([0, 0, math.pi / 2, 0, 0, 0])
    np.testing.assert_allclose(q[:4], [0, 0, math.sqrt(0.5), math.sqrt(0.5)], atol=1e-15)
    # small-angle branch boundary (theta < 1e-5 uses R = I + Om + Om^2, se3quat.h:236-241)
    a = _exp([9e-6, 0, 0, 1, 2, 3])
    b = _exp([1.1e-5, 0, 0, 1, 2, 3])
    np.testing.assert_allclose(a[4:], [1, 2, 3], atol=1e-4)
    np.testing.assert_allclose(b[4:], [1, 2, 3], atol=1e-4)


@pytest.mark.parametrize("dim", [2, 3])
def test_pose_edge_jacobian_matches_numeric(dim):
    """Analytic b = -J^T e and H = J^T J against central differences of the residual."""
    g = synth.rng(11 + dim)
    T = synth.random_pose(g)
    T12 = synth.to12(T)
    Xc = np.array([0.4, -0.3, 6.0])
    Xw = T[:3, :3].T @ (Xc - T[:3, 3])
    meas = np.array([700.0, 300.0, 0.0]) if dim == 2 else Xc + np.array([0.05, -0.02, 0.03])
    K4 = np.array([500.0, 480.0, 640.0, 360.0])

    def resid(T12_):
        err = np.zeros(3)
        J = np.zeros(42)
        O.lib().orc_pose_edge(dim, C.c_void_p(T12_.ctypes.data), C.c_void_p(Xw.ctypes.data), C.c_void_p(meas.ctypes.data),
                              C.c_void_p(K4.ctypes.data), C.c_void_p(err.ctypes.data), C.c_void_p(J.ctypes.data))
        return err[:dim].copy(), J[:6].copy(), J[6:].reshape(6, 6).copy()

    e0, b, H = resid(T12)
    # numeric Jacobian w.r.t. the left-multiplicative update exp(d) * T, in float64 via our own numpy SE3
    Td = np.eye(4)
    Td[:3, :4] = T12.reshape(3, 4).astype(np.float64)

    def r_np(Tm):
        p = Tm[:3, :3] @ Xw + Tm[:3, 3]
        if dim == 2:
            return meas[:2] - np.array([p[0] / p[2] * K4[0] + K4[2], p[1] / p[2] * K4[1] + K4[3]])
        return meas - p

    J = np.zeros((dim, 6))
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        def upd(dd):
            D = np.eye(4)
            D[:3, :3] = synth.so3_exp(dd[:3])
            D[:3, 3] = dd[3:]   # first order in the translation part is enough for a derivative at 0
            return D @ Td
        J[:, k] = (r_np(upd(d)) - r_np(upd(-d))) / (2 * h)
    np.testing.assert_allclose(b, -(J.T @ r_np(Td)), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(H, J.T @ J, rtol=1e-5, atol=1e-5)


def test_pose_opt_noise_free_recovers_pose():
    p = synth.make_pose_problem(3300, n_front=300, n_bird=100, outlier_frac=0.0)
    T = p["T_true"]
    Xc = (T[:3, :3] @ p["front_xw"].astype(np.float64).T).T + T[:3, 3]
    p["front_obs"] = np.ascontiguousarray(np.stack([Xc[:, 0] / Xc[:, 2] * p["fx"] + p["cx"], Xc[:, 1] / Xc[:, 2] * p["fy"] + p["cy"]], 1).astype(np.float32))
    p["bird_xc"] = np.ascontiguousarray(((T[:3, :3] @ p["bird_xw"].astype(np.float64).T).T + T[:3, 3]).astype(np.float32))
    for mode in (cabi.FB_POSE_FRONT, cabi.FB_POSE_FRONT_BIRD):
        a, out, keep = P.pose_args([p], mode=mode)
        O.call("orc_pose_opt", a)
        assert out["ninliers"][0] == 300 and out["front_outlier"][0].sum() == 0
        assert np.abs(out["Tcw"][0].reshape(3, 4) - T[:3, :4]).max() < 2e-4


def test_deterministic_sincos_and_atan2_accuracy():
    """fb_detmath restates libm cosf/sinf and cv::fastAtan2; check them against float64 references."""
    import subprocess, os, tempfile
    src = r'''
#include <cstdio>
#include <cmath>
#include "fb_detmath.h"
int main(){ double worst=0, worstA=0; int diff=0, n=0;
 for (float a=0.f; a<360.f; a+=0.0137f){ float x=a*0x1.1df46ap-6f, s, c; fb_sincos_f(x,&s,&c);
   worst=fmax(worst,fmax(fabs((double)s-sin((double)x)),fabs((double)c-cos((double)x))));
   if (s!=sinf(x)||c!=cosf(x)) diff++; n++;
   float y=sinf(x)*37.f, xx=cosf(x)*37.f; double t=atan2((double)y,(double)xx)*180/M_PI; if(t<0)t+=360;
   double e=fabs(fb_fast_atan2(y,xx)-t); if(e>180)e=360-e; worstA=fmax(worstA,e);}
 printf("%g %g %d %d\n", worst, worstA, diff, n); }'''
    d = tempfile.mkdtemp()
    open(os.path.join(d, "t.cpp"), "w").write(src)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(O.ROOT, "oracle"), os.path.join(d, "t.cpp"), "-o", os.path.join(d, "t")])
    worst, worstA, diff, n = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    assert float(worst) < 6e-8          # half an ulp of float near 1
    assert float(worstA) < 0.3          # cv::fastAtan2 accuracy ~0.3 degrees
    # glibc's cosf/sinf are not correctly rounded (<1 ulp); ours is the correctly rounded value, so a few
    # percent of the angles differ by one ulp.  This is the documented 'parity unpinned' libm seam.
    assert int(diff) <= int(n) // 20


def test_grid_window_inclusive_vs_exclusive():
    """GetFeaturesInArea uses inclusive cell loops, GetFeaturesInAreaBirdview exclusive ones."""
    def one(x):
        cur = np.zeros(2, cabi.KP_DTYPE)
        cur["x"] = [x, 3.0]
        cur["y"] = [100.0, 3.0]
        ref = cur.copy()
        d = synth.random_descriptors(synth.rng(5), 2)
        prob = dict(cols=512, rows=512, cur_kps=cur, cur_desc=d, ref_kps=ref, ref_desc=d.copy())
        geom = P.grid_geom(synth.bird_grid_geom(512, 512))
        cs, ci = P.build_grid_host([cur], geom, O.grid_build, 2)
        a, out, keep = P.birdview_args([prob], cs, ci, check_ori=0)
        O.call("orc_match_birdview", a)
        return out["match_ref_to_cur"][0].tolist()
    assert one(100.0)[0] == 0      # cell 6, window cells [5,7) -> found (index 0: counted, see next test)
    assert one(500.0)[0] == -1     # keypoint sits in cell 31 but the exclusive loop stops at ix < 31


def test_birdview_index_zero_is_dropped_from_dmatches():
    """vnMatches12[i] > 0 (ORBmatcher.cc:1755): a match to train index 0 is counted but never emitted."""
    cur = np.zeros(3, cabi.KP_DTYPE)
    cur["x"] = [100.0, 200.0, 300.0]
    cur["y"] = [100.0, 200.0, 300.0]
    d = synth.random_descriptors(synth.rng(6), 3)
    prob = dict(cols=512, rows=512, cur_kps=cur, cur_desc=d, ref_kps=cur.copy(), ref_desc=d.copy())
    geom = P.grid_geom(synth.bird_grid_geom(512, 512))
    cs, ci = P.build_grid_host([cur], geom, O.grid_build, 3)
    a, out, keep = P.birdview_args([prob], cs, ci, check_ori=0)
    O.call("orc_match_birdview", a)
    assert out["match_ref_to_cur"][0].tolist() == [0, 1, 2]
    assert out["nmatches"][0] == 3 and out["n_dmatches"][0] == 2


def test_resize_and_blur_of_constant_images():
    p = O.orb_params()
    img = np.full((240, 320), 77, np.uint8)
    for l in range(8):
        assert np.all(O.orb_level(p, img, l) == 77)
    out = np.zeros_like(img)
    O.lib().orc_gaussian_blur7(C.c_void_p(img.ctypes.data), 320, 240, C.c_void_p(out.ctypes.data))
    # OpenCV 3.0-3.3 integer kernel {18,34,49,55,49,34,18} sums to 257: (77*257*257 + 2^15) >> 16 = 78
    assert np.all(out == (77 * 257 * 257 + 32768) >> 16)


def test_fast_detects_an_isolated_corner():
    img = np.full((120, 160), 40, np.uint8)
    img[50:, 70:] = 200   # one bright quadrant -> an L-corner at (70, 50)
    # a perfect step corner gives equal scores on neighbouring pixels and the strict 3x3 NMS of cv::FAST
    # then removes all of them: that is the restated behaviour
    assert len(O.orb_candidates(O.orb_params(), img, 0)) == 0
    img[50, 70] = 255     # make the corner pixel the unique maximum
    c = O.orb_candidates(O.orb_params(), img, 0)
    assert len(c) == 1 and tuple(c[0][:2]) == (70, 50)
    # 11 contiguous ring pixels are darker by 255-40: score = min over the best 9-arc - 1
    assert c[0][2] == 255 - 40 - 1


def test_extract_is_deterministic_and_bounded():
    p = O.orb_params()
    img = synth.synth_image(1000, 640, 480)
    k1, d1 = O.orb_extract(p, img)
    k2, d2 = O.orb_extract(p, img)
    assert np.array_equal(k1, k2) and np.array_equal(d1, d2)
    per = np.bincount(k1["octave"], minlength=8)
    t = O.orb_tables(p)
    for l in range(8):
        assert per[l] <= t.features_per_level[l] + 2       # DistributeOctTree stops at >= N, overshoot <= 2
    assert np.all(k1["x"] / np.array(t.scale_factor[:8])[k1["octave"]] >= 19 - 1e-3)


def test_local_ba_noise_free_converges():
    from fishbirdeyevisualslam_amd import ba_problem
    p = synth.make_ba_problem(4001, n_kf=6, n_mp=300, n_mpb=80, outlier_frac=0.0)
    K = p["kf_true"].reshape(-1, 3, 4).astype(np.float64)
    X = p["mp_true"].astype(np.float64)
    pc = np.einsum("nij,nj->ni", K[p["obs_kf"]][:, :, :3], X[p["obs_mp"]]) + K[p["obs_kf"]][:, :, 3]
    p["obs_uv"] = np.ascontiguousarray(np.stack([pc[:, 0] / pc[:, 2] * p["fx"] + p["cx"], pc[:, 1] / pc[:, 2] * p["fy"] + p["cy"]], 1).astype(np.float32))
    a, out, keep = ba_problem.local_ba_args(p, with_odom=0)
    e0 = np.abs(out["kf_Tcw"] - p["kf_true"]).max()
    O.call("orc_local_ba", a)
    assert np.abs(out["kf_Tcw"] - p["kf_true"]).max() < 0.01 * e0
    assert out["obs_outlier"].sum() == 0
