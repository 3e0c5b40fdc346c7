"""fb_sim3_solver_dev / fb_sim3_solver on the device against the CPU restatement of the reference's serial class
(tests/sim3_solver_ref.py), and the loop-closing chain SearchByBoW -> Sim3Solver -> SearchBySim3 without a host copy."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import sim3_solver_ref as R
from fishbirdeyevisualslam_amd import cabi, sim3_problem as SP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXH = cabi.FB_SIM3_MAX_HYP
# Worst element-wise difference of the device against the restatement over all non-razor hypotheses of PARITY_PROBLEMS, measured
# on one MI355X (R absolute, t over max(1, |t|), s relative): R 2.4e-7, t 3.9e-6, s 2.4e-7 (t carries
# dR times the centroid's distance, 10 to 25 here).  The two sides
# share every float expression up to the eigenvector and differ in the rotation route (quaternion in double against
# atan2 -> float angle-axis -> Rodrigues).  Bound = measured x 4 for libm drift, far inside the project's 1e-4 pose tolerance.
SRT_TOL = dict(R=9.6e-7, t=1.6e-5, s=9.6e-7)


def _to_dev(a, keep, out):
    import torch
    dev = torch.device("cuda:0")
    d = {}
    for sub, field, key in SP.INPUT_FIELDS:
        if key not in keep:
            continue
        v = keep[key]
        d[key] = torch.from_numpy(np.ascontiguousarray(v.view(np.uint8) if v.dtype == cabi.KP_DTYPE else v).copy()).to(dev)
        tgt = a if sub is None else getattr(a, sub)
        if getattr(tgt, field):  # (fields the builder left NULL stay NULL)
            cabi.fill(tgt, **{field: d[key]})
    for k in SP.OUTPUT_FIELDS:
        v = out[k]
        d[k] = torch.from_numpy(np.ascontiguousarray(v.view(np.uint8) if v.dtype == cabi.SIM3_CORR_DTYPE else v).copy()).to(dev)
        cabi.fill(a, **{k: d[k]})
    return d


def _run_dev(p, accept_above=None, with_index=True, tweak=None):
    """-> (rc, host copies of the outputs, (device tensors, args))"""
    import torch
    import fishbirdeyevisualslam_amd as fb
    a, out, keep = SP.solver_args(p, accept_above, with_index)
    d = _to_dev(a, keep, out)
    lib = fb.lib()
    lib.fb_sim3_solver_workspace.restype = C.c_size_t
    wsb = lib.fb_sim3_solver_workspace(a.n_cand, a.kf1.kf_stride)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=torch.device("cuda:0"))
    cabi.fill(a, workspace=ws, workspace_bytes=wsb)
    if tweak:
        tweak(a)
    s = torch.cuda.current_stream()
    rc = lib.fb_sim3_solver_dev(C.byref(a), C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    host = {k: d[k].cpu().numpy() for k in SP.OUTPUT_FIELDS}
    host["corr"] = host["corr"].view(cabi.SIM3_CORR_DTYPE).reshape(p["C"], p["n1"])
    return rc, host, (d, a, ws, keep)


def _check(p, got, tab, accept_above=None):
    """-> worst s / R / t differences over the non-razor rows"""
    worst = dict(R=0.0, t=0.0, s=0.0)
    for c, T in enumerate(tab):
        N, nh = T["N"], T["n_hyp_done"]
        assert int(got["N"][c]) == N
        np.testing.assert_array_equal(got["indices1"][c, :N], T["indices1"])
        for f in cabi.SIM3_CORR_DTYPE.names:  # float expressions with no libm in them: equal
            assert np.array_equal(got["corr"][c, :N][f], T["corr"][f], equal_nan=True), (c, f)
        assert int(got["max_its"][c]) == T["max_its"] and int(got["n_hyp_done"][c]) == nh
        # the accept rule against the device's OWN counts
        above = p["min_inliers"] if accept_above is None else int(accept_above[c])
        mine = R.accept_rule(got["n_inliers"][c, :nh], above)
        np.testing.assert_array_equal(got["accept"][c, :nh], mine)
        assert not got["accept"][c, nh:].any()
        hits = np.nonzero(mine)[0]
        assert int(got["first_accept"][c]) == (hits[0] if len(hits) else -1)
        assert int(got["no_more"][c]) == (0 if len(hits) else 1)
        if N < p["min_inliers"]:
            assert nh == 0 and int(got["first_accept"][c]) == -1 and int(got["no_more"][c]) == 1
        ok = ~T["razor_row"]
        words = (N + 31) // 32
        # a row set aside for a decision inside the band still has to agree on every correspondence outside the band
        for k in np.nonzero(T["razor_row"] & (T["gap"] >= R.RAZOR_GAP))[0]:
            diff = (got["inlier_mask"][c, k, :words] ^ T["inlier_mask"][k, :words]) & ~T["band_mask"][k, :words]
            assert not diff.any(), "razor row %d of candidate %d differs outside the band" % (k, c)
            assert abs(int(got["n_inliers"][c, k]) - int(T["n_inliers"][k])) <= int(T["n_razor"][k])
        np.testing.assert_array_equal(got["n_inliers"][c, :nh][ok], T["n_inliers"][ok], err_msg="n_inliers of candidate %d" % c)
        np.testing.assert_array_equal(got["inlier_mask"][c, :nh, :words][ok], T["inlier_mask"][:, :words][ok])
        # ... and against the restatement's wherever no razor hypothesis precedes
        clean = nh if ok.all() else int(np.argmin(ok))
        np.testing.assert_array_equal(got["accept"][c, :clean], T["accept"][:clean])
        if ok.all():
            assert int(got["first_accept"][c]) == T["first_accept"] and int(got["no_more"][c]) == T["no_more"]
        for k in np.nonzero(ok)[0]:
            tn = max(1.0, float(np.linalg.norm(T["t"][k].astype(np.float64))))
            dR = np.abs(got["R"][c, k].astype(np.float64) - T["R"][k])
            dt = np.abs(got["t"][c, k].astype(np.float64) - T["t"][k]) / tn
            ds = abs(float(got["s"][c, k]) - float(T["s"][k])) / abs(float(T["s"][k]))
            if not (np.isfinite(T["R"][k]).all() and np.isfinite(T["t"][k]).all() and np.isfinite(T["s"][k])):
                assert np.array_equal(np.isfinite(got["R"][c, k]), np.isfinite(T["R"][k]))  # inf / NaN stay inf / NaN
                continue
            worst["R"] = max(worst["R"], float(dR.max()))
            worst["t"] = max(worst["t"], float(dt.max()))
            worst["s"] = max(worst["s"], ds)
    return worst


@pytest.mark.parametrize("seed,n_corr,kw", R.PARITY_PROBLEMS)
def test_parity_with_the_serial_class(seed, n_corr, kw):
    p = SP.make_problem(seed, n_corr, **kw)
    tab = R.full_table(p)
    dec, hyp = R.razor_shares(p, tab)
    assert dec <= R.RAZOR_DECISION_CAP and hyp <= R.RAZOR_HYPOTHESIS_CAP
    rc, got, _ = _run_dev(p)
    assert rc == 0
    worst = _check(p, got, tab)
    print("sim3 solver seed %d worst |dR| %.3g |dt|/max(1,|t|) %.3g |ds|/s %.3g razor rows %d of %d" % (
        seed, worst["R"], worst["t"], worst["s"], sum(int(t["razor_row"].sum()) for t in tab), sum(t["n_hyp_done"] for t in tab)))
    for k in ("R", "t", "s"):
        assert worst[k] <= SRT_TOL[k] <= 1e-4, (k, worst[k])
    assert any(t["first_accept"] >= 0 for t in tab) or max(n_corr) <= 20


def test_accept_above_and_null_index_arrays():
    p = SP.make_problem(211, [120, 64, 30], n1=500, n2=500, outlier_share=0.55, pixel_noise=0.3)
    above = np.array([15, 20, 15], np.int32)
    rc, got, _ = _run_dev(p, accept_above=above)
    assert rc == 0
    _check(p, got, R.full_table(p, accept_above=above), above)
    rc, got2, _ = _run_dev(p, with_index=False)  # NULL index arrays = identity: the index -1 plants are kept now
    assert rc == 0
    tab2 = R.full_table(p, with_index=False)
    assert [t["N"] for t in tab2] == [n + 12 for n in (120, 64, 30)]
    p2 = dict(p, rand_idx=p["rand_idx"])
    _check(p2, got2, tab2)


def test_accept_boundary_matches_the_restatement():
    """The kernel's `n > accept_above` against the restatement's iterate() where a best-so-far count EQUALS the threshold:
    candidate 0 has N == 20 noise-free correspondences (one hypothesis, exactly 20 inliers), candidate 1 has 16 true and 14
    wrong matches (best count exactly 16)."""
    p = SP.make_problem(216, [20, 30], n1=300, n2=300, pixel_noise=0.0, n_outliers=[0, 14])
    for above, want_first0 in ((np.array([20, 16], np.int32), -1), (np.array([19, 15], np.int32), 0)):
        tab = R.full_table(p, accept_above=above)
        assert tab[0]["n_inliers"].tolist() == [20] and tab[1]["n_inliers"].max() == 16
        assert not any(t["razor_row"].any() for t in tab)
        rc, got, _ = _run_dev(p, accept_above=above)
        assert rc == 0
        _check(p, got, tab, above)
        for c, T in enumerate(tab):  # no razor row: the whole accept column, first_accept and no_more are the restatement's
            nh = T["n_hyp_done"]
            np.testing.assert_array_equal(got["n_inliers"][c, :nh], T["n_inliers"])
            np.testing.assert_array_equal(got["accept"][c, :nh], T["accept"])
            assert int(got["first_accept"][c]) == T["first_accept"] and int(got["no_more"][c]) == T["no_more"]
        assert int(got["first_accept"][0]) == want_first0 and int(got["n_inliers"][0, 0]) == 20
        at16 = (tab[1]["n_inliers"] == 16) & (tab[1]["is_best"] == 1)
        assert at16.any() and (got["accept"][1, :len(at16)][at16] == (1 if above[1] == 15 else 0)).all()
    # default threshold (accept_above = NULL) is min_inliers itself
    rc, got, _ = _run_dev(p)
    assert rc == 0 and int(got["accept"][0, 0]) == 0 and int(got["no_more"][0]) == 1


def test_key_frame_too_large_for_lds_reads_the_workspace():
    """3500 features are 168 000 B of correspondence fields, above the LDS of a CU: k_sim3_hypotheses' global-memory variant."""
    p = SP.make_problem(217, [500, 25, 1200], n1=3500, n2=1500, outlier_share=0.3, pixel_noise=0.2)
    tab = R.full_table(p)
    rc, got, _ = _run_dev(p)
    assert rc == 0
    worst = _check(p, got, tab)
    for k in ("R", "t", "s"):
        assert worst[k] <= SRT_TOL[k], (k, worst[k])
    assert tab[0]["first_accept"] >= 0 and tab[2]["first_accept"] >= 0


@pytest.mark.parametrize("n1", R.LDS_BOUNDARY_STRIDES)
def test_last_stride_in_lds_and_first_on_the_workspace(n1):
    """KF1 strides 3402 and 3403: 163 296 B of correspondence fields are the last that fit beside k_sim3_hypotheses' LDS budget
    (160 KiB - 512 B), 163 344 B the first that do not (csrc/sim3_plan.h).  A few dozen kept pairs; the parity test's checks."""
    p = SP.make_problem(219, [60, 25], n1=n1, n2=300, outlier_share=0.3, pixel_noise=0.2)
    tab = R.full_table(p)
    rc, got, _ = _run_dev(p)
    assert rc == 0
    worst = _check(p, got, tab)
    print("sim3 solver stride %d worst |dR| %.3g |dt|/max(1,|t|) %.3g |ds|/s %.3g" % (n1, worst["R"], worst["t"], worst["s"]))
    for k in ("R", "t", "s"):
        assert worst[k] <= SRT_TOL[k], (k, worst[k])
    assert [t["N"] for t in tab] == [60, 25] and tab[0]["first_accept"] >= 0


def _check_walk(got, tab):
    for c, T in enumerate(tab):
        N = T["N"]
        assert int(got["N"][c]) == N
        np.testing.assert_array_equal(got["indices1"][c, :N], T["indices1"])
        assert (got["indices1"][c, N:] == -7).all()  # rows past N are not written
        for f in cabi.SIM3_CORR_DTYPE.names:
            assert np.array_equal(got["corr"][c, :N][f], T["corr"][f], equal_nan=True), (c, f)


def test_walk_at_the_block_seams_and_with_every_skip_clause():
    """The walk of k_sim3_prepare (s3::walk_pairs): kept counts 255 / 256 / 257 around the 256 threads of k_sim3_prepare,
    and one candidate in which every clause of s3::keep_pair skips a pair.  N, indices1 and corr equal the restatement's."""
    seed, n_corr, kw = R.SEAM_PROBLEM
    p = SP.make_problem(seed, n_corr, **kw)
    tab = R.full_table(p)
    assert [t["N"] for t in tab] == [255, 256, 257]
    rc, got, _ = _run_dev(p)
    assert rc == 0
    _check_walk(got, tab)
    p, ref, N = R.skip_clause_problem()
    tab = R.full_table(ref)
    assert tab[0]["N"] == N
    rc, got, _ = _run_dev(p)
    assert rc == 0
    _check_walk(got, tab)
    _check(ref, got, tab)


def test_other_ransac_parameters_follow_set_ransac_parameters():
    """mRansacMaxIts for min_inliers = 100 and a cap of 150 (N at, just above and far above min_inliers), and p = 0.9."""
    for prob, mi, cap in ((0.99, 100, 150), (0.9, 40, 300)):
        p = SP.make_problem(218, [mi, mi + 1, mi + 50, 4 * mi, 8 * mi + 3], n1=1200, n2=1200, outlier_share=0.2, pixel_noise=0.1,
                            min_inliers=mi, max_iterations=cap)
        p["ransac_prob"] = prob
        tab = R.full_table(p)
        assert tab[0]["max_its"] == 1 and tab[1]["max_its"] <= tab[2]["max_its"] and 1 < tab[2]["max_its"] < cap and tab[4]["max_its"] == cap
        rc, got, _ = _run_dev(p)
        assert rc == 0
        _check(p, got, tab)


def test_host_drop_in_is_byte_equal_to_dev():
    import fishbirdeyevisualslam_amd as fb
    p = SP.make_problem(212, [300, 19, 700, 45], n1=1100, n2=1000, outlier_share=0.3, pixel_noise=0.2)
    rc, got, _ = _run_dev(p)
    assert rc == 0
    a, out, keep = SP.solver_args(p)
    assert fb.lib().fb_sim3_solver(C.byref(a)) == 0, fb.lib().fb_last_error()
    for k in SP.OUTPUT_FIELDS:
        assert out[k].tobytes() == np.ascontiguousarray(got[k]).tobytes(), k
    assert out["N"].tolist() == [300, 19, 700, 45]


def test_bad_arguments_are_rejected_before_any_launch():
    import fishbirdeyevisualslam_amd as fb
    p = SP.make_problem(213, [100], n1=300, n2=300)
    lib = fb.lib()
    for tweak in (lambda a: setattr(a, "n_cand", 0), lambda a: setattr(a, "max_iterations", MAXH + 1), lambda a: setattr(a, "min_inliers", 2),
                  lambda a: setattr(a, "workspace_bytes", 16), lambda a: setattr(a, "rand_idx", None), lambda a: setattr(a.mp1, "mp_stride", 299),
                  lambda a: setattr(a, "ransac_prob", 1.0)):
        rc, got, _ = _run_dev(p, tweak=tweak)
        assert rc == cabi.FB_ERR_ARG, lib.fb_last_error()
        assert (got["N"] == -7).all() and (got["accept"] == 9).all()  # nothing ran
    rc, got, _ = _run_dev(p, tweak=lambda a: setattr(a, "min_inliers", 400))  # any min_inliers is served; here N = 100 is below it
    assert rc == 0 and int(got["N"][0]) == 100 and int(got["n_hyp_done"][0]) == 0 and int(got["no_more"][0]) == 1
    rc, got, _ = _run_dev(p)  # and the library works afterwards
    assert rc == 0
    _check(p, got, R.full_table(p))


def test_host_header_solver_replays_iterate_round_robin():
    """tests/cpp/sim3_solver_host_test.cpp drives fishbird::Sim3Solver (host/fishbird_host.hpp) with iterate(5) round-robin over
    three candidates in one fresh child process; the restatement (linked in) gets the same draws and must return alike."""
    import fishbirdeyevisualslam_amd as fb
    pkg = os.path.dirname(fb.LIB_PATH)
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "sim3_solver_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"),
                           os.path.join(ROOT, "tests", "cpp", "sim3_solver_host_test.cpp"), os.path.join(ROOT, "tests", "cpp", "sim3_solver_ref.cpp"),
                           "-o", exe, "-L", pkg, "-lfishbird_hip", "-Wl,-rpath," + pkg])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"sim3_solver_host_test ok" in r.stdout


def _on_device(struct, arrays, hold):
    import torch
    for k, v in arrays.items():
        t = torch.from_numpy(np.ascontiguousarray(v.view(np.uint8) if v.dtype == cabi.KP_DTYPE else v).copy()).to("cuda:0")
        hold.append(t)
        cabi.fill(struct, **{k: t})
        arrays[k] = t


def test_bow_matches_feed_the_solver_and_search_by_sim3_on_the_device():
    """LoopClosing::ComputeSim3's chain for one candidate: fb_match_bow_kf_dev's matches12 is the solver's input where it lies,
    and the accepted hypothesis' rows of the s / R / t tables are fb_match_sim3_dev's s12 / R12 / t12 (picked by a device-side
    gather on first_accept) -- one stream, no host copy in between.  Equal to the three host-pointer calls run one by one."""
    import torch
    import fishbirdeyevisualslam_amd as fb
    import oracle_lib as O
    from fishbirdeyevisualslam_amd import kf_problems as KP, more_problems as M, problems as P, synth
    lib = fb.lib()
    n1, n2 = 1500, 1400
    q = KP.make_sim3_problem(8300, n1, n2, 900)
    bp = dict(kps1=q["kps1"], desc1=q["desc1"], has_mp1=q["mp_valid1"], kps2=q["kps2"], desc2=q["desc2"], has_mp2=q["mp_valid2"])
    geom = P.grid_geom(synth.front_grid_geom(KP.W, KP.H))
    g1 = P.build_grid_host([q["kps1"]], geom, O.grid_build, n1)
    g2 = P.build_grid_host([q["kps2"]], geom, O.grid_build, n2)
    sig2 = np.asarray(synth.scale_tables()[2], np.float32)

    def solver_problem(m12, rand_idx=None):
        p = dict(C=1, n1=n1, n2=n2, kps1=q["kps1"], valid1=q["mp_valid1"], index1=np.arange(n1, dtype=np.int32), xw1=q["mp_xw1"], T1=q["T1w"],
                 cands=[dict(kps2=q["kps2"], valid2=q["mp_valid2"], index2=np.arange(n2, dtype=np.int32), xw2=q["mp_xw2"], T2=q["T2w"], matches12=m12)],
                 level_sigma2=sig2, fix_scale=1, fx=KP.FX, fy=KP.FY, cx=KP.W / 2.0, cy=KP.H / 2.0, ransac_prob=0.99, min_inliers=20,
                 max_iterations=MAXH, rand_idx=rand_idx)
        return p

    # ---- the three steps from host memory, one by one
    ab, ob, _kb = M.bow_kf_args([bp])
    assert lib.fb_match_bow_kf(C.byref(ab)) == 0, lib.fb_last_error()
    p = solver_problem(ob["matches12"][0].copy())
    N = SP.count_kept(p, 0)
    assert N >= 40  # enough above min_inliers for the RANSAC to run (SearchByBoW keeps a few dozen of the 900 shared points)
    p["rand_idx"] = SP.random_int_table(np.random.default_rng(8301), N)[None]
    a_s, o_s, _ks = SP.solver_args(p, with_index=False)
    assert lib.fb_sim3_solver(C.byref(a_s)) == 0, lib.fb_last_error()
    k = int(o_s["first_accept"][0])
    assert int(o_s["N"][0]) == N and k >= 0 and o_s["n_inliers"][0, k] > 20
    q_h = dict(q, s12=o_s["s"][0, k], R12=o_s["R"][0, k].copy(), t12=o_s["t"][0, k].copy())
    a_m, o_m, _km = KP.sim3_args([q_h], g1, g2)
    assert lib.fb_match_sim3(C.byref(a_m)) == 0, lib.fb_last_error()
    assert o_m["nfound"][0] > 20
    # ---- the same on the device, each call reading the previous one's output where it lies
    hold = []
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ab2, ob2, (kb2, f1, f2) = M.bow_kf_args([bp])
    _on_device(ab2, kb2, hold)
    _on_device(ab2, ob2, hold)
    for fv, kk in ((ab2.fv1, f1), (ab2.fv2, f2)):
        _on_device(fv, dict(zip(("n_nodes", "node_ids", "node_start", "items"), kk)), hold)
    assert lib.fb_match_bow_kf_dev(C.byref(ab2), st) == 0, lib.fb_last_error()
    a2, o2, k2 = SP.solver_args(p, with_index=False)
    d = _to_dev(a2, k2, o2)
    cabi.fill(a2, matches12=ob2["matches12"])  # the matcher's device output
    lib.fb_sim3_solver_workspace.restype = C.c_size_t
    wsb = lib.fb_sim3_solver_workspace(1, n1)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda:0")
    cabi.fill(a2, workspace=ws, workspace_bytes=wsb)
    assert lib.fb_sim3_solver_dev(C.byref(a2), st) == 0, lib.fb_last_error()
    row = d["first_accept"].long().clamp(min=0)  # device-side choice of the accepted row
    s12 = d["s"][0].index_select(0, row).contiguous()
    R12 = d["R"][0].index_select(0, row).contiguous()
    t12 = d["t"][0].index_select(0, row).contiguous()
    a3, o3, (kk1, kk2, mk1, mk2, k3) = KP.sim3_args([q_h], g1, g2)
    for struct, arrays in ((a3.kf1, kk1), (a3.kf2, kk2), (a3.mp1, mk1), (a3.mp2, mk2), (a3, k3), (a3, o3)):
        _on_device(struct, arrays, hold)
    cabi.fill(a3, s12=s12, R12=R12, t12=t12)
    assert lib.fb_match_sim3_dev(C.byref(a3), st) == 0, lib.fb_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ob2["matches12"].cpu().numpy(), ob["matches12"])
    for f in ("N", "first_accept", "n_inliers", "s", "R", "t", "accept"):
        assert d[f].cpu().numpy().tobytes() == o_s[f].tobytes(), f
    np.testing.assert_array_equal(o3["matches12"].cpu().numpy(), o_m["matches12"])
    np.testing.assert_array_equal(o3["nfound"].cpu().numpy(), o_m["nfound"])
