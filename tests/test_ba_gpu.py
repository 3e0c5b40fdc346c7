"""GPU parity: HIP local bundle adjustment (C-ABI fb_local_ba) vs the CPU oracle.

Tolerance (BASELINE.json north_star): poses / landmarks within 1e-4 relative, PER ELEMENT (each pose by max(1, max|T_k|) of
its own 3x4, each landmark by max(1, ||x||): ba_cases.pose_rel / point_rel); the outlier flags are integer results and must
be identical.
"""
import time

import numpy as np
import pytest

import ba_cases as BC
import hip_lib as H
import oracle_lib as O
from fishbirdeyevisualslam_amd import ba_problem, synth

pytestmark = pytest.mark.gpu
REL_TOL = 1e-4


def _rel_pose(a, b):
    return BC.worst_pose_rel(a, b)


def _rel_pt(a, b):
    return BC.worst_point_rel(a, b)


def _run(p, **kw):
    a, out_o, keep = ba_problem.local_ba_args(p, **kw)
    t0 = time.perf_counter()
    O.call("orc_local_ba", a)
    t_cpu = time.perf_counter() - t0
    a2, out_h, keep2 = ba_problem.local_ba_args(p, **kw)
    t0 = time.perf_counter()
    H.call("fb_local_ba", a2)
    t_gpu = time.perf_counter() - t0
    return out_o, out_h, t_cpu, t_gpu


def _compare(p, out_o, out_h, with_odom):
    wp, wl = _rel_pose(out_h["kf_Tcw"], out_o["kf_Tcw"]), _rel_pt(out_h["mp_xw"], out_o["mp_xw"])
    wb = _rel_pt(out_h["mpb_xw"], out_o["mpb_xw"]) if with_odom else 0.0
    print("worst per-element difference: poses %.3g, landmarks %.3g, bird landmarks %.3g" % (wp, wl, wb))
    assert wp <= REL_TOL
    # landmarks: each relative to its own distance from the origin
    assert wl <= REL_TOL
    np.testing.assert_array_equal(out_h["obs_outlier"], out_o["obs_outlier"])
    if with_odom:
        assert wb <= REL_TOL
        np.testing.assert_array_equal(out_h["bobs_outlier"][: len(p["bobs_kf"])], out_o["bobs_outlier"][: len(p["bobs_kf"])])
    # fixed keyframes are returned untouched
    fx = p["kf_fixed"] == 1
    np.testing.assert_array_equal(out_h["kf_Tcw"][fx], p["kf_Tcw"][fx])


@pytest.mark.parametrize("with_odom", [1, 0])
def test_local_ba_small(with_odom):
    p = synth.make_ba_problem(4000, n_kf=6, n_mp=500, n_mpb=120)
    out_o, out_h, _, _ = _run(p, with_odom=with_odom)
    _compare(p, out_o, out_h, with_odom)
    # the optimiser moved the free keyframes towards the generating poses
    e0 = np.abs(p["kf_Tcw"] - p["kf_true"]).max()
    e1 = np.abs(out_h["kf_Tcw"] - p["kf_true"]).max()
    assert e1 < 0.5 * e0


def test_local_ba_config4():
    """BASELINE config 4: 20 keyframes x 8k map points (+2k bird points, odometry chain)."""
    p = synth.make_ba_problem(4000, n_kf=20, n_mp=8000, n_mpb=2000)
    out_o, out_h, t_cpu, t_gpu = _run(p, with_odom=1)
    _compare(p, out_o, out_h, 1)
    print("config4: %d front + %d bird edges, oracle %.1f ms, HIP %.1f ms (incl. upload/download)" %
          (len(p["obs_kf"]), len(p["bobs_kf"]), t_cpu * 1e3, t_gpu * 1e3))


def test_local_ba_stop_flag_and_weights():
    p = synth.make_ba_problem(4002, n_kf=5, n_mp=300, n_mpb=60)
    stop = np.ones(1, np.uint8)  # pbStopFlag already set: nothing is touched (Optimizer.cc:2498-2500)
    out_o, out_h, _, _ = _run(p, with_odom=1, stop_flag=stop)
    np.testing.assert_array_equal(out_h["kf_Tcw"], p["kf_Tcw"])
    np.testing.assert_array_equal(out_o["kf_Tcw"], p["kf_Tcw"])
    out_o, out_h, _, _ = _run(p, with_odom=1, wF=2.0, wB=0.5)
    _compare(p, out_o, out_h, 1)


def test_local_ba_rejects_duplicate_observation():
    import fishbirdeyevisualslam_amd as fb
    p = synth.make_ba_problem(4003, n_kf=4, n_mp=50, n_mpb=10)
    p["obs_kf"] = p["obs_kf"].copy()
    p["obs_kf"][1] = p["obs_kf"][0]
    p["obs_mp"] = p["obs_mp"].copy()
    p["obs_mp"][1] = p["obs_mp"][0]
    a, out, keep = ba_problem.local_ba_args(p, with_odom=1)
    with pytest.raises(fb.FishbirdError):
        H.call("fb_local_ba", a)


def test_local_ba_observations_in_any_order():
    """The host side has a fast path for observations grouped by point (the order the reference produces); shuffled
    observations take the general CSR build: same result as the oracle, and a duplicate is still refused there."""
    import fishbirdeyevisualslam_amd as fb
    p = synth.make_ba_problem(4006, n_kf=6, n_mp=400, n_mpb=80)
    g = np.random.default_rng(7)
    pf, pb = g.permutation(len(p["obs_kf"])), g.permutation(len(p["bobs_kf"]))
    for k in ("obs_kf", "obs_mp", "obs_uv", "obs_inv_sigma2"):
        p[k] = np.ascontiguousarray(p[k][pf])
    for k in ("bobs_kf", "bobs_mpb", "bobs_xc", "bobs_inv_sigma2"):
        p[k] = np.ascontiguousarray(p[k][pb])
    out_o, out_h, _, _ = _run(p, with_odom=1)
    _compare(p, out_o, out_h, 1)
    q = dict(p)
    q["obs_kf"] = p["obs_kf"].copy(); q["obs_mp"] = p["obs_mp"].copy()
    q["obs_kf"][-1] = q["obs_kf"][0]; q["obs_mp"][-1] = q["obs_mp"][0]
    a, out, keep = ba_problem.local_ba_args(q, with_odom=1)
    with pytest.raises(fb.FishbirdError):
        H.call("fb_local_ba", a)


def test_local_ba_structure_only_and_no_bird():
    """Edge cases of the device-resident schedule: every key frame fixed (no pose system at all: structure-only BA), and a
    graph without bird points / odometry edges."""
    p = synth.make_ba_problem(4004, n_kf=5, n_mp=300, n_mpb=60)
    p["kf_fixed"] = np.ones_like(p["kf_fixed"])
    out_o, out_h, _, _ = _run(p, with_odom=1)
    _compare(p, out_o, out_h, 1)
    assert np.abs(out_h["mp_xw"] - p["mp_xw"]).max() > 0          # the points did move
    q = synth.make_ba_problem(4005, n_kf=6, n_mp=400, n_mpb=80)
    for k in ("bobs_kf", "bobs_mpb", "bobs_inv_sigma2", "odom_kf_i", "odom_kf_j", "odom_info"):
        q[k] = q[k][:0]
    q["bobs_xc"] = q["bobs_xc"][:0]
    q["odom_Tij"] = q["odom_Tij"][:0]
    out_o, out_h, _, _ = _run(q, with_odom=1)
    wp, wl = _rel_pose(out_h["kf_Tcw"], out_o["kf_Tcw"]), _rel_pt(out_h["mp_xw"], out_o["mp_xw"])
    print("no bird points: worst per-element difference: poses %.3g, landmarks %.3g" % (wp, wl))
    assert wp <= REL_TOL and wl <= REL_TOL
    np.testing.assert_array_equal(out_h["obs_outlier"], out_o["obs_outlier"])


def test_local_ba_host_paced_schedule_still_matches(monkeypatch):
    """FB_BA_HOST_LM=1 runs the device-resident Levenberg-Marquardt schedule host-paced (one slot per batch, the control block
    read back after each) on a small problem."""
    monkeypatch.setenv("FB_BA_HOST_LM", "1")
    p = synth.make_ba_problem(4006, n_kf=6, n_mp=500, n_mpb=120)
    out_o, out_h, _, _ = _run(p, with_odom=1)
    _compare(p, out_o, out_h, 1)


def test_local_ba_28_free_key_frames_host_paced_equals_default(monkeypatch):
    """28 free key frames (P6 = 168: three full panels of 48 and a last one 24 wide) on the HBM-resident path against the
    oracle, and the same call host-paced (FB_BA_HOST_LM=1): byte-equal, so the kernels of ba_big.inc do nothing in the slots
    the default take enqueues beyond the end of the schedule."""
    p = synth.make_ba_problem(4210, n_kf=30, n_fixed=2, n_mp=300, n_mpb=60)
    assert int((p["kf_fixed"] == 0).sum()) == 28
    out_o, out_h, _, _ = _run(p, with_odom=1)
    _compare(p, out_o, out_h, 1)
    monkeypatch.setenv("FB_BA_HOST_LM", "1")
    a, out_p, keep = ba_problem.local_ba_args(p, with_odom=1)
    H.call("fb_local_ba", a)
    for k in ("kf_Tcw", "mp_xw", "mpb_xw", "obs_outlier", "bobs_outlier"):
        assert out_p[k].tobytes() == out_h[k].tobytes(), k


def test_local_ba_stop_flag_raised_while_running():
    """pbStopFlag set from another thread while the schedule runs: the call returns early with a valid (finite) state; the same
    call without the flag does more work."""
    import threading
    p = synth.make_ba_problem(4000, n_kf=20, n_mp=8000, n_mpb=2000)
    stop = np.zeros(1, np.uint8)
    a, out, keep = ba_problem.local_ba_args(p, with_odom=1, stop_flag=stop)
    t = threading.Timer(0.0008, lambda: stop.__setitem__(0, 1))
    t.start()
    H.call("fb_local_ba", a)
    t.join()
    assert np.isfinite(out["kf_Tcw"]).all() and np.isfinite(out["mp_xw"]).all()
    assert set(np.unique(out["obs_outlier"]).tolist()) <= {0, 1}


# ---- fb_local_ba_dev: the graph resident in HBM, built by kernels ------------------------------------------------------------
def _run_dev(p, **kw):
    import ctypes as C
    import torch
    import fishbirdeyevisualslam_amd as fb
    a, dev, keep = ba_problem.local_ba_args_dev(p, **kw)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc = fb.lib().fb_local_ba_dev(C.byref(a), C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in dev.items()}


@pytest.mark.parametrize("with_odom,shuffle", [(1, False), (1, True), (0, True)])
def test_local_ba_dev_equals_host_entry(with_odom, shuffle):
    """Device-resident inputs + device graph builder: bit-identical to fb_local_ba (same edge order inside every landmark /
    key frame, so the same sums), and therefore the same parity with the oracle."""
    p = synth.make_ba_problem(4100, n_kf=12, n_mp=2500, n_mpb=600)
    if shuffle:  # observations in arbitrary order: the builder's sort has to restore the ascending edge order
        g = synth.rng(1)
        perm = g.permutation(len(p["obs_kf"]))
        for k in ("obs_kf", "obs_mp", "obs_uv", "obs_inv_sigma2"):
            p[k] = np.ascontiguousarray(p[k][perm])
        permb = g.permutation(len(p["bobs_kf"]))
        for k in ("bobs_kf", "bobs_mpb", "bobs_xc", "bobs_inv_sigma2"):
            p[k] = np.ascontiguousarray(p[k][permb])
    out_o, out_h, _, _ = _run(p, with_odom=with_odom)
    rc, out_d = _run_dev(p, with_odom=with_odom)
    assert rc == 0
    _compare(p, out_o, out_h, with_odom)
    for k in ("kf_Tcw", "mp_xw", "obs_outlier") + (("mpb_xw",) if with_odom else ()):
        np.testing.assert_array_equal(out_d[k], out_h[k], err_msg=k)
    if with_odom:
        nb = len(p["bobs_kf"])
        np.testing.assert_array_equal(out_d["bobs_outlier"][:nb], out_h["bobs_outlier"][:nb])


def test_local_ba_dev_config4_time():
    """BASELINE configs[3] from device inputs (verdict of round 2: <= 2.1 ms wall); prints the wall time."""
    import ctypes as C
    import torch
    import fishbirdeyevisualslam_amd as fb
    p = synth.make_ba_problem(4000, n_kf=20, n_mp=8000, n_mpb=2000)
    out_o, out_h, _, _ = _run(p, with_odom=1)
    times = []
    for _ in range(5):
        a, dev, keep = ba_problem.local_ba_args_dev(p, with_odom=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fb.lib().fb_local_ba_dev(C.byref(a), None)
        times.append(time.perf_counter() - t0)
        assert rc == 0
    out_d = {k: v.cpu().numpy() for k, v in dev.items()}
    _compare(p, out_o, out_d, 1)
    print("fb_local_ba_dev config 4: %.2f ms wall (median of 5; fb_local_ba from host pointers on the same problem is timed by bench.py)" % (sorted(times)[2] * 1e3))


def test_local_ba_dev_rejects_bad_graphs():
    import fishbirdeyevisualslam_amd as fb
    from fishbirdeyevisualslam_amd import cabi
    p = synth.make_ba_problem(4200, n_kf=6, n_mp=300, n_mpb=60)
    q = dict(p)
    q["obs_mp"] = p["obs_mp"].copy(); q["obs_mp"][5] = len(p["mp_xw"]) + 3       # index out of range
    rc, _ = _run_dev(q, with_odom=1)
    assert rc == cabi.FB_ERR_ARG and b"out of range" in fb.lib().fb_last_error()
    q = dict(p)
    q["obs_kf"] = p["obs_kf"].copy(); q["obs_mp"] = p["obs_mp"].copy()
    q["obs_kf"][1], q["obs_mp"][1] = q["obs_kf"][0], q["obs_mp"][0]                # the same (key frame, point) twice
    rc, _ = _run_dev(q, with_odom=1)
    assert rc == cabi.FB_ERR_ARG and b"duplicate" in fb.lib().fb_last_error()
    rc, _ = _run_dev(p, with_odom=1)                                               # and the library is fine afterwards
    assert rc == 0


def _dev_inputs(p, **kw):
    """The in/out device arrays of a fb_local_ba_dev call as host copies, before the call."""
    a, dev, keep = ba_problem.local_ba_args_dev(p, **kw)
    return a, dev, keep, {k: v.cpu().numpy().copy() for k, v in dev.items()}


def test_local_ba_dev_refuses_a_big_system_before_touching_anything():
    """More than 23 free key frames from device inputs: refused by the plan, before anything is staged or enqueued -- the
    caller's device arrays keep their bytes, and the thread's staging block (filled by an earlier, larger host-pointer
    call) is not read.  The library works afterwards."""
    import ctypes as C
    import torch
    import fishbirdeyevisualslam_amd as fb
    from fishbirdeyevisualslam_amd import cabi
    warm = synth.make_ba_problem(4212, n_kf=6, n_mp=900, n_mpb=120)   # leaves the staging block non-empty
    a0, _, keep0 = ba_problem.local_ba_args(warm, with_odom=1)
    H.call("fb_local_ba", a0)
    p = synth.make_ba_problem(4210, n_kf=30, n_fixed=2, n_mp=300, n_mpb=60)
    assert int((p["kf_fixed"] == 0).sum()) == 28
    a, dev, keep, before = _dev_inputs(p, with_odom=1)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc = fb.lib().fb_local_ba_dev(C.byref(a), C.c_void_p(s.cuda_stream))
    assert rc == cabi.FB_ERR_CAPACITY
    assert b"23 free key frames" in fb.lib().fb_last_error()
    torch.cuda.synchronize()
    for k in ("kf_Tcw", "mp_xw", "mpb_xw", "obs_outlier", "bobs_outlier"):
        got = dev[k].cpu().numpy()
        assert got.tobytes() == before[k].tobytes(), k
    q = synth.make_ba_problem(4211, n_kf=6, n_mp=300, n_mpb=60)
    rc, out_d = _run_dev(q, with_odom=1)
    assert rc == 0
    a2, out_h, keep2 = ba_problem.local_ba_args(q, with_odom=1)
    H.call("fb_local_ba", a2)
    for k in ("kf_Tcw", "mp_xw", "mpb_xw", "obs_outlier"):
        assert out_d[k].tobytes() == out_h[k].tobytes(), k
    nb = len(q["bobs_kf"])
    np.testing.assert_array_equal(out_d["bobs_outlier"][:nb], out_h["bobs_outlier"][:nb])


def test_local_ba_plan_boundary_23_24_free_key_frames():
    """The plan's threshold between the LDS-resident and the HBM-resident reduced system: 23 free key frames run the
    device-resident schedule from either entry point (byte-equal), 24 are refused from device inputs and take the
    HBM-resident path from host pointers; both sides of the boundary meet the oracle bar."""
    from fishbirdeyevisualslam_amd import cabi
    p = synth.make_ba_problem(4220, n_kf=25, n_fixed=2, n_mp=300, n_mpb=60)
    assert int((p["kf_fixed"] == 0).sum()) == 23
    out_o, out_h, _, _ = _run(p, with_odom=1)
    rc, out_d = _run_dev(p, with_odom=1)
    assert rc == 0
    for k in ("kf_Tcw", "mp_xw", "mpb_xw", "obs_outlier"):
        assert out_d[k].tobytes() == out_h[k].tobytes(), k
    nb = len(p["bobs_kf"])
    np.testing.assert_array_equal(out_d["bobs_outlier"][:nb], out_h["bobs_outlier"][:nb])
    _compare(p, out_o, out_h, 1)
    _compare(p, out_o, out_d, 1)
    p = synth.make_ba_problem(4221, n_kf=26, n_fixed=2, n_mp=300, n_mpb=60)
    assert int((p["kf_fixed"] == 0).sum()) == 24
    rc, _ = _run_dev(p, with_odom=1)
    assert rc == cabi.FB_ERR_CAPACITY
    out_o, out_h, _, _ = _run(p, with_odom=1)
    _compare(p, out_o, out_h, 1)


@pytest.mark.parametrize("n_odom", [103, 104])
def test_local_ba_odometry_records_boundary_lds_hbm(n_odom):
    """The plan's threshold for the odometry records (csrc/ba_plan.h, odom_home): up to 103 edges the records and the
    products' scratch lie in LDS (k_ba_lin_c<false>), from 104 the records lie in the scratch block and an edge's products run
    on its lane (k_ba_lin_c<true>).  23 free key frames, so both sides use the LDS-resident reduced system.  The generator
    makes 3 n_kf - 6 edges (105 at 37 key frames): the chain is cut to the count."""
    p = synth.make_ba_problem(4230, n_kf=37, n_fixed=14, n_mp=300, n_mpb=60)
    assert int((p["kf_fixed"] == 0).sum()) == 23 and len(p["odom_kf_i"]) == 105
    for k in ("odom_kf_i", "odom_kf_j", "odom_Tij", "odom_info"):
        p[k] = np.ascontiguousarray(p[k][:n_odom])
    a, _, keep = ba_problem.local_ba_args(p, with_odom=1)
    assert a.n_odom == n_odom
    out_o, out_h, _, _ = _run(p, with_odom=1)
    _compare(p, out_o, out_h, 1)


def test_triangulation_matches_feed_the_ba_on_the_device():
    """LocalMapping's hand-over without a host copy (LocalMapping.cc:231-476 -> :87-96): SearchForTriangulation (M7) runs on
    the device, its match array is turned into new points and observations by device code (torch ops standing in for the host's
    triangulation, LocalMapping.cc:318-470), and fb_local_ba_dev consumes those arrays where they lie.  The same graph
    downloaded and given to the oracle must agree."""
    import ctypes as C
    import torch
    import fishbirdeyevisualslam_amd as fb
    from fishbirdeyevisualslam_amd import bow_problem as BP, cabi
    dev = torch.device("cuda:0")
    prob = BP.make_triangulation_problem(6300, 1800, 1800)
    a, out, (keep, k1, k2) = BP.triangulation_args([prob])
    d = {}

    def up(struct, fields, src):
        for f in fields:
            if src.get(f) is not None:
                d[id(struct), f] = torch.from_numpy(np.ascontiguousarray(src[f])).to(dev)
                cabi.fill(struct, **{f: d[id(struct), f]})
    up(a, ("n1", "kps1", "desc1", "has_mp1", "n2", "kps2", "desc2", "has_mp2", "F12", "Cw1", "R2w", "t2w"), {k: (v.view(np.uint8) if v.dtype == cabi.KP_DTYPE else v) for k, v in keep.items()})
    for fv, kk in ((a.fv1, k1), (a.fv2, k2)):
        up(fv, ("n_nodes", "node_ids", "node_start", "items"), dict(zip(("n_nodes", "node_ids", "node_start", "items"), kk)))
    m12 = torch.full((1, 1800), -1, dtype=torch.int32, device=dev)
    nm = torch.zeros(1, dtype=torch.int32, device=dev)
    cabi.fill(a, matches12=m12, nmatches=nm)
    s = torch.cuda.current_stream()
    fb.check(fb.lib().fb_match_triangulation_dev(C.byref(a), C.c_void_p(s.cuda_stream)), "M7")
    # ---- device-side stand-in for CreateNewMapPoints: matched pairs -> points (midpoint of the two rays) + 2 observations each
    kp1 = torch.from_numpy(np.stack([prob["kps1"]["x"], prob["kps1"]["y"]], 1)).to(dev)
    kp2 = torch.from_numpy(np.stack([prob["kps2"]["x"], prob["kps2"]["y"]], 1)).to(dev)
    oc1 = torch.from_numpy(prob["kps1"]["octave"].astype(np.int64)).to(dev)
    oc2 = torch.from_numpy(prob["kps2"]["octave"].astype(np.int64)).to(dev)
    i1 = torch.nonzero(m12[0] >= 0)[:, 0]
    i2 = m12[0][i1].long()
    npt = int(i1.numel())
    assert npt > 100
    fx, fy, cx, cy = prob["fx"], prob["fy"], prob["cx"], prob["cy"]
    # poses: KF1 = identity frame of reference, KF2 from R2w/t2w and Cw1 (world = the generator's world)
    R2 = torch.from_numpy(prob["R2w"].reshape(3, 3).astype(np.float64)).to(dev)
    t2 = torch.from_numpy(prob["t2w"].astype(np.float64)).to(dev)
    F12 = prob["F12"]
    # recover T1 from the generator (same seed): the test only needs a consistent pair of poses
    g = synth.rng(6300)
    T1 = synth.random_pose(g)
    R1 = torch.from_numpy(T1[:3, :3]).to(dev); t1 = torch.from_numpy(T1[:3, 3]).to(dev)
    ray = lambda kp, R: (torch.stack([(kp[:, 0].double() - cx) / fx, (kp[:, 1].double() - cy) / fy, torch.ones(len(kp), dtype=torch.float64, device=dev)], 1)) @ R
    C1, C2 = -(R1.T @ t1), -(R2.T @ t2)
    r1, r2 = ray(kp1[i1], R1), ray(kp2[i2], R2)
    # closest points of the two rays
    w0 = (C1 - C2)[None]
    a_, b_, c_ = (r1 * r1).sum(1), (r1 * r2).sum(1), (r2 * r2).sum(1)
    d_, e_ = (r1 * w0).sum(1), (r2 * w0).sum(1)
    den = a_ * c_ - b_ * b_
    sc = (b_ * e_ - c_ * d_) / den
    tc = (a_ * e_ - b_ * d_) / den
    X = 0.5 * ((C1 + sc[:, None] * r1) + (C2 + tc[:, None] * r2))
    ok = (den.abs() > 1e-9) & (sc > 0.5) & (tc > 0.5)
    i1, i2, X = i1[ok], i2[ok], X[ok]
    npt = int(i1.numel())
    inv_sigma2 = torch.from_numpy(synth.scale_tables()[3]).to(dev)
    ar = torch.arange(npt, device=dev, dtype=torch.int32)
    dv = dict(kf_Tcw=torch.from_numpy(np.stack([synth.to12(T1), synth.to12(np.vstack([np.hstack([prob["R2w"].reshape(3, 3), prob["t2w"].reshape(3, 1)]), [0, 0, 0, 1]]))])).to(dev),
              mp_xw=X.float().contiguous(), mpb_xw=torch.zeros(1, 3, device=dev),
              obs_kf=torch.stack([torch.zeros_like(ar), torch.ones_like(ar)], 1).reshape(-1).contiguous(),
              obs_mp=torch.stack([ar, ar], 1).reshape(-1).contiguous(),
              obs_uv=torch.stack([kp1[i1], kp2[i2]], 1).reshape(-1, 2).contiguous(),
              obs_inv_sigma2=torch.stack([inv_sigma2[oc1[i1]], inv_sigma2[oc2[i2]]], 1).reshape(-1).contiguous(),
              obs_outlier=torch.full((2 * npt,), 9, dtype=torch.uint8, device=dev), bobs_outlier=torch.zeros(1, dtype=torch.uint8, device=dev))
    host = dict(kf_fixed=np.array([1, 0], np.uint8))
    ba = cabi.LocalBAArgs()
    cabi.fill(ba, with_odom=0, fx=fx, fy=fy, cx=cx, cy=cy, wF=1.0, wB=1.0, wP=3.0, n_kf=2, n_mp=npt, n_mpb=0, n_obs=2 * npt, n_bobs=0, n_odom=0,
              kf_fixed=host["kf_fixed"], **{k: v for k, v in dv.items() if k != "mpb_xw"})
    graph_host = {k: v.cpu().numpy().copy() for k, v in dv.items()}   # the graph as it was handed over (for the oracle)
    rc = fb.lib().fb_local_ba_dev(C.byref(ba), C.c_void_p(s.cuda_stream))
    assert rc == 0, fb.lib().fb_last_error()
    torch.cuda.synchronize()
    p = dict(fx=fx, fy=fy, cx=cx, cy=cy, wP=3.0, kf_Tcw=graph_host["kf_Tcw"], kf_fixed=host["kf_fixed"], mp_xw=graph_host["mp_xw"], mpb_xw=np.zeros((0, 3), np.float32),
             obs_kf=graph_host["obs_kf"], obs_mp=graph_host["obs_mp"], obs_uv=graph_host["obs_uv"], obs_inv_sigma2=graph_host["obs_inv_sigma2"],
             bobs_kf=np.zeros(0, np.int32), bobs_mpb=np.zeros(0, np.int32), bobs_xc=np.zeros((0, 3), np.float32), bobs_inv_sigma2=np.zeros(0, np.float32),
             odom_kf_i=np.zeros(0, np.int32), odom_kf_j=np.zeros(0, np.int32), odom_Tij=np.zeros((0, 12), np.float32), odom_info=np.zeros(0, np.float64))
    a1, out_o, keep1 = ba_problem.local_ba_args(p, with_odom=0)
    O.call("orc_local_ba", a1)
    wp, wl = _rel_pose(dv["kf_Tcw"].cpu().numpy(), out_o["kf_Tcw"]), _rel_pt(dv["mp_xw"].cpu().numpy(), out_o["mp_xw"])
    print("triangulated graph: worst per-element difference: poses %.3g, landmarks %.3g" % (wp, wl))
    assert wp <= REL_TOL
    assert wl <= REL_TOL
    np.testing.assert_array_equal(dv["obs_outlier"].cpu().numpy(), out_o["obs_outlier"])


def test_shutdown_releases_and_the_library_keeps_working():
    """fb_shutdown frees the scratch pool, the calling thread's staging block and its BA stream / event / pinned control block;
    the next calls allocate again."""
    import fishbirdeyevisualslam_amd as fb
    p = synth.make_ba_problem(4300, n_kf=6, n_mp=300, n_mpb=60)
    out_o, out_h, _, _ = _run(p, with_odom=1)
    assert fb.lib().fb_shutdown() == 0
    assert fb.lib().fb_shutdown() == 0
    out_o2, out_h2, _, _ = _run(p, with_odom=1)
    np.testing.assert_array_equal(out_h2["kf_Tcw"], out_h["kf_Tcw"])
    np.testing.assert_array_equal(out_h2["obs_outlier"], out_h["obs_outlier"])
