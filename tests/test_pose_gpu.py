"""GPU parity: HIP pose optimisation (C-ABI) vs the CPU oracle.

Tolerance (BASELINE.json north_star): pose within 1e-4 relative; inlier/outlier masks and the
returned inlier count are integer results and must be identical.
"""
import numpy as np
import pytest

import hip_lib as H
import oracle_lib as O
import pose_cases as PC
from fishbirdeyevisualslam_amd import cabi, problems as P, synth

pytestmark = pytest.mark.gpu
REL_TOL = 1e-4


def _run(probs, **kw):
    a, out_o, keep = P.pose_args(probs, **kw)
    O.call("orc_pose_opt", a)
    a2, out_h, keep2 = P.pose_args(probs, **kw)
    H.call("fb_pose_opt", a2)
    return out_o, out_h


def _compare(out_o, out_h, mode):
    To, Th = out_o["Tcw"].reshape(-1, 3, 4), out_h["Tcw"].reshape(-1, 3, 4)
    scale = np.maximum(1.0, np.abs(To).max(axis=(1, 2), keepdims=True))
    rel = np.abs(Th - To) / scale
    assert rel.max() <= REL_TOL, rel.max()
    np.testing.assert_array_equal(out_h["ninliers"], out_o["ninliers"])
    if mode != cabi.FB_POSE_BIRD:
        np.testing.assert_array_equal(out_h["front_outlier"], out_o["front_outlier"])
    if mode != cabi.FB_POSE_FRONT:
        np.testing.assert_array_equal(out_h["bird_outlier"], out_o["bird_outlier"])
    return rel.max()


@pytest.mark.parametrize("mode", [cabi.FB_POSE_FRONT, cabi.FB_POSE_FRONT_BIRD, cabi.FB_POSE_BIRD])
def test_pose_opt_config3(mode):
    """BASELINE config 3: 2000 front + 1000 bird edges."""
    probs = [synth.make_pose_problem(3000 + i) for i in range(4)]
    out_o, out_h = _run(probs, mode=mode)
    _compare(out_o, out_h, mode)
    # the optimiser must actually have moved towards the generating pose
    Tt = np.stack([p["T_true"][:3, :4] for p in probs])
    e0 = np.abs(np.stack([p["Tcw0"].reshape(3, 4) for p in probs]) - Tt).max()
    e1 = np.abs(out_h["Tcw"].reshape(-1, 3, 4) - Tt).max()
    assert e1 < (0.2 if mode != cabi.FB_POSE_BIRD else 0.5) * e0


def test_pose_opt_weights_and_masks():
    g = synth.rng(5)
    probs = [synth.make_pose_problem(3100 + i, n_front=700 + 50 * i, n_bird=300 + 20 * i) for i in range(3)]
    fv = [(g.random(len(p["front_xw"])) < 0.7).astype(np.uint8) for p in probs]
    bv = [(g.random(len(p["bird_xw"])) < 0.6).astype(np.uint8) for p in probs]
    bo = [(g.random(len(p["bird_xw"])) < 0.2).astype(np.uint8) for p in probs]
    out_o, out_h = _run(probs, mode=cabi.FB_POSE_FRONT_BIRD, wF=1.0, wB=3.0, front_valid=fv, bird_valid=bv,
                        bird_outlier_in=bo)
    _compare(out_o, out_h, cabi.FB_POSE_FRONT_BIRD)
    # slots without an edge are left untouched (front buffer was pre-filled with 9)
    for b in range(3):
        assert np.all(out_h["front_outlier"][b, : len(fv[b])][fv[b] == 0] == 9)


def test_pose_opt_degenerate_counts():
    # < 3 correspondences -> returns 0 and leaves the pose alone (Optimizer.cc:379,607,776)
    p = synth.make_pose_problem(3200, n_front=2, n_bird=2)
    for mode in (cabi.FB_POSE_FRONT, cabi.FB_POSE_FRONT_BIRD, cabi.FB_POSE_BIRD):
        out_o, out_h = _run([p], mode=mode)
        assert out_h["ninliers"][0] == 0 and out_o["ninliers"][0] == 0
        np.testing.assert_array_equal(out_h["Tcw"], np.stack([p["Tcw0"]]))
    # fewer than 10 edges in total -> a single round (Optimizer.cc:462,688)
    p = synth.make_pose_problem(3201, n_front=5, n_bird=3, outlier_frac=0.0)
    out_o, out_h = _run([p], mode=cabi.FB_POSE_FRONT_BIRD)
    _compare(out_o, out_h, cabi.FB_POSE_FRONT_BIRD)


def test_pose_opt_noise_free_recovers_pose():
    """Known answer: noise-free data -> generating pose, zero outliers."""
    p = synth.make_pose_problem(3300, n_front=400, n_bird=0)
    T = p["T_true"]
    Xw = p["front_xw"].astype(np.float64)
    Xc = (T[:3, :3] @ Xw.T).T + T[:3, 3]
    p["front_obs"] = np.ascontiguousarray(
        np.stack([Xc[:, 0] / Xc[:, 2] * p["fx"] + p["cx"], Xc[:, 1] / Xc[:, 2] * p["fy"] + p["cy"]], 1).astype(np.float32))
    out_o, out_h = _run([p], mode=cabi.FB_POSE_FRONT)
    _compare(out_o, out_h, cabi.FB_POSE_FRONT)
    assert out_h["ninliers"][0] == 400 and out_h["front_outlier"][0, :400].sum() == 0
    assert np.abs(out_h["Tcw"][0].reshape(3, 4) - T[:3, :4]).max() < 1e-3


@pytest.mark.parametrize("variant", ["512", "256", "0"])
def test_pose_opt_other_kernel_variants(variant):
    """The default is k_pose_opt_regs<512, 448> (448 edge threads + a solver wave); FB_POSE_NT selects its one-role
    instantiations with 512 / 256 threads or the LDS-staged kernel (read once per process, hence a child process; the
    children run one after the other).  Same parity bar for each."""
    import os, subprocess, sys
    env = dict(os.environ, FB_POSE_NT=variant)
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_pose_gpu.py"), "-q", "-x", "-m", "gpu",
                        "-k", "config3 or weights_and_masks or register_slot_boundary or constructed_case or case_batch or "
                        "generic_schedule_writes_the_bird_mask", "-p", "no:cacheprovider"],
                       env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_pose_opt_batch_of_64_takes_the_throughput_kernel():
    """Batches of 64 frames or more run k_pose_opt_regs<256, 256> (it shares its CUs with other streams' kernels); same bar."""
    probs = [synth.make_pose_problem(3300 + i, n_front=260 + 7 * (i % 9), n_bird=120 + 5 * (i % 7)) for i in range(64)]
    out_o, out_h = _run(probs, mode=cabi.FB_POSE_FRONT_BIRD)
    _compare(out_o, out_h, cabi.FB_POSE_FRONT_BIRD)


@pytest.mark.parametrize("batch", [2, 64])
def test_pose_opt_more_edges_than_register_slots(batch):
    """Frames with more edges than the register kernels hold (2240 + 1344 in k_pose_opt_regs<512, 448>, 2560 + 1536 in
    k_pose_opt_regs<256, 256>) leave through the in-kernel generic schedule (edges re-read from HBM); e.g. the 4000-feature
    initialisation extractor.  A batch of 64 mixes them with ordinary frames."""
    big = [synth.make_pose_problem(3400, n_front=3100, n_bird=300), synth.make_pose_problem(3401, n_front=900, n_bird=1700)]
    small = [synth.make_pose_problem(3410 + i, n_front=200 + 11 * (i % 5), n_bird=90 + 3 * (i % 4)) for i in range(batch - 2)]
    probs = small[: len(small) // 2] + [big[0]] + small[len(small) // 2:] + [big[1]]
    out_o, out_h = _run(probs, mode=cabi.FB_POSE_FRONT_BIRD)
    _compare(out_o, out_h, cabi.FB_POSE_FRONT_BIRD)


def _spread_valid(n, n_invalid):
    """n slots of which n_invalid, spread evenly over the whole range, hold no edge."""
    v = np.ones(n, np.uint8)
    v[np.round(np.linspace(0, n - 1, n_invalid)).astype(np.int64)] = 0
    assert int(v.sum()) == n - n_invalid
    return v


def test_pose_opt_register_slot_boundary():
    """On the capacity of the register slots (EF * NE front, EB * NE bird valid edges): a frame that fills the last slot, one
    more front / one more bird edge (the in-kernel way out to the generic schedule), and frames whose valid edges are
    exactly / one beyond the capacity among slot indices that run 360 past it (compaction, outlier flags written back
    through the slot index)."""
    import os
    F, B = (2560, 1536) if os.environ.get("FB_POSE_NT") in ("256", "512") else (2240, 1344)
    shapes = [(F, B), (F + 1, 300), (900, B + 1), (F + 360, 500), (F + 360, 500)]
    probs = [synth.make_pose_problem(3500 + i, n_front=nf, n_bird=nb) for i, (nf, nb) in enumerate(shapes)]
    fv = [np.ones(nf, np.uint8) for nf, _ in shapes[:3]] + [_spread_valid(F + 360, 360), _spread_valid(F + 360, 359)]
    out_o, out_h = _run(probs, mode=cabi.FB_POSE_FRONT_BIRD, front_valid=fv)
    _compare(out_o, out_h, cabi.FB_POSE_FRONT_BIRD)
    for b in range(5):
        n = len(fv[b])
        # the front masks compared are not trivial, and slots without an edge keep the prefill value
        assert 0 < np.count_nonzero(out_o["front_outlier"][b, :n][fv[b] == 1]) < n
        assert np.all(out_h["front_outlier"][b, :n][fv[b] == 0] == 9)


# ---- the constructed cases of tests/pose_cases.py (proven on the CPU by tests/test_pose_cases.py) ---------------------------
CASES = PC.cases()


def _assert_case_masks_not_trivial(case, out_o, b=0):
    """what makes the comparison of a case's masks worth something, on the oracle's side of it"""
    n_b = len(case["prob"]["bird_xw"])
    if "bird_flagged" in case["expect"] or "displaced_mixed" in case["expect"] or "displaced_all_flagged" in case["expect"]:
        assert 0 < np.count_nonzero(out_o["bird_outlier"][b, :n_b] == 1) < n_b, case["id"]
    if "bird_prefill_kept" in case["expect"]:
        assert np.count_nonzero(out_o["bird_outlier"][b, :n_b] == PC.PREFILL) > 0, case["id"]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_pose_opt_constructed_case(case):
    out_o, out_h = _run([case["prob"]], **case["kw"])
    _compare(out_o, out_h, case["kw"]["mode"])
    # both masks whatever the mode: the one a mode does not own must come back as it went in
    np.testing.assert_array_equal(out_h["front_outlier"], out_o["front_outlier"])
    np.testing.assert_array_equal(out_h["bird_outlier"], out_o["bird_outlier"])
    _assert_case_masks_not_trivial(case, out_o)


def _front_bird_case_batch():
    """every FRONT_BIRD case at unit weights as one batch: (cases, problems, keyword arguments with per-frame bird masks)"""
    cs = [c for c in CASES if c["kw"]["mode"] == cabi.FB_POSE_FRONT_BIRD and set(c["kw"]) <= {"mode", "bird_valid", "bird_outlier_in"}]
    assert len(cs) >= 12 and any("bird_outlier_in" in c["kw"] for c in cs) and any("bird_valid" in c["kw"] for c in cs)
    bv = [c["kw"]["bird_valid"][0] if "bird_valid" in c["kw"] else np.ones(len(c["prob"]["bird_xw"]), np.uint8) for c in cs]
    bo = [c["kw"]["bird_outlier_in"][0] if "bird_outlier_in" in c["kw"] else np.zeros(len(c["prob"]["bird_xw"]), np.uint8) for c in cs]
    return cs, [c["prob"] for c in cs], dict(mode=cabi.FB_POSE_FRONT_BIRD, bird_valid=bv, bird_outlier_in=bo)


def test_pose_opt_case_batch_of_64_takes_the_throughput_kernel():
    """k_pose_opt_regs<256, 256> (batches of 64 or more) on the constructed cases mixed with ordinary frames"""
    cs, probs, kw = _front_bird_case_batch()
    extra = [synth.make_pose_problem(3600 + i, n_front=150 + 7 * (i % 9), n_bird=70 + 5 * (i % 7)) for i in range(64 - len(cs))]
    order = np.argsort(synth.rng(11).random(64), kind="stable")            # cases spread among the ordinary frames
    allp = probs + extra
    bv = kw["bird_valid"] + [np.ones(len(p["bird_xw"]), np.uint8) for p in extra]
    bo = kw["bird_outlier_in"] + [np.zeros(len(p["bird_xw"]), np.uint8) for p in extra]
    out_o, out_h = _run([allp[i] for i in order], mode=cabi.FB_POSE_FRONT_BIRD, bird_valid=[bv[i] for i in order],
                        bird_outlier_in=[bo[i] for i in order])
    _compare(out_o, out_h, cabi.FB_POSE_FRONT_BIRD)
    for b, i in enumerate(order):
        if i < len(cs):
            _assert_case_masks_not_trivial(cs[i], out_o, b)


def test_pose_opt_case_batch_dev_on_a_callers_stream():
    """fb_pose_opt_batch_dev takes bird_outlier as in/out device memory: flags set on entry, prefilled slots without an edge"""
    import ctypes as C
    from device_mirror import Mirror, _lib, _stream, _sync
    cs, probs, kw = _front_bird_case_batch()
    a, out_o, keep = P.pose_args(probs, **kw)
    O.call("orc_pose_opt", a)
    a2, out_h, keep2 = P.pose_args(probs, **kw)
    mir = Mirror(out_h, keep2)
    d = mir.struct(a2)
    assert _lib().fb_pose_opt_batch_dev(C.byref(d), _stream()) == 0, _lib().fb_last_error()
    _sync()
    out_d = {k: mir.host(v) for k, v in out_h.items()}
    _compare(out_o, out_d, cabi.FB_POSE_FRONT_BIRD)
    for b, c in enumerate(cs):
        _assert_case_masks_not_trivial(c, out_o, b)


def test_pose_opt_generic_schedule_writes_the_bird_mask():
    """One bird edge more than the register slots hold: the frame leaves through the in-kernel generic schedule, the only
    other place that writes bird_outlier, with bird outliers displaced to both sides of the gate and holes in bird_valid."""
    import os
    B = 1536 if os.environ.get("FB_POSE_NT") in ("256", "512") else 1344
    holes = 37
    p = synth.make_pose_problem(3700, n_front=300, n_bird=B + 1 + holes)
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    PC._displace_bird(p, synth.rng(3701), np.nonzero(p["bird_is_outlier"])[0], 0.3, 2.0)
    bv = PC.spread_valid(B + 1 + holes, holes)
    bo = np.where(bv == 0, PC.PREFILL, 0).astype(np.uint8)
    bo[np.nonzero(bv)[0][::5]] = 1                                         # and flags set on entry
    out_o, out_h = _run([p], mode=cabi.FB_POSE_FRONT_BIRD, bird_valid=[bv], bird_outlier_in=[bo])
    _compare(out_o, out_h, cabi.FB_POSE_FRONT_BIRD)
    flags = out_o["bird_outlier"][0]
    disp = p["bird_displaced"][bv[p["bird_displaced"]] == 1]
    assert 0 < np.count_nonzero(flags[disp] == 1) < len(disp)
    assert np.all(out_h["bird_outlier"][0][bv == 0] == PC.PREFILL)
