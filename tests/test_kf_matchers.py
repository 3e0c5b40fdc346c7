"""Key-frame side matcher entry points and ComputeDistinctiveDescriptors.

CPU part: structural invariants of the oracle restatement (the reference ships no fixtures for these: "parity unpinned").
GPU part (-m gpu): the HIP kernels through the C-ABI reproduce the oracle bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from fishbirdeyevisualslam_amd import kf_problems as KP, problems as P, synth

GEOM = lambda: P.grid_geom(synth.front_grid_geom(KP.W, KP.H))


def _ham(a, b):
    return np.unpackbits(a ^ b, axis=1).sum(1)


def _grid(kps_list, stride, fn=None):
    return P.build_grid_host(kps_list, GEOM(), fn or O.grid_build, max(stride, 1))


def _distinct(lib, prefix, start, desc):
    n = len(start) - 1
    best = np.full(n, -9, np.int32)
    rc = getattr(lib, prefix + "distinctive_descriptors")(C.c_void_p(start.ctypes.data), C.c_void_p(desc.ctypes.data), n,
                                                         C.c_void_p(best.ctypes.data))
    assert rc == 0
    return best


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_fuse_search_invariants():
    for sim3, name in ((False, "orc_fuse_search"), (True, "orc_fuse_sim3_search")):
        probs = [KP.make_kf_points_problem(8000 + i, 1500, 2500, sim3) for i in range(2)]
        cs, ci = _grid([p["kf_kps"] for p in probs], 1500)
        a, out, keep = KP.fuse_args(probs, cs, ci, th=3.0)
        O.call(name, a)
        for b, p in enumerate(probs):
            bi = out["best_idx"][b][: len(p["mp_xw"])]
            hit = bi >= 0
            assert hit.sum() > 500
            assert (p["mp_valid"][hit] == 1).all()
            assert _ham(p["mp_desc"][hit], p["kf_desc"][bi[hit]]).max() <= 50
        # a wider search radius can only find more
        a2, out2, keep2 = KP.fuse_args(probs, cs, ci, th=6.0)
        O.call(name, a2)
        assert ((out2["best_idx"] >= 0).sum() >= (out["best_idx"] >= 0).sum())


def test_projection_sim3_invariants():
    probs = [KP.make_kf_points_problem(8050 + i, 1500, 2500, True) for i in range(2)]
    cs, ci = _grid([p["kf_kps"] for p in probs], 1500)
    a, out, keep = KP.proj_sim3_args(probs, cs, ci)
    O.call("orc_match_projection_sim3", a)
    for b, p in enumerate(probs):
        m = out["match_kf_to_mp"][b][: len(p["kf_kps"])]
        hit = m >= 0
        assert hit.sum() == out["nmatches"][b] > 300
        assert len(np.unique(m[hit])) == hit.sum()
        assert not (hit & (p["kf_matched"] == 1)).any()
        assert _ham(p["kf_desc"][hit], p["mp_desc"][m[hit]]).max() <= 50


def test_sim3_agreement():
    probs = [KP.make_sim3_problem(8100 + i, 1200, 1300, 700) for i in range(2)]
    g1 = _grid([p["kps1"] for p in probs], 1200)
    g2 = _grid([p["kps2"] for p in probs], 1300)
    a, out, keep = KP.sim3_args(probs, g1, g2)
    O.call("orc_match_sim3", a)
    for b, p in enumerate(probs):
        m = out["matches12"][b][:1200]
        hit = m >= 0
        assert hit.sum() == out["nfound"][b] > 300
        assert len(np.unique(m[hit])) == hit.sum()               # mutual best => one-to-one
        assert (p["mp_valid1"][hit] == 1).all() and (p["mp_valid2"][m[hit]] == 1).all()
        assert _ham(p["mp_desc1"][hit], p["desc2"][m[hit]]).max() <= 100


def test_initialization_matches():
    probs = [KP.make_init_problem(8200 + i, 1800, 2000) for i in range(2)]
    cs, ci = _grid([p["kps2"] for p in probs], 2000)
    for ori in (1, 0):
        a, out, keep = KP.init_args(probs, cs, ci, check_ori=ori)
        O.call("orc_match_initialization", a)
        for b, p in enumerate(probs):
            m = out["matches12"][b][:1800]
            hit = m >= 0
            assert hit.sum() == out["nmatches"][b] > 100
            assert len(np.unique(m[hit])) == hit.sum()           # vnMatches21: an F2 feature keeps one F1 partner
            assert (p["kps1"]["octave"][hit] == 0).all() and (p["kps2"]["octave"][m[hit]] == 0).all()
            assert _ham(p["desc1"][hit], p["desc2"][m[hit]]).max() <= 50
            # vbPrevMatched follows the matches (:514-516), untouched elsewhere
            np.testing.assert_array_equal(out["prev_matched"][b][:1800][hit, 0], p["kps2"]["x"][m[hit]])
            np.testing.assert_array_equal(out["prev_matched"][b][:1800][~hit], p["prev"][~hit])


def test_distinctive_descriptor_is_the_least_median():
    start, desc = KP.make_distinctive_problem(8300, 400, max_obs=25, big=2)
    best = _distinct(O.lib(), "orc_", start, desc)
    for p in range(400):
        n = start[p + 1] - start[p]
        if n == 0:
            assert best[p] == -1
            continue
        D = desc[start[p]:start[p + 1]]
        dist = np.unpackbits(D[:, None, :] ^ D[None, :, :], axis=2).sum(2)
        med = np.sort(dist, axis=1)[:, int(0.5 * (n - 1))]
        assert best[p] == int(np.argmin(med))                    # first minimum, strict <


# ---------------------------------------------------------------------------------------------------------------- GPU
def _hip():
    import hip_lib as H
    return H


@pytest.mark.gpu
@pytest.mark.parametrize("seed,nkf,nmp", [(8000, 2000, 3000), (8001, 2064, 900), (8002, 250, 4000), (8003, 30, 0)])
def test_gpu_fuse_and_projection_sim3(seed, nkf, nmp):
    H = _hip()
    for sim3, oname, hname in ((False, "orc_fuse_search", "fb_fuse_search"), (True, "orc_fuse_sim3_search", "fb_fuse_sim3_search")):
        probs = [KP.make_kf_points_problem(seed + 10 * i, nkf, nmp, sim3) for i in range(3)]
        cs, ci = _grid([p["kf_kps"] for p in probs], nkf)
        for th in (3.0, 8.0):
            a, oo, k = KP.fuse_args(probs, cs, ci, th=th)
            O.call(oname, a)
            a2, oh, k2 = KP.fuse_args(probs, cs, ci, th=th)
            H.call(hname, a2)
            for b, p in enumerate(probs):
                n = len(p["mp_xw"])
                np.testing.assert_array_equal(oh["best_idx"][b, :n], oo["best_idx"][b, :n])
        if sim3:
            for th in (10, 40):  # 40: heavy contention for the free slots
                a, oo, k = KP.proj_sim3_args(probs, cs, ci, th=th)
                O.call("orc_match_projection_sim3", a)
                a2, oh, k2 = KP.proj_sim3_args(probs, cs, ci, th=th)
                H.call("fb_match_projection_sim3", a2)
                for b, p in enumerate(probs):
                    n = len(p["kf_kps"])
                    np.testing.assert_array_equal(oh["match_kf_to_mp"][b, :n], oo["match_kf_to_mp"][b, :n])
                np.testing.assert_array_equal(oh["nmatches"], oo["nmatches"])


@pytest.mark.gpu
@pytest.mark.parametrize("blocked", [True, False])
def test_gpu_projection_sim3_contention(blocked):
    """2000 points compete for 150 key points in a wide window: the serial 'slot already written to vpMatched' rule, with
    and without slots that are matched on entry.  The rule fires: the free slots limit the number of matches."""
    H = _hip()
    probs = [KP.make_kf_points_problem(8500 + i, 150, 2000, True) for i in range(2)]
    if not blocked:
        for p in probs:
            p["kf_matched"] = np.zeros_like(p["kf_matched"])
    cs, ci = _grid([p["kf_kps"] for p in probs], 150)
    a, oo, k = KP.proj_sim3_args(probs, cs, ci, th=40)
    O.call("orc_match_projection_sim3", a)
    a2, oh, k2 = KP.proj_sim3_args(probs, cs, ci, th=40)
    H.call("fb_match_projection_sim3", a2)
    np.testing.assert_array_equal(oh["match_kf_to_mp"], oo["match_kf_to_mp"])
    np.testing.assert_array_equal(oh["nmatches"], oo["nmatches"])
    for b, p in enumerate(probs):
        free = int((p["kf_matched"] == 0).sum())
        assert (free < 150) == blocked
        assert 2 * oo["nmatches"][b] >= free


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n1,n2,ns", [(8100, 1500, 1500, 900), (8101, 2064, 800, 500), (8102, 40, 60, 20)])
def test_gpu_search_by_sim3(seed, n1, n2, ns):
    H = _hip()
    probs = [KP.make_sim3_problem(seed + 10 * i, n1, n2, ns) for i in range(3)]
    g1 = _grid([p["kps1"] for p in probs], n1)
    g2 = _grid([p["kps2"] for p in probs], n2)
    a, oo, k = KP.sim3_args(probs, g1, g2)
    O.call("orc_match_sim3", a)
    a2, oh, k2 = KP.sim3_args(probs, g1, g2)
    H.call("fb_match_sim3", a2)
    np.testing.assert_array_equal(oh["matches12"][:, :n1], oo["matches12"][:, :n1])
    np.testing.assert_array_equal(oh["nfound"], oo["nfound"])
    if ns >= 500:
        assert oo["nfound"].min() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n1,n2", [(8200, 2000, 2000), (8201, 4000, 4000), (8202, 700, 2064), (8203, 20, 1)])
def test_gpu_search_for_initialization(seed, n1, n2):
    H = _hip()
    probs = [KP.make_init_problem(seed + 10 * i, n1, n2) for i in range(3)]
    cs, ci = _grid([p["kps2"] for p in probs], n2)
    for window, ori in ((100, 1), (100, 0), (250, 1)):  # 250: many queries per target, exercises the steal rule
        a, oo, k = KP.init_args(probs, cs, ci, window=window, check_ori=ori)
        O.call("orc_match_initialization", a)
        a2, oh, k2 = KP.init_args(probs, cs, ci, window=window, check_ori=ori)
        H.call("fb_match_initialization", a2)
        np.testing.assert_array_equal(oh["matches12"][:, :n1], oo["matches12"][:, :n1])
        np.testing.assert_array_equal(oh["nmatches"], oo["nmatches"])
        np.testing.assert_array_equal(oh["prev_matched"][:, :n1], oo["prev_matched"][:, :n1])


@pytest.mark.gpu
def test_gpu_distinctive_descriptors():
    import fishbirdeyevisualslam_amd as fb
    for seed, n, mx in ((8300, 3000, 40), (8301, 50, 3), (8302, 1, 0)):
        start, desc = KP.make_distinctive_problem(seed, n, max_obs=mx, big=min(3, n))
        bo = _distinct(O.lib(), "orc_", start, desc)
        bh = _distinct(fb.lib(), "fb_", start, desc)
        np.testing.assert_array_equal(bh, bo)
