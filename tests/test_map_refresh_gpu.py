"""fb_covis_refresh_points / process_new_keyframe / map_point_culling on the device against the literal model
(tests/map_refresh_ref.py), through the C ABI.

Integer outputs and descriptors are compared for equality.  Normals (absolutely) and distances (over max(1, |v|)) are
compared to BOUND.  The worst difference against the model measured on an MI355X over every case of this file is 0 (no
contraction, correctly rounded sqrt and division, the model's operation order), so BOUND = 4 * 0 = 0: equality.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import covis_ref as CR
import map_refresh_cases as MC
import map_refresh_ref as R
from fishbirdeyevisualslam_amd import cabi, lib
from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceMap

pytestmark = pytest.mark.gpu
BOUND = 0.0
GUARD = 3
REFRESH_KEYS = ("kf_Tcw", "kf_bad", "kf_desc", "scale_factors", "mp_xw", "mp_ref_kf", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc")


def setup(c, obs_spare=0):
    G = CovisibilityGraph(c["K"])
    m = DeviceMap(c, obs_spare=obs_spare)
    t, a = G.refresh_arrays(m, *(c[k] for k in REFRESH_KEYS), guard=GUARD)
    return G, m, t, a


def check_refreshed(t, w, n_mp):
    """the four in/out arrays against the model's, their guard rows against the fill"""
    worst = 0.0
    for name, exp, width in (("mp_normal", w.normal, 3), ("mp_min_dist", w.min_dist, 1), ("mp_max_dist", w.max_dist, 1)):
        got = t[name].cpu().numpy()
        assert np.all(got[n_mp * width:] == np.float32(7.0)), name + ": guard rows"
        got, exp = got[:n_mp * width].reshape(exp.shape), np.asarray(exp, np.float32)
        d = np.abs(got.astype(np.float64) - exp) / (1.0 if name == "mp_normal" else np.maximum(1.0, np.abs(exp)))
        worst = max(worst, float(d.max()) if d.size else 0.0)
    print("worst normal / distance difference: %g" % worst)
    assert worst <= BOUND
    got = t["mp_desc"].cpu().numpy()
    assert np.all(got[n_mp * 32:] == 0xEE), "mp_desc: guard rows"
    assert np.array_equal(got[:n_mp * 32].reshape(-1, 32), w.desc)


@pytest.mark.parametrize("mode", ["list", "all"])
@pytest.mark.parametrize("what", [1, 2, 3])
def test_refresh_points(mode, what):
    c = MC.refresh_case()
    n_mp = len(c["mp_bad"])
    pts = None if mode == "all" else list(range(len(MC.REFRESH_COUNTS))) + [7, 4, 4, n_mp - 1, n_mp + 3]   # repeats, one out of range
    G, m, t, a = setup(c)
    w = R.World(c)
    R.refresh_points(w, pts, what)
    G.refresh_points(m, a, pts, what=what)
    check_refreshed(t, w, n_mp)
    assert G.error_count() == w.errors == (0 if pts is None else 1)
    G.close()


def test_refresh_points_device_count_and_host_form():
    c = MC.refresh_case()
    n_mp = len(c["mp_bad"])
    pts = [8, 9, 10, 2, 5]
    G, m, t, a = setup(c)
    G.refresh_points(m, a, pts, n_points=torch.tensor([3], dtype=torch.int32, device="cuda"))         # the device count cuts the list
    w = R.World(c)
    R.refresh_points(w, pts[:3])
    check_refreshed(t, w, n_mp)
    # host pointers throughout
    h = {k: np.ascontiguousarray(c[k]).copy() for k in REFRESH_KEYS + ("kf_n", "kf_mp", "kf_octave", "mp_bad", "obs_mp", "obs_kf", "obs_idx", "kf_order")}
    hm = cabi.fill(cabi.CovisMap(), max_keyframes=c["K"], kp_stride=c["S"], n_mp=n_mp, n_obs=len(c["obs_kf"]),
                   **{k: h[k] for k in ("kf_n", "kf_mp", "kf_octave", "mp_bad", "obs_mp", "obs_kf", "obs_idx", "kf_order")})
    lst = np.array(pts, np.int32)
    ha = cabi.fill(cabi.PointRefreshArgs(), d_list=lst, n_list=len(pts), what=3, n_levels=len(c["scale_factors"]), **{k: h[k] for k in REFRESH_KEYS})
    assert lib().fb_covis_refresh_points(G.h, C.byref(hm), C.byref(ha)) == 0
    w = R.World(c)
    R.refresh_points(w, pts)
    assert np.array_equal(h["mp_desc"], w.desc) and np.array_equal(h["mp_normal"], w.normal)
    assert np.array_equal(h["mp_min_dist"], w.min_dist) and np.array_equal(h["mp_max_dist"], w.max_dist)
    G.close()


def local_map_out(G, m, c, reuse):
    K, n_mp = c["K"], len(c["mp_bad"])
    t, a = G.local_map_arrays([c["S"]], np.asarray(c["kf_mp"][:1]), c["kf_bad"], max(K, 83), max(n_mp, 1))
    G.local_map(m, a, reuse_index=reuse)
    return b"".join(t[k].cpu().numpy().tobytes() for k in ("d_map_point", "d_local_kf", "d_n_local_kf", "d_local_mp", "d_n_local_mp", "d_ref_kf", "d_n_voters"))


def test_refresh_reuses_the_index_of_a_local_map():
    c = MC.refresh_case()
    out = []
    for reuse in (False, True):
        G, m, t, a = setup(c)
        local_map_out(G, m, c, False)
        G.refresh_points(m, a, None, reuse_index=reuse)
        out.append(b"".join(t[k].cpu().numpy().tobytes() for k in ("mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc")))
        G.close()
    assert out[0] == out[1]


def check_edges(m, w):
    for k, exp in (("obs_mp", w.obs_mp), ("obs_kf", w.obs_kf), ("obs_idx", w.obs_idx)):
        got = m.t[k].cpu().numpy()
        assert np.array_equal(got[:len(exp)], exp), k
        assert np.all(got[len(exp):] == -1), k + ": past the block"


@pytest.mark.parametrize("N,S,declared", [(70, 96, None), (0, 96, None), (96, 96, None), (70, 96, 69)])
def test_process_new_keyframe(N, S, declared):
    c, slot, nf = MC.new_keyframe_case(N, S, 12, declared)
    n_mp, base = len(c["mp_bad"]), len(c["obs_kf"])
    G, m, t, a = setup(c, obs_spare=nf + GUARD)
    recent, n_recent = G.recent_list(20 + N, c["recent"])
    n_added = G.process_new_keyframe(m, a, slot, nf, recent, n_recent)
    w = R.World(c)
    rl = [int(x) for x in c["recent"]]
    exp_added = R.process_new_keyframe(w, slot, nf, rl)
    assert int(n_added.cpu()[0]) == exp_added
    assert m.n_obs == base + nf
    check_edges(m, w)
    blk = m.t["obs_kf"].cpu().numpy()[base:base + nf]
    assert np.all(blk[:exp_added] == slot) and np.all(blk[exp_added:] == -1)                           # the new edges first, then tombstones
    assert int(n_recent.cpu()[0]) == len(rl) and recent.cpu().numpy()[:len(rl)].tolist() == rl
    assert np.all(recent.cpu().numpy()[len(rl):] == -1)
    check_refreshed(t, w, n_mp)
    assert G.error_count() == w.errors == (1 if (N >= 20 or declared is not None) else 0)
    G.close()


def culling_expect(c, lst):
    w = R.World(c)
    kept, culled, erased = R.map_point_culling(w, lst, MC.CUR_KF_ID, c["mp_first_kf_id"], c["mp_found"], c["mp_visible"])
    return w, kept, culled, erased


def check_culling(m, w, out, recent, n_recent, kept, culled, erased):
    assert int(n_recent.cpu()[0]) == len(kept) and recent.cpu().numpy()[:len(kept)].tolist() == kept
    assert int(out["n_culled"].cpu()[0]) == len(culled) and out["culled"].cpu().numpy()[:len(culled)].tolist() == culled
    assert int(out["n_erased"].cpu()[0]) == len(erased)
    assert out["erased"].cpu().numpy()[:len(erased)].tolist() == [list(r) for r in erased]
    assert np.array_equal(m.t["mp_bad"].cpu().numpy()[:len(w.mp_bad)], w.mp_bad)
    assert np.array_equal(m.t["kf_mp"].cpu().numpy(), w.kf_mp)
    assert np.array_equal(m.t["obs_kf"].cpu().numpy()[:len(w.obs_kf)], w.obs_kf)


@pytest.mark.parametrize("n_list", [40, 0, 300])
def test_map_point_culling(n_list):
    c, lst = MC.culling_case(n_list)
    G = CovisibilityGraph(c["K"])
    m = DeviceMap(c)
    recent, n_recent = G.recent_list(n_list + GUARD, lst)
    out = G.map_point_culling(m, MC.CUR_KF_ID, c["mp_first_kf_id"], c["mp_found"], c["mp_visible"], recent, n_recent)
    w, kept, culled, erased = culling_expect(c, lst)
    check_culling(m, w, out, recent, n_recent, kept, culled, erased)
    assert G.error_count() == 0
    G.close()


def test_map_point_culling_host_form():
    c, lst = MC.culling_case(40)
    n_mp, n_obs = len(c["mp_bad"]), len(c["obs_kf"])
    h = {k: np.ascontiguousarray(c[k]).copy() for k in ("kf_n", "kf_mp", "kf_octave", "mp_bad", "obs_mp", "obs_kf", "obs_idx", "kf_order",
                                                        "mp_first_kf_id", "mp_found", "mp_visible")}
    hm = cabi.fill(cabi.CovisMap(), max_keyframes=c["K"], kp_stride=c["S"], n_mp=n_mp, n_obs=n_obs,
                   **{k: h[k] for k in ("kf_n", "kf_mp", "kf_octave", "mp_bad", "obs_mp", "obs_kf", "obs_idx", "kf_order")})
    recent, n_recent = np.concatenate([lst, np.full(GUARD, -1, np.int32)]), np.array([len(lst)], np.int32)
    culled, n_culled, n_erased, erased = np.full(len(recent), -1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.full((n_obs, 4), -1, np.int32)
    ha = cabi.fill(cabi.MapPointCullingArgs(), cur_kf_id=MC.CUR_KF_ID, n_th_obs=2, mp_first_kf_id=h["mp_first_kf_id"], mp_found=h["mp_found"],
                   mp_visible=h["mp_visible"], recent_cap=len(recent), d_recent=recent, d_n_recent=n_recent, kf_mp=h["kf_mp"], mp_bad=h["mp_bad"],
                   obs_kf=h["obs_kf"], d_n_culled=n_culled, d_culled=culled, d_n_erased=n_erased, erased_cap=n_obs, d_erased=erased)
    G = CovisibilityGraph(c["K"])
    assert lib().fb_covis_map_point_culling(G.h, C.byref(hm), C.byref(ha)) == 0
    w, kept, exp_culled, exp_erased = culling_expect(c, lst)
    assert recent[:n_recent[0]].tolist() == kept and culled[:n_culled[0]].tolist() == exp_culled
    assert erased[:n_erased[0]].tolist() == [list(r) for r in exp_erased]
    assert np.array_equal(h["mp_bad"], w.mp_bad) and np.array_equal(h["kf_mp"], w.kf_mp) and np.array_equal(h["obs_kf"], w.obs_kf)
    G.close()


def test_sequence_on_one_handle():
    """process_new_keyframe -> update_connections -> first_connection -> map_point_culling -> local_map with reuse_index = 1:
    both edits must leave the handle's index invalid, and the graph must be the model's"""
    c, slot, nf = MC.new_keyframe_case(70, 96, 12, None)
    K = c["K"]
    outs = []
    for reuse in (True, False):
        G, m, t, a = setup(c, obs_spare=nf)
        G.update_connections(m, list(range(K - 1)))                                                    # the graph before the new key frame
        recent, n_recent = G.recent_list(120, c["recent"])
        G.process_new_keyframe(m, a, slot, nf, recent, n_recent)
        nc, fr = G.update_connections(m, [slot])
        G.first_connection([slot], nc, fr)
        G.map_point_culling(m, MC.CUR_KF_ID, c["mp_first_kf_id"], c["mp_found"], c["mp_visible"], recent, n_recent)
        c2 = dict(c, kf_mp=m.t["kf_mp"].cpu().numpy(), mp_bad=m.t["mp_bad"].cpu().numpy()[:len(c["mp_bad"])])
        outs.append(local_map_out(G, m, c2, reuse))
        if not reuse:
            w = R.World(c)
            g = CR.Graph(K, c["kf_order"])
            as_map = lambda: CR.Map(w.kf_n, w.kf_mp, w.kf_octave, w.mp_bad, w.obs_mp, w.obs_kf, w.obs_idx, c["kf_order"])
            for s in range(K - 1):
                g.update_connections(as_map(), s)
            rl = [int(x) for x in c["recent"]]
            R.process_new_keyframe(w, slot, nf, rl)
            g.update_connections(as_map(), slot)
            R.map_point_culling(w, rl, MC.CUR_KF_ID, c["mp_first_kf_id"], c["mp_found"], c["mp_visible"])
            for s in range(K):
                n, sl, wt = G.ordered(s)
                n = int(n.cpu()[0])
                assert sl.cpu().numpy()[:n].tolist() == g.ordered[s] and wt.cpu().numpy()[:n].tolist() == g.ordered_w[s]
            assert np.array_equal(m.t["obs_kf"].cpu().numpy()[:len(w.obs_kf)], w.obs_kf) and np.array_equal(m.t["kf_mp"].cpu().numpy(), w.kf_mp)
        G.close()
    assert outs[0] == outs[1]
