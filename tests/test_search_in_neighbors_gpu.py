"""fb_covis_fuse_targets / fb_covis_search_in_neighbors on the device against the literal model
(tests/search_in_neighbors_ref.py), through the C ABI, in the device-pointer and the host-pointer form.  Integer and byte
outputs are compared for equality; mp_normal, mp_min_dist and mp_max_dist as tests/test_map_refresh_gpu.py compares them."""
import ctypes as C

import numpy as np
import pytest
import torch

import covis_ref as CR
import loop_fuse_ref as LR
import search_in_neighbors_cases as SC
import search_in_neighbors_ref as SR
from fishbirdeyevisualslam_amd import cabi, kf_problems as KP, lib
from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceMap

pytestmark = pytest.mark.gpu
GUARD = 3
CELLS = 64 * 48
FUSE_CASES = SC.all_fuse_cases()
MAP_KEYS = ("kf_n", "kf_mp", "kf_octave", "mp_bad", "obs_mp", "obs_kf", "obs_idx", "kf_order")


def kf_target(c):
    return KP.kf_target([dict(kf_kps=c["kf_keys_un"][0], kf_desc=c["kf_desc"][0])], "kf_", np.zeros((1, CELLS + 1), np.int32),
                        np.zeros((1, c["S"]), np.int32))[0]


def caps(d, n_launch):
    c = d["c"]
    return d.get("new_edge_cap", c["S"] * (len(d["targets"]) + 1)), d.get("cand_cap", len(c["mp_bad"]))


def run_model(d, n_launch=None, graph=None):
    c = d["c"]
    w = LR.World(c)
    g = CR.Graph(c["K"], c["kf_order"]) if graph is None else graph
    n_launch = len(d["targets"]) if n_launch is None else n_launch
    new_edge_cap, cand_cap = caps(d, n_launch)
    out = SR.search_in_neighbors(w, g, c, d["cur"], d.get("n_features_arg", d["n_features"]), d["targets"], n_launch=n_launch,
                                 new_edge_cap=new_edge_cap, cand_cap=cand_cap)
    return w, g, out


@pytest.fixture(scope="module")
def model():
    """the model's answers, computed once and left unchanged"""
    return {name: run_model(d) for name, d in FUSE_CASES}


def run_device(d, n_launch=None):
    c = d["c"]
    n_real = len(d["targets"])
    n_launch = n_real if n_launch is None else n_launch
    new_edge_cap, cand_cap = caps(d, n_launch)
    G = CovisibilityGraph(c["K"])
    m = DeviceMap(c, obs_spare=new_edge_cap + GUARD)
    t, fuse = G.point_fuse_arrays(m, c["kf_bad"], c["kf_desc"], c["mp_desc"], c["mp_found"], c["mp_visible"],
                                  replaced_cap=len(c["mp_bad"]) * 2, guard=GUARD)
    rt, refresh = G.refresh_arrays(m, c["kf_Tcw"], c["kf_bad"], c["kf_desc"], c["scale_factors"], c["mp_xw"], c["mp_ref_kf"], c["mp_normal"],
                                   c["mp_min_dist"], c["mp_max_dist"], c["mp_desc"], guard=GUARD)
    d_n = torch.tensor([n_real], dtype=torch.int32, device="cuda")
    d_t = torch.tensor(list(d["targets"]) + [-9] * (max(n_launch, 1) - n_real), dtype=torch.int32, device="cuda")
    out = G.search_in_neighbors(m, fuse, refresh, kf_target(c), d["cur"], d.get("n_features_arg", d["n_features"]), n_launch, d_n, d_t,
                                c["kf_keys_un"], new_edge_cap, cand_cap, added_cap=d.get("added_cap"), guard=GUARD)
    return G, m, t, rt, out


BOUND = 0.0        # as tests/test_map_refresh_gpu.py: the refresh repeats the model's float operations one by one


def close(a, b, normal=False):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    d = np.abs(a.astype(np.float64) - b) / (1.0 if normal else np.maximum(1.0, np.abs(b)))
    return d.size == 0 or float(d.max()) <= BOUND


def check(d, w, g, mo, G, m, t, rt, out, n_launch=None):
    c = d["c"]
    n_mp, n0 = len(c["mp_bad"]), len(c["obs_kf"])
    n_launch = len(d["targets"]) if n_launch is None else n_launch
    new_edge_cap, cand_cap = caps(d, n_launch)
    nf = out["n_fused"].cpu().numpy()
    print("nFused", nf[:n_launch + 1].tolist(), mo.n_fused)
    assert nf[:n_launch + 1].tolist() == mo.n_fused and np.all(nf[n_launch + 1:] == -5)
    cand = out["candidates"].cpu().numpy()
    assert int(out["n_candidates"].cpu()[0]) == mo.n_candidates
    assert cand[:len(mo.candidates)].tolist() == mo.candidates and np.all(cand[len(mo.candidates):] == -5)
    n_add, arr = int(out["n_added"].cpu()[0]), out["added"].cpu().numpy()
    n_row = min(n_add, d.get("added_cap", n_add))                                                      # rows past added_cap are not written
    assert n_add == len(w.added_rows) and arr[:4 * n_row].reshape(-1, 4).tolist() == [list(r) for r in w.added_rows[:n_row]]
    assert np.all(arr[4 * n_row:] == -5)
    n_rep, rows = int(t["d_n_replaced"].cpu()[0]), t["d_replaced"].cpu().numpy()
    assert n_rep == len(w.replaced_rows) and rows[:2 * n_rep].reshape(-1, 2).tolist() == [list(r) for r in w.replaced_rows]
    assert np.all(rows[2 * n_rep:] == -5)
    assert np.array_equal(m.t["kf_mp"].cpu().numpy(), w.kf_mp)
    assert np.array_equal(m.t["mp_bad"].cpu().numpy()[:n_mp], w.mp_bad)
    got = {k: m.t[k].cpu().numpy() for k in ("obs_mp", "obs_kf", "obs_idx")}
    keep = got["obs_kf"] >= 0
    assert sorted(zip(got["obs_mp"][keep].tolist(), got["obs_kf"][keep].tolist(), got["obs_idx"][keep].tolist())) == w.live_edges()
    for k, exp in (("obs_mp", w.obs_mp), ("obs_kf", w.obs_kf), ("obs_idx", w.obs_idx)):
        assert np.array_equal(got[k][n0:len(exp)], exp[n0:]), k + ": the owned block (new edges in order, the rest tombstones)"
        assert np.all(got[k][len(exp):] == -1), k + ": past the block"
    for k, exp, width, fill in (("mp_desc", w.desc, 32, 0xEE), ("mp_found", w.found, 1, -5), ("mp_visible", w.visible, 1, -5),
                                ("mp_replaced", w.replaced, 1, -5)):
        a = t[k].cpu().numpy()
        assert np.array_equal(a[:n_mp * width].reshape(np.asarray(exp).shape), exp), k
        assert np.all(a[max(n_mp, 1) * width:] == fill), k + ": guard rows"
    for k, exp, width in (("mp_normal", w.normal, 3), ("mp_min_dist", w.min_dist, 1), ("mp_max_dist", w.max_dist, 1)):
        a = rt[k].cpu().numpy()
        assert close(a[:n_mp * width], exp, k == "mp_normal"), k
        assert np.all(a[max(n_mp, 1) * width:] == np.float32(7.0)), k + ": guard rows"
    assert int(out["n_counter"].cpu()[0]) == mo.n_counter and int(out["front"].cpu()[0]) == mo.front
    for s in range(c["K"]):
        n, sl, wt = G.ordered(s)
        n = int(n.cpu()[0])
        assert sl.cpu().numpy()[:n].tolist() == g.ordered[s] and wt.cpu().numpy()[:n].tolist() == g.ordered_w[s], "the graph row of %d" % s
    assert G.error_count() == w.errors


@pytest.mark.parametrize("name", [n for n, _ in FUSE_CASES])
def test_dev_form_matches_the_model(model, name):
    d = dict(FUSE_CASES)[name]
    w, g, mo = model[name]
    for key, got in (("n_fused", mo.n_fused), ("added", [r[:3] for r in w.added_rows]), ("replaced", w.replaced_rows), ("candidates", mo.candidates),
                     ("errors", w.errors)):
        if key in d:
            assert got == d[key], "the hand answer: " + key
    G, m, t, rt, out = run_device(d)
    check(d, w, g, mo, G, m, t, rt, out)
    G.close()


def test_idle_launches_change_nothing(model):
    """n_targets = the cap with fewer real targets: the same map, nFused 0 for the idle launches"""
    d = dict(FUSE_CASES)["candidate_order"]
    w, g, mo = run_model(d, n_launch=6)
    assert mo.n_fused[:2] == model["candidate_order"][2].n_fused[:2] and mo.n_fused[2:6] == [0] * 4
    G, m, t, rt, out = run_device(d, n_launch=6)
    check(d, w, g, mo, G, m, t, rt, out, n_launch=6)
    w0 = model["candidate_order"][0]
    assert np.array_equal(w.kf_mp, w0.kf_mp) and w.live_edges() == w0.live_edges() and np.array_equal(w.desc, w0.desc)
    G.close()


def without_edges_of(c, slot):
    """the map as it is before ProcessNewKeyFrame of `slot`: kf_mp[slot] is filled, its points have no edge to it yet"""
    keep = np.asarray(c["obs_kf"]) != slot
    return dict(c, obs_mp=c["obs_mp"][keep], obs_kf=c["obs_kf"][keep], obs_idx=c["obs_idx"][keep])


def test_chain_on_the_generated_scene():
    """process_new_keyframe -> update_connections of every key frame -> fuse_targets -> search_in_neighbors with n_targets =
    nn * (1 + nn2) (idle launches past the device count) and a block of new edges that fills -> refresh_points of every point
    with reuse_index (the index the call left) -> local_window on the grown map; one stream, no host read in between; equal to
    the model chain"""
    import local_window_ref as LW
    import map_refresh_ref as R
    from fishbirdeyevisualslam_amd.covis import DeviceTables
    from test_local_window_gpu import _assert_window
    full, cur = SC.generated()
    c = without_edges_of(full, cur)
    K, S, N, cap, new_edge_cap = c["K"], c["S"], int(c["kf_n"][cur]), 20 * 6, SC.GEN_NEW_EDGE_CAP
    # the model chain
    w, g, recent = LR.World(c), CR.Graph(K, c["kf_order"]), []
    R.process_new_keyframe(w, cur, N, recent)
    w.home = w.obs_mp.copy()
    order = sorted(range(K), key=g.key)
    for s in order:
        g.update_connections(CR.Map(w.kf_n, w.kf_mp, w.kf_octave, w.mp_bad, w.obs_mp, w.obs_kf, w.obs_idx, w.kf_order), s)
    targets = SR.fuse_targets(g, cur, c["kf_bad"], 20, 5)
    assert len(targets) != len(set(targets)) and len(targets) < cap
    d = SC.case(c, cur, targets, new_edge_cap=new_edge_cap)
    mo = SR.search_in_neighbors(w, g, c, cur, N, targets, n_launch=cap, new_edge_cap=new_edge_cap, cand_cap=len(c["mp_bad"]))
    assert w.stats["block_full"] >= 1 and len(w.added_rows) == new_edge_cap
    R.refresh_points(w)
    tables = dict(kf_Tcw=w.kf_Tcw, kf_bad=w.kf_bad, kf_init=np.zeros(K, np.uint8), kf_keys_un=c["kf_keys_un"],
                  inv_level_sigma2=np.ones(len(c["scale_factors"]), np.float32), mp_xw=w.mp_xw)
    ref = LW.local_window(g, dict(tables, kf_order=c["kf_order"], kf_n=w.kf_n, kf_mp=w.kf_mp, mp_bad=w.mp_bad, obs_mp=w.obs_mp, obs_kf=w.obs_kf,
                                  obs_idx=w.obs_idx), cur, False)
    # the device chain
    G = CovisibilityGraph(K)
    m = DeviceMap(c, obs_spare=N + new_edge_cap + GUARD)
    t, fuse = G.point_fuse_arrays(m, c["kf_bad"], c["kf_desc"], c["mp_desc"], c["mp_found"], c["mp_visible"], replaced_cap=len(c["mp_bad"]) * 2,
                                  guard=GUARD)
    rt, refresh = G.refresh_arrays(m, c["kf_Tcw"], c["kf_bad"], c["kf_desc"], c["scale_factors"], c["mp_xw"], c["mp_ref_kf"], c["mp_normal"],
                                   c["mp_min_dist"], c["mp_max_dist"], c["mp_desc"], guard=GUARD)
    refresh.mp_desc = fuse.mp_desc                                                                     # one descriptor array for the chain
    dt = DeviceTables(tables)
    rec, n_rec = G.recent_list(N + 4)
    G.process_new_keyframe(m, refresh, cur, N, rec, n_rec)
    G.update_connections(m, order)
    d_n, d_t = G.fuse_targets(cur, c["kf_bad"], 20, 5, target_cap=cap, guard=GUARD)
    out = G.search_in_neighbors(m, fuse, refresh, kf_target(c), cur, N, cap, d_n, d_t, c["kf_keys_un"], new_edge_cap, len(c["mp_bad"]),
                                guard=GUARD)
    G.refresh_points(m, refresh, reuse_index=True)
    win = G.local_window(m, dt, cur, False)
    torch.cuda.synchronize()
    got_t = d_t.cpu().numpy()
    assert int(d_n.cpu()[0]) == len(targets) and got_t[:len(targets)].tolist() == targets and np.all(got_t[len(targets):] == -5)
    assert rec.cpu().numpy()[:int(n_rec.cpu()[0])].tolist() == recent
    check(d, w, g, mo, G, m, t, rt, out, n_launch=cap)
    _assert_window(win, ref)
    G.close()


# ---- the target list -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.TARGET_CASES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("form", ["dev", "host"])
def test_target_list(case, form):
    d = case()
    G = CovisibilityGraph(d["K"])
    G.set_order(d["kf_order"])
    for a, b, wt in d["connections"]:
        G.add_connection(a, b, wt)
    cap = d["nn"] * (1 + d["nn2"]) if d["target_cap"] is None else d["target_cap"]
    if form == "dev":
        n, t = G.fuse_targets(d["cur"], d["kf_bad"], d["nn"], d["nn2"], target_cap=cap, guard=GUARD)
        n, t = int(n.cpu()[0]), t.cpu().numpy()
    else:
        torch.cuda.synchronize()
        n, t = np.full(1, -1, np.int32), np.full(cap + GUARD, -5, np.int32)
        bad = np.ascontiguousarray(d["kf_bad"], np.uint8)
        assert lib().fb_covis_fuse_targets(G.h, d["cur"], d["nn"], d["nn2"], C.c_void_p(bad.ctypes.data), cap, C.c_void_p(n.ctypes.data),
                                           C.c_void_p(t.ctypes.data)) == 0
        n = int(n[0])
    exp = d["expected"]
    assert n == d.get("n_uncut", len(exp)) and t[:len(exp)].tolist() == exp and np.all(t[len(exp):] == -5)
    assert G.error_count() == d.get("errors", 0)
    G.close()


# ---- the host-pointer form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in FUSE_CASES])
def test_host_pointer_form_matches_the_model(model, name):
    d = dict(FUSE_CASES)[name]
    c = d["c"]
    w, g, mo = model[name]
    n_t = len(d["targets"])
    new_edge_cap, cand_cap = caps(d, n_t)
    added_cap = d.get("added_cap", new_edge_cap)
    n_mp = len(c["mp_bad"])
    h = {k: np.ascontiguousarray(c[k]).copy() for k in MAP_KEYS + ("kf_bad", "kf_desc", "mp_desc", "mp_found", "mp_visible", "kf_Tcw", "mp_xw",
                                                                   "mp_normal", "mp_min_dist", "mp_max_dist", "mp_ref_kf")}
    for k in ("obs_mp", "obs_kf", "obs_idx"):
        h[k] = np.concatenate([h[k], np.full(new_edge_cap, -1, np.int32)])
    h["mp_replaced"] = np.full(max(n_mp, 1), -1, np.int32)
    hm = cabi.fill(cabi.CovisMap(), max_keyframes=c["K"], kp_stride=c["S"], n_mp=n_mp, n_obs=len(c["obs_kf"]), **{k: h[k] for k in MAP_KEYS})
    n_rows = 2 * n_mp
    n_rep, rows = np.full(1, -1, np.int32), np.full((n_rows, 2), -5, np.int32)
    fuse = cabi.fill(cabi.PointFuseArrays(), d_n_replaced=n_rep, replaced_cap=n_rows, d_replaced=rows,
                     **{k: h[k] for k in ("kf_mp", "mp_bad", "obs_mp", "obs_kf", "mp_found", "mp_visible", "mp_replaced", "kf_bad", "kf_desc", "mp_desc")})
    target = kf_target(c)
    kps = np.ascontiguousarray(c["kf_keys_un"]).copy()
    o = dict(d_n_fused=np.full(n_t + 1, -5, np.int32), d_n_candidates=np.full(1, -1, np.int32), d_candidates=np.full(max(cand_cap, 1), -5, np.int32),
             d_n_added=np.full(1, -1, np.int32), d_added=np.full((max(new_edge_cap, 1), 4), -5, np.int32), d_n_counter=np.full(1, -1, np.int32),
             d_front=np.full(1, -7, np.int32))
    a = cabi.fill(cabi.SearchInNeighborsArgs(), cur_slot=d["cur"], n_features=d.get("n_features_arg", d["n_features"]), n_targets=n_t,
                  d_n_targets=np.array([n_t], np.int32), d_targets=np.array(d["targets"], np.int32), th=3.0,
                  log_scale_factor=target.log_scale_factor, n_levels=target.n_levels, kf_keys_un=kps.view(np.uint8).reshape(-1),
                  obs_cap=len(h["obs_kf"]), obs_idx=h["obs_idx"], new_edge_cap=new_edge_cap, cand_cap=cand_cap, added_cap=added_cap,
                  **{k: h[k] for k in ("kf_Tcw", "mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_ref_kf")}, **o)
    a.cam, a.grid, a.scale_factors, a.inv_level_sigma2, a.map = target.cam, target.grid, target.scale_factors, target.inv_level_sigma2, fuse
    G = CovisibilityGraph(c["K"])
    assert lib().fb_covis_search_in_neighbors(G.h, C.byref(hm), C.byref(a)) == 0
    assert o["d_n_fused"].tolist() == mo.n_fused and o["d_n_candidates"][0] == mo.n_candidates
    assert o["d_candidates"][:len(mo.candidates)].tolist() == mo.candidates and np.all(o["d_candidates"][len(mo.candidates):] == -5)
    n_add = int(o["d_n_added"][0])
    n_row = min(n_add, added_cap)
    assert n_add == len(w.added_rows) and o["d_added"][:n_row].tolist() == [list(r) for r in w.added_rows[:n_row]]
    assert np.all(o["d_added"][n_row:] == -5)
    assert n_rep[0] == len(w.replaced_rows) and rows[:n_rep[0]].tolist() == [list(r) for r in w.replaced_rows]
    assert np.array_equal(h["kf_mp"], w.kf_mp) and np.array_equal(h["mp_bad"], w.mp_bad) and np.array_equal(h["obs_idx"], w.obs_idx)
    assert np.array_equal(h["obs_mp"], w.obs_mp) and np.array_equal(h["obs_kf"], w.obs_kf)
    assert np.array_equal(h["mp_desc"].reshape(-1, 32), w.desc) and np.array_equal(h["mp_found"], w.found)
    assert np.array_equal(h["mp_visible"], w.visible) and np.array_equal(h["mp_replaced"][:n_mp], w.replaced)
    assert close(h["mp_normal"], w.normal, True) and close(h["mp_min_dist"], w.min_dist) and close(h["mp_max_dist"], w.max_dist)
    assert o["d_n_counter"][0] == mo.n_counter and o["d_front"][0] == mo.front
    assert G.error_count() == w.errors
    G.close()
