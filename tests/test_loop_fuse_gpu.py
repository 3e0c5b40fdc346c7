"""fb_covis_replace_points / fb_covis_loop_fuse on the device against the literal model (tests/loop_fuse_ref.py), through the
C ABI, and the d_set_Scw output of fb_covis_correct_loop.  Everything is integer or byte work (the Scw rows are casts of
the doubles the model also holds): every output is compared for equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import covis_ref as CR
import loop_fuse_cases as LC
import loop_fuse_ref as LR
import map_correct_cases as MCC
from fishbirdeyevisualslam_amd import cabi, lib
from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceMap, DeviceTables

pytestmark = pytest.mark.gpu
GUARD = 3
CASES = LC.all_cases()
MAP_KEYS = ("kf_n", "kf_mp", "kf_octave", "mp_bad", "obs_mp", "obs_kf", "obs_idx", "kf_order")


@pytest.fixture(scope="module")
def model():
    """the model's answers, computed once and left unchanged"""
    out = {}
    for name, (c, op) in CASES:
        w = LR.World(c)
        if op[0] == "replace":
            LR.replace_points(w, op[1], op[2])
        else:
            LR.loop_fuse(w, op[1], len(op[2]), op[2])
        out[name] = w
    return out


def run_device(c, op, n_pairs=None, replaced_cap=None, added_cap=None, null_logs=False):
    """null_logs: both caps 0 and both log pointers NULL"""
    spare = (len(op[2]) if op[0] == "loop_fuse" else 0) + GUARD
    G = CovisibilityGraph(c["K"])
    m = DeviceMap(c, obs_spare=spare)
    n_rows = len(op[1]) if op[0] == "replace" else len(op[2])
    n_rows = 0 if null_logs else (n_rows if replaced_cap is None else replaced_cap)
    t, fuse = G.point_fuse_arrays(m, c["kf_bad"], c["kf_desc"], c["mp_desc"], c["mp_found"], c["mp_visible"], replaced_cap=n_rows, guard=GUARD)
    if null_logs:
        fuse.d_replaced = None
    if op[0] == "replace":
        G.replace_points(m, fuse, op[1], op[2], n_pairs=n_pairs)
        added = None
    elif null_logs:
        mt, n_added = torch.tensor(op[2], dtype=torch.int32, device="cuda"), G._i32(1, -1)
        a = cabi.fill(cabi.LoopFuseArgs(), cur_slot=op[1], n_features=len(op[2]), d_matched=mt, obs_cap=m.obs_cap, obs_idx=m.t["obs_idx"],
                      d_n_added=n_added, added_cap=0)
        a.map = fuse
        assert lib().fb_covis_loop_fuse_dev(G.h, C.byref(m.c), C.byref(a), None) == 0
        m.grow(len(op[2]))
        torch.cuda.synchronize()
        added = (n_added, torch.full((4 * GUARD,), -5, dtype=torch.int32))
    else:
        added = G.loop_fuse(m, fuse, op[1], op[2], added_cap=added_cap, guard=GUARD)
    return G, m, t, added, n_rows


def check_map(c, w, G, m, t):
    n_mp, n0 = len(c["mp_bad"]), len(c["obs_kf"])
    assert np.array_equal(m.t["kf_mp"].cpu().numpy(), w.kf_mp)
    assert np.array_equal(m.t["mp_bad"].cpu().numpy()[:n_mp], w.mp_bad)
    got = {k: m.t[k].cpu().numpy() for k in ("obs_mp", "obs_kf", "obs_idx")}
    keep = got["obs_kf"] >= 0
    assert sorted(zip(got["obs_mp"][keep].tolist(), got["obs_kf"][keep].tolist(), got["obs_idx"][keep].tolist())) == w.live_edges()
    for k, exp in (("obs_mp", w.obs_mp), ("obs_kf", w.obs_kf), ("obs_idx", w.obs_idx)):
        assert np.array_equal(got[k][n0:len(exp)], exp[n0:]), k + ": the owned block (new edges packed, the rest tombstones)"
        assert np.all(got[k][len(exp):] == -1), k + ": past the block"
    for k, exp, width, fill in (("mp_desc", w.desc, 32, 0xEE), ("mp_found", w.found, 1, -5), ("mp_visible", w.visible, 1, -5),
                                ("mp_replaced", w.replaced, 1, -5)):
        a = t[k].cpu().numpy()
        assert np.array_equal(a[:n_mp * width].reshape(np.asarray(exp).shape), exp), k
        assert np.all(a[max(n_mp, 1) * width:] == fill), k + ": guard rows"
    assert G.error_count() == w.errors


def check(c, w, G, m, t, added, n_rows):
    check_map(c, w, G, m, t)
    n_rep = int(t["d_n_replaced"].cpu()[0])
    rows = t["d_replaced"].cpu().numpy()
    assert n_rep == len(w.replaced_rows) and rows[:2 * n_rep].reshape(-1, 2).tolist() == [list(r) for r in w.replaced_rows]
    assert np.all(rows[2 * max(n_rows, 1):] == -5) and np.all(rows[2 * n_rep:2 * n_rows] == -5)
    if added is not None:
        n_add, arr = int(added[0].cpu()[0]), added[1].cpu().numpy()
        assert n_add == len(w.added_rows) and arr[:4 * n_add].reshape(-1, 4).tolist() == [list(r) for r in w.added_rows]
        assert np.all(arr[4 * n_add:] == -5)


def check_cut(c, w, G, m, t, added, replaced_cap, added_cap):
    """the logs cut at their caps: the counts are the full ones, rows [0, cap) are the model's first, the rest keeps its fill"""
    check_map(c, w, G, m, t)
    rows, arr = t["d_replaced"].cpu().numpy(), added[1].cpu().numpy()
    assert int(t["d_n_replaced"].cpu()[0]) == len(w.replaced_rows) and int(added[0].cpu()[0]) == len(w.added_rows)
    nr, na = min(replaced_cap, len(w.replaced_rows)), min(added_cap, len(w.added_rows))
    assert rows[:2 * nr].reshape(-1, 2).tolist() == [list(r) for r in w.replaced_rows[:nr]] and np.all(rows[2 * nr:] == -5)
    assert arr[:4 * na].reshape(-1, 4).tolist() == [list(r) for r in w.added_rows[:na]] and np.all(arr[4 * na:] == -5)


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_dev_form_matches_the_model(model, name):
    c, op = dict(CASES)[name]
    G, m, t, added, n_rows = run_device(c, op)
    check(c, model[name], G, m, t, added, n_rows)
    G.close()


def test_the_device_count_cuts_the_pair_list():
    c, op = LC.generated_replace()
    G, m, t, added, n_rows = run_device(c, op, n_pairs=torch.tensor([45], dtype=torch.int32, device="cuda"))
    w = LR.World(c)
    LR.replace_points(w, op[1][:45], op[2][:45])
    check(c, w, G, m, t, added, n_rows)
    G.close()


def host_arrays(c, extra_edges):
    h = {k: np.ascontiguousarray(c[k]).copy() for k in MAP_KEYS + ("kf_bad", "kf_desc", "mp_desc", "mp_found", "mp_visible")}
    for k in ("obs_mp", "obs_kf", "obs_idx"):
        h[k] = np.concatenate([h[k], np.full(extra_edges, -1, np.int32)])
    n_mp = len(c["mp_bad"])
    h["mp_replaced"] = np.full(max(n_mp, 1), -1, np.int32)
    hm = cabi.fill(cabi.CovisMap(), max_keyframes=c["K"], kp_stride=c["S"], n_mp=n_mp, n_obs=len(c["obs_kf"]), **{k: h[k] for k in MAP_KEYS})
    return h, hm


@pytest.mark.parametrize("name", ["chain", "generated_replace", "loop_replace_and_add", "generated_loop_fuse"])
def test_host_pointer_form_matches_the_model(model, name):
    c, op = dict(CASES)[name]
    w = model[name]
    nf = len(op[2]) if op[0] == "loop_fuse" else 0
    h, hm = host_arrays(c, nf)
    n_rows = max(len(op[1]) if op[0] == "replace" else nf, 1)
    n_rep, rows = np.full(1, -1, np.int32), np.full((n_rows, 2), -5, np.int32)
    fuse = cabi.fill(cabi.PointFuseArrays(), d_n_replaced=n_rep, replaced_cap=n_rows, d_replaced=rows,
                     **{k: h[k] for k in ("kf_mp", "mp_bad", "obs_mp", "obs_kf", "mp_found", "mp_visible", "mp_replaced", "kf_bad", "kf_desc", "mp_desc")})
    G = CovisibilityGraph(c["K"])
    if op[0] == "replace":
        f, t = np.array(op[1], np.int32), np.array(op[2], np.int32)
        a = cabi.fill(cabi.ReplacePointsArgs(), n_pairs=len(f), d_from=f, d_to=t)
        a.map = fuse
        assert lib().fb_covis_replace_points(G.h, C.byref(hm), C.byref(a)) == 0
    else:
        mt, n_add, added = np.array(op[2], np.int32), np.full(1, -1, np.int32), np.full((nf, 4), -5, np.int32)
        a = cabi.fill(cabi.LoopFuseArgs(), cur_slot=op[1], n_features=nf, d_matched=mt, obs_cap=len(h["obs_kf"]), obs_idx=h["obs_idx"],
                      d_n_added=n_add, added_cap=nf, d_added=added)
        a.map = fuse
        assert lib().fb_covis_loop_fuse(G.h, C.byref(hm), C.byref(a)) == 0
        assert n_add[0] == len(w.added_rows) and added[:n_add[0]].tolist() == [list(r) for r in w.added_rows]
        assert np.array_equal(h["obs_idx"], w.obs_idx)
    n_mp = len(c["mp_bad"])
    assert np.array_equal(h["kf_mp"], w.kf_mp) and np.array_equal(h["mp_bad"], w.mp_bad)
    assert np.array_equal(h["obs_mp"], w.obs_mp) and np.array_equal(h["obs_kf"], w.obs_kf)
    assert np.array_equal(h["mp_desc"].reshape(-1, 32), w.desc) and np.array_equal(h["mp_found"], w.found)
    assert np.array_equal(h["mp_visible"], w.visible) and np.array_equal(h["mp_replaced"][:n_mp], w.replaced)
    assert n_rep[0] == len(w.replaced_rows) and rows[:n_rep[0]].tolist() == [list(r) for r in w.replaced_rows]
    G.close()


def test_loop_fuse_capacity_is_checked_on_the_host():
    c, op = LC.loop_replace_and_add()
    G = CovisibilityGraph(c["K"])
    m = DeviceMap(c, obs_spare=len(op[2]) - 1)
    t, fuse = G.point_fuse_arrays(m, c["kf_bad"], c["kf_desc"], c["mp_desc"], c["mp_found"], c["mp_visible"], replaced_cap=4)
    a = cabi.fill(cabi.LoopFuseArgs(), cur_slot=op[1], n_features=len(op[2]), d_matched=torch.tensor(op[2], dtype=torch.int32, device="cuda"),
                  obs_cap=m.obs_cap, obs_idx=m.t["obs_idx"], d_n_added=G._i32(1), added_cap=0)
    a.map = fuse
    assert lib().fb_covis_loop_fuse_dev(G.h, C.byref(m.c), C.byref(a), None) == cabi.FB_ERR_CAPACITY
    G.close()


# ---- d_set_Scw of fb_covis_correct_loop -------------------------------------------------------------------------------------------
def table_arrays(c):
    K, S, BS = c["K"], c["S"], c["BS"]
    return dict(kf_Tcw=c["kf_Tcw"], kf_bad=np.zeros(K, np.uint8), kf_init=np.zeros(K, np.uint8), kf_keys_un=np.zeros((K, S), cabi.KP_DTYPE),
                inv_level_sigma2=np.ones(len(c["scale_factors"]), np.float32), mp_xw=c["mp_xw"], kf_nb=c["kf_nb"], kf_mpb=c["kf_mpb"],
                kf_bird_octave=np.zeros((K, BS), np.uint8), kf_bird_xc=np.zeros((K, BS, 3), np.float32), mpb_bad=c["mpb_bad"],
                mpb_xw=c["mpb_xw"], bobs_mpb=np.zeros(0, np.int32), bobs_kf=np.zeros(0, np.int32), bobs_idx=np.zeros(0, np.int32))


def correct_loop_on_device(c, with_scw):
    G = CovisibilityGraph(c["K"])
    G.set_order(c["kf_order"])
    for a, b, wgt in c["connections"]:
        G.add_connection(a, b, wgt)
    m, t = DeviceMap(c), DeviceTables(table_arrays(c))
    d, a = G.correct_loop_arrays(m, c["scale_factors"], c["mp_ref_kf"], c["mp_normal"], c["mp_min_dist"], c["mp_max_dist"],
                                 with_set_scw=with_scw, guard=GUARD)
    G.correct_loop(m, t, a, c["cur"], c["q"], c["t"], c["s"])
    out = b"".join(x.cpu().numpy().tobytes() for x in (t.t["kf_Tcw"], t.t["mp_xw"], t.t["mpb_xw"], d["mp_normal"], d["mp_min_dist"], d["mp_max_dist"],
                                                       d["d_mp_corrected_ref"], d["d_n_set"], d["d_set_slots"]))
    scw = d["d_set_Scw"].cpu().numpy() if with_scw else None
    G.close()
    return out, scw


@pytest.mark.parametrize("seed", [100, 101, 102])
def test_set_scw_is_the_models_cast_and_null_changes_nothing(seed):
    from fishbirdeyevisualslam_amd import covis_problem as P
    c = P.make_map_correct_problem(seed)
    g, _, _ = MCC.models(c)
    order, exp = LR.corrected_scw(g, c)
    assert len(order) >= 2                                                                             # the product with Scw is exercised
    with_out, scw = correct_loop_on_device(c, True)
    without, _ = correct_loop_on_device(c, False)
    assert with_out == without
    n = len(order)
    assert np.array_equal(scw[:12 * n].view(np.uint32), exp.reshape(-1).view(np.uint32))               # bit-equal
    assert np.all(scw[12 * n:] == np.float32(7.0))                                                     # rows past the set and the guard


# ---- the loop fusion between two UpdateConnections, one stream, one synchronisation at the end ---------------------------------
def test_chain_update_connections_loop_fuse_update_connections():
    c, op = LC.generated_loop_fuse()
    K, cur = c["K"], op[1]
    G = CovisibilityGraph(K)
    m = DeviceMap(c, obs_spare=len(op[2]))
    t, fuse = G.point_fuse_arrays(m, c["kf_bad"], c["kf_desc"], c["mp_desc"], c["mp_found"], c["mp_visible"], replaced_cap=len(op[2]))
    G.update_connections(m, list(range(K)))
    G.loop_fuse(m, fuse, cur, op[2])
    G.update_connections(m, list(range(K)))
    rows = [G.ordered(s) for s in range(K)]
    torch.cuda.synchronize()
    w = LR.World(c)
    g = CR.Graph(K, c["kf_order"])
    as_map = lambda: CR.Map(w.kf_n, w.kf_mp, w.kf_octave, w.mp_bad, w.obs_mp, w.obs_kf, w.obs_idx, c["kf_order"])
    for s in range(K):
        g.update_connections(as_map(), s)
    before = [dict(zip(g.ordered[s], g.ordered_w[s])) for s in range(K)]
    LR.loop_fuse(w, cur, len(op[2]), op[2])
    for s in range(K):
        g.update_connections(as_map(), s)
    for s in range(K):
        n, sl, wt = rows[s]
        n = int(n.cpu()[0])
        assert sl.cpu().numpy()[:n].tolist() == g.ordered[s] and wt.cpu().numpy()[:n].tolist() == g.ordered_w[s]
    after = dict(zip(g.ordered[cur], g.ordered_w[cur]))
    assert any(after[k] > before[cur].get(k, 0) for k in after), "the fusion must strengthen or make a connection of cur"
    G.close()


# ---- SearchAndFuse ---------------------------------------------------------------------------------------------------------------
def saf_device(c, slots, scw, loop, before=None, replaced_cap=None, added_cap=None):
    from fishbirdeyevisualslam_amd import kf_problems as KP
    K, S = c["K"], c["S"]
    G = CovisibilityGraph(K)
    m = DeviceMap(c, obs_spare=len(slots) * S + GUARD)
    t, fuse = G.point_fuse_arrays(m, c["kf_bad"], c["kf_desc"], c["mp_desc"], c["mp_found"], c["mp_visible"],
                                  replaced_cap=len(loop) * len(slots) if replaced_cap is None else replaced_cap, guard=GUARD)
    cells = np.zeros((1, 64 * 48 + 1), np.int32)
    target, keep = KP.kf_target([dict(kf_kps=c["kf_keys_un"][0], kf_desc=c["kf_desc"][0])], "kf_", cells, np.zeros((1, S), np.int32))
    if before:
        before(G, m)
    out = G.search_and_fuse(m, fuse, target, slots, scw, loop, c["kf_keys_un"], c["mp_xw"], c["mp_normal"], c["mp_min_dist"], c["mp_max_dist"],
                            added_cap=added_cap, guard=GUARD)
    return G, m, t, out


def test_search_and_fuse_matches_the_model():
    c, slots, scw, loop = LC.search_and_fuse_scene()
    w = LR.World(c)
    n_fused = LR.search_and_fuse(w, c, slots, scw, loop)
    G, m, t, (d_n_fused, d_n_added, d_added) = saf_device(c, slots, scw, loop)
    got = d_n_fused.cpu().numpy()
    print("nFused", got[:len(slots)].tolist(), n_fused, w.stats)
    assert got[:len(slots)].tolist() == n_fused and np.all(got[len(slots):] == -5)
    check(c, w, G, m, t, (d_n_added, d_added), len(loop) * len(slots))
    G.close()


def test_search_and_fuse_host_pointer_form_matches_the_model():
    from fishbirdeyevisualslam_amd import kf_problems as KP
    c, slots, scw, loop = LC.search_and_fuse_scene()
    w = LR.World(c)
    n_fused = LR.search_and_fuse(w, c, slots, scw, loop)
    S, n_set, n_mp = c["S"], len(slots), len(c["mp_bad"])
    h, hm = host_arrays(c, n_set * S)
    n_rows = n_set * len(loop)
    n_rep, rows = np.full(1, -1, np.int32), np.full((n_rows, 2), -5, np.int32)
    fuse = cabi.fill(cabi.PointFuseArrays(), d_n_replaced=n_rep, replaced_cap=n_rows, d_replaced=rows,
                     **{k: h[k] for k in ("kf_mp", "mp_bad", "obs_mp", "obs_kf", "mp_found", "mp_visible", "mp_replaced", "kf_bad", "kf_desc", "mp_desc")})
    target, keep = KP.kf_target([dict(kf_kps=c["kf_keys_un"][0], kf_desc=c["kf_desc"][0])], "kf_", np.zeros((1, 64 * 48 + 1), np.int32),
                                np.zeros((1, S), np.int32))
    f = {k: np.ascontiguousarray(c[k], np.float32).copy() for k in ("mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist")}
    kps = np.ascontiguousarray(c["kf_keys_un"]).copy()
    d_fused, n_add, added = np.full(n_set, -5, np.int32), np.full(1, -1, np.int32), np.full((n_set * S, 4), -5, np.int32)
    a = cabi.fill(cabi.SearchAndFuseArgs(), n_set=n_set, d_set_slots=np.array(slots, np.int32), d_set_Scw=np.ascontiguousarray(scw, np.float32),
                  n_loop=len(loop), d_loop_mp=np.array(loop, np.int32), th=4.0, log_scale_factor=target.log_scale_factor, n_levels=target.n_levels,
                  kf_keys_un=kps.view(np.uint8).reshape(-1), obs_cap=len(h["obs_kf"]), obs_idx=h["obs_idx"], d_n_fused=d_fused, d_n_added=n_add,
                  added_cap=n_set * S, d_added=added, **f)
    a.cam, a.grid, a.scale_factors, a.inv_level_sigma2, a.map = target.cam, target.grid, target.scale_factors, target.inv_level_sigma2, fuse
    G = CovisibilityGraph(c["K"])
    assert lib().fb_covis_search_and_fuse(G.h, C.byref(hm), C.byref(a)) == 0
    assert d_fused.tolist() == n_fused
    assert n_add[0] == len(w.added_rows) and added[:n_add[0]].tolist() == [list(r) for r in w.added_rows] and np.all(added[n_add[0]:] == -5)
    assert n_rep[0] == len(w.replaced_rows) and rows[:n_rep[0]].tolist() == [list(r) for r in w.replaced_rows]
    assert np.array_equal(h["kf_mp"], w.kf_mp) and np.array_equal(h["mp_bad"], w.mp_bad) and np.array_equal(h["obs_idx"], w.obs_idx)
    assert np.array_equal(h["obs_mp"], w.obs_mp) and np.array_equal(h["obs_kf"], w.obs_kf)
    assert np.array_equal(h["mp_desc"].reshape(-1, 32), w.desc) and np.array_equal(h["mp_found"], w.found)
    assert np.array_equal(h["mp_visible"], w.visible) and np.array_equal(h["mp_replaced"][:n_mp], w.replaced)
    assert G.error_count() == w.errors
    G.close()


def test_search_and_fuse_without_loop_points_leaves_tombstones():
    c, slots, scw, loop = LC.search_and_fuse_scene()
    G, m, t, (d_n_fused, d_n_added, d_added) = saf_device(c, slots, scw, [])
    w = LR.World(c)
    assert LR.search_and_fuse(w, c, slots, scw, [], search=lambda *a: []) == [0] * len(slots)
    assert d_n_fused.cpu().numpy()[:len(slots)].tolist() == [0] * len(slots)
    check(c, w, G, m, t, (d_n_added, d_added), 0)
    G.close()


def loop_scene_with_poses():
    """the generated scene as a CorrectLoop problem: the set key frames get the rigid poses their loop points were made for,
    cur = the last of them with the other two as its covisibles, and mg2oScw = cur's own pose with s = 1, so that every
    CorrectedSim3 is the key frame's pose again up to rounding and the loop points still project where they were made to"""
    import map_correct_ref as MCR
    c, slots, scw, loop = LC.search_and_fuse_scene()
    K, cur = c["K"], slots[-1]
    c = dict(c)
    Tcw = np.array(c["kf_Tcw"], np.float32).reshape(K, 12)
    for slot, row in zip(slots, scw):
        Tcw[slot] = (row.astype(np.float64) / np.linalg.norm(row[:3].astype(np.float64))).astype(np.float32)
    T = Tcw[cur].reshape(3, 4).astype(np.float64)
    c.update(kf_Tcw=Tcw, cur=cur, q=MCR.quat_from_R(T[:, :3]), t=T[:, 3].copy(), s=1.0, BS=1, kf_nb=np.zeros(K, np.int32),
             kf_mpb=np.full((K, 1), -1, np.int32), mpb_bad=np.zeros(0, np.uint8), mpb_xw=np.zeros((0, 3), np.float32))
    return c, slots, loop


def chain_front(c, slots):
    """update_connections of every key frame -> the covisibles of cur -> correct_loop with d_set_Scw, enqueued on one handle"""
    K, S, cur = c["K"], c["S"], c["cur"]
    G = CovisibilityGraph(K)
    m, tt = DeviceMap(c, obs_spare=S + K * S), DeviceTables(table_arrays(c))
    G.update_connections(m, list(range(K)))
    for s in slots[:-1]:
        G.add_connection(cur, s, 30)
    d, a = G.correct_loop_arrays(m, c["scale_factors"], c["mp_ref_kf"], c["mp_normal"], c["mp_min_dist"], c["mp_max_dist"], with_set_scw=True)
    G.correct_loop(m, tt, a, cur, c["q"], c["t"], c["s"])
    return G, m, tt, d


def test_chain_correct_loop_loop_fuse_search_and_fuse_update_connections():
    """update_connections -> correct_loop (with d_set_Scw) -> loop_fuse -> search_and_fuse on the d_set_slots / d_set_Scw that
    correct_loop wrote -> batched update_connections, one stream, one synchronisation at the end.  The model takes the floats
    correct_loop leaves (pinned in test_map_correct_gpu.py) from a run of that front part alone, and its own CorrectedSim3."""
    from fishbirdeyevisualslam_amd import kf_problems as KP
    c, slots, loop = loop_scene_with_poses()
    K, S, cur, n_mp = c["K"], c["S"], c["cur"], len(c["mp_bad"])
    matched = np.full(S, -1, np.int32)
    matched[1], matched[2] = loop[-1], loop[-2]                                                        # two empty features of cur
    # the model's graph and set
    w0 = LR.World(c)
    g = CR.Graph(K, c["kf_order"])
    as_map = lambda w: CR.Map(w.kf_n, w.kf_mp, w.kf_octave, w.mp_bad, w.obs_mp, w.obs_kf, w.obs_idx, c["kf_order"])
    for s in range(K):
        g.update_connections(as_map(w0), s)
    for s in slots[:-1]:
        g.add_connection(cur, s, 30)
    order, exp_scw = LR.corrected_scw(g, c)
    n_set = len(order)
    assert set(slots) <= set(order)
    # the front part alone: what correct_loop leaves
    G, m, tt, d = chain_front(c, slots)
    torch.cuda.synchronize()
    assert int(d["d_n_set"].cpu()[0]) == n_set and d["d_set_slots"].cpu().numpy()[:n_set].tolist() == order
    assert np.array_equal(d["d_set_Scw"].cpu().numpy()[:12 * n_set].view(np.uint32), exp_scw.reshape(-1).view(np.uint32))
    left = dict(mp_xw=tt.t["mp_xw"].cpu().numpy()[:3 * n_mp].reshape(-1, 3), mp_normal=d["mp_normal"].cpu().numpy()[:3 * n_mp].reshape(-1, 3),
                mp_min_dist=d["mp_min_dist"].cpu().numpy()[:n_mp], mp_max_dist=d["mp_max_dist"].cpu().numpy()[:n_mp])
    G.close()
    # the whole chain, one synchronisation
    G, m, tt, d = chain_front(c, slots)
    t, fuse = G.point_fuse_arrays(m, c["kf_bad"], c["kf_desc"], c["mp_desc"], c["mp_found"], c["mp_visible"], replaced_cap=n_set * len(loop))
    target, keep = KP.kf_target([dict(kf_kps=c["kf_keys_un"][0], kf_desc=c["kf_desc"][0])], "kf_", np.zeros((1, 64 * 48 + 1), np.int32),
                                np.zeros((1, S), np.int32))
    G.loop_fuse(m, fuse, cur, matched)
    d_n_fused, d_n_added, d_added = G.search_and_fuse(m, fuse, target, d["d_set_slots"][:n_set], d["d_set_Scw"][:12 * n_set], loop, c["kf_keys_un"],
                                                      tt.t["mp_xw"][:3 * n_mp], d["mp_normal"][:3 * n_mp], d["mp_min_dist"][:n_mp], d["mp_max_dist"][:n_mp])
    G.update_connections(m, d["d_set_slots"][:n_set])
    rows = [G.ordered(s) for s in range(K)]
    conn = [G.connected(s) for s in slots]
    torch.cuda.synchronize()
    # the model on the same floats
    w = LR.World(dict(c, **left))
    LR.loop_fuse(w, cur, S, matched)
    n_loop_fuse_rep, n_loop_fuse_add = len(w.replaced_rows), len(w.added_rows)
    n_fused = LR.search_and_fuse(w, c, order, exp_scw, loop)
    print("set", order, "nFused", n_fused, w.stats)
    assert w.stats["add"] > 0 and w.stats["rep"] > 0 and w.stats["collision"] > 0 and w.stats["skipped_bad"] > 0
    for s in order:
        g.update_connections(as_map(w), s)
    assert d_n_fused.cpu().numpy()[:n_set].tolist() == n_fused
    n_add, arr = int(d_n_added.cpu()[0]), d_added.cpu().numpy()
    assert arr[:4 * n_add].reshape(-1, 4).tolist() == [list(r) for r in w.added_rows[n_loop_fuse_add:]]
    n_rep = int(t["d_n_replaced"].cpu()[0])
    assert t["d_replaced"].cpu().numpy()[:2 * n_rep].reshape(-1, 2).tolist() == [list(r) for r in w.replaced_rows[n_loop_fuse_rep:]]
    assert np.array_equal(m.t["kf_mp"].cpu().numpy(), w.kf_mp) and np.array_equal(m.t["mp_bad"].cpu().numpy()[:n_mp], w.mp_bad)
    assert np.array_equal(t["mp_desc"].cpu().numpy()[:32 * n_mp].reshape(-1, 32), w.desc)
    for s in range(K):
        n, sl, wt = rows[s]
        n = int(n.cpu()[0])
        assert sl.cpu().numpy()[:n].tolist() == g.ordered[s] and wt.cpu().numpy()[:n].tolist() == g.ordered_w[s]
    new_links = 0
    for s, (n, sl) in zip(slots, conn):
        new_links += len(set(sl.cpu().numpy()[:int(n.cpu()[0])].tolist()) & {0, 1})                   # the loop side: no link before
    assert new_links > 0
    G.close()


# ---- more live edges than key frames, the log cut, the device count, K = 1 and 33, SearchAndFuse on a shared view ----------------
def saf_host(c, slots, scw, loop, replaced_cap=None, added_cap=None):
    """fb_covis_search_and_fuse on host arrays -> (G, host arrays, d_n_fused, n_rep, rows, n_add, added), logs with GUARD rows"""
    from fishbirdeyevisualslam_amd import kf_problems as KP
    S, n_set = c["S"], len(slots)
    h, hm = host_arrays(c, n_set * S)
    rcap = n_set * len(loop) if replaced_cap is None else replaced_cap
    acap = n_set * S if added_cap is None else added_cap
    n_rep, rows = np.full(1, -1, np.int32), np.full((rcap + GUARD, 2), -5, np.int32)
    fuse = cabi.fill(cabi.PointFuseArrays(), d_n_replaced=n_rep, replaced_cap=rcap, d_replaced=rows,
                     **{k: h[k] for k in ("kf_mp", "mp_bad", "obs_mp", "obs_kf", "mp_found", "mp_visible", "mp_replaced", "kf_bad", "kf_desc", "mp_desc")})
    target, keep = KP.kf_target([dict(kf_kps=c["kf_keys_un"][0], kf_desc=c["kf_desc"][0])], "kf_", np.zeros((1, 64 * 48 + 1), np.int32),
                                np.zeros((1, S), np.int32))
    f = {k: np.ascontiguousarray(c[k], np.float32).copy() for k in ("mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist")}
    kps = np.ascontiguousarray(c["kf_keys_un"]).copy()
    d_fused, n_add, added = np.full(n_set, -5, np.int32), np.full(1, -1, np.int32), np.full((acap + GUARD, 4), -5, np.int32)
    a = cabi.fill(cabi.SearchAndFuseArgs(), n_set=n_set, d_set_slots=np.array(slots, np.int32), d_set_Scw=np.ascontiguousarray(scw, np.float32),
                  n_loop=len(loop), d_loop_mp=np.array(loop, np.int32), th=4.0, log_scale_factor=target.log_scale_factor, n_levels=target.n_levels,
                  kf_keys_un=kps.view(np.uint8).reshape(-1), obs_cap=len(h["obs_kf"]), obs_idx=h["obs_idx"], d_n_fused=d_fused, d_n_added=n_add,
                  added_cap=acap, d_added=added, **f)
    a.cam, a.grid, a.scale_factors, a.inv_level_sigma2, a.map = target.cam, target.grid, target.scale_factors, target.inv_level_sigma2, fuse
    G = CovisibilityGraph(c["K"])
    assert lib().fb_covis_search_and_fuse(G.h, C.byref(hm), C.byref(a)) == 0
    return G, h, d_fused, n_rep, rows, n_add, added


def check_host(c, w, G, h, n_rep, rows, n_add, added, replaced_cap, added_cap):
    """the host arrays against the model, the logs cut at their caps (rows past them and the guard rows keep their fill)"""
    n_mp = len(c["mp_bad"])
    assert np.array_equal(h["kf_mp"], w.kf_mp) and np.array_equal(h["mp_bad"], w.mp_bad) and np.array_equal(h["obs_idx"], w.obs_idx)
    assert np.array_equal(h["obs_mp"], w.obs_mp) and np.array_equal(h["obs_kf"], w.obs_kf)
    assert np.array_equal(h["mp_desc"].reshape(-1, 32), w.desc) and np.array_equal(h["mp_found"], w.found)
    assert np.array_equal(h["mp_visible"], w.visible) and np.array_equal(h["mp_replaced"][:n_mp], w.replaced)
    assert n_rep[0] == len(w.replaced_rows) and n_add[0] == len(w.added_rows)
    nr, na = min(replaced_cap, len(w.replaced_rows)), min(added_cap, len(w.added_rows))
    assert rows[:nr].tolist() == [list(r) for r in w.replaced_rows[:nr]] and np.all(rows[nr:] == -5)
    assert added[:na].tolist() == [list(r) for r in w.added_rows[:na]] and np.all(added[na:] == -5)
    assert G.error_count() == w.errors


def test_overflow_pairs_are_skipped_whole():
    c, op, w = LC.overflow_replace()
    G, m, t, added, n_rows = run_device(c, op)
    check(c, w, G, m, t, added, n_rows)
    for k in ("kf_mp", "obs_mp", "obs_kf", "obs_idx"):                                                 # what belongs to points 0 and 1 is as it came
        got, came = m.t[k].cpu().numpy().reshape(-1)[:c[k].size], np.asarray(c[k]).reshape(-1)
        own = np.isin(np.asarray(c["kf_mp"] if k == "kf_mp" else c["obs_mp"]).reshape(-1), (0, 1))
        assert np.array_equal(got[own], came[own]), k
    G.close()


def test_overflow_in_the_loop_fusion():
    c, op, w = LC.overflow_loop_fuse()
    G, m, t, added, n_rows = run_device(c, op)
    check(c, w, G, m, t, added, n_rows)
    G.close()


def test_overflow_in_search_and_fuse():
    c, slots, scw, loop, w, n_fused = LC.shared_view_overflow()
    G, m, t, (d_n_fused, d_n_added, d_added) = saf_device(c, slots, scw, loop)
    assert d_n_fused.cpu().numpy()[:len(slots)].tolist() == n_fused
    check(c, w, G, m, t, (d_n_added, d_added), len(loop) * len(slots))
    G.close()


LOG_CUTS = {"one_row": dict(replaced_cap=1, added_cap=1), "null": dict(null_logs=True), "full": {}}


@pytest.fixture(scope="module")
def cut_maps():
    return {}


@pytest.mark.parametrize("cut", list(LOG_CUTS))
def test_loop_fuse_logs_are_cut_at_their_caps(model, cut_maps, cut):
    c, op = LC.loop_two_adds()
    w = model["loop_two_adds"]
    assert len(w.replaced_rows) == 2 and len(w.added_rows) == 2
    G, m, t, added, n_rows = run_device(c, op, **LOG_CUTS[cut])
    caps = dict(one_row=(1, 1), null=(0, 0), full=(4, 4))[cut]
    check_cut(c, w, G, m, t, added, *caps)
    cut_maps[cut] = m.bytes() + b"".join(t[k].cpu().numpy().tobytes() for k in ("mp_desc", "mp_found", "mp_visible", "mp_replaced"))
    assert len(set(cut_maps.values())) == 1                                                            # the same map whatever the caps
    G.close()


@pytest.mark.parametrize("cut", list(LOG_CUTS))
def test_loop_fuse_host_pointer_logs_are_cut_at_their_caps(model, cut):
    c, op = LC.loop_two_adds()
    w = model["loop_two_adds"]
    rcap, acap = dict(one_row=(1, 1), null=(0, 0), full=(4, 4))[cut]
    nf = len(op[2])
    h, hm = host_arrays(c, nf)
    n_rep, rows = np.full(1, -1, np.int32), np.full((rcap + GUARD, 2), -5, np.int32)
    fuse = cabi.fill(cabi.PointFuseArrays(), d_n_replaced=n_rep, replaced_cap=rcap, d_replaced=None if cut == "null" else rows,
                     **{k: h[k] for k in ("kf_mp", "mp_bad", "obs_mp", "obs_kf", "mp_found", "mp_visible", "mp_replaced", "kf_bad", "kf_desc", "mp_desc")})
    mt, n_add, added = np.array(op[2], np.int32), np.full(1, -1, np.int32), np.full((acap + GUARD, 4), -5, np.int32)
    a = cabi.fill(cabi.LoopFuseArgs(), cur_slot=op[1], n_features=nf, d_matched=mt, obs_cap=len(h["obs_kf"]), obs_idx=h["obs_idx"],
                  d_n_added=n_add, added_cap=acap, d_added=None if cut == "null" else added)
    a.map = fuse
    G = CovisibilityGraph(c["K"])
    assert lib().fb_covis_loop_fuse(G.h, C.byref(hm), C.byref(a)) == 0
    check_host(c, w, G, h, n_rep, rows, n_add, added, rcap, acap)
    G.close()


@pytest.fixture(scope="module")
def saf_cut():
    """the generated scene, the model's answer, and caps one less than what the first key frame alone produces"""
    c, slots, scw, loop = LC.search_and_fuse_scene()
    first = LR.World(c)
    LR.search_and_fuse(first, c, slots[:1], scw[:1], loop)
    w = LR.World(c)
    n_fused = LR.search_and_fuse(w, c, slots, scw, loop)
    rcap, acap = len(first.replaced_rows) - 1, len(first.added_rows) - 1
    assert 0 < rcap < len(w.replaced_rows) - 1 and 0 < acap < len(w.added_rows) - 1                   # later key frames produce rows too
    return c, slots, scw, loop, w, n_fused, rcap, acap


def test_search_and_fuse_logs_are_cut_inside_the_first_key_frame(saf_cut):
    c, slots, scw, loop, w, n_fused, rcap, acap = saf_cut
    G, m, t, (d_n_fused, d_n_added, d_added) = saf_device(c, slots, scw, loop, replaced_cap=rcap, added_cap=acap)
    assert d_n_fused.cpu().numpy()[:len(slots)].tolist() == n_fused
    check_cut(c, w, G, m, t, (d_n_added, d_added), rcap, acap)
    G.close()


def test_search_and_fuse_host_pointer_logs_are_cut(saf_cut):
    c, slots, scw, loop, w, n_fused, rcap, acap = saf_cut
    G, h, d_fused, n_rep, rows, n_add, added = saf_host(c, slots, scw, loop, rcap, acap)
    assert d_fused.tolist() == n_fused
    check_host(c, w, G, h, n_rep, rows, n_add, added, rcap, acap)
    G.close()


@pytest.mark.parametrize("count", [0, -3, 1, 2, 7])
def test_the_device_count_on_the_chain(count):
    c, op = LC.chain()
    n = min(max(count, 0), 2)
    G, m, t, added, n_rows = run_device(c, op, n_pairs=torch.tensor([count], dtype=torch.int32, device="cuda"))
    w = LR.World(c)
    LR.replace_points(w, op[1][:n], op[2][:n])
    check(c, w, G, m, t, added, n_rows)
    if n == 0:
        assert int(t["d_n_replaced"].cpu()[0]) == 0 and m.bytes() == DeviceMap(c, obs_spare=GUARD).bytes()
    G.close()


SHARED = {"shared_view_scene": LC.shared_view_scene, "shared_view_bad_entries": LC.shared_view_bad_entries,
          "shared_view_short": LC.shared_view_short}


@pytest.fixture(scope="module")
def shared_model():
    out = {}
    for name, f in SHARED.items():
        c, slots, scw, loop = f()
        w = LR.World(c)
        out[name] = (w, LR.search_and_fuse(w, c, slots, scw, loop))
    return out


@pytest.mark.parametrize("name", list(SHARED))
def test_search_and_fuse_on_a_shared_view_matches_the_model(shared_model, name):
    c, slots, scw, loop = SHARED[name]()
    w, n_fused = shared_model[name]
    G, m, t, (d_n_fused, d_n_added, d_added) = saf_device(c, slots, scw, loop)
    got = d_n_fused.cpu().numpy()
    assert got[:len(slots)].tolist() == n_fused and np.all(got[len(slots):] == -5)
    check(c, w, G, m, t, (d_n_added, d_added), len(loop) * len(slots))
    if name == "shared_view_short":
        arr = d_added.cpu().numpy()[:4 * len(w.added_rows)].reshape(-1, 4)
        changed = m.t["kf_mp"].cpu().numpy() != c["kf_mp"]
        assert np.all(arr[:, 2] < 40) and not changed[:, 40:].any()
    G.close()


@pytest.mark.parametrize("name", list(SHARED))
def test_search_and_fuse_host_pointer_form_on_a_shared_view_matches_the_model(shared_model, name):
    c, slots, scw, loop = SHARED[name]()
    w, n_fused = shared_model[name]
    G, h, d_fused, n_rep, rows, n_add, added = saf_host(c, slots, scw, loop)
    assert d_fused.tolist() == n_fused
    check_host(c, w, G, h, n_rep, rows, n_add, added, len(slots) * len(loop), len(slots) * c["S"])
    G.close()
