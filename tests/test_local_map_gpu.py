"""The spanning tree and Tracking::UpdateLocalMap on the device (fb_covis_tree_*, fb_covis_local_map*) against the literal
model tests/local_map_ref.py.  Everything is integer work: the comparisons are exact equality, on every output array and on
the tree state."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import covis_ref as R
import local_map_cases as LC
import local_map_ref as LR
from fishbirdeyevisualslam_amd import cabi, covis_problem as P
from test_covis import _host_map, ref_map
from test_local_map import model_of, set_bad_case

pytestmark = pytest.mark.gpu
GUARD = 4


def _dev(arr, K):
    from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceMap
    return CovisibilityGraph(K), DeviceMap(arr)


def _device_of(case):
    G, M = _dev(case["arr"], case["K"])
    G.set_order(case["arr"]["kf_order"])
    for a, b, w in case["conns"]:
        G.add_connection(a, b, w)
    for c, p in case["parents"]:
        G.change_parent(c, p)
    return G, M


def _pad(frames, S=None):
    S = max(1, max(len(f) for f in frames)) if S is None else S
    mp = np.full((len(frames), S), -1, np.int32)
    for b, f in enumerate(frames):
        mp[b, :len(f)] = f
    return mp


def both(G, M, t, m, frames, kf_bad, local_in=None, ref_in=None, cap_kf=None, cap_mp=None, gate=None, reuse=False, S=None, what=""):
    """the device call on the batch `frames` and the model a sequence at a time; everything compared; -> (device arrays, model outs)"""
    import torch
    B, K = len(frames), G.K
    cap_kf = LR.list_limit(K) if cap_kf is None else cap_kf
    cap_mp = max(m.n_mp, 1) if cap_mp is None else cap_mp
    local_in = [[] for _ in frames] if local_in is None else local_in
    ref_in = [-1] * B if ref_in is None else ref_in
    mp = _pad(frames, S)
    n = [len(f) for f in frames]
    d, a = G.local_map_arrays(n, mp, kf_bad, cap_kf, cap_mp, local_kf=local_in, ref_kf=ref_in, gate_row=None if gate is None else gate[0],
                              gate_min=0 if gate is None else gate[1], guard=GUARD)
    before = {k: v.cpu().numpy().copy() for k, v in d.items()}
    G.local_map(M, a, reuse_index=reuse)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    obs = m.observations()
    outs = []
    for b in range(B):
        kf, pts = got["d_local_kf"][b * cap_kf:(b + 1) * cap_kf], got["d_local_mp"][b * cap_mp:(b + 1) * cap_mp]
        if gate is not None and gate[0][b] < gate[1]:                             # left entirely alone
            for k in ("d_n_local_kf", "d_n_local_mp", "d_ref_kf", "d_n_voters", "d_overflow"):
                assert got[k][b] == before[k][b], (what, b, k)
            assert np.array_equal(got["d_map_point"][b], before["d_map_point"][b]), (what, b)
            assert np.array_equal(kf, before["d_local_kf"][b * cap_kf:(b + 1) * cap_kf]) and (pts == -5).all(), (what, b)
            outs.append(None)
            continue
        fr = list(frames[b])
        w = LR.update_local_map(t, m, len(fr), fr, kf_bad, local_in[b], ref_in[b], cap_kf, cap_mp, obs=obs)
        outs.append(w)
        assert got["d_n_voters"][b] == w["n_voters"] and got["d_ref_kf"][b] == w["ref_kf"], (what, b)
        assert got["d_n_local_kf"][b] == w["n_local_kf"], (what, b, got["d_n_local_kf"][b], w["n_local_kf"])
        assert kf[:len(w["local_kf"])].tolist() == w["local_kf"], (what, b)
        assert (kf[max(len(w["local_kf"]), len(local_in[b])):] == -5).all(), (what, b)   # nothing past the list (or what came in)
        assert got["d_n_local_mp"][b] == w["n_local_mp"] and got["d_overflow"][b] == w["overflow"], (what, b)
        assert pts[:len(w["local_mp"])].tolist() == w["local_mp"] and (pts[len(w["local_mp"]):] == -5).all(), (what, b)
        assert got["d_map_point"][b][:len(fr)].tolist() == fr and (got["d_map_point"][b][len(fr):] == -1).all(), (what, b)
    assert (got["d_local_kf"][B * cap_kf:] == -5).all() and (got["d_local_mp"][B * cap_mp:] == -5).all(), what   # nothing past a capacity
    return got, outs


def _same_tree(G, t, what=""):
    import torch
    p, l, f = G.tree_get()
    torch.cuda.synchronize()
    wp, wl, wf = t.state()
    assert np.array_equal(p.cpu().numpy(), wp) and np.array_equal(l.cpu().numpy(), wl) and np.array_equal(f.cpu().numpy(), wf), what


def test_hand_cases_one_per_quirk():
    for name, case in list(LC.local_map_cases().items()) + [("limit", LC.expansion_limit_case()), ("voters_95", LC.expansion_limit_case(95))]:
        G, M = _device_of(case)
        g, t, m = model_of(case)
        got, outs = both(G, M, t, m, [case["frame"]], case["kf_bad"], [case["local_in"]], [case["ref_in"]], what=name)
        for k, v in case["want"].items():
            if k != "map_point":
                assert outs[0][k] == v, (name, k)
        if name == "limit":                                                      # capacities one below the needed lengths
            both(G, M, t, m, [case["frame"]], case["kf_bad"], cap_kf=81, cap_mp=79, what="caps")
            both(G, M, t, m, [case["frame"]], case["kf_bad"], cap_kf=82, cap_mp=80, what="caps exact")
        _same_tree(G, t, name)
        assert G.error_count() == 0, name
        G.close()


@pytest.fixture(scope="module")
def planted():
    """make_covis_problem with its graph, a random tree over the used slots and some bad key frames, on the device and in the model"""
    import torch
    p = P.make_covis_problem(1, K=70, S=96)
    m = ref_map(p)
    G, M = _dev(p, p["K"])
    g = R.Graph(p["K"], p["kf_order"])
    G.update_connections(M, p["used"])
    for a in p["used"]:
        g.update_connections(m, a)
    rng = np.random.default_rng(7)
    K, used = p["K"], p["used"]
    parent, linked = np.full(K, -1, np.int32), np.zeros(K, np.uint8)
    for i, s in enumerate(used[1:], 1):
        parent[s] = used[int(rng.integers(0, i))] if rng.random() < 0.9 else -1
        linked[s] = 1 if parent[s] >= 0 and rng.random() < 0.9 else 0
    first = (rng.random(K) < 0.3).astype(np.uint8)
    t = LR.Tree(g)
    t.set_state(parent, linked, first)
    G.tree_set(parent, linked, first)
    kf_bad = np.zeros(K, np.uint8)
    kf_bad[rng.choice(used, 6, replace=False)] = 1
    torch.cuda.synchronize()
    yield p, m, G, M, g, t, kf_bad, rng
    G.close()


def _frame(rng, m, n, bad_share=0.1):
    live = np.nonzero(m.mp_bad == 0)[0]
    dead = np.nonzero(m.mp_bad != 0)[0]
    f = [int(rng.choice(dead)) if rng.random() < bad_share else int(rng.choice(live)) for _ in range(n)]
    for i in range(0, n, 7):
        f[i] = -1                                                                # NULL features
    if n > 20:
        f[11] = f[3]                                                             # a point at two features
    return f


def test_planted_map_random_tree_every_frame_size(planted):
    p, m, G, M, g, t, kf_bad, rng = planted
    _same_tree(G, t, "set")
    sizes = [0, 1, 63, 64, 65, 96]
    frames = [_frame(rng, m, n) for n in sizes]
    carried = [[int(x) for x in rng.choice(p["used"], 5, replace=False)] for _ in sizes]
    for f, l in zip(frames, carried):                                            # batch 1
        both(G, M, t, m, [f], kf_bad, [l], [3], S=96, what="batch 1, n = %d" % len(f))
    both(G, M, t, m, frames[:3], kf_bad, carried[:3], [3, 4, 5], S=96, what="batch 3 a")
    got, outs = both(G, M, t, m, frames[3:], kf_bad, carried[3:], [3, 4, 5], S=96, what="batch 3 b")
    assert outs[0]["n_voters"] > 0 and G.error_count() == 0
    # a small local list for one sequence: few voters, so the expansion runs (most frames above have more than 80 * 0 voters)
    few = [[int(x) for x in m.kf_mp[s][:int(m.kf_n[s])] if x >= 0][:6] for s in (9, 30, 47)]
    got, outs = both(G, M, t, m, few, kf_bad, what="few voters")
    assert all(o["n_local_kf"] <= 83 for o in outs)


def test_capacities_dirty_entries_and_the_gate(planted):
    p, m, G, M, g, t, kf_bad, rng = planted
    frames = [_frame(rng, m, 64) for _ in range(3)]
    carried = [[5, 9, 30], [12, 400000, -3, 9], [7]]                             # out-of-range key frames in a list that comes in
    frames[1] = [-1] * 10                                                        # ... which is the list an empty counter keeps
    frames[2][5] = m.n_mp + 77                                                   # an out-of-range point of the frame
    e0 = G.error_count()
    got, outs = both(G, M, t, m, frames, kf_bad, carried, [1, 2, 3], gate=([10, 12, 10], 10), what="dirty")
    assert outs[1]["carried"] and outs[1]["local_mp"] and G.error_count() - e0 == sum(o["errors"] for o in outs) == 3
    got, outs = both(G, M, t, m, frames, kf_bad, carried, [1, 2, 3], gate=([10, 9, 10], 10), what="gated")
    assert outs[1] is None and outs[0] is not None
    need_kf, need_mp = outs[0]["n_local_kf"], outs[0]["n_local_mp"]
    got, outs = both(G, M, t, m, frames[:1], kf_bad, cap_kf=need_kf - 1, cap_mp=need_mp, what="cap_kf - 1")
    assert outs[0]["overflow"] == 1
    got, outs = both(G, M, t, m, frames[:1], kf_bad, cap_kf=need_kf, cap_mp=need_mp - 1, what="cap_mp - 1")
    assert outs[0]["overflow"] == 1 and outs[0]["n_local_mp"] == need_mp
    got, outs = both(G, M, t, m, frames[:1], kf_bad, cap_kf=need_kf, cap_mp=need_mp, what="exact")
    assert outs[0]["overflow"] == 0


def test_reuse_index_after_a_window_call_and_the_host_twin(planted):
    import torch
    import fishbirdeyevisualslam_amd as fb
    from fishbirdeyevisualslam_amd.covis import DeviceTables
    p, m, G, M, g, t, kf_bad, rng = planted
    frames = [_frame(rng, m, 96), _frame(rng, m, 30)]
    T = DeviceTables(dict(p, **P.window_tables(p, 7)))
    G.reserve_local_map(M.n_mp, M.n_obs, n_q=1, batch=2, with_window=True)
    w = G.local_window(M, T, p["cur"], False)
    got1, _ = both(G, M, t, m, frames, kf_bad, reuse=True, what="reuse after the window")
    rc, hd, slots, fixed = G.window_header()                                     # the window's own arrays are still there
    assert rc == 0 and hd["n_local"] >= 1 and slots[0] == p["cur"]
    got0, _ = both(G, M, t, m, frames, kf_bad, reuse=False, what="rebuilt")
    G.update_connections(M, [p["cur"]]); g.update_connections(m, p["cur"])
    got2, _ = both(G, M, t, m, frames, kf_bad, reuse=True, what="reuse after update_connections")
    for k in got0:
        assert np.array_equal(got0[k], got1[k]), k
    # the host-pointer twin on a handle of its own with the same graph and tree
    L = fb.lib()
    hm, keep = _host_map(p)
    h = C.c_void_p()
    fb.check(L.fb_covis_create(p["K"], C.byref(h)), "create")
    vp = lambda x: C.c_void_p(x.ctypes.data)
    slots = np.array(p["used"], np.int32)
    o1, o2 = np.zeros(len(slots), np.int32), np.zeros(len(slots), np.int32)
    g2 = R.Graph(p["K"], p["kf_order"])
    fb.check(L.fb_covis_update_connections(h, C.byref(hm), len(slots), vp(slots), vp(o1), vp(o2)), "update")
    for a in p["used"]:
        g2.update_connections(m, a)
    t2 = LR.Tree(g2)
    for c in range(p["K"]):
        if t.parent[c] >= 0 and t.parent[c] != c:
            fb.check(L.fb_covis_change_parent_dev(h, c, t.parent[c], None), "change_parent")
            t2.change_parent(c, t.parent[c])
    K, S, B = p["K"], 96, 2
    cap_kf, cap_mp = LR.list_limit(K), m.n_mp
    a = cabi.LocalMapArgs()
    arrs = dict(d_n=np.array([len(f) for f in frames], np.int32), d_map_point=_pad(frames, S), d_kf_bad=kf_bad.copy(),
                d_local_kf=np.full(B * cap_kf, -5, np.int32), d_n_local_kf=np.zeros(B, np.int32), d_local_mp=np.full(B * cap_mp, -5, np.int32),
                d_n_local_mp=np.zeros(B, np.int32), d_ref_kf=np.full(B, -1, np.int32), d_n_voters=np.zeros(B, np.int32),
                d_overflow=np.zeros(B, np.int32))
    cabi.fill(a, batch=B, kp_stride=S, cap_kf=cap_kf, cap_mp=cap_mp, **arrs)
    fb.check(L.fb_covis_local_map(h, C.byref(hm), C.byref(a)), "local_map")
    par, lk, fi = np.zeros(K, np.int32), np.zeros(K, np.uint8), np.zeros(K, np.uint8)
    fb.check(L.fb_covis_tree_get(h, vp(par), vp(lk), vp(fi)), "tree_get")
    assert np.array_equal(par, t2.state()[0]) and np.array_equal(lk, t2.state()[1]) and fi.all()
    obs = m.observations()
    for b in range(B):
        fr = list(frames[b])
        w = LR.update_local_map(t2, m, len(fr), fr, kf_bad, [], -1, cap_kf, cap_mp, obs=obs)
        assert arrs["d_n_local_kf"][b] == w["n_local_kf"] and arrs["d_local_kf"][b * cap_kf:][:w["n_local_kf"]].tolist() == w["local_kf"]
        assert arrs["d_n_local_mp"][b] == w["n_local_mp"] and arrs["d_local_mp"][b * cap_mp:][:w["n_local_mp"]].tolist() == w["local_mp"]
        assert arrs["d_ref_kf"][b] == w["ref_kf"] and arrs["d_map_point"][b][:len(fr)].tolist() == fr
    root = max(range(K), key=lambda s: len(t2.childs[s]))
    n, out = np.zeros(1, np.int32), np.full(K, -7, np.int32)
    fb.check(L.fb_covis_children(h, root, vp(n), vp(out)), "children")
    assert out[:n[0]].tolist() == t2.get_childs(root) and (out[n[0]:] == -7).all() and n[0] >= 2
    L.fb_covis_destroy(h)


def test_window_header_ends_with_an_index_built_over_it(planted):
    """The window's lists lie at the start of the scratch.  A local_map that reuses the window's index keeps them; an
    update_connections or a keyframe_culling builds its index over them, and the header call then refuses."""
    from fishbirdeyevisualslam_amd.covis import DeviceTables
    p, m, G, M, g, t, kf_bad, rng = planted
    frames = [_frame(rng, m, 40)]
    T = DeviceTables(dict(p, **P.window_tables(p, 7)))
    e0 = G.error_count()                                                         # (the handle is shared: earlier tests count on purpose)
    G.reserve_local_map(M.n_mp, M.n_obs, n_q=1, batch=1, with_window=True)
    G.local_window(M, T, p["cur"], False)
    both(G, M, t, m, frames, kf_bad, reuse=True, what="reuse behind the window")
    rc, hd, slots, fixed = G.window_header()
    assert rc == cabi.FB_OK and hd["n_local"] >= 1 and slots[0] == p["cur"]
    G.update_connections(M, [p["cur"]]); g.update_connections(m, p["cur"])
    assert G.window_header()[0] == cabi.FB_ERR_ARG, "update_connections wrote its index over the window's lists"
    G.local_window(M, T, p["cur"], False)
    assert G.window_header()[0] == cabi.FB_OK
    G.keyframe_culling(M, p["cur"])
    assert G.window_header()[0] == cabi.FB_ERR_ARG, "keyframe_culling wrote its index over the window's lists"
    assert G.error_count() == e0


def test_reuse_index_whose_tail_does_not_fit_rebuilds_once():
    """A fresh handle without a reserve: update_connections sizes the scratch for its index alone, so the local map's own
    arrays do not fit behind it.  reuse_index = 1 then rebuilds (the scratch grows), and the next one reuses."""
    p = P.make_covis_problem(1, K=70, S=96)
    m = ref_map(p)
    G, M = _dev(p, p["K"])
    g = R.Graph(p["K"], p["kf_order"])
    G.update_connections(M, p["used"])
    for a in p["used"]:
        g.update_connections(m, a)
    t = LR.Tree(g)
    kf_bad = np.zeros(p["K"], np.uint8)
    rng = np.random.default_rng(11)
    frames = [_frame(rng, m, 96), _frame(rng, m, 30)]
    got1, _ = both(G, M, t, m, frames, kf_bad, reuse=True, what="reuse that has to grow")
    got2, _ = both(G, M, t, m, frames, kf_bad, reuse=True, what="reuse again")
    got0, _ = both(G, M, t, m, frames, kf_bad, reuse=False, what="rebuilt")
    for k in got0:
        assert np.array_equal(got0[k], got1[k]) and np.array_equal(got0[k], got2[k]), k
    assert G.error_count() == 0
    G.close()


def test_tree_maintenance_chain_against_the_model():
    import torch
    p = P.make_covis_problem(1, K=70, S=96)
    m = ref_map(p)
    G, M = _dev(p, p["K"])
    g = R.Graph(p["K"], p["kf_order"])
    t = LR.Tree(g)
    K = p["K"]
    rng = np.random.default_rng(3)
    fid = rng.permutation(K).astype(np.int32)                                    # one key frame has frame id 0
    in_map = np.ones(K, np.uint8)
    in_map[[23, 32]] = 0
    rest = [s for s in p["used"] if s not in p["batch"]]
    for state4, batch in ((False, rest[:30]), (True, rest[30:]), (True, p["batch"][:5] + [p["batch"][0]])):   # the last: a batch of 5 and a repeat
        nc, fr = G.update_connections(M, batch)
        G.first_connection(batch, nc, fr, id0_slot=rest[0], now_state4=state4, kf_frame_id=fid, kf_in_map=in_map)
        for a in batch:
            t.update_connections(m, a, id0=rest[0], now_state4=state4, frame_id=fid, in_map=in_map)
        _same_tree(G, t, "first_connection")
    assert (t.state()[0] >= 0).sum() > 40 and t.first[rest[0]]
    kf_bad = np.zeros(K, np.uint8)
    inner = sorted((s for s in range(K) if t.parent[s] >= 0), key=lambda s: -len(t.childs[s]))[:3]
    assert len(t.childs[inner[0]]) >= 2
    for i, s in enumerate(inner):                                                # SetBadFlag: the tree and the graph part, in either order
        if i % 2:
            G.erase_keyframe(s); G.tree_erase_keyframe(s, kf_bad)
        else:
            G.tree_erase_keyframe(s, kf_bad); G.erase_keyframe(s)
        t.set_bad_flag(s, kf_bad); g.erase_keyframe(s)
        kf_bad[s] = 1
        _same_tree(G, t, "set_bad_flag %d" % s)
    for s in inner[:2] + [rest[3]]:
        n, sl = G.children(s)
        par = G.parent(s)
        torch.cuda.synchronize()
        assert par.cpu().tolist() == [t.parent[s]]
        if not kf_bad[s]:
            assert sl.cpu().numpy()[:int(n.cpu()[0])].tolist() == t.get_childs(s)
    frames = [_frame(rng, m, 40), _frame(rng, m, 8)]
    both(G, M, t, m, frames, kf_bad, what="after the chain")
    G.tree_erase_keyframe(rest[0], kf_bad); t.set_bad_flag(rest[0], kf_bad)      # no parent: nothing but the counter
    _same_tree(G, t, "no parent")
    assert G.error_count() == 1 == t.errors
    G.clear(); t.clear()
    _same_tree(G, t, "clear")
    G.close()


def test_set_bad_flag_hand_case_and_more_children_than_a_workgroup():
    g, t, bad = set_bad_case()
    from fishbirdeyevisualslam_amd.covis import CovisibilityGraph
    G = CovisibilityGraph(8)
    G.set_order(np.array(g.kf_order, np.uint64))
    G.change_parent(1, 0)
    for c in (2, 3, 4, 5, 6):
        G.change_parent(c, 1)
    for a, b, w in ((3, 0, 20), (4, 0, 20), (2, 4, 9), (2, 1, 30), (6, 0, 50), (5, 7, 40)):
        G.add_connection(a, b, w)
    G.tree_erase_keyframe(1, bad); t.set_bad_flag(1, bad)
    _same_tree(G, t, "hand")
    assert t.state()[0].tolist() == [-1, 0, 4, 0, 0, 0, 0, -1]
    G.erase_child(0, 2); t.erase_child(0, 2)
    G.erase_child(4, 2); t.erase_child(4, 2)
    _same_tree(G, t, "erase_child")
    G.close()
    # the hub: slot 1 (parent 0) has 1100 children; a chain of links makes a round's new candidate unlock the next child
    p = P.make_hub_problem()
    K = p["K"]
    G = CovisibilityGraph(K)
    G.set_order(p["kf_order"])
    g = R.Graph(K, p["kf_order"])
    t = LR.Tree(g)
    kids = list(range(2, 1102))
    parent, linked = np.full(K, -1, np.int32), np.zeros(K, np.uint8)
    parent[1], linked[1] = 0, 1
    parent[kids], linked[kids] = 1, 1
    G.tree_set(parent, linked, np.ones(K, np.uint8)); t.set_state(parent, linked, np.ones(K, np.uint8))
    rng = np.random.default_rng(9)
    bad = np.zeros(K, np.uint8)
    bad[rng.choice(kids, 20, replace=False)] = 1
    links = [(c, 0, int(rng.integers(1, 4))) for c in kids[:40]]                 # these see the parent's parent
    links += [(c, kids[int(rng.integers(0, i))], int(rng.integers(1, 6))) for i, c in enumerate(kids[:70]) if i >= 40]   # ... these an earlier child
    for c, o, w in links:
        G.add_connection(c, o, w); g.add_connection(c, o, w)
    G.tree_erase_keyframe(1, bad); t.set_bad_flag(1, bad)
    _same_tree(G, t, "1100 children")
    assert (t.state()[0][kids] != 0).sum() >= 5 and (t.state()[0][kids[70:]] == 0).all() and G.error_count() == 0
    G.close()


def test_a_point_with_more_observers_than_a_workgroup_and_the_full_slot_range():
    p = P.make_hub_problem()
    hub = P.add_point(p, list(range(1, 1201)))                                   # 1200 observers: more than 80 voters, more than 1024 edges
    m = ref_map(p)
    G, M = _dev(p, p["K"])
    g = R.Graph(p["K"], p["kf_order"])
    t = LR.Tree(g)
    kf_bad = np.zeros(p["K"], np.uint8)
    kf_bad[[5, 700]] = 1
    got, outs = both(G, M, t, m, [[hub, 3, hub], [7]], kf_bad, what="hub")
    assert outs[0]["n_voters"] == 1201 and outs[0]["n_local_kf"] == 1199 and outs[1]["n_local_kf"] == 2
    assert G.error_count() == 0
    G.close()
    p = P.make_sparse_problem()                                                  # slots 0 and 4095 in use
    m = ref_map(p)
    G, M = _dev(p, p["K"])
    g = R.Graph(p["K"], p["kf_order"])
    t = LR.Tree(g)
    G.update_connections(M, p["used"])
    for a in p["used"]:
        g.update_connections(m, a)
    for c, q in ((4095, 0), (4094, 4095), (2048, 4095), (1, 4093)):
        G.change_parent(c, q); t.change_parent(c, q)
    kf_bad = np.zeros(p["K"], np.uint8)
    f0 = [int(x) for x in m.kf_mp[0][:4]]
    f1 = [int(x) for x in m.kf_mp[4093][:3]]
    got, outs = both(G, M, t, m, [f0, f1, []], kf_bad, [[], [], [4095, 0]], what="sparse")
    assert 4095 in outs[0]["local_kf"] and 0 in outs[0]["local_kf"] and outs[2]["carried"] and outs[2]["local_mp"]
    _same_tree(G, t, "sparse")
    assert G.error_count() == 0
    G.close()


# ---- the chain on the synthetic drive (helpers after tests/test_track_chain_gpu.py) ----------------------------------------
def _drive(seed):
    """one sequence of the synthetic drive with its first frame in the chain; local lists in use"""
    import torch
    from fishbirdeyevisualslam_amd import sequence as S, track as T
    wh, bwh = (640, 480), (384, 384)
    seq = S.Sequence(1, 5, seed=seed, front_wh=wh, bird_wh=bwh, fx=250.0, fy=250.0, device="cuda:0")
    tc = T.TrackChain(1, wh, bwh, K=seq.Kc, D=seq.D, use_lists=True)
    mask = torch.from_numpy(seq.mask).cuda()
    f, b, c = seq.render(0)
    tc.extract(f, b, c, mask)
    M, MB, mp0, mpb0, Tcw0 = seq.build_map(tc.view("cur"), tc.tables, map_cap=tc.map_cap, bird_cap=tc.bird_cap)
    nb = int(MB["n"][0])
    lb = np.zeros((1, tc.bird_cap), np.int32)
    lb[0, :nb] = np.arange(nb)
    tc.set_map(M, MB, (np.zeros((1, tc.map_cap), np.int32), np.zeros(1, np.int32)), (lb, np.array([nb], np.int32)))
    tc.init_first(mp0, mpb0, Tcw0)
    return seq, tc, mask, M


def _graph_over(M, seed, Kc=12, S=1024):
    """a random observation graph over the drive's map points: every point is seen by one to three of Kc key frames"""
    rng = np.random.default_rng(seed)
    n = int(M["n"][0])
    b = P.MapBuilder(Kc, S, seed)
    b.mp_bad = [int(x) for x in M["bad"][0][:n]]
    for mp in range(n):
        for kf in rng.choice(Kc, int(rng.integers(1, 4)), replace=False):
            b.observe(mp, int(kf), int(rng.integers(0, 8)))
    arr = b.arrays(P.pointer_like_order(rng, Kc, list(range(Kc))), tombstones=0.05)
    arr.update(K=Kc, S=S)
    return arr


def test_track_graph_chain_equals_the_chain_with_a_host_built_list():
    """Run A: TrackWithMotionModel, wait, download mvpMapPoints, the model builds the list, upload, TrackLocalMap.  Run B: the
    same frames through fb_frame_update_local_map_dev (frame 1) and fb_frame_track_graph_dev (frames 2, 3, 4) with no wait in
    between.  The device list equals the model's; B's frame arrays (mvpMapPoints with its cleared bad points included), pose and
    counters are byte-equal to A's."""
    import torch
    import fishbirdeyevisualslam_amd as fb
    L = fb.lib()
    seqA, tcA, mask, MA = _drive(9300)
    arr = _graph_over(MA, 17)
    m = ref_map(arr)
    G, Md = _dev(arr, arr["K"])
    g = R.Graph(arr["K"], arr["kf_order"])
    t = LR.Tree(g)
    every = list(range(arr["K"]))
    nc, fr = G.update_connections(Md, every)
    G.first_connection(every, nc, fr, id0_slot=0)
    for a in every:
        t.update_connections(m, a, id0=0)
    _same_tree(G, t, "drive graph")
    kf_bad = np.zeros(arr["K"], np.uint8)
    kf_bad[5] = 1
    cap_kf, mc, obs = LR.list_limit(arr["K"]), tcA.map_cap, m.observations()
    s = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    MM = cabi.FB_CNT["MATCHES_MAP"]
    local_kf, ref, viewsA, lists, cleared = [], -1, [], [], 0
    for k in range(1, 5):                                                        # ---- run A
        f, b, c = seqA.render(k)
        tcA.set_delta(seqA.delta(k))
        tcA.extract(f, b, c, mask)
        fb.check(L.fb_frame_track_motion_model_dev(tcA.cur, tcA.last, C.byref(tcA.targs), s()), "motion model")
        v = tcA.view("cur")                                                      # the wait and the download
        assert v["counts"][MM][0] >= 10
        n = int(v["n"][0])
        mp = v["map_point"][0, :n].tolist()
        held = list(mp)
        w = LR.update_local_map(t, m, n, mp, kf_bad, local_kf, ref, cap_kf, mc, obs=obs)
        assert w["n_voters"] > 0 and w["overflow"] == 0
        if mp != held:                                                           # :2138 cleared bad points: mvpMapPoints goes back up
            assert not v["outlier"][0, :n].any()                                 # (the upload call also clears mvbOutlier, which is clear: :1364)
            back = v["map_point"].copy()
            back[0, :n] = mp
            back_d = torch.from_numpy(back).cuda()
            fb.check(L.fb_frame_set_map_points_dev(tcA.cur, C.c_void_p(back_d.data_ptr()), None, s()), "set_map_points")
            cleared += 1
        local_kf, ref = w["local_kf"], w["ref_kf"]
        up = np.zeros((1, mc), np.int32)
        up[0, :w["n_local_mp"]] = w["local_mp"]
        tcA.local_mp.copy_(torch.from_numpy(up).cuda())
        tcA.n_local_mp.copy_(torch.tensor([w["n_local_mp"]], dtype=torch.int32).cuda())
        fb.check(L.fb_frame_track_local_map_dev(tcA.cur, tcA.last, C.byref(tcA.targs), s()), "local map")
        tcA.k += 1
        viewsA.append(tcA.view("last"))
        lists.append(w)
    tcA.close()
    assert cleared >= 1                                                          # the drive does hold bad points after the first half
    seqB, tcB, mask, MB = _drive(9300)                                           # ---- run B
    assert all(np.array_equal(MA[k], MB[k]) for k in MA)
    d, a = G.local_map_arrays([0], np.full((1, 1), -1, np.int32), kf_bad, cap_kf, mc)
    cabi.fill(a, d_local_mp=tcB.local_mp, d_n_local_mp=tcB.n_local_mp)
    G.reserve_local_map(Md.n_mp, Md.n_obs, n_q=arr["K"], batch=1)
    for k in range(1, 5):
        f, b, c = seqB.render(k)
        tcB.set_delta(seqB.delta(k))
        tcB.extract(f, b, c, mask)
        a.reuse_index = 0 if k <= 2 else 1                                       # the graph call with a rebuilt index, then with the kept one
        if k == 1:
            fb.check(L.fb_frame_track_motion_model_dev(tcB.cur, tcB.last, C.byref(tcB.targs), s()), "motion model")
            fb.check(L.fb_frame_update_local_map_dev(tcB.cur, G.h, C.byref(Md.c), C.byref(a), s()), "update local map")
            fb.check(L.fb_frame_track_local_map_dev(tcB.cur, tcB.last, C.byref(tcB.targs), s()), "local map")
        else:
            fb.check(L.fb_frame_track_graph_dev(tcB.cur, tcB.last, C.byref(tcB.targs), G.h, C.byref(Md.c), C.byref(a), s()), "track graph")
        tcB.k += 1
        vB, vA, w = tcB.view("last"), viewsA[k - 1], lists[k - 1]
        nl = int(tcB.n_local_mp.cpu()[0])
        assert nl == w["n_local_mp"] and tcB.local_mp.cpu().numpy()[0, :nl].tolist() == w["local_mp"], k
        nk = int(d["d_n_local_kf"].cpu()[0])
        assert nk == w["n_local_kf"] and d["d_local_kf"].cpu().numpy()[:nk].tolist() == w["local_kf"] and int(d["d_ref_kf"].cpu()[0]) == w["ref_kf"], k
        assert int(d["d_n_voters"].cpu()[0]) == w["n_voters"] and int(d["d_overflow"].cpu()[0]) == 0
        n, nbird = int(vA["n"][0]), int(vA["n_bird"][0])
        assert n == int(vB["n"][0]) and nbird == int(vB["n_bird"][0])
        for key in vA:                                                           # per-feature arrays up to the counts, the rest whole
            cut = n if key in ("kps", "kps_un", "desc", "map_point", "outlier") else nbird if key in (
                "kps_bird", "desc_bird", "bird_cam_xyz", "map_point_bird", "bird_outlier") else None
            x, y = (vA[key], vB[key]) if cut is None else (vA[key][0, :cut], vB[key][0, :cut])
            assert x.tobytes() == y.tobytes(), (k, key)
        assert vB["counts"][cabi.FB_CNT["LOCAL_MATCHES"]][0] > 0
    wrong = cabi.LocalMapArgs.from_buffer_copy(a)
    cabi.fill(wrong, d_local_mp=d["d_local_mp"])
    assert L.fb_frame_track_graph_dev(tcB.cur, tcB.last, C.byref(tcB.targs), G.h, C.byref(Md.c), C.byref(wrong), s()) == cabi.FB_ERR_ARG
    assert G.error_count() == 0
    tcB.close()
    G.close()


def test_host_program_drives_the_host_pointer_variants(tmp_path):
    """tests/cpp/local_map_host_test.cpp (fb_covis_tree_get, fb_covis_children, fb_covis_local_map) in a fresh child process."""
    import fishbirdeyevisualslam_amd as fb
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.dirname(fb.LIB_PATH)
    exe = str(tmp_path / "local_map_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"), "-I", os.path.join(pkg, "host"),
                           os.path.join(root, "tests", "cpp", "local_map_host_test.cpp"), "-o", exe, "-L", pkg, "-lfishbird_hip",
                           "-Wl,-rpath," + pkg])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"local_map_host_test ok" in r.stdout
