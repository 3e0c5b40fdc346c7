"""fb_covis_detect_loop, fb_covis_loop_map_points and fb_covis_loop_connections on the device against the literal model
(tests/loop_detect_ref.py) on the constructed cases (tests/loop_detect_cases.py), through the C ABI, with guard elements
behind every output.  Everything is integer work: every comparison is for equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import loop_detect_cases as LD
import loop_detect_ref as LR
from fishbirdeyevisualslam_amd import cabi, lib
from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceMap

pytestmark = pytest.mark.gpu
GUARD = 3


def device_graph(K, ops):
    G = CovisibilityGraph(K)
    keep = []
    for op in ops:
        if op[0] == "add":
            G.add_connection(op[1], op[2], op[3])
        else:
            m = DeviceMap(op[1])
            G.update_connections(m, op[2])
            keep.append(m)
    torch.cuda.synchronize()
    return G


def i32(x):
    return torch.tensor(list(x) if len(x) else [0], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("name,c", LD.detect_cases(), ids=[n for n, _ in LD.detect_cases()])
def test_consistency_groups(name, c):
    K = c["K"]
    G = device_graph(K, c["ops"])
    g = LD.model_graph(K, c["ops"])
    cg = LR.ConsistencyGroups()
    cap = c.get("cap_groups")
    if cap is not None:
        G.reserve_loop_groups(cap)
    for k, (cands, th) in enumerate(c["calls"]):
        cg.th = th
        exp = cg.detect(g, [x for x in cands if 0 <= x < K])
        over = 0
        if cap is not None:
            over = int(len(cg.groups) > cap)
            cg.groups = cg.groups[:cap]
        cand = torch.full((K,), -9, dtype=torch.int32, device="cuda")   # entries past the count are never read as candidates
        cand[:len(cands)] = i32(cands)[:len(cands)]
        n_enough, enough, header = G.detect_loop(i32([len(cands)]), cand, th, guard=GUARD)
        groups = G.loop_groups()
        print(name, "call", k, "enough", n_enough.tolist(), enough.tolist()[:len(exp) + GUARD], "header", header.tolist(), "groups", groups)
        assert n_enough.item() == len(exp)
        assert enough.tolist() == exp + [-5] * (K + GUARD - len(exp))
        assert header.tolist() == [len(cg.groups), over] + [-5] * GUARD
        assert groups == [(sorted(s), n) for s, n in cg.groups]
        assert exp == c["expect"][k][0] and over == c.get("overflow", [0] * 9)[k]
    assert G.error_count() == c.get("errors", 0)
    G.close()


def test_clear_empties_the_groups_and_erase_keyframe_does_not():
    c = LD.dl_no_previous()
    G = device_graph(8, c["ops"])
    G.detect_loop(i32([2]), i32([0, 5, 0, 0, 0, 0, 0, 0]), 3)
    G.erase_keyframe(1)
    assert G.loop_groups() == [([0, 1], 0), ([5], 0)]
    G.clear()
    assert G.loop_groups() == []
    G.close()


def test_detect_loop_host_pointers():
    c = LD.dl_four_calls()
    G = device_graph(8, c["ops"])
    cand = np.array([2, 0, 0, 0, 0, 0, 0, 0], np.int32)
    for k in range(4):
        n, ne, en, h = C.c_int32(1), C.c_int32(-5), np.full(8, -5, np.int32), cabi.LoopGroupsHeader()
        assert lib().fb_covis_detect_loop(G.h, C.byref(n), C.c_void_p(cand.ctypes.data), 3, C.byref(ne), C.c_void_p(en.ctypes.data), C.byref(h)) == 0
        assert (ne.value, en.tolist(), h.n_groups, h.overflow) == ((1, [2] + [-5] * 7, 1, 0) if k == 3 else (0, [-5] * 8, 1, 0))
    assert G.loop_groups() == [([2, 3], 3)]
    G.close()


POINTS = LD.points_cases()


@pytest.mark.parametrize("name,c", POINTS, ids=[n for n, _ in POINTS])
@pytest.mark.parametrize("short", [0, 1], ids=["fits", "cap_one_short"])
def test_loop_map_points(name, c, short):
    m = DeviceMap(c["map"])
    G = device_graph(m.K, c["ops"])
    ref = LD.ref_map(c["map"])
    exp = LR.loop_map_points(LD.model_graph(m.K, c["ops"], ref.kf_order), ref, c["matched"])
    assert exp == c["expect"]
    cap = len(exp) - short
    n_loop, loop_mp, overflow = G.loop_map_points(m, c["matched"], cap=cap, guard=GUARD)
    print(name, n_loop.tolist(), loop_mp.tolist(), overflow.tolist())
    assert n_loop.item() == cap and overflow.item() == short
    assert loop_mp.tolist() == exp[:cap] + [-5] * (GUARD + 1)
    assert G.error_count() == c.get("errors", 0)
    G.close()


def test_loop_map_points_host_pointers():
    c = LD.lp_first_holder_wins()
    G = device_graph(8, c["ops"])
    arrays = {k: np.ascontiguousarray(v) for k, v in c["map"].items() if k != "K"}
    hm = cabi.fill(cabi.CovisMap(), max_keyframes=8, kp_stride=arrays["kf_mp"].shape[1], n_mp=len(arrays["mp_bad"]),
                   n_obs=len(arrays["obs_kf"]), **arrays)
    n, over, out = C.c_int32(-5), C.c_int32(-5), np.full(6, -5, np.int32)
    assert lib().fb_covis_loop_map_points(G.h, C.byref(hm), 0, 4, C.byref(n), C.c_void_p(out.ctypes.data), C.byref(over)) == 0
    assert (n.value, over.value, out.tolist()) == (4, 0, c["expect"] + [-5, -5])
    G.close()


CONN = LD.connections_cases()


def graph_state(G, K):
    out = []
    for s in range(K):
        n, sl, w = G.ordered(s)
        nc, cs = G.connected(s)
        n, nc = n.item(), nc.item()
        out.append((sl[:n].tolist(), w[:n].tolist(), cs[:nc].tolist()))
    return out


@pytest.mark.parametrize("name,c", CONN, ids=[n for n, _ in CONN])
def test_loop_connections(name, c):
    m = DeviceMap(c["map"])
    K, n = m.K, len(c["set"])
    ref = LD.ref_map(c["map"])
    g = LD.model_graph(K, c["ops"], ref.kf_order)
    rows, n_counter, front = LR.loop_connections(g, ref, c["set"])
    assert rows == c["expect"]
    flat = [x for r in rows for x in r]
    off = np.cumsum([0] + [len(r) for r in rows]).tolist()
    G = device_graph(K, c["ops"])
    out = G.loop_connections(m, c["set"], lc_cap=len(flat), guard=GUARD)
    print(name, {k: v.tolist() for k, v in out.items()})
    assert out["header"].tolist() == [len(flat), 0] + [-5] * GUARD
    assert out["lc_off"].tolist() == off + [-5] * GUARD
    assert out["lc_slots"].tolist()[:len(flat) + GUARD] == flat + [-5] * GUARD
    assert out["n_counter"].tolist() == n_counter + [-5] * GUARD and out["front"].tolist() == front + [-5] * GUARD
    # the graph afterwards and the update's outputs: a plain fb_covis_update_connections on a second handle, and the model
    G2 = device_graph(K, c["ops"])
    nc2, fr2 = G2.update_connections(DeviceMap(c["map"]), c["set"])
    assert nc2.tolist() == n_counter and fr2.tolist() == front
    state = graph_state(G, K)
    assert state == graph_state(G2, K)
    assert state == [(g.ordered[s], g.ordered_w[s], g.get_connected_keyframes(s)) for s in range(K)]
    G.close()
    G2.close()


def test_loop_connections_list_length_on_the_device_and_overflow():
    """set_cap = 5 rows are launched, *d_n_set = 3: rows past the list are empty and their outputs untouched; lc_cap = 0 with
    one entry to report: overflow, nothing written."""
    c = LD.lc_set_members_excluded()
    m = DeviceMap(c["map"])
    G = device_graph(8, c["ops"])
    out = G.loop_connections(m, c["set"] + [4, 5], n_set=i32([3]), lc_cap=0, guard=GUARD)
    assert out["header"].tolist()[:2] == [1, 1]
    assert out["lc_off"].tolist() == [0, 0, 1, 1, 1, 1] + [-5] * GUARD
    assert out["lc_slots"].tolist() == [-5] * GUARD
    assert out["n_counter"].tolist() == c["n_counter"] + [-5] * (2 + GUARD)
    G.close()


def test_loop_connections_host_pointers():
    c = LD.lc_order_is_kf_order()
    G = device_graph(8, c["ops"])
    arrays = {k: np.ascontiguousarray(v) for k, v in c["map"].items() if k != "K"}
    hm = cabi.fill(cabi.CovisMap(), max_keyframes=8, kp_stride=arrays["kf_mp"].shape[1], n_mp=len(arrays["mp_bad"]),
                   n_obs=len(arrays["obs_kf"]), **arrays)
    n_set, st = np.array([1], np.int32), np.array([0], np.int32)
    ncnt, fr, off, sl = np.full(1, -5, np.int32), np.full(1, -5, np.int32), np.full(2, -5, np.int32), np.full(5, -5, np.int32)
    h = cabi.LoopConnectionsHeader()
    a = cabi.fill(cabi.LoopConnectionsArgs(), set_cap=1, d_n_set=n_set, d_set=st, d_n_counter=ncnt, d_front=fr, lc_cap=5, d_lc_off=off,
                  d_lc_slots=sl, d_header=C.addressof(h))
    assert lib().fb_covis_loop_connections(G.h, C.byref(hm), C.byref(a)) == 0
    assert (h.total, h.overflow, off.tolist(), sl.tolist(), ncnt.tolist(), fr.tolist()) == (3, 0, [0, 3], [7, 6, 5, -5, -5], [3], [5])
    G.close()


def test_loop_points_feed_search_and_fuse_unchanged():
    """The generated scene of loop_fuse_cases: its 60 loop points are held by key frame 0 (point i at feature i) and the even
    ones by key frame 1 (at feature 7 i mod 64).  With GetVectorCovisibleKeyFrames(0) = [1] the list walked is [1, 0]: the
    even points in key frame 1's feature order, then the odd ones ascending.  The device's d_loop_mp goes into
    fb_covis_search_and_fuse as it is and gives the model's result for the model's list."""
    import loop_fuse_cases as LC
    import loop_fuse_ref as LF
    from fishbirdeyevisualslam_amd import kf_problems as KP
    c, slots, scw, loop = LC.search_and_fuse_scene()
    K, S = c["K"], c["S"]
    ref = LD.ref_map(c)
    g = LD.model_graph(K, [("add", 0, 1, 20)], ref.kf_order)
    exp = LR.loop_map_points(g, ref, 0)
    even = sorted(range(0, 60, 2), key=lambda i: (i * 7) % S)
    assert exp == even + list(range(1, 60, 2)) and sorted(exp) == loop
    w = LF.World(c)
    n_fused = LF.search_and_fuse(w, c, slots, scw, exp)
    G = CovisibilityGraph(K)
    G.add_connection(0, 1, 20)
    m = DeviceMap(c, obs_spare=len(slots) * S + GUARD)
    n_loop, loop_mp, overflow = G.loop_map_points(m, 0, cap=len(exp), guard=GUARD)
    assert (n_loop.item(), overflow.item()) == (len(exp), 0)
    t, fuse = G.point_fuse_arrays(m, c["kf_bad"], c["kf_desc"], c["mp_desc"], c["mp_found"], c["mp_visible"],
                                  replaced_cap=len(exp) * len(slots), guard=GUARD)
    cells = np.zeros((1, 64 * 48 + 1), np.int32)
    target, keep = KP.kf_target([dict(kf_kps=c["kf_keys_un"][0], kf_desc=c["kf_desc"][0])], "kf_", cells, np.zeros((1, S), np.int32))
    d_n_fused, d_n_added, d_added = G.search_and_fuse(m, fuse, target, slots, scw, loop_mp[:len(exp)], c["kf_keys_un"], c["mp_xw"],
                                                      c["mp_normal"], c["mp_min_dist"], c["mp_max_dist"])
    print("nFused", d_n_fused.tolist(), n_fused)
    assert d_n_fused.tolist()[:len(slots)] == n_fused and sum(n_fused) > 0
    assert np.array_equal(m.t["kf_mp"].cpu().numpy(), w.kf_mp)
    assert np.array_equal(m.t["mp_bad"].cpu().numpy()[:len(c["mp_bad"])], w.mp_bad)
    got = {k: m.t[k].cpu().numpy() for k in ("obs_mp", "obs_kf", "obs_idx")}
    live = got["obs_kf"] >= 0
    assert sorted(zip(got["obs_mp"][live].tolist(), got["obs_kf"][live].tolist(), got["obs_idx"][live].tolist())) == w.live_edges()
    assert G.error_count() == w.errors
    G.close()


def test_chain_connected_min_score_query_detect_loop():
    """DetectLoop from :127 to :228 for seven consecutive key frames on the two handles: fb_covis_connected_dev ->
    fb_kfdb_min_score_dev -> fb_kfdb_query_dev -> fb_covis_detect_loop_dev, then KeyFrameDatabase::add.  The slot lists and the
    candidates stay on the device: the host reads two scalars per key frame, the length of the connected list and minScore,
    which fb_kfdb_query_args takes by value.  The database is the planted one of kfdb_problem (3 places x 12 key frames); the
    key frames revisit place 0 four times (the fourth detection is enough), then place 1 (two candidates, new groups), place 0
    again (counter back to 0), then see nothing known (no candidate: the groups are cleared).  Compared with tests/kfdb_ref.py
    plus the consistency model, everything at the end."""
    import kfdb_ref as KR
    from fishbirdeyevisualslam_amd import kfdb_problem as P
    from fishbirdeyevisualslam_amd.kfdb import KeyFrameDatabase
    p = P.make_kfdb_problem(5, n_places=3, per_place=12)
    n, places = p["n_kf"], [0, 0, 0, 0, 1, 0, -1]
    K = n + len(places)
    G, db = CovisibilityGraph(K), KeyFrameDatabase(K, 256)
    g, ref, cg = LD.CR.Graph(K), KR.KeyFrameDatabase(K), LR.ConsistencyGroups(3)

    def connect(a, b, w):
        G.add_connection(a, b, w)
        g.add_connection(a, b, w)
    for s in range(n):
        for j, nb in enumerate(p["covis"][s]):
            if nb >= 0:
                connect(s, int(nb), 30 - j)
        db.add(s, *p["bows"][s])
        ref.add(s, *p["bows"][s])
    rng = np.random.default_rng(1)
    seen, got, want = {}, [], []
    for t, place in enumerate(places):
        cur = n + t
        if place >= 0:
            ids, vals, _, conn = p["queries"][place]
            keep = rng.random(len(ids)) < 0.9
            ids, vals = P.l1_normalised(ids[keep], vals[keep])
        else:
            ids, vals, conn = np.arange(10, dtype=np.uint32) + np.uint32(3000000), np.full(10, 0.1), []
        for j, nb in enumerate(conn + seen.get(place, [])):
            connect(cur, nb, 20 + j)
            connect(nb, cur, 20 + j)
        # the device
        db.set_covisibility(G.kfdb_rows())
        n_conn, conn_d = G.connected(cur)
        nc = int(n_conn.item())
        ms = float(db.min_score(ids, vals, conn_d[:nc])[1].item()) if nc else 1.0
        q = db.detect_loop_candidates(1000 + t, ids, vals, ms, conn_d[:nc])
        n_enough, enough, header = G.detect_loop(q["n_candidates"], q["candidates"], 3, guard=GUARD)
        got.append((ms, q, n_enough, enough, header, G.loop_groups()))
        db.add(cur, ids, vals)
        # the model
        ms_ref = float(ref.min_score(ids, vals, g.get_vector_covisible_keyframes(cur))[1])
        w = ref.detect_loop_candidates(1000 + t, ids, vals, ms_ref, g.get_connected_keyframes(cur), g.kfdb_rows())
        want.append((ms_ref, w["candidates"], cg.detect(g, w["candidates"]), [(sorted(s), k) for s, k in cg.groups]))
        ref.add(cur, ids, vals)
        seen.setdefault(place, []).append(cur)
    torch.cuda.synchronize()
    for t, ((ms, q, n_enough, enough, header, groups), (ms_ref, cands, exp, exp_groups)) in enumerate(zip(got, want)):
        nq = int(q["n_candidates"].item())
        print("step", t, "minScore", ms, "candidates", q["candidates"].tolist()[:nq], "enough", enough.tolist()[:len(exp) + 1], "groups", groups)
        assert ms == ms_ref
        assert q["candidates"].tolist()[:nq] == cands
        assert n_enough.item() == len(exp) and enough.tolist() == exp + [-5] * (K + GUARD - len(exp))
        assert header.tolist() == [len(exp_groups), 0] + [-5] * GUARD and groups == exp_groups
    # the construction: what the sequence is there to show
    assert [len(w[1]) for w in want] == [1, 1, 1, 1, 2, 1, 0]
    assert [len(w[2]) for w in want] == [0, 0, 0, 1, 0, 0, 0] and [k for _, k in want[3][3]] == [3]
    assert [k for _, k in want[4][3]] == [0, 0] and [k for _, k in want[5][3]] == [0] and want[6][3] == []
    assert G.error_count() == 0
    G.close()
    db.close()
