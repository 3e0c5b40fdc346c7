"""fb_covis_* on the device against the literal model tests/covis_ref.py.  Everything is integer work: the comparisons are
exact equality."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import covis_ref as R
from fishbirdeyevisualslam_amd import cabi, covis_problem as P
from test_covis import MAP_FIELDS, _host_map, ref_map

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(p):
    from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceMap
    return CovisibilityGraph(p["K"]), DeviceMap(p)


def _same_graph(G, g, slots, what=""):
    """every getter of the listed slots (enqueued first, read back once) against the model"""
    import torch
    got = [(a, G.ordered(a), G.connected(a), G.by_weight(a, 15), G.by_weight(a, 1), G.by_weight(a, 16)) for a in slots]
    rows = G.kfdb_rows()
    torch.cuda.synchronize()
    for a, (n, s, w), (nc, sc), bw15, bw1, bw16 in got:
        n = int(n.cpu()[0])
        assert s.cpu().numpy()[:n].tolist() == g.ordered[a], (what, a)
        assert w.cpu().numpy()[:n].tolist() == g.ordered_w[a], (what, a)
        nc = int(nc.cpu()[0])
        assert sc.cpu().numpy()[:nc].tolist() == g.get_connected_keyframes(a), (what, a)
        for (nb, sb), wv in ((bw15, 15), (bw1, 1), (bw16, 16)):
            assert sb.cpu().numpy()[:int(nb.cpu()[0])].tolist() == g.get_covisibles_by_weight(a, wv), (what, a, wv)
    assert np.array_equal(rows.cpu().numpy(), g.kfdb_rows()), what


def _weights_equal(G, g, pairs):
    import torch
    got = [G.weight(a, b) for a, b in pairs]
    torch.cuda.synchronize()
    assert [int(t.cpu()[0]) for t in got] == [g.get_weight(a, b) for a, b in pairs]


@pytest.fixture(scope="module")
def planted():
    p = P.make_covis_problem(1)
    return p, ref_map(p)


def test_batch_update_then_edits_then_every_getter(planted):
    import torch
    p, m = planted
    G, M = _dev(p)
    g = R.Graph(p["K"], p["kf_order"])
    nc, fr = G.update_connections(M, p["batch"])
    want = [g.update_connections(m, a) for a in p["batch"]]
    torch.cuda.synchronize()
    assert nc.cpu().numpy().tolist() == [w[0] for w in want] and fr.cpu().numpy().tolist() == [w[1] for w in want]
    _same_graph(G, g, p["used"][:24], "batch")
    # the rest of the map, one call; an unused slot and a repeated slot are in the list
    rest = [s for s in range(p["K"]) if s not in p["batch"]] + [p["batch"][0]]
    nc, fr = G.update_connections(M, rest)
    want = [g.update_connections(m, a) for a in rest]
    torch.cuda.synchronize()
    assert nc.cpu().numpy().tolist() == [w[0] for w in want] and fr.cpu().numpy().tolist() == [w[1] for w in want]
    _same_graph(G, g, range(p["K"]), "all")
    rng = np.random.default_rng(5)
    used = p["used"]
    for step in range(60):
        r = rng.random()
        a, b = (int(x) for x in rng.choice(used, 2, replace=False))
        if r < 0.45:
            w = int(rng.choice([1, 14, 15, 16, g.get_weight(a, b) or 3, 300]))
            G.add_connection(a, b, w); g.add_connection(a, b, w)
        elif r < 0.85:
            if rng.random() < 0.7 and g.weights[a]:
                b = int(rng.choice(sorted(g.weights[a])))
            G.erase_connection(a, b); g.erase_connection(a, b)
        else:
            G.erase_keyframe(a); g.erase_keyframe(a)
    _same_graph(G, g, range(p["K"]), "edits")
    _weights_equal(G, g, [(int(a), int(b)) for a, b in rng.choice(used, (40, 2))])
    assert G.error_count() == 0
    G.clear(); g.clear()
    _same_graph(G, g, used[:6], "clear")
    G.close()


def test_hub_row_longer_than_a_workgroup():
    import torch
    p = P.make_hub_problem()
    m = ref_map(p)
    G, M = _dev(p)
    g = R.Graph(p["K"], p["kf_order"])
    nc, fr = G.update_connections(M, [0, 7])
    want = [g.update_connections(m, 0), g.update_connections(m, 7)]
    n1 = G.ordered(0)
    G.add_connection(0, 1299, 1); g.add_connection(0, 1299, 1)
    n, s, w = G.ordered(0)
    ncn, scn = G.connected(0)
    torch.cuda.synchronize()
    assert nc.cpu().numpy().tolist() == [1250, 1] and [tuple(x) for x in want] == list(zip(nc.cpu().tolist(), fr.cpu().tolist()))
    assert int(n1[0].cpu()[0]) == 1 == len(want) - 1
    n = int(n.cpu()[0])
    assert n == 1251 and s.cpu().numpy()[:n].tolist() == g.ordered[0] and set(w.cpu().numpy()[:n].tolist()) == {1}
    order = [int(p["kf_order"][x]) for x in g.ordered[0]]
    assert order == sorted(order, reverse=True)                         # all of weight 1: purely by kf_order, descending
    assert scn.cpu().numpy()[:int(ncn.cpu()[0])].tolist() == g.get_connected_keyframes(0)
    assert G.error_count() == 0
    G.close()


def test_full_slot_range_with_sparse_content():
    import torch
    p = P.make_sparse_problem()
    m = ref_map(p)
    G, M = _dev(p)
    g = R.Graph(p["K"], p["kf_order"])
    q = p["used"] + [4000]
    nc, fr = G.update_connections(M, q)
    want = [g.update_connections(m, a) for a in q]
    torch.cuda.synchronize()
    assert list(zip(nc.cpu().tolist(), fr.cpu().tolist())) == [tuple(x) for x in want]
    _same_graph(G, g, p["used"], "sparse")
    G.erase_keyframe(4095); g.erase_keyframe(4095)
    G.add_connection(4095, 0, 2); g.add_connection(4095, 0, 2)
    _same_graph(G, g, p["used"], "sparse edits")
    assert G.error_count() == 0
    G.close()


def _culling_equal(out, want):
    n = int(out["n"].cpu()[0])
    assert out["slots"].cpu().numpy()[:n].tolist() == want["slots"]
    for k in ("n_redundant", "n_mps", "culled"):
        assert out[k].cpu().numpy()[:n].tolist() == want[k], k
    assert np.array_equal(out["mp_bad_after"].cpu().numpy()[:len(want["mp_bad_after"])], want["mp_bad_after"])


def test_culling_chain_of_dependent_removals_leaves_map_and_graph_untouched(planted):
    import torch
    p, m = planted
    G, M = _dev(p)
    g = R.Graph(p["K"], p["kf_order"])
    G.update_connections(M, p["used"])
    for a in p["used"]:
        g.update_connections(m, a)
    torch.cuda.synchronize()
    map_before, W_before = M.bytes(), G.kfdb_rows().cpu().numpy().copy()
    state = lambda: [t.cpu().numpy().copy() for a in p["used"] for t in G.ordered(a) + G.connected(a)]
    before = state()
    cur = p["cur"]
    want = R.keyframe_culling(g, m, cur)
    at = [want["slots"].index(x) for x in p["X"]]
    assert [want["culled"][i] for i in at] == [1, 1, 1, 0]             # three dependent removals, then one that no longer happens
    ne = np.zeros(p["K"], np.uint8)
    ne[p["X"][1]] = 1
    runs = [(G.keyframe_culling(M, cur), want),
            (G.keyframe_culling(M, cur, id0_slot=p["X"][0]), R.keyframe_culling(g, m, cur, id0=p["X"][0])),
            (G.keyframe_culling(M, cur, not_erase=ne), R.keyframe_culling(g, m, cur, not_erase=ne)),
            (G.keyframe_culling(M, 30), R.keyframe_culling(g, m, 30)),
            (G.keyframe_culling(M, 23), R.keyframe_culling(g, m, 23))]   # an unused slot: an empty list
    torch.cuda.synchronize()
    for out, w in runs:
        _culling_equal(out, w)
    assert M.bytes() == map_before and np.array_equal(G.kfdb_rows().cpu().numpy(), W_before)
    after = state()
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))
    assert G.error_count() == 0
    G.close()


def test_out_of_range_edge_is_skipped_and_counted(planted):
    import torch
    p, m = planted
    q = dict(p)
    for k in ("obs_mp", "obs_kf", "obs_idx"):
        q[k] = np.concatenate([p[k], p[k][:1]])
    q["obs_kf"][-1] = p["K"] + 1000000                                  # never used as an index
    q["obs_mp"][-1] = int(np.nonzero(p["kf_n"] > 0)[0][0])
    mq = ref_map(q)                                                     # the model skips it: the results of the map without it
    for culling in (False, True):
        G, M = _dev(q)
        g = R.Graph(p["K"], p["kf_order"])
        nc, fr = G.update_connections(M, p["batch"])
        want = [g.update_connections(m, a) for a in p["batch"]]
        if culling:
            G.clear(); g.clear()
            G.add_connection(p["cur"], p["X"][0], 20); g.add_connection(p["cur"], p["X"][0], 20)
            out = G.keyframe_culling(M, p["cur"])
            torch.cuda.synchronize()
            _culling_equal(out, R.keyframe_culling(g, mq, p["cur"]))
        else:
            torch.cuda.synchronize()
            assert list(zip(nc.cpu().tolist(), fr.cpu().tolist())) == [tuple(x) for x in want]
            _same_graph(G, g, p["batch"], "planted edge")
        assert G.error_count() == 1
        G.close()


def test_host_pointer_variants_equal_the_dev_variants(planted):
    import torch
    import fishbirdeyevisualslam_amd as fb
    p, m = planted
    L = fb.lib()
    G, M = _dev(p)
    G.update_connections(M, p["used"])
    hm, keep = _host_map(p)
    h = C.c_void_p()
    fb.check(L.fb_covis_create(p["K"], C.byref(h)), "create")
    K = p["K"]
    vp = lambda x: C.c_void_p(x.ctypes.data)
    slots = np.array(p["used"], np.int32)
    ncnt, front = np.zeros(len(slots), np.int32), np.zeros(len(slots), np.int32)
    fb.check(L.fb_covis_update_connections(h, C.byref(hm), len(slots), vp(slots), vp(ncnt), vp(front)), "update")
    for a in (0, 2, 5, p["cur"], 30, 23):
        n, s, w = np.zeros(1, np.int32), np.full(K, -7, np.int32), np.full(K, -7, np.int32)
        fb.check(L.fb_covis_ordered(h, a, vp(n), vp(s), vp(w)), "ordered")
        dn, ds, dw = G.ordered(a)
        k = int(dn.cpu()[0])
        assert n[0] == k and np.array_equal(s[:k], ds.cpu().numpy()[:k]) and np.array_equal(w[:k], dw.cpu().numpy()[:k])
        assert (s[k:] == -7).all() and (w[k:] == -7).all()
        fb.check(L.fb_covis_by_weight(h, a, 16, vp(n), vp(s)), "by_weight")
        dn, ds = G.by_weight(a, 16)
        k = int(dn.cpu()[0])
        assert n[0] == k and np.array_equal(s[:k], ds.cpu().numpy()[:k])
        fb.check(L.fb_covis_connected(h, a, vp(n), vp(s)), "connected")
        dn, ds = G.connected(a)
        k = int(dn.cpu()[0])
        assert n[0] == k and np.array_equal(s[:k], ds.cpu().numpy()[:k])
        fb.check(L.fb_covis_weight(h, 0, a, vp(n)), "weight")
        assert n[0] == int(G.weight(0, a).cpu()[0])
    rows = np.full((K, 10), -9, np.int32)
    some = np.array([0, 8, 30], np.int32)
    fb.check(L.fb_covis_kfdb_rows(h, 3, vp(some), vp(rows)), "rows")
    drows = G.kfdb_rows().cpu().numpy()
    assert np.array_equal(rows[some], drows[some]) and (np.delete(rows, some, 0) == -9).all()
    fb.check(L.fb_covis_kfdb_rows(h, 0, None, vp(rows)), "rows")
    assert np.array_equal(rows, drows)
    o = dict(n=np.zeros(1, np.int32), slots=np.full(K, -7, np.int32), n_redundant=np.zeros(K, np.int32), n_mps=np.zeros(K, np.int32),
             culled=np.zeros(K, np.uint8), bad=np.zeros(len(p["mp_bad"]), np.uint8))
    fb.check(L.fb_covis_keyframe_culling(h, C.byref(hm), p["cur"], -1, None, vp(o["n"]), vp(o["slots"]), vp(o["n_redundant"]),
                                         vp(o["n_mps"]), vp(o["culled"]), vp(o["bad"])), "culling")
    d = G.keyframe_culling(M, p["cur"])
    torch.cuda.synchronize()
    k = int(d["n"].cpu()[0])
    assert o["n"][0] == k and k >= 8
    for a, b in (("slots", "slots"), ("n_redundant", "n_redundant"), ("n_mps", "n_mps"), ("culled", "culled")):
        assert np.array_equal(o[a][:k], d[b].cpu().numpy()[:k]), a
    assert np.array_equal(o["bad"], d["mp_bad_after"].cpu().numpy()[:len(o["bad"])])
    L.fb_covis_destroy(h)
    G.close()


def test_rows_and_connected_feed_the_loop_query_without_a_host_copy():
    import torch
    import kfdb_ref as KR
    from fishbirdeyevisualslam_amd import kfdb_problem as KP
    from fishbirdeyevisualslam_amd.covis import CovisibilityGraph
    from fishbirdeyevisualslam_amd.kfdb import KeyFrameDatabase
    kp = KP.make_kfdb_problem(3)
    K = kp["n_kf"]
    G, g = CovisibilityGraph(K), R.Graph(K)
    rng = np.random.default_rng(11)
    # key frames of one place see each other: weights from the planted rows, plus the query's own connections
    for a in range(K):
        for c, b in enumerate(kp["covis"][a]):
            if b >= 0 and b != a:
                w = int(40 - 3 * c + rng.integers(0, 3))
                G.add_connection(a, int(b), w); g.add_connection(a, int(b), w)
    db, ref = KeyFrameDatabase(K, 256), KR.KeyFrameDatabase(K)
    for s, (ids, vals) in enumerate(kp["bows"]):
        db.add(s, ids, vals)
        ref.add(s, ids, vals)
    rows = G.kfdb_rows()
    db.covis = rows                                                     # the device tensor itself
    model_rows = g.kfdb_rows()
    hits = 0
    for q, (ids, vals, place, conn) in enumerate(kp["queries"]):
        src = int(np.nonzero(kp["place"] != place)[0][0])                # pKF's connected key frames: of another place here
        n_conn, d_conn = G.connected(src)
        n, bi, bv = db._bow(None, ids, vals)
        out = dict(n_candidates=torch.zeros(1, dtype=torch.int32, device="cuda"), candidates=torch.full((K,), -1, dtype=torch.int32, device="cuda"))
        a = cabi.KfdbQueryArgs()
        want_conn = g.get_connected_keyframes(src)
        cabi.fill(a, mode=cabi.FB_KFDB_LOOP, query_id=900 + q, n_words=n, bow_ids=bi, bow_vals=bv, min_score=0.02,
                  n_connected=len(want_conn), connected=d_conn, covis=rows, **out)
        import fishbirdeyevisualslam_amd as fb
        fb.check(fb.lib().fb_kfdb_query_dev(db.h, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "query")
        want = ref.detect_loop_candidates(900 + q, ids, vals, 0.02, want_conn, model_rows)
        torch.cuda.synchronize()
        k = int(out["n_candidates"].cpu()[0])
        assert int(n_conn.cpu()[0]) == len(want_conn)
        assert out["candidates"].cpu().numpy()[:k].tolist() == want["candidates"], q
        hits += len(want["candidates"])
    assert hits >= 2 and (model_rows >= 0).sum() > K
    db.close()
    G.close()


def test_host_header_graph_builds_and_runs():
    """tests/cpp/covis_host_test.cpp drives fishbird::CovisibilityGraph (host/fishbird_host.hpp) in a fresh child process."""
    import fishbirdeyevisualslam_amd as fb
    pkg = os.path.dirname(fb.LIB_PATH)
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "covis_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"),
                           os.path.join(ROOT, "tests", "cpp", "covis_host_test.cpp"), "-o", exe, "-L", pkg, "-lfishbird_hip",
                           "-Wl,-rpath," + pkg])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"covis_host_test ok" in r.stdout
