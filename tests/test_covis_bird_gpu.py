"""fb_covis_update_bird_connections, fb_covis_bird_connected and fb_covis_local_bird_map on the device against the literal
model tests/bird_map_ref.py, device and host-pointer variants.  Every comparison is exact equality.  The generators' branch
coverage is asserted without a GPU in tests/test_covis_bird.py."""
import ctypes as C

import numpy as np
import pytest

import bird_map_cases as CS
import bird_map_ref as R
from fishbirdeyevisualslam_amd import cabi
from test_covis_bird import UPDATE_CASES

pytestmark = pytest.mark.gpu


def _handle(p):
    from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceBirdTables
    return CovisibilityGraph(p["K"]), DeviceBirdTables(p)


def _lists(G, slots):
    """the bird list and weights of the listed slots, enqueued first and read back once"""
    import torch
    got = [G.bird_connected(a) for a in slots]
    torch.cuda.synchronize()
    out = {}
    for a, (n, s, w) in zip(slots, got):
        n = int(n.cpu()[0])
        out[a] = (s.cpu().numpy()[:n].tolist(), w.cpu().numpy()[:n].tolist())
    return out


def _check_batch(G, T, p, model_p, state, n_counter, what):
    import torch
    g = CS.graph_of(model_p)
    G.clear()
    G.tree_set(p["parent"], p["linked"], p["first"])
    nc = None if n_counter is None else G._dev(n_counter)
    nbc, bf = G.update_bird_connections(T.map, T, p["used"], nc, state, p["id0"], p["frame_id"], p["in_map"])
    want = g.run_batch(CS.tables_of(model_p), p["used"], n_counter, state, p["id0"], p["frame_id"], p["in_map"])
    par, lnk, fst = G.tree_get()
    torch.cuda.synchronize()
    assert nbc.cpu().numpy().tolist() == want[0], what
    assert bf.cpu().numpy().tolist() == want[1], what
    got = _lists(G, p["used"])
    for a in p["used"]:
        assert got[a] == (g.bird_connected[a], g.bird_weights[a]), (what, a)
    assert par.cpu().numpy().tolist() == g.parent, what
    assert fst.cpu().numpy().tolist() == [int(x) for x in g.first], what
    assert lnk.cpu().numpy().tolist() == g.linked(), what
    return g


@pytest.fixture(scope="module")
def problems():
    return {k: CS.make_bird_problem(**v) for k, v in UPDATE_CASES.items()}


@pytest.mark.parametrize("state", [1, 3, 4])
def test_a_small_map_every_state(problems, state):
    p = problems["a"]
    G, T = _handle(p)
    g = _check_batch(G, T, p, p, state, CS.front_counter(p, p["used"]), ("a", state))
    assert G.error_count() == g.errors
    g = _check_batch(G, T, p, p, state, None, ("a all act", state))
    assert G.error_count() == g.errors      # clear() reset the counter
    # a second batch on the lists and the tree the first left: the order of the members does not depend on what was there
    g2 = R.BirdGraph(p["K"], p["kf_order"], g.parent, g.linked(), g.first)
    g2.bird_connected, g2.bird_weights = g.bird_connected, g.bird_weights
    half = p["used"][::2]
    nbc, bf = G.update_bird_connections(T.map, T, half, None, state, p["id0"], p["frame_id"], p["in_map"])
    want = g2.run_batch(CS.tables_of(p), half, None, state, p["id0"], p["frame_id"], p["in_map"])
    assert (nbc.cpu().numpy().tolist(), bf.cpu().numpy().tolist()) == want
    assert G.tree_get()[0].cpu().numpy().tolist() == g2.parent
    G.close()


def test_a_erase_keyframe_leaves_bird_lists_and_front_getters_keep_front_weights(problems):
    p = problems["a"]
    G, T = _handle(p)
    g = _check_batch(G, T, p, p, 1, None, "a")
    a = p["used"][0]
    G.add_connection(a, p["used"][2], 17)
    G.erase_keyframe(p["used"][1])          # SetBadFlag never edits a bird list, its own included
    assert _lists(G, [a, p["used"][1]]) == {s: (g.bird_connected[s], g.bird_weights[s]) for s in (a, p["used"][1])}
    n, s, w = G.ordered(a)
    assert int(n.cpu()[0]) == 1 and w.cpu().numpy()[:1].tolist() == [17]    # mvOrderedWeights of the front, not the bird weights
    G.clear()
    assert _lists(G, p["used"]) == {s: ([], []) for s in p["used"]}
    G.close()


def test_b_last_bin_and_12_bit_ranks(problems):
    p = problems["b"]
    G, T = _handle(p)
    g = _check_batch(G, T, p, p, 3, CS.front_counter(p, p["used"]), "b")
    assert G.error_count() == g.errors
    G.close()


def test_c_rows_longer_than_256_members(problems):
    p = problems["c"]
    G, T = _handle(p)
    g = _check_batch(G, T, p, p, 4, None, "c")
    assert max(len(l) for l in g.bird_connected) > 256
    assert G.error_count() == g.errors
    G.close()


def test_d_out_of_range_entries_are_skipped_and_counted(problems):
    dirty, clean, n = CS.inject_out_of_range(problems["a"])
    G, T = _handle(dirty)
    g = _check_batch(G, T, dirty, clean, 3, None, "d")
    assert G.error_count() == n + g.errors
    nbc, bf = G.update_bird_connections(T.map, T, [dirty["K"], -1], None, 1)        # query slots outside the handle
    assert nbc.cpu().numpy().tolist() == [0, 0] and bf.cpu().numpy().tolist() == [-1, -1]
    assert G.error_count() == n + g.errors + 2 + 6    # (the six edges are counted again by the index of the second call)
    G.close()


def _host_struct(p, with_Tcw=False):
    keep = {k: np.ascontiguousarray(p[k], dt) for k, dt in (("kf_nb", np.int32), ("kf_mpb", np.int32), ("mpb_bad", np.uint8),
                                                            ("bobs_mpb", np.int32), ("bobs_kf", np.int32), ("bobs_idx", np.int32))}
    keep["kf_order"] = np.ascontiguousarray(p["kf_order"], np.uint64)
    if with_Tcw:
        keep["kf_Tcw"] = np.ascontiguousarray(p["kf_Tcw"], np.float32)
    t = cabi.CovisKfTables()
    cabi.fill(t, bird_stride=p["bird_stride"], n_mpb=len(keep["mpb_bad"]), n_bobs=len(keep["bobs_kf"]),
              **{k: v for k, v in keep.items() if k != "kf_order" and v.size})
    m = cabi.CovisMap()
    cabi.fill(m, max_keyframes=p["K"], kp_stride=1, kf_order=keep["kf_order"])
    return m, t, keep


def test_a_host_pointer_variant(problems):
    from fishbirdeyevisualslam_amd import check, lib
    p = problems["a"]
    G, _ = _handle(p)
    G.tree_set(p["parent"], p["linked"], p["first"])
    m, t, keep = _host_struct(p)
    n = len(p["used"])
    slots, ncnt = np.asarray(p["used"], np.int32), CS.front_counter(p, p["used"])
    fid, inm = np.ascontiguousarray(p["frame_id"], np.int32), np.ascontiguousarray(p["in_map"], np.uint8)
    nbc, bf = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    check(lib().fb_covis_update_bird_connections(G.h, C.byref(m), C.byref(t), n, vp(slots), vp(ncnt), 3, p["id0"], vp(fid), vp(inm),
                                                 vp(nbc), vp(bf)), "fb_covis_update_bird_connections")
    g = CS.graph_of(p)
    want = g.run_batch(CS.tables_of(p), p["used"], ncnt, 3, p["id0"], p["frame_id"], p["in_map"])
    assert (nbc.tolist(), bf.tolist()) == want
    K = p["K"]
    for a in p["used"]:
        cnt, s, w = np.zeros(1, np.int32), np.full(K, -9, np.int32), np.full(K, -9, np.int32)
        check(lib().fb_covis_bird_connected(G.h, a, vp(cnt), vp(s), vp(w)), "fb_covis_bird_connected")
        k = int(cnt[0])
        assert (s[:k].tolist(), w[:k].tolist()) == (g.bird_connected[a], g.bird_weights[a])
        assert (s[k:] == -9).all() and (w[k:] == -9).all()
    par, lnk, fst = np.zeros(K, np.int32), np.zeros(K, np.uint8), np.zeros(K, np.uint8)
    check(lib().fb_covis_tree_get(G.h, vp(par), vp(lnk), vp(fst)), "fb_covis_tree_get")
    assert par.tolist() == g.parent and lnk.tolist() == g.linked() and fst.tolist() == [int(x) for x in g.first]
    G.close()


# ---- (e) the local bird map ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def local():
    return CS.make_local_problem(21)


def _run_local(p, order, kf_ow, cap_mpb=None, with_Tcw=False, reserve=False):
    """the whole AddKeyFrame sequence on one stream, the results copied aside after every call, one synchronisation"""
    import torch
    from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceBirdTables
    arrays = dict(p)
    if not with_Tcw:
        arrays.pop("kf_Tcw")
    G, T = CovisibilityGraph(p["K"]), DeviceBirdTables(arrays)
    if reserve:
        G.reserve_local_bird_map(p["n_mpb"], 0)
    cap_kf, cap = p["K"], p["n_mpb"] if cap_mpb is None else cap_mpb
    t, a = G.local_bird_map_arrays(cap_kf, cap, kf_ow=kf_ow, mpb_order=order, guard=4)
    snaps = []
    for s in p["slots"]:
        G.local_bird_map(T.map, T, a, s)
        snaps.append({k: t[k].clone() for k in ("d_local_kf_bird", "d_n_local_kf_bird", "d_local_mpb", "d_n_local_mpb", "d_overflow")})
    torch.cuda.synchronize()
    err = G.error_count()
    G.close()
    return [{k: v.cpu().numpy() for k, v in s.items()} for s in snaps], err, cap_kf, cap


@pytest.mark.parametrize("variant", ["order", "index_order", "derived_centres"])
def test_e_sequence_of_add_keyframe(local, variant):
    p = local
    order = p["mpb_order"] if variant == "order" else None
    kf_ow = None if variant == "derived_centres" else p["kf_ow"]
    snaps, err, cap_kf, cap = _run_local(p, order, kf_ow, with_Tcw=variant == "derived_centres", reserve=variant == "order")
    _, want = CS.run_local_model(p, order)      # kf_ow of the generator IS the derived centres
    assert err == 0
    for j, (s, (kfs, pts)) in enumerate(zip(snaps, want)):
        assert int(s["d_n_local_kf_bird"][0]) == len(kfs) and s["d_local_kf_bird"][:len(kfs)].tolist() == kfs, (variant, j)
        assert int(s["d_n_local_mpb"][0]) == len(pts) and s["d_local_mpb"][:len(pts)].tolist() == pts, (variant, j)
        assert int(s["d_overflow"][0]) == 0
        assert (s["d_local_kf_bird"][cap_kf:] == -5).all() and (s["d_local_mpb"][cap:] == -5).all()


def test_e_capacity_too_small_gives_prefix_and_flag(local):
    p = local
    _, want = CS.run_local_model(p, p["mpb_order"])
    cap = sorted(len(pts) for _, pts in want)[len(want) // 2]     # about half of the calls overflow
    snaps, err, cap_kf, _ = _run_local(p, p["mpb_order"], p["kf_ow"], cap_mpb=cap)
    over = 0
    for s, (kfs, pts) in zip(snaps, want):
        n = min(len(pts), cap)
        assert int(s["d_n_local_mpb"][0]) == n and s["d_local_mpb"][:n].tolist() == pts[:n]
        assert int(s["d_overflow"][0]) == (1 if len(pts) > cap else 0)
        assert (s["d_local_mpb"][cap:] == -5).all()
        assert s["d_local_kf_bird"][:len(kfs)].tolist() == kfs
        over += len(pts) > cap
    assert 0 < over < len(want)


def test_e_distance_boundary_on_the_device():
    """3-4-0 is exactly 5 and stays; one float step further leaves"""
    far = float(np.nextafter(np.float32(4.0), np.float32(5.0)))
    for y, kept in ((4.0, [1, 0]), (far, [1])):
        K, BS = 2, 16
        kf_mpb = np.full((K, BS), -1, np.int32)
        kf_mpb[0, :12], kf_mpb[1, :12] = np.arange(12), np.arange(100, 112)
        p = dict(K=K, bird_stride=BS, slots=[0, 1], kf_nb=np.array([12, 12], np.int32), kf_mpb=kf_mpb, mpb_bad=np.zeros(112, np.uint8),
                 bobs_mpb=np.zeros(0, np.int32), bobs_kf=np.zeros(0, np.int32), bobs_idx=np.zeros(0, np.int32),
                 kf_order=np.arange(K, dtype=np.uint64), kf_ow=np.array([[3.0, y, 0.0], [0.0, 0.0, 0.0]], np.float32), n_mpb=112,
                 kf_Tcw=np.zeros((K, 12), np.float32))
        snaps, err, _, _ = _run_local(p, None, p["kf_ow"])
        _, want = CS.run_local_model(p, None)
        assert want[-1][0] == kept
        s = snaps[-1]
        assert s["d_local_kf_bird"][:int(s["d_n_local_kf_bird"][0])].tolist() == kept
        assert s["d_local_mpb"][:int(s["d_n_local_mpb"][0])].tolist() == want[-1][1]


def test_e_host_pointer_variant(local):
    from fishbirdeyevisualslam_amd import check, lib
    from fishbirdeyevisualslam_amd.covis import CovisibilityGraph
    p = local
    G = CovisibilityGraph(p["K"])
    m, t, keep = _host_struct(p, with_Tcw=True)
    _, want = CS.run_local_model(p, p["mpb_order"])
    K, cap = p["K"], p["n_mpb"]
    lkf, nkf = np.full(K, -5, np.int32), np.zeros(1, np.int32)
    lmp, nmp, ovf = np.full(cap, -5, np.int32), np.full(1, -5, np.int32), np.full(1, -5, np.int32)
    order = np.ascontiguousarray(p["mpb_order"], np.uint64)
    a = cabi.LocalBirdMapArgs()
    cabi.fill(a, new_slot=0, d_mpb_order=order, cap_kf=K, d_local_kf_bird=lkf, d_n_local_kf_bird=nkf, cap_mpb=cap, d_local_mpb=lmp,
              d_n_local_mpb=nmp, d_overflow=ovf)           # d_kf_ow NULL: the centres come from kf_Tcw
    for s, (kfs, pts) in list(zip(p["slots"], want))[:8]:
        a.new_slot = s
        check(lib().fb_covis_local_bird_map(G.h, C.byref(m), C.byref(t), C.byref(a)), "fb_covis_local_bird_map")
        assert lkf[:int(nkf[0])].tolist() == kfs and lmp[:int(nmp[0])].tolist() == pts and int(ovf[0]) == 0
    G.close()


# ---- (f) the chain: ProcessNewKeyFrame -> UpdateConnections (front, tree, bird) -> AddKeyFrame -> the next frame's M9 ---------
def _chain_bird_tables(K, n_mpb, new_slot, kf_order, seed=77, BS=128):
    """Bird tables over the bird-point table of a track chain (indices 0 .. n_mpb-1) for the K key frames of the front case:
    40 .. 100 random points per key frame; the new key frame at the origin, slots in ascending distance, two of them far."""
    rng = np.random.default_rng(seed)
    kf_nb, kf_mpb, edges = np.zeros(K, np.int32), np.full((K, BS), -1, np.int32), []
    for kf in range(K):
        pts = rng.choice(n_mpb, int(rng.integers(40, 101)), replace=False)
        kf_mpb[kf, :len(pts)], kf_nb[kf] = pts, len(pts)
        edges += [[int(p), kf, i] for i, p in enumerate(pts)]
    kf_mpb[new_slot, kf_nb[new_slot]] = kf_mpb[new_slot, 0]             # one point at two features
    kf_nb[new_slot] += 1
    e = np.asarray(edges, np.int32)[rng.permutation(len(edges))]
    e[rng.choice(len(e), len(e) // 20, replace=False), 1] = -1         # tombstones
    others = [s for s in range(K) if s != new_slot]
    kf_ow = np.zeros((K, 3), np.float32)
    for j, s in enumerate(others):
        d = 0.4 * (j + 1) if j < len(others) - 2 else 6.0 + 2.0 * j
        kf_ow[s] = [d * np.cos(j), d * np.sin(j), 0.01 * j]
    return dict(K=K, bird_stride=BS, kf_nb=kf_nb, kf_mpb=kf_mpb, mpb_bad=(rng.random(n_mpb) < 0.1).astype(np.uint8), bobs_mpb=e[:, 0].copy(),
                bobs_kf=e[:, 1].copy(), bobs_idx=e[:, 2].copy(), kf_order=np.asarray(kf_order, np.uint64), kf_ow=kf_ow, n_mpb=n_mpb,
                mpb_order=(rng.permutation(n_mpb).astype(np.uint64) * np.uint64(16) + np.uint64(0x560000000000)),
                local_in=others[::-1])


def test_f_chain_into_the_next_frames_bird_mappoint_match():
    import torch
    import map_refresh_cases as MC
    from fishbirdeyevisualslam_amd import check, lib, sequence as S, track as TR
    from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceBirdTables, DeviceMap
    # the tracking side: frame 0 initialises the bird-point table, frame 1 is "the next frame"
    wh, bwh = (640, 480), (384, 384)
    seq = S.Sequence(1, 2, seed=9100, front_wh=wh, bird_wh=bwh, fx=250.0, fy=250.0, device="cuda:0")
    tc = TR.TrackChain(1, wh, bwh, K=seq.Kc, D=seq.D, use_lists=False)
    mask_d = torch.from_numpy(seq.mask.copy()).cuda()
    f0, b0, c0 = seq.render(0)
    tc.extract(f0, b0, c0, mask_d)
    M, MB, mp0, mpb0, Tcw0 = seq.build_map(tc.view("cur"), tc.tables, map_cap=tc.map_cap, bird_cap=tc.bird_cap)
    tc.set_map(M, MB)
    tc.init_first(mp0, mpb0, Tcw0)
    tc.set_delta(seq.delta(1))
    f1, b1, c1 = seq.render(1)
    n_mpb = int(MB["n"][0])
    assert n_mpb > 200
    # the mapping side: the front map of the ProcessNewKeyFrame case, with bird tables over the chain's bird points
    c, slot, nf = MC.new_keyframe_case(70, 96, 12)
    K = c["K"]
    p = _chain_bird_tables(K, n_mpb, slot, c["kf_order"])
    G, m = CovisibilityGraph(K), DeviceMap(c, obs_spare=nf + 3)
    rt, ra = G.refresh_arrays(m, *(c[k] for k in ("kf_Tcw", "kf_bad", "kf_desc", "scale_factors", "mp_xw", "mp_ref_kf", "mp_normal",
                                                  "mp_min_dist", "mp_max_dist", "mp_desc")))
    recent, n_recent = G.recent_list(20 + nf, c["recent"])
    T = DeviceBirdTables(p)
    # sized ahead, so that nothing below reallocates: a front index, then room behind it for the bird calls
    G.update_connections(m, [0])
    G.reserve_local_bird_map(4 * n_mpb + 4096, 4 * T.n_bobs + 4096)
    lt, la = G.local_bird_map_arrays(K, tc.bird_cap, kf_ow=p["kf_ow"], mpb_order=p["mpb_order"])
    lt["d_local_kf_bird"][:len(p["local_in"])] = G._dev(p["local_in"])
    lt["d_n_local_kf_bird"][0] = len(p["local_in"])
    slots = G._dev([slot])
    m09 = cabi.MatcherParams(0.9, 1)

    def next_frame_m9(d_local, d_n_local):
        L, s = tc.L, tc._stream()
        tc.extract(f1, b1, c1, mask_d)
        check(L.fb_frame_predict_pose_dev(tc.cur, tc.last, C.c_void_p(tc.delta.data_ptr()), s), "predict")
        check(L.fb_frame_bird_mappoint_match_dev(tc.cur, C.byref(tc.targs.mpb), C.c_void_p(d_local.data_ptr()), C.c_void_p(d_n_local.data_ptr()),
                                                 10, C.c_float(0.05), C.byref(m09), s), "M9")
    torch.cuda.synchronize()
    # ---- the chain: one stream, nothing read back in between ----
    G.process_new_keyframe(m, ra, slot, nf, recent, n_recent)
    nc, fr = G.update_connections(m, slots)
    G.first_connection(slots, nc, fr, id0_slot=0)
    nbc, bf = G.update_bird_connections(m, T, slots, nc, 1, 0)
    G.local_bird_map(m, T, la, slot)
    next_frame_m9(lt["d_local_mpb"], lt["d_n_local_mpb"])           # fb_track_args.d_local_mpb / d_n_local_mpb, unchanged
    reuse = local_map_bytes(G, m, c, True)                           # the front index is still the one a reuse_index reads
    torch.cuda.synchronize()
    got = tc.view("cur")
    got_counts = tc.counts("cur")[0]
    # ---- the model ----
    nc0, fr0 = int(nc.cpu()[0]), int(fr.cpu()[0])
    assert nc0 > 0 and fr0 >= 0
    g = R.BirdGraph(K, p["kf_order"])
    g.parent[slot], g.first[slot] = fr0, False                      # the first connection (:665-690)
    g.children[fr0].add(slot)
    want = g.run_batch(CS.tables_of(p), [slot], [nc0], 1, 0)
    assert (nbc.cpu().numpy().tolist(), bf.cpu().numpy().tolist()) == want and want[0][0] > 0
    assert _lists(G, [slot])[slot] == (g.bird_connected[slot], g.bird_weights[slot]) and g.bird_connected[slot]
    par, lnk, fst = (x.cpu().numpy() for x in G.tree_get())
    assert (int(par[slot]), int(lnk[slot]), int(fst[slot])) == (g.parent[slot], g.linked()[slot], int(g.first[slot]))
    lm = R.LocalBirdMap(p["mpb_order"])
    lm.local_kf = list(p["local_in"])
    lm.add_keyframe(CS.tables_of(p), p["kf_ow"], slot)
    assert lm.counters["far_member"] == 2 and len(lm.local_mpb) > 100
    n_kf, n_pts = int(lt["d_n_local_kf_bird"].cpu()[0]), int(lt["d_n_local_mpb"].cpu()[0])
    assert lt["d_local_kf_bird"].cpu().numpy()[:n_kf].tolist() == lm.local_kf
    assert lt["d_local_mpb"].cpu().numpy()[:n_pts].tolist() == lm.local_mpb and int(lt["d_overflow"].cpu()[0]) == 0
    fresh = local_map_bytes(G, m, c, False)
    assert all(torch.equal(a, b) for a, b in zip(reuse, fresh))
    # ---- the same frame against the model's list uploaded from the host ----
    up = torch.zeros(tc.bird_cap, dtype=torch.int32, device="cuda")
    up[:len(lm.local_mpb)] = torch.as_tensor(lm.local_mpb, dtype=torch.int32)
    n_up = torch.tensor([len(lm.local_mpb)], dtype=torch.int32, device="cuda")
    next_frame_m9(up, n_up)
    torch.cuda.synchronize()
    ref = tc.view("cur")
    nb = int(ref["n_bird"][0])
    assert np.array_equal(got["map_point_bird"][0, :nb], ref["map_point_bird"][0, :nb]) and np.array_equal(got["n_bird"], ref["n_bird"])
    assert np.array_equal(got_counts, tc.counts("cur")[0])
    matched = got["map_point_bird"][0, :nb]
    assert (matched >= 0).sum() > 20 and set(matched[matched >= 0].tolist()) <= set(lm.local_mpb)
    G.close()
    tc.close()


def local_map_bytes(G, m, c, reuse):
    K, n_mp = c["K"], len(c["mp_bad"])
    t, a = G.local_map_arrays([c["S"]], np.asarray(c["kf_mp"][:1]), c["kf_bad"], max(K, 83), max(n_mp, 1))
    G.local_map(m, a, reuse_index=reuse)
    return [t[k] for k in ("d_map_point", "d_local_kf", "d_n_local_kf", "d_local_mp", "d_n_local_mp", "d_ref_kf", "d_n_voters")]
