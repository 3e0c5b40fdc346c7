"""fb_kfdb_* / fb_bow_score* on the device against the CPU restatement of the reference (tests/kfdb_ref.py) and the fixture
recorded from the reference's own L1Scoring::score.  Integers and floats are compared bit for bit: the device performs the
same IEEE operations in the same order (sums in ascending word order on one accumulator, no FMA), so equality is derived,
not measured."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import kfdb_ref as R
from fishbirdeyevisualslam_amd import cabi, kfdb_problem as P
from test_kfdb import fixture_pairs, planted_min_score

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = ("n_sharing", "max_common_words", "n_scored")


def _db(K, S):
    from fishbirdeyevisualslam_amd.kfdb import KeyFrameDatabase
    return KeyFrameDatabase(K, S)


def _same(got, ref, what=""):
    """got: device tensors of one query (after a synchronisation); ref: the restatement's info"""
    n = int(got["n_candidates"].cpu()[0])
    assert got["candidates"].cpu().numpy()[:n].tolist() == ref["candidates"], what
    for k in EXTRA:
        assert int(got[k].cpu()[0]) == ref[k], (what, k)
    K = len(ref["common_words"])
    assert np.array_equal(got["common_words"].cpu().numpy()[:K], ref["common_words"]), what
    assert got["scores"].cpu().numpy()[:K].tobytes() == ref["scores"].tobytes(), what


def _pairs_arrays():
    pairs = fixture_pairs()
    stride = max(max(len(p["a"][0]), len(p["b"][0])) for p in pairs)
    B = len(pairs)
    arr = dict(a_ids=np.zeros((B, stride), np.uint32), a_vals=np.zeros((B, stride)), b_ids=np.zeros((B, stride), np.uint32),
               b_vals=np.zeros((B, stride)), na=np.zeros(B, np.int32), nb=np.zeros(B, np.int32))
    for i, p in enumerate(pairs):
        for t in "ab":
            n = len(p[t][0])
            arr[t + "_ids"][i, :n], arr[t + "_vals"][i, :n], arr["n" + t][i] = p[t][0], p[t][1], n
    return pairs, arr, stride


def test_bow_score_equals_the_reference_fixture():
    import fishbirdeyevisualslam_amd as fb
    from fishbirdeyevisualslam_amd.kfdb import bow_score
    pairs, a, stride = _pairs_arrays()
    want = np.array([p["score"] for p in pairs]).tobytes()
    want_ba = np.array([p["score_ba"] for p in pairs]).tobytes()
    assert bow_score(a["a_ids"], a["a_vals"], a["na"], a["b_ids"], a["b_vals"], a["nb"]).cpu().numpy().tobytes() == want
    assert bow_score(a["b_ids"], a["b_vals"], a["nb"], a["a_ids"], a["a_vals"], a["na"]).cpu().numpy().tobytes() == want_ba
    out = np.zeros(len(pairs))
    vp = lambda x: C.c_void_p(x.ctypes.data)
    fb.check(fb.lib().fb_bow_score(len(pairs), stride, vp(a["na"]), vp(a["a_ids"]), vp(a["a_vals"]), vp(a["nb"]), vp(a["b_ids"]),
                                   vp(a["b_vals"]), vp(out)), "fb_bow_score")
    assert out.tobytes() == want


def _queries_of(p, g, extra_random=2):
    qs = [(ids, vals, conn) for ids, vals, _, conn in p.get("queries", [])]
    n = p["n_kf"]
    for _ in range(extra_random):
        src = p["bows"][int(g.integers(0, n))] if n else P.l1_normalised(np.arange(50, dtype=np.uint32), np.ones(50))
        keep = g.random(len(src[0])) < 0.7
        ids, vals = P.l1_normalised(src[0][keep], g.uniform(0.1, 5.0, int(keep.sum()))) if keep.any() else src
        qs.append((ids, vals, [int(x) for x in g.choice(n, min(n, 3), replace=False)] if n else []))
    qs.append((np.zeros(0, np.uint32), np.zeros(0), []))                                      # a query with 0 words
    qs.append((np.arange(10, dtype=np.uint32) + np.uint32(3000000), np.full(10, 0.1), []))   # nothing shares a word
    return qs


def _run_database(p, K, S, seed):
    import torch
    g = np.random.default_rng(seed)
    dev, ref = _db(K, S), R.KeyFrameDatabase(K)
    covis = np.full((K, 10), -1, np.int32)
    covis[: len(p["covis"])][: p["n_kf"]] = p["covis"][: p["n_kf"]] if p["n_kf"] else covis[:0]
    dev.set_covisibility(covis)
    for s, (ids, vals) in enumerate(p["bows"]):
        dev.add(s, ids, vals)
        ref.add(s, ids, vals)
    qid = 10
    for ids, vals, conn in _queries_of(p, g):
        qid += 1
        got = dev.detect_relocalization_candidates(qid, ids, vals, extras=True)
        want = ref.detect_relocalization_candidates(qid, ids, vals, covis)
        torch.cuda.synchronize()
        _same(got, want, "reloc %d" % qid)
        ms = float(np.median(want["scores"][want["scores"] > 0])) if (want["scores"] > 0).any() else 0.05
        got = dev.detect_loop_candidates(qid, ids, vals, ms, conn, extras=True)
        want = ref.detect_loop_candidates(qid, ids, vals, ms, conn, covis)
        torch.cuda.synchronize()
        _same(got, want, "loop %d" % qid)
    dev.close()


@pytest.mark.parametrize("seed", [1, 3, 4])
def test_planted_database(seed):
    p = P.make_kfdb_problem(seed)
    _run_database(p, 256, 512, seed)


@pytest.mark.parametrize("n_kf,words,K,S", [(0, (1, 50), 8, 64), (1, (1, 4096), 1, 4096), (37, (1, 4096), 64, 4096),
                                             (37, (1, 300), 37, 300), (3000, (1, 4096), 4096, 4096)])
def test_random_database(n_kf, words, K, S):
    _run_database(P.make_random_database(700 + n_kf, n_kf, words), K, S, n_kf)


def test_interleaved_script_without_host_synchronisation():
    """~200 add / erase / query / clear steps on one stream; nothing is read back before the end."""
    import torch
    g = np.random.default_rng(99)
    p = P.make_kfdb_problem(8)
    K = p["n_kf"]
    dev, ref = _db(K, 256), R.KeyFrameDatabase(K)
    dev.set_covisibility(p["covis"])
    inside, results = set(), []
    for step in range(200):
        r = g.random()
        if step == 120:
            dev.clear(); ref.clear(); inside.clear()
        elif r < 0.5 and len(inside) < K:
            s = int(g.choice(sorted(set(range(K)) - inside)))
            dev.add(s, *p["bows"][s]); ref.add(s, *p["bows"][s]); inside.add(s)
        elif r < 0.65 and inside:
            s = int(g.choice(sorted(inside)))
            dev.erase(s); ref.erase(s); inside.discard(s)
        else:
            ids, vals, _, conn = p["queries"][int(g.integers(0, len(p["queries"])))]
            qid = int(g.integers(0, 6))  # small range: repeated ids (and 0, the value add() leaves) carry state across queries
            if g.random() < 0.5:
                results.append((dev.detect_relocalization_candidates(qid, ids, vals, extras=True),
                                ref.detect_relocalization_candidates(qid, ids, vals, p["covis"]), step))
            else:
                ms = float(g.uniform(0.05, 0.3))
                results.append((dev.detect_loop_candidates(qid, ids, vals, ms, conn, extras=True),
                                ref.detect_loop_candidates(qid, ids, vals, ms, conn, p["covis"]), step))
    torch.cuda.synchronize()
    assert len(results) > 40 and sum(1 for _, w, _ in results if w["candidates"]) > 10
    for got, want, step in results:
        _same(got, want, "step %d" % step)
    dev.close()


def test_host_pointer_variants_and_min_score():
    import torch
    import fishbirdeyevisualslam_amd as fb
    L = fb.lib()
    p = P.make_kfdb_problem(3)
    K = p["n_kf"]
    ref = R.KeyFrameDatabase(K)
    h = C.c_void_p()
    fb.check(L.fb_kfdb_create(C.byref(cabi.KfdbParams(K, 256)), C.byref(h)), "create")
    vp = lambda x: C.c_void_p(x.ctypes.data)
    for s, (ids, vals) in enumerate(p["bows"]):
        fb.check(L.fb_kfdb_add(h, s, len(ids), vp(ids), vp(vals)), "fb_kfdb_add")
        ref.add(s, ids, vals)
    covis = np.ascontiguousarray(p["covis"])
    for q, (ids, vals, place, conn) in enumerate(p["queries"]):
        for mode in (cabi.FB_KFDB_RELOC, cabi.FB_KFDB_LOOP):
            ms = planted_min_score(ref, p, q)
            o = dict(n_candidates=np.zeros(1, np.int32), candidates=np.full(K, -7, np.int32), n_sharing=np.zeros(1, np.int32),
                     max_common_words=np.zeros(1, np.int32), n_scored=np.zeros(1, np.int32), common_words=np.zeros(K, np.int32),
                     scores=np.zeros(K, np.float32))
            a = cabi.KfdbQueryArgs()
            nw, cn = np.array([len(ids)], np.int32), np.array(conn, np.int32)
            cabi.fill(a, mode=mode, query_id=50 + q, n_words=nw, bow_ids=ids, bow_vals=vals, min_score=ms, n_connected=len(cn),
                      connected=cn, covis=covis, **o)
            fb.check(L.fb_kfdb_query(h, C.byref(a)), "fb_kfdb_query")
            want = (ref.detect_relocalization_candidates(50 + q, ids, vals, covis) if mode == cabi.FB_KFDB_RELOC else
                    ref.detect_loop_candidates(50 + q, ids, vals, ms, conn, covis))
            n = int(o["n_candidates"][0])
            assert o["candidates"][:n].tolist() == want["candidates"] and (o["candidates"][n:] == -7).all()
            assert [int(o[k][0]) for k in EXTRA] == [want[k] for k in EXTRA]
            assert np.array_equal(o["common_words"], want["common_words"]) and o["scores"].tobytes() == want["scores"].tobytes()
        # DetectLoop's reference score over the connected key frames (one erased = bad, one skipped)
        slots = np.array(conn + [int(x) for x in np.nonzero(p["place"] == place)[0][:6]], np.int32)
        skip = np.zeros(len(slots), np.uint8)
        skip[2] = 1
        scores, mn = np.zeros(len(slots), np.float32), np.zeros(1, np.float32)
        fb.check(L.fb_kfdb_min_score(h, len(ids), vp(ids), vp(vals), len(slots), vp(slots), vp(skip), vp(scores), vp(mn)), "min_score")
        ws, wm = ref.min_score(ids, vals, slots, skip)
        assert scores.tobytes() == ws.tobytes() and mn.tobytes() == np.float32(wm).tobytes() and mn[0] < 1
    fb.check(L.fb_kfdb_min_score(h, len(ids), vp(ids), vp(vals), 0, None, None, None, vp(mn)), "min_score empty")
    assert mn[0] == 1.0
    L.fb_kfdb_destroy(h)
    # the _dev variant through the torch wrapper on the same database
    dev = _db(K, 256)
    for s, (ids, vals) in enumerate(p["bows"]):
        dev.add(s, ids, vals)
    ids, vals, place, conn = p["queries"][0]
    slots = np.array(conn + [5, 6, 7], np.int32)
    sc, mn = dev.min_score(ids, vals, slots)
    torch.cuda.synchronize()
    ws, wm = ref.min_score(ids, vals, slots)
    assert sc.cpu().numpy().tobytes() == ws.tobytes() and mn.cpu().numpy().tobytes() == np.float32(wm).tobytes()
    dev.close()


def test_argument_errors_leave_the_handle_usable():
    import fishbirdeyevisualslam_amd as fb
    L = fb.lib()
    h = C.c_void_p()
    assert L.fb_kfdb_create(C.byref(cabi.KfdbParams(4, 5000)), C.byref(h)) == cabi.FB_ERR_ARG
    assert L.fb_kfdb_create(C.byref(cabi.KfdbParams(5000, 16)), C.byref(h)) == cabi.FB_ERR_ARG
    assert L.fb_kfdb_create(C.byref(cabi.KfdbParams(4, 16)), C.byref(h)) == 0
    ids, vals = np.arange(8, dtype=np.uint32), np.full(8, 0.125)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    E = cabi.FB_ERR_ARG
    assert L.fb_kfdb_add(h, 4, 8, vp(ids), vp(vals)) == E and L.fb_kfdb_add(h, -1, 8, vp(ids), vp(vals)) == E
    assert L.fb_kfdb_add(h, 0, 17, vp(ids), vp(vals)) == E and L.fb_kfdb_add(h, 0, 8, None, vp(vals)) == E
    assert L.fb_kfdb_erase(h, 0, None) == E and b"not in the database" in L.fb_last_error()
    assert L.fb_kfdb_add(h, 0, 8, vp(ids), vp(vals)) == 0
    assert L.fb_kfdb_add(h, 0, 8, vp(ids), vp(vals)) == E and b"already" in L.fb_last_error()
    assert L.fb_kfdb_add_dev(h, 1, None, None, None, None) == E
    a = cabi.KfdbQueryArgs()
    assert L.fb_kfdb_query(h, C.byref(a)) == E and L.fb_kfdb_query_dev(h, C.byref(a), None) == E
    o = dict(n_candidates=np.zeros(1, np.int32), candidates=np.zeros(4, np.int32))
    cabi.fill(a, mode=7, query_id=1, n_words=np.array([8], np.int32), bow_ids=ids, bow_vals=vals, covis=np.full((4, 10), -1, np.int32), **o)
    assert L.fb_kfdb_query_dev(h, C.byref(a), None) == E
    a.mode = cabi.FB_KFDB_RELOC
    assert L.fb_kfdb_query(h, C.byref(a)) == 0 and o["n_candidates"][0] == 1 and o["candidates"][0] == 0
    assert L.fb_kfdb_erase(h, 0, None) == 0 and L.fb_kfdb_erase(h, 0, None) == E
    a.query_id = 2
    assert L.fb_kfdb_query(h, C.byref(a)) == 0 and o["n_candidates"][0] == 0
    L.fb_kfdb_destroy(h)


def test_frames_to_candidates_to_search_by_bow_on_handles():
    """fb_frame_extract -> fb_frame_compute_bow_dev -> fb_kfdb_add_frame_dev for synthetic frames, a query with another frame's
    device BowVector, and the first candidate through fb_frame_search_by_bow_dev with no host copy in between; the candidates
    equal the restatement fed with the oracle's BowVectors."""
    import torch
    import oracle_lib as O
    from fishbirdeyevisualslam_amd import sequence as S, track as T
    from fishbirdeyevisualslam_amd.bow_problem import make_vocabulary
    from test_bow_transform import make_args
    wh, bwh, NKF = (640, 480), (384, 384), 5
    seq = S.Sequence(1, NKF + 1, seed=9850, front_wh=wh, bird_wh=bwh, fx=250.0, fy=250.0, device="cuda:0")
    tc = T.TrackChain(1, wh, bwh, K=seq.Kc, D=seq.D)
    L = tc.L
    mask_d = torch.from_numpy(seq.mask).cuda()
    vv, vk, first_leaf = make_vocabulary(9851, k=6, L=5)
    tc.set_vocabulary(vk, 5)
    s = tc._stream()
    dev, ref = _db(16, tc.cap), R.KeyFrameDatabase(16)
    covis = np.full((16, 10), -1, np.int32)
    for j in range(NKF):
        covis[j, :2] = [(j + 1) % NKF, (j - 1) % NKF]
    dev.set_covisibility(covis)

    def oracle_bow(which):
        v = tc.view(which)
        a, out, keep = make_args([v["desc"][0, : v["n"][0]]], levelsup=4)
        assert O.lib().orc_bow_transform(C.byref(vv), C.byref(a)) == 0
        nw = int(out["n_words"][0])
        return out["bow_ids"][0, :nw].copy(), out["bow_vals"][0, :nw].copy()
    kfs = []
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for j in range(NKF):
        f, b, c = seq.render(j)
        tc.extract(f, b, c, mask_d)
        if j == 0:
            M, MB, mp0, mpb0, Tcw0 = seq.build_map(tc.view("cur"), tc.tables, map_cap=tc.map_cap, bird_cap=tc.bird_cap)
            tc.set_map(M, MB)
            d_mp, d_mpb = up(mp0), up(mpb0)
        # every key frame carries map points (SearchByBoW only uses key-frame features that have one)
        assert L.fb_frame_set_map_points_dev(tc.cur, C.c_void_p(d_mp.data_ptr()), C.c_void_p(d_mpb.data_ptr()), s) == 0
        assert L.fb_frame_compute_bow_dev(tc.cur, C.byref(tc.voc), s) == 0, L.fb_last_error()
        kf = C.c_void_p()
        assert L.fb_frame_create(C.byref(tc.params), C.byref(kf)) == 0
        assert L.fb_frame_copy_dev(kf, tc.cur, s) == 0, L.fb_last_error()
        kfs.append(kf)
        dev.add_frame(j, kf)
        ref.add(j, *oracle_bow("cur"))
    empty = C.c_void_p()
    assert L.fb_frame_create(C.byref(tc.params), C.byref(empty)) == 0
    assert L.fb_kfdb_add_frame_dev(dev.h, 9, empty, s) == cabi.FB_ERR_ARG      # no BoW on that frame
    f, b, c = seq.render(NKF)
    tc.extract(f, b, c, mask_d)
    assert L.fb_frame_compute_bow_dev(tc.cur, C.byref(tc.voc), s) == 0
    view = cabi.BowTransformArgs()
    assert L.fb_frame_bow_view_dev(tc.cur, C.byref(view)) == 0
    out = dict(n_candidates=torch.zeros(1, dtype=torch.int32, device="cuda"), candidates=torch.full((16,), -1, dtype=torch.int32, device="cuda"))
    a = cabi.KfdbQueryArgs()
    cabi.fill(a, mode=cabi.FB_KFDB_RELOC, query_id=77, covis=dev.covis, **out)
    a.n_words, a.bow_ids, a.bow_vals = view.n_words, view.bow_ids, view.bow_vals
    assert L.fb_kfdb_query_dev(dev.h, C.byref(a), s) == 0, L.fb_last_error()
    # the host decides which candidate to try (Relocalization's loop); here: the restatement's first, checked below
    want = ref.detect_relocalization_candidates(77, *oracle_bow("cur"), covis)
    assert want["candidates"]
    first = want["candidates"][0]
    m07 = cabi.MatcherParams(0.75, 1)
    assert L.fb_frame_search_by_bow_dev(tc.cur, kfs[first], C.byref(tc.targs.map), C.byref(m07), 0, s) == 0, L.fb_last_error()
    torch.cuda.synchronize()
    n = int(out["n_candidates"].cpu()[0])
    assert out["candidates"].cpu().numpy()[:n].tolist() == want["candidates"]
    assert tc.counts("cur")[0][cabi.FB_CNT["BOW_MATCHES"]][0] > 0
    for kf in kfs + [empty]:
        L.fb_frame_destroy(kf)
    dev.close()
    tc.close()


def test_host_header_database_builds_and_runs():
    """tests/cpp/kfdb_host_test.cpp drives fishbird::KeyFrameDatabase (host/fishbird_host.hpp) in a fresh child process."""
    import fishbirdeyevisualslam_amd as fb
    pkg = os.path.dirname(fb.LIB_PATH)
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "kfdb_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"),
                           os.path.join(ROOT, "tests", "cpp", "kfdb_host_test.cpp"), "-o", exe, "-L", pkg, "-lfishbird_hip",
                           "-Wl,-rpath," + pkg])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"kfdb_host_test ok" in r.stdout
