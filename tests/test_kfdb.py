"""KeyFrameDatabase (fb_kfdb_*) without a device: the CPU restatement tests/kfdb_ref.py against the fixture recorded from the
reference's own L1Scoring::score (tests/golden/kfdb_score_ref.npz), the behaviour of the restatement that the GPU comparison
relies on, the C-ABI mirrors, and the no-device answers of the new entry points."""
import ctypes as C
import importlib.util
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kfdb_ref as R
from fishbirdeyevisualslam_amd import cabi, kfdb_problem as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "kfdb_score_ref.npz")


def fixture_pairs():
    z = np.load(GOLD)
    return [dict(a=(z["p%d_a_ids" % i], z["p%d_a_vals" % i]), b=(z["p%d_b_ids" % i], z["p%d_b_vals" % i]),
                 score=z["p%d_score" % i], score_ba=z["p%d_score_ba" % i]) for i in range(int(z["n_pairs"]))]


def _generator():
    spec = importlib.util.spec_from_file_location("make_kfdb_ref_golden", os.path.join(HERE, "golden", "make_kfdb_ref_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_restatement_score_equals_the_reference_fixture_bit_for_bit():
    pairs = fixture_pairs()
    assert len(pairs) >= 12
    sizes = set()
    for p in pairs:
        a, b = R.BowVector(*p["a"]), R.BowVector(*p["b"])
        sizes.update((len(a), len(b)))
        assert np.float64(R.l1_score(a, b)).tobytes() == p["score"].tobytes()
        assert np.float64(R.l1_score(b, a)).tobytes() == p["score_ba"].tobytes()
    assert 0 in sizes and 1 in sizes and max(sizes) > 1000
    assert any(int(p["a"][0].max(initial=0)) > 2 ** 32 - 400 for p in pairs)


def test_fixture_is_reproduced_by_the_reference_build():
    m = _generator()
    if not os.path.isdir(m.dbow2_dir()):
        pytest.skip("the reference tree is not present")
    r, z = m.generate(), np.load(GOLD)
    assert sorted(r) == sorted(z.files)
    for k in z.files:
        assert np.asarray(r[k]).tobytes() == z[k].tobytes(), k


def test_score_known_answers():
    pairs = fixture_pairs()
    assert float(pairs[3]["score"]) == 0.0 and float(pairs[5]["score"]) == 0.0 and float(pairs[6]["score"]) == 0.0  # disjoint, empty
    assert np.array_equal(pairs[4]["a"][0], pairs[4]["b"][0]) and abs(float(pairs[4]["score"]) - 1.0) <= 1e-15       # identical
    # symmetric only up to the summation order: the fixture holds pairs that differ in the last bits
    assert any(p["score"].tobytes() != p["score_ba"].tobytes() for p in pairs)
    assert all(abs(float(p["score"]) - float(p["score_ba"])) <= 1e-15 for p in pairs)
    ids = np.arange(7, dtype=np.uint32) * 3
    v = R.BowVector(ids, np.full(7, 1.0 / 7))
    assert abs(R.l1_score(v, v) - 1.0) <= 1e-15
    assert R.l1_score(v, R.BowVector(ids + 1, np.full(7, 1.0 / 7))) == 0.0


def loaded(p):
    db = R.KeyFrameDatabase(p["n_kf"])
    for s, (ids, vals) in enumerate(p["bows"]):
        db.add(s, ids, vals)
    return db


def planted_min_score(db, p, q):
    """A LOOP threshold between the scores of the query's own place: its upper quartile."""
    ids, vals = p["queries"][q][:2]
    sc = sorted(R.l1_score(R.BowVector(ids, vals), R.BowVector(*p["bows"][s])) for s in range(p["n_kf"]) if p["place"][s] == p["queries"][q][2])
    return float(np.float32(sc[(3 * len(sc)) // 4]))


@pytest.mark.parametrize("seed", [1, 3, 4])
def test_planted_database_exercises_every_step(seed):
    p = P.make_kfdb_problem(seed)
    db = loaded(p)
    tot = dict(below_threshold=0, neighbour_best=0, duplicates_removed=0, below_min_score=0)
    for q, (ids, vals, place, connected) in enumerate(p["queries"]):
        r = db.detect_relocalization_candidates(1000 + q, ids, vals, p["covis"])
        assert len(r["candidates"]) >= 2 and all(p["place"][c] == place for c in r["candidates"])
        assert r["below_threshold"] >= 1
        for k in ("below_threshold", "neighbour_best", "duplicates_removed"):
            tot[k] += r[k]
        l = db.detect_loop_candidates(1000 + q, ids, vals, planted_min_score(db, p, q), connected, p["covis"])
        assert len(l["candidates"]) >= 1 and all(p["place"][c] == place for c in l["candidates"])
        assert not set(l["candidates"]) & set(connected) and not set(l["listed"]) & set(connected)
        assert l["below_min_score"] >= 1
        tot["below_min_score"] += l["below_min_score"]
        tot["neighbour_best"] += l["neighbour_best"]
    assert all(v >= 1 for v in tot.values()), tot


def test_erase_keeps_the_relative_order_and_readding_moves_to_the_end():
    p = P.make_kfdb_problem(5)
    ids, vals, place, _ = p["queries"][0]
    no_covis = np.full_like(p["covis"], -1)   # every entry is its own pBestKF: the candidates are the retained list
    db = loaded(p)
    base = db.detect_relocalization_candidates(1, ids, vals, no_covis)
    assert len(base["candidates"]) >= 3
    victim = base["candidates"][0]
    db = loaded(p)
    db.erase(victim)
    r = db.detect_relocalization_candidates(1, ids, vals, no_covis)
    assert victim not in r["listed"] and r["listed"] == [s for s in base["listed"] if s != victim]
    db.add(victim, *p["bows"][victim])
    r = db.detect_relocalization_candidates(2, ids, vals, no_covis)
    # the same set, but the re-added key frame is now last in every word's list: where it led a word's list it falls back
    assert sorted(r["listed"]) == sorted(base["listed"]) and r["listed"] != base["listed"]
    first_word = {}
    for w in ids:
        for s in base["listed"]:
            if int(w) in set(int(x) for x in p["bows"][s][0]):
                first_word.setdefault(s, int(w))
    expect = sorted(base["listed"], key=lambda s: (first_word[s], s == victim, base["listed"].index(s)))
    assert r["listed"] == expect


def test_same_query_id_twice_returns_nothing_and_keeps_counting():
    p = P.make_kfdb_problem(6)
    db = loaded(p)
    ids, vals, place, connected = p["queries"][1]
    a = db.detect_relocalization_candidates(7, ids, vals, p["covis"])
    b = db.detect_relocalization_candidates(7, ids, vals, p["covis"])
    assert a["candidates"] and b["candidates"] == [] and b["n_sharing"] == 0
    assert np.array_equal(b["common_words"], 2 * a["common_words"])
    a = db.detect_loop_candidates(7, ids, vals, 0.0, connected, p["covis"])
    b = db.detect_loop_candidates(7, ids, vals, 0.0, connected, p["covis"])
    assert a["candidates"] and b["candidates"] == []
    assert all(b["common_words"][c] == 1 for c in connected)   # connected: reset on every encounter


def test_stale_reloc_score_of_an_unscored_neighbour_is_added():
    """KeyFrameDatabase.cc:273-276: a neighbour touched by this query but below the threshold contributes its OLD mRelocScore."""
    w = lambda ids: (np.array(ids, np.uint32), np.full(len(ids), 1.0 / len(ids)))
    db = R.KeyFrameDatabase(3)
    db.add(0, *w(range(0, 10)))
    db.add(1, *w([0, 100, 101, 102, 103, 104, 105, 106, 107, 108]))
    covis = np.full((3, 10), -1, np.int32)
    covis[0, 0] = 1
    first = db.detect_relocalization_candidates(1, *w(range(100, 109)), covis)   # scores slot 1 alone
    old = db.kf[1].mRelocScore
    assert first["candidates"] == [1] and old > 0
    r = db.detect_relocalization_candidates(2, *w(range(0, 10)), covis)          # slot 1 shares one word: listed, not scored
    assert r["listed"] == [0, 1] and r["n_scored"] == 1 and db.kf[1].mRelocScore == old
    assert r["acc"] == [(np.float32(db.kf[0].mRelocScore + old), 0)]


def test_struct_layout_matches_the_header():
    src = ('#include <stdio.h>\n#include "fishbird.h"\nint main(void){printf("%zu %zu %d %d %d %d %d\\n", sizeof(fb_kfdb_params), '
           'sizeof(fb_kfdb_query_args), FB_KFDB_MAX_KEYFRAMES, FB_KFDB_MAX_WORDS, FB_KFDB_COVIS, FB_KFDB_RELOC, FB_KFDB_LOOP);return 0;}\n')
    d = tempfile.mkdtemp()
    open(os.path.join(d, "s.c"), "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
    got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert got == [C.sizeof(cabi.KfdbParams), C.sizeof(cabi.KfdbQueryArgs), cabi.FB_KFDB_MAX_KEYFRAMES, cabi.FB_KFDB_MAX_WORDS,
                   cabi.FB_KFDB_COVIS, cabi.FB_KFDB_RELOC, cabi.FB_KFDB_LOOP]


def test_no_device_no_answer():
    import fishbirdeyevisualslam_amd as fb
    lib = fb.lib()
    one = np.ones(1, np.int32)
    ids, vals, out = np.zeros(1, np.uint32), np.ones(1), np.zeros(1)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    rc = lib.fb_bow_score(1, 1, vp(one), vp(ids), vp(vals), vp(one), vp(ids), vp(vals), vp(out))
    h = C.c_void_p()
    prm = cabi.KfdbParams(8, 16)
    assert lib.fb_kfdb_create(C.byref(cabi.KfdbParams(0, 16)), C.byref(h)) == cabi.FB_ERR_ARG
    assert lib.fb_kfdb_create(C.byref(prm), C.byref(h)) == cabi.FB_OK
    rc_add = lib.fb_kfdb_add(h, 0, 1, vp(ids), vp(vals))
    rc_clear = lib.fb_kfdb_clear(h, None)
    lib.fb_kfdb_destroy(h)
    if lib.fb_device_count() > 0:
        assert (rc, rc_add, rc_clear) == (0, 0, 0) and out[0] == 1.0
    else:
        assert (rc, rc_add, rc_clear) == (cabi.FB_ERR_NODEVICE,) * 3
        assert b"no CPU fallback" in lib.fb_last_error()
