"""Constructed images on the decisions of ComputeKeyPointsOctTree / DistributeOctTree -- TEST INFRASTRUCTURE ONLY.

The building block is the one-pixel spot of height d on a flat image: a FAST-9-16 corner of response d - 1, detected at
threshold T iff d > T.  Spots at Chebyshev distance >= 4 lie on nobody's ring and touch nobody's 3x3 neighbourhood, so the
candidates are exactly the spots above the threshold; two spots at distance 1 or 2 are still both corners (neither offset
is on the radius-3 ring), which the seam, tie and narrow-node cases use.

A case is (images, parameters, the branch it must take by the model's trace, the variants of orb_ref.VARIANTS it must kill).
One level (N = nfeatures) unless stated.  tests/test_orb_cases.py checks branch and kills on the CPU against the oracle's
levels; tests/test_orb_cases_gpu.py sends the same cases through the HIP entry points.
"""
import ctypes as C

import numpy as np

import orb_ref as R
from fishbirdeyevisualslam_amd import cabi, synth

BASE = 100
B = 16    # minBorderX / minBorderY


def params(nfeatures, nlevels=1, ini=20, mn=7, scale=1.2):
    return cabi.OrbParams(nfeatures=nfeatures, scale_factor=scale, nlevels=nlevels, ini_th_fast=ini, min_th_fast=mn)


def spots(w, h, pts):
    """Flat w x h image with one-pixel spots [(x, y, d)] in image coordinates."""
    img = np.full((h, w), BASE, np.uint8)
    for x, y, d in pts:
        assert 0 <= x < w and 0 <= y < h and img[y, x] == BASE, (x, y)
        img[y, x] = BASE + d
    return img


def rel(pts):
    """[(x, y, d)] relative to the border corner (the coordinates DistributeOctTree works in) -> image coordinates."""
    return [(x + B, y + B, d) for x, y, d in pts]


def lattice(w, h, n, seed, lo=21, hi=119, step=4):
    """n spots on a lattice of spacing `step` over the tested pixels, random positions and heights lo..hi."""
    rng = np.random.default_rng(seed)
    pts = [(x, y) for y in range(19, h - 19, step) for x in range(19, w - 19, step)]
    assert n <= len(pts), (n, len(pts))
    img = np.full((h, w), BASE, np.uint8)
    for q in rng.permutation(len(pts))[:n]:
        img[pts[q][1], pts[q][0]] = BASE + rng.integers(lo, hi + 1)
    return img


class Case:
    def __init__(self, name, img, p, branch, kills=(), doc=""):
        self.name, self.img, self.p, self.branch, self.kills, self.doc = name, img, p, branch, tuple(kills), doc

    def __repr__(self):
        return self.name


# ---- branch predicates over the model's result (trace of level 0 unless stated) ----
def _t(m, level=0):
    return m["trace"][level]


def _full(m):
    return [r for r in _t(m)["rounds"] if r["phase"] == "full"]


def _sorted(m):
    return [r for r in _t(m)["rounds"] if r["phase"] == "sorted"]


def n_cand(n):
    return lambda m: _t(m)["candidates"] == n


def n_kps(n):
    return lambda m: len(m["kps"]) == n


def all_of(*fs):
    return lambda m: all(f(m) for f in fs)


def skipped(n):
    return lambda m: _t(m)["cells_skipped"] == n


def redone(n):
    return lambda m: _t(m)["cells_redone"] == n


def n_ini(n):
    return lambda m: _t(m)["nIni"] == n


def exit_is(e, phase):
    return lambda m: _t(m)["exit"] == e and _t(m)["rounds"][-1]["phase"] == phase


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
        assert len(set(c.name for c in _CASES)) == len(_CASES)
    return _CASES


def by_name(name):
    return next(c for c in cases() if c.name == name)


def _build():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))

    # ================= cell grid =================
    # 152 x 122: 4 x 3 cells of 30 x 30, tested pixels x 19..132, y 19..102
    w, h = 152, 122
    add("grid_last_column_and_row", spots(w, h, [(132, 40, 40), (133, 60, 40), (50, 102, 40), (80, 103, 40), (19, 19, 41), (18, 30, 40),
                                                 (30, 18, 40)]),
        params(1500), all_of(n_cand(3), n_kps(3)), doc="x = w-20 / y = h-20 are the last tested; one past them, and one before 19, is not")
    seams = []
    for k, x in enumerate((48, 78, 108)):          # the cells' interiors meet between x = 48|49, 78|79, 108|109
        seams += [(x, 25 + 6 * k, 50), (x + 1, 25 + 6 * k, 50)]
    for k, y in enumerate((48, 78)):               # and between y = 48|49, 78|79
        seams += [(25 + 6 * k, y, 50), (25 + 6 * k, y + 1, 50)]
    seams += [(60, 60, 50), (61, 60, 50)]          # the same pair inside one cell: a tie, both suppressed
    add("grid_seams", spots(w, h, seams), params(1500), all_of(n_cand(10), n_kps(5)),
        doc="equal neighbours across a seam both survive (no suppression across cells); inside a cell neither does.  No split "
            "line falls between the two of a pair, so the tree stalls with five nodes of two")
    # strips: 30 columns of 31 (widths 933..962) and 29 rows of 31; the last column starts at 915, the last row at 884
    for W, nskip in ((937, 2), (938, 0)):
        add("grid_column_skip_%d" % W, spots(W, 92, [(W - 20, 40, 40), (900, 50, 41), (30, 30, 42)]), params(1500),
            all_of(skipped(nskip), n_cand(3)),
            doc="iniX = 915 against maxBorderX - 6 = W - 22: equal at 937 (skipped; the column before it tests up to x = 917 = W - 20), "
                "one less at 938 (a 7 px window whose one tested column, x = 918 = W - 20, belongs to no other cell)")
    for H, nskip in ((903, 14), (904, 0), (907, 0)):   # 470 wide: 438 / 871 >= 0.5, so the level has an initial node
        add("grid_row_skip_%d" % H, spots(470, H, [(40, H - 20, 40), (300, 500, 41), (30, 30, 42)]), params(1500),
            all_of(skipped(nskip), n_cand(3), n_kps(3), n_ini(1)),
            doc="iniY = 884 against maxBorderY - 3 = H - 19: equal at 903 (skipped; the row before it tests up to y = 884); at 904 "
                "the row is 4 px high (narrower than 7 after the clamp: nothing tested), at 907 it is 7 px high and its one tested "
                "row, y = 887 = H - 20, belongs to no other cell")
    for ini, mn in ((15, 5), (20, 7)):
        pts = [(30, 30, ini + 1), (36, 30, ini),              # cell (0,0): only the first is a candidate
               (60, 30, ini), (66, 30, mn),                  # cell (0,1): redone; the first is a candidate, the second is not
               (90, 30, mn + 1),                             # cell (0,2): redone, one candidate
               (120, 30, ini + 1), (126, 30, mn + 1),        # cell (0,3): one candidate at iniThFAST; not redone, not merged
               (30, 60, ini + 30), (36, 60, ini + 1), (30, 66, mn + 2)]   # cell (1,0): two at iniThFAST
        add("thresholds_%d_%d" % (ini, mn), spots(w, h, pts), params(1500, ini=ini, mn=mn), all_of(n_cand(6), redone(9), n_kps(6)),
            kills=("second_fast_below_count", "fast_merged"), doc="d = T + 1 against d = T at both thresholds, passed explicitly")

    # ================= initial nodes =================
    ini_pts = lambda W_, H_, seed: lattice(W_, H_, 14, seed)
    add("nini_ratio_1.49", ini_pts(181, 132, 11), params(3), n_ini(1), doc="149 / 100")
    add("nini_ratio_1.5", ini_pts(122, 92, 12), params(3), n_ini(2), kills=("nini_floor",), doc="90 / 60: half away from zero")
    add("nini_ratio_2.5", ini_pts(182, 92, 13), params(4), n_ini(3), kills=("nini_floor", "nini_half_even"), doc="150 / 60")
    add("nini_zero", ini_pts(92, 160, 14), params(10), all_of(n_ini(0), n_cand(14), n_kps(0)), doc="60 / 128 < 0.5: no node, no key point")
    # 132 x 72: region 100 x 40, nIni = 3, hX = 33.33: truncated bounds 0, 33, 66, 100 (rounded: 67); children split at +17
    pts = []
    ys = [3, 7, 11, 15, 19, 23, 27, 31, 35]
    for k, x in enumerate((32, 33, 34, 65, 66, 67, 82, 83, 84)):
        pts.append((x, ys[k], 30 + k))
    pts += [(3, 20, 60), (96, 20, 61), (49, 5, 62), (50, 33, 63), (16, 30, 64), (17, 6, 65)]
    add("ini_bounds_non_integer_hx", spots(132, 72, rel(pts)), params(9), all_of(n_ini(3), n_cand(15)), kills=("bounds_rounded",),
        doc="spots on (int)(hX*i) - 1, +0, +1 and around the children's split lines, which move with a rounded bound")
    add("ini_empty_node_between", spots(132, 72, rel([(5, 5, 40), (20, 30, 41), (30, 12, 42), (70, 8, 43), (90, 30, 44), (80, 20, 45)])),
        params(4), all_of(n_ini(3), lambda m: _t(m)["ini_sizes"] == [3, 0, 3]))
    add("ini_node_with_one_spot", spots(132, 72, rel([(5, 5, 40), (40, 30, 41), (50, 12, 42), (70, 8, 43), (90, 30, 44)])),
        params(3), all_of(n_ini(3), lambda m: _t(m)["ini_sizes"] == [1, 2, 2]))

    # ================= splits =================
    for side, name in ((93, "odd"), (92, "even")):   # region 61 x 61 (halves 31) / 60 x 60 (halves 30)
        mid = 31 if side == 93 else 30
        pts = [(mid - 1, 10, 40), (mid, 14, 41), (10, mid - 1, 42), (14, mid, 43), (mid - 1, mid - 1, 44), (mid, mid + 3, 45),
               (50, 50, 46), (5, 5, 47), (mid + 4, mid - 1, 48)]
        add("split_lines_" + name, spots(side, side, rel(pts)), params(4), all_of(n_ini(1), n_cand(9)),
            kills=("split_le",) + (("floor_halves",) if name == "odd" else ()), doc="spots on mx-1, mx and my-1, my")
    # region 30 x 60 (62 x 92): widths 30 -> 15 -> 7 -> 3 -> 1 (columns 0..14 | 8..14 | 12..14 | 14); two spots 2 px apart in column
    # 14, and ten spots elsewhere that keep the list growing until that node is reached
    img = lattice(62, 92, 10, 0)
    assert img[B:B + 11, B + 10:B + 19].max() == BASE
    img[B + 4, B + 14], img[B + 6, B + 14] = BASE + 40, BASE + 41
    add("split_node_1px_wide", img, params(50),
        all_of(n_ini(1), n_cand(12), lambda m: any(wd == 1 and n > 1 for wd, ht, n in _t(m)["divided"]), n_kps(12)))
    add("split_same_child_stalls", spots(92, 92, rel([(5, 5, 40), (10, 10, 41)])), params(10),
        all_of(n_cand(2), n_kps(1), exit_is("size==prevSize", "full"), lambda m: len(_full(m)) == 1),
        doc="both spots fall into n1: the list does not grow, fewer key points than N and than candidates")
    add("n_zero_last_level", synth.synth_image(3, 640, 480)[100:220, 200:360].copy(), params(1, nlevels=2),
        lambda m: m["features_per_level"] == [1, 0] and _t(m, 1)["candidates"] > 1 and len(_t(m, 1)["rounds"]) == 1
        and _t(m, 1)["keypoints"] >= 1, doc="the quotas already sum to nfeatures: the last level has N = 0")

    # ================= termination (layout of 29 spots; N chosen by the model's trace) =================
    lay = lattice(152, 122, 29, 0)

    def last_sorted(f):
        return lambda m: bool(_sorted(m)) and f(_sorted(m)[-1])

    add("term_full_exact_n", lay, params(4), all_of(lambda m: not _sorted(m) and _full(m)[-1]["size"] == 4, exit_is("size>=N", "full")),
        kills=("finish_gt_n",), doc="the list reaches exactly N after a full pass")
    add("term_expand_eq_n", lay, params(16), lambda m: any(r["size"] + 3 * r["nToExpand"] == 16 and r["size"] < 16 for r in _full(m)[:-1]),
        kills=("expand_ge_n",), doc="size + 3 nToExpand == N: another full pass")
    add("term_expand_eq_n_plus_1", lay, params(15), lambda m: _full(m)[-1]["size"] + 3 * _full(m)[-1]["nToExpand"] == 16 and bool(_sorted(m)),
        doc="size + 3 nToExpand == N + 1: the sorted phase")
    add("term_break_after_1", lay, params(5), last_sorted(lambda r: r["broke"] and r["split"] == 1 and r["expandable"] >= 3),
        kills=("no_break",))
    add("term_break_all_but_one", lay, params(10), last_sorted(lambda r: r["broke"] and r["split"] == r["expandable"] - 1 >= 2),
        kills=("no_break",))
    add("term_break_after_all", lay, params(11), last_sorted(lambda r: r["broke"] and r["split"] == r["expandable"] >= 2))
    add("term_sorted_twice", lay, params(13), lambda m: len(_sorted(m)) == 2)
    add("term_sorted_three_times", lay, params(28), lambda m: len(_sorted(m)) >= 3)
    add("term_sorted_ends_on_prev_size", lay, params(30), all_of(exit_is("size==prevSize", "sorted"), n_kps(29)))
    add("term_sort_ties", lay, params(25),
        last_sorted(lambda r: r["broke"] and r["top_sizes"][0] == r["top_sizes"][2] and r["split"] < r["top_sizes"].count(r["top_sizes"][0])),
        kills=("sort_tie_oldest_first",), doc="at least three nodes share the largest size and N falls among them")
    # four quadrants of 3 spots each in a 60 x 60 region, N = 6: the walk order alone decides which quadrant is split
    q = []
    for k, (ox, oy) in enumerate(((0, 0), (30, 0), (0, 30), (30, 30))):
        q += [(ox + 5, oy + 5, 40 + k), (ox + 20, oy + 8, 50 + k), (ox + 9, oy + 22, 60 + k)]
    add("term_sort_ties_quadrants", spots(92, 92, rel(q)), params(6),
        last_sorted(lambda r: r["top_sizes"][:4] == [3, 3, 3, 3] and r["split"] == 1 and r["broke"]), kills=("sort_tie_oldest_first", "no_break"))

    # ================= best per node =================
    # 152 x 122, N = 1: one node (120 / 90 -> nIni 1), one full pass, quadrants of 60 x 45 over cells of 30 x 30
    pts = [(10, 20, 50), (40, 10, 50), (20, 8, 30),      # UL: equal maxima in cell (0,0) and, higher up in the image, cell (0,1)
           (80, 25, 50), (70, 35, 50), (100, 5, 25),     # UR: equal maxima in cell rows 0 and 1
           (10, 60, 50), (20, 60, 50), (5, 70, 22),      # BL: a tie inside one cell
           (100, 50, 50), (70, 60, 30), (110, 80, 25)]   # BR: the maximum first
    add("best_ties_across_cells", spots(152, 122, rel(pts)), params(1),
        all_of(n_kps(4), lambda m: all(ties >= 2 for pos, n, ties in _t(m)["best_pos"][1:])), kills=("best_ge", "best_tie_raster"),
        doc="the earlier cell's spot wins even when the other is above it in the image")
    pts = [(10, 10, 30), (20, 20, 25), (25, 5, 50),        # maximum first (raster order inside cell (0,0): y = 5 comes first)
           (70, 5, 25), (80, 20, 50), (100, 30, 30),       # middle
           (10, 50, 25), (20, 60, 30), (30, 80, 50),       # last
           (100, 70, 33)]
    add("best_first_middle_last", spots(152, 122, rel(pts)), params(1),
        lambda m: sorted(p for p, n, t in _t(m)["best_pos"] if n == 3) == [0, 1, 2])

    # ================= kernel sizes =================
    for n in (1, 2, 255, 256, 257, 1023, 1024, 1025):
        add("cand_%d_all_kept" % n, lattice(200, 200, n, 100 + n), params(1500), all_of(n_cand(n), n_kps(n)),
            doc="%d candidates, each ends in a node of its own: the final list holds exactly %d" % (n, n))
    for n in (4095, 4096, 4097):
        add("cand_%d" % n, lattice(320, 300, n, 100 + n), params(1024), all_of(n_cand(n), lambda m: 1024 <= len(m["kps"]) <= 1026))
    for N in (255, 256, 257):
        add("n_%d" % N, lattice(200, 200, 1025, 1125), params(N), lambda m, N=N: N <= len(m["kps"]) <= N + 2)
    for N in (1023, 1025):
        add("n_%d" % N, lattice(320, 300, 4097, 4197), params(N), lambda m, N=N: N <= len(m["kps"]) <= N + 2)
    add("n_at_plan_limit", lattice(320, 300, 4097, 4197), params(octree_max_nfeatures(320, 300)), lambda m: len(m["kps"]) >= 2666,
        doc="the largest nfeatures the LDS quadtree accepts for one level of this size")

    # ================= above level 0 =================
    crop = synth.synth_image(5, 640, 480)[150:270, 220:380].copy()
    add("levels_3", crop, params(200, nlevels=3), lambda m: all(t["keypoints"] > 0 for t in m["trace"]), kills=("scale_missing",))
    add("levels_8", synth.synth_image(6, 640, 480)[150:270, 220:380].copy(), params(300, nlevels=8),
        lambda m: sum(t["keypoints"] > 0 for t in m["trace"]) >= 4, kills=("scale_missing",))
    add("middle_level_empty", cone_image(), params(50, nlevels=3, scale=1.5),
        lambda m: [t["keypoints"] > 0 for t in m["trace"]] == [True, False, True], kills=("scale_missing",),
        doc="a faint one-pixel spot (gone after one resize) and a shallow cone that becomes a corner only at scale 2.25")
    return out


def octree_max_nfeatures(w, h):
    """The largest one-level nfeatures whose quadtree lists fit k_octree's 160 KiB - 512 B of LDS (csrc/orb_plan.h: 61 B per
    node slot + 16, N + 11 slots when 4 nIni < N); asserted against the library by test_orb_cases_gpu.py (this one is accepted,
    one more is refused)."""
    return (160 * 1024 - 512 - 16) // 61 - 11


def cone_image():
    """200 x 160: level sizes 200x160, 133x107, 89x71 at scale 1.5.  A spot of height 8 at (60, 60) is a corner at minThFAST = 7
    on level 0 only; a cone of slope 1.3 / px around (100, 80) differs from its ring by 3.9 on level 0, 5.9 on level 1 and 8.8
    on level 2."""
    yy, xx = np.mgrid[0:160, 0:200]
    r = np.hypot(xx - 100.0, yy - 80.0)
    img = (BASE + np.maximum(0.0, 40.0 - 1.3 * r)).astype(np.uint8)
    img[60, 60] = BASE + 8
    return img


# ---- batches for the device entry point: equally sized images under one parameter set, an empty image between full ones ----
def batches():
    flat = lambda w, h: np.full((h, w), BASE, np.uint8)
    return [
        ("batch_320x300_n1024", params(1024), [by_name("cand_4097").img, flat(320, 300), by_name("cand_4095").img, lattice(320, 300, 1, 7),
                                                 lattice(320, 300, 2, 8), by_name("cand_4096").img, flat(320, 300), lattice(320, 300, 1025, 9)]),
        ("batch_152x122_n10", params(10), [by_name("term_break_all_but_one").img, flat(152, 122), by_name("grid_seams").img,
                                            by_name("best_ties_across_cells").img, by_name("thresholds_20_7").img]),
        ("batch_160x120_l8", params(300, nlevels=8), [by_name("levels_8").img, flat(160, 120), by_name("levels_3").img]),
    ]


# ---- the two sides' levels and the model on them ----
def oracle_levels(p, img):
    import oracle_lib as O
    pyr = [O.orb_level(p, img, l) for l in range(p.nlevels)]
    blur = []
    for lv in pyr:
        b = np.zeros_like(lv)
        O.lib().orc_gaussian_blur7(C.c_void_p(lv.ctypes.data), lv.shape[1], lv.shape[0], C.c_void_p(b.ctypes.data))
        blur.append(b)
    return pyr, blur


_MODEL = {}


def model_on_oracle_levels(p, img, variant=None, key=None):
    """orb_ref.extract on the oracle's pyramid; computed once per (case, variant) and shared."""
    k = (key, variant)
    if key is None or k not in _MODEL:
        pyr, blur = oracle_levels(p, img)
        m = R.extract(p, pyr, blur, variant)
        if key is None:
            return m
        _MODEL[k] = m
    return _MODEL[k]


def same_keypoints(a, b):
    return (len(a["kps"]) == len(b["kps"]) and a["kps"].tobytes() == b["kps"].tobytes() and a["desc"].tobytes() == b["desc"].tobytes())
