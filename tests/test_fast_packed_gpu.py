"""k_fast scores its listed pixels two per lane in trips of 128 (64 when 64 or fewer are left): images whose level-0 cells
list exactly 0, 1, 2, 63, 64, 65, 127, 128, 129, ... pixels, and more than 256, against the CPU oracle, bit-exact.

How the counts are obtained: `listed()` below restates the kernel's necessary test in numpy (a pixel is listed at
threshold T iff max(v - A, B - v) > T with A = max(min(n0, n8), min(n4, n12)), B = min(max(n0, n8), max(n4, n12)) over
the four compass pixels at distance 3), and `cell_counts()` counts it over the interior of every level-0 cell of the
extractor's grid; every test asserts the counts it relies on.  One-pixel spots on a lattice of spacing 2 inside a flat
cell are listed one by one and list nothing else (a compass pixel of a lattice point is never a lattice point)."""
import ctypes as C

import numpy as np
import pytest

import fishbirdeyevisualslam_amd as fb
import hip_lib as H
import oracle_lib as O
from fishbirdeyevisualslam_amd import synth

pytestmark = pytest.mark.gpu
BORDER, INI_TH, MIN_TH = 16, 20, 7
# 4 x 3 cells; the cells of the last column / row are 6 px narrower and hold fewer lattice points (130 / 100)
COUNTS = [63, 64, 65, 127,
          128, 129, 160, 126,
          0, 1, 66, 2]


def params(**kw):
    """The thresholds the counts of this file are computed at, passed explicitly (the package default is 15 / 5)."""
    return O.orb_params(ini_th_fast=INI_TH, min_th_fast=MIN_TH, **kw)


def redone_cells_hold_low_responses(c, w, h, counts):
    """Evidence that the redo pass, not the first pass, produced the candidates of the large cells: every cell with 63 or
    more spots holds candidates whose response lies below 15 (a first pass at any threshold >= 15 finds none of them)."""
    for k, (x0, y0, x1, y1) in enumerate(interiors(w, h)):
        if counts[k] >= 63:
            r = c[(c[:, 0] >= x0) & (c[:, 0] < x1) & (c[:, 1] >= y0) & (c[:, 1] < y1), 2]
            assert len(r) > 0 and r.min() < 15, (k, counts[k], len(r))


def grid(w, h):
    """Level-0 cell grid of ComputeKeyPointsOctTree: (nCols, nRows, wCell, hCell)."""
    width, height = w - 2 * BORDER, h - 2 * BORDER
    nc, nr = int(width / 30), int(height / 30)
    return nc, nr, -(-width // nc), -(-height // nr)


def interiors(w, h):
    """(x0, y0, x1, y1) of the pixels each level-0 cell tests (its window minus the 3-px rim), row-major."""
    nc, nr, wc, hc = grid(w, h)
    return [(BORDER + j * wc + 3, BORDER + i * hc + 3, min(BORDER + j * wc + wc + 6, w - BORDER) - 3, min(BORDER + i * hc + hc + 6, h - BORDER) - 3)
            for i in range(nr) for j in range(nc)]


def listed(img, T):
    v = img.astype(np.int32)
    c = v[3:-3, 3:-3]
    n0, n8, n4, n12 = v[6:, 3:-3], v[:-6, 3:-3], v[3:-3, 6:], v[3:-3, :-6]
    A = np.maximum(np.minimum(n0, n8), np.minimum(n4, n12))
    B = np.minimum(np.maximum(n0, n8), np.maximum(n4, n12))
    out = np.zeros(img.shape, bool)
    out[3:-3, 3:-3] = np.maximum(c - A, B - c) > T
    return out


def cell_counts(img, T):
    m = listed(img, T)
    return [int(m[y0:y1, x0:x1].sum()) for x0, y0, x1, y1 in interiors(img.shape[1], img.shape[0])]


def spots_image(w, h, counts, lo, hi, seed, noise_cells=()):
    """Flat image (100) with counts[k] one-pixel spots of height lo..hi in cell k (lattice of spacing 2, random positions);
    cells in noise_cells are filled with black / white noise instead."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 100, np.uint8)
    cells = interiors(w, h)
    assert len(counts) == len(cells)
    for k, (n, (x0, y0, x1, y1)) in enumerate(zip(counts, cells)):
        if k in noise_cells:
            img[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = rng.choice(np.array([0, 255], np.uint8), (y1 - y0 - 2, x1 - x0 - 2))
            continue
        # lattice points at least 2 px inside the interior: the spots of neighbouring cells stay out of one another's rings
        pts = [(x, y) for y in range(y0 + 2, y1 - 2, 2) for x in range(x0 + 2, x1 - 2, 2)]
        assert n <= len(pts), (k, n, len(pts))
        for q in rng.permutation(len(pts))[:n]:
            img[pts[q][1], pts[q][0]] = 100 + rng.integers(lo, hi + 1)
    return img


def check_image(params, img):
    """Level-0 candidate set, key points and descriptors against the oracle; returns the oracle's level-0 candidates."""
    orb = H.Orb(params)
    try:
        k_h, d_h = orb.extract(img)
        buf = np.zeros(400000, np.uint32)
        n = fb.lib().fb_orb_debug_candidates(orb.h, 0, 0, C.c_void_p(buf.ctypes.data), len(buf))
        assert 0 <= n <= len(buf)
        r = buf[:n]
        c_h = np.stack([r & 0xFFF, (r >> 12) & 0xFFF, r >> 24], 1).astype(np.int32)
        c_o = O.orb_candidates(params, img, 0)
        np.testing.assert_array_equal(c_h[np.lexsort((c_h[:, 0], c_h[:, 1]))], c_o[np.lexsort((c_o[:, 0], c_o[:, 1]))],
                                      err_msg="FAST candidates, level 0")
        k_o, d_o = O.orb_extract(params, img)
        assert len(k_h) == len(k_o)
        for f in ("octave", "x", "y", "response", "size", "angle"):
            np.testing.assert_array_equal(k_h[f], k_o[f], err_msg=f)
        np.testing.assert_array_equal(d_h, d_o)
        return c_o
    finally:
        orb.close()


@pytest.mark.parametrize("nlevels", [1, 8])
def test_trip_boundaries_at_ini_threshold(nlevels):
    """152x122: 4x3 cells of 30x30 (44-byte tile pitch when level 0 is the only level); cell k lists exactly COUNTS[k]
    pixels at iniThFAST."""
    assert grid(152, 122) == (4, 3, 30, 30)
    img = spots_image(152, 122, COUNTS, 30, 150, seed=1)
    assert cell_counts(img, INI_TH) == COUNTS
    c = check_image(params(nfeatures=1500 if nlevels == 1 else 3000, nlevels=nlevels), img)
    assert 0 < len(c) <= sum(COUNTS)  # a spot with spots on its ring (lattice diagonals) may be listed and still be no corner


def test_trip_boundaries_of_the_redo_pass():
    """The same counts with spots of height 9..20: nothing is listed at iniThFAST (strength <= 20), every cell is redone at
    minThFAST and scores list B only."""
    img = spots_image(152, 122, COUNTS, 9, 20, seed=2)
    assert cell_counts(img, INI_TH) == [0] * 12 and cell_counts(img, MIN_TH) == COUNTS
    c = check_image(params(nfeatures=1500, nlevels=1), img)
    assert 0 < len(c) <= sum(COUNTS) and c[:, 2].max() < INI_TH
    redone_cells_hold_low_responses(c, 152, 122, COUNTS)


def test_redo_pass_with_both_lists():
    """A diagonal step edge (+60 where x + y > 150) across the spots of height 9..20: the pixels along the edge pass the
    necessary test at iniThFAST (list A) but only 7 contiguous ring pixels differ, so they are no corners; the cells
    the edge crosses are redone with list A (already scored) and list B (scored in the redo pass) both non-empty."""
    img = spots_image(152, 122, COUNTS, 9, 20, seed=3).astype(np.int32)
    yy, xx = np.mgrid[0:122, 0:152]
    s = xx + yy - 150
    img[np.abs(s) <= 6] = 100        # no spots near the edge
    img[s > 0] += 60
    img = img.astype(np.uint8)
    a, b = cell_counts(img, INI_TH), cell_counts(img, MIN_TH)
    crossed = [k for k in range(12) if a[k] > 0]
    assert len(crossed) >= 4 and all(b[k] > a[k] for k in crossed if COUNTS[k] >= 63)
    c = check_image(params(nfeatures=1500, nlevels=1), img)
    assert len(c) > 100 and c[:, 2].max() < INI_TH   # no cell kept a corner at iniThFAST
    redone_cells_hold_low_responses(c, 152, 122, COUNTS)


def test_more_than_256_listed_pixels():
    """Cells of black / white noise beside spot cells: several hundred listed pixels per cell (three and more packed trips),
    dense score neighbourhoods for the NMS."""
    noise = (0, 5, 10)
    img = spots_image(152, 122, COUNTS, 30, 150, seed=4, noise_cells=noise)
    got = cell_counts(img, INI_TH)
    assert min(got[k] for k in noise) > 256, got
    check_image(params(nfeatures=1500, nlevels=1), img)
    check_image(params(nfeatures=3000), img)


@pytest.mark.parametrize("w,h,pitch,counts", [
    (120, 120, 56, [64, 65, 128, 129]),    # 2 x 2 cells of 44 x 44
    (91, 91, 72, [129]),                   # one cell of 59 x 59
    (91, 150, 72, [65, 128, 300]),         # 1 x 3 cells of 59 x 40
])
def test_wide_cells(w, h, pitch, counts):
    """The 56- and 72-byte-pitch instantiations (cells wider than 32 px; level 0 is the only level, so it alone decides
    the pitch: the smallest of 44 / 56 / 72 that holds (wCell + 12) & ~3 bytes)."""
    wc = grid(w, h)[2]
    assert (44 if pitch == 56 else 56) < ((wc + 12) & ~3) <= pitch
    img = spots_image(w, h, counts, 30, 150, seed=5)
    assert cell_counts(img, INI_TH) == counts
    c = check_image(params(nfeatures=1500, nlevels=1), img)
    assert 0 < len(c) <= sum(counts)
    img2 = spots_image(w, h, counts, 9, 20, seed=6)  # and through the redo pass
    assert cell_counts(img2, MIN_TH) == counts and sum(cell_counts(img2, INI_TH)) == 0
    c = check_image(params(nfeatures=1500, nlevels=1), img2)
    assert 0 < len(c) <= sum(counts)
    redone_cells_hold_low_responses(c, w, h, counts)


def test_scene_crop_with_wide_cells():
    """A crop of a synthetic scene, 209 x 91 at one level: 5 x 1 cells of 36 x 59 (56-byte pitch, tall cells)."""
    img = synth.synth_image(1000, 640, 480)[100:191, 200:409].copy()
    assert grid(209, 91) == (5, 1, 36, 59)
    check_image(params(nfeatures=1500, nlevels=1), img)
