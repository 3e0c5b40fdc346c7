"""Known answers for the literal model of fb_orb_detect (tests/orb_detect_ref.py), on the CPU: the model is the contract the
kernels are held to bit for bit (tests/test_orb_detect_gpu.py), so what it says is pinned here by hand-derived values."""
import numpy as np
import pytest

import describe_at_ref as D
import orb_detect_cases as K
import orb_detect_ref as R
from orb_image_ref import level_sizes, resize_linear_u8

f32 = np.float32


def square(w=K.W, h=K.H, x0=70, y0=60, x1=119, y1=99, corner=230):
    """A bright rectangle [x0, x1] x [y0, y1] on a dark ground; its four corner pixels are brighter still, which makes each
    the strict maximum of its neighbourhood (on a plain rectangle the corner shares its score with two neighbours)."""
    img = np.full((h, w), 40, np.uint8)
    img[max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] = 200
    if corner:
        for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
            if 0 <= x < w and 0 <= y < h:
                img[y, x] = corner
    return img


def test_harris_on_a_flat_patch_and_on_a_vertical_step_edge():
    flat = np.full((40, 40), 123, np.uint8)
    assert R.harris_abc(flat, 20, 20) == (0, 0, 0)
    assert R.harris(flat, 20, 20) == 0 and not np.signbit(R.harris(flat, 20, 20))
    # a step of height d between the columns 19 and 20: the Sobel x-derivative is 4 d in those two columns and 0 elsewhere,
    # Iy = 0 everywhere.  A block centred on column 20 holds both columns, 7 rows each: a = 14 (4 d)^2.
    d = 100
    edge = np.full((40, 40), 50, np.uint8)
    edge[:, 20:] = 50 + d
    a = 14 * (4 * d) ** 2
    assert R.harris_abc(edge, 20, 20) == (a, 0, 0) and R.harris_abc(edge, 19, 20) == (a, 0, 0)
    assert R.harris_abc(edge, 23, 20) == (a // 2, 0, 0) and R.harris_abc(edge, 24, 20) == (0, 0, 0)
    s = f32(f32(1.0) / f32(7140.0))
    s4 = f32(f32(f32(s * s) * s) * s)
    want = f32(f32(f32(0.0) - f32(f32(f32(0.04) * f32(a)) * f32(a))) * s4)      # -k a^2 s4
    got = R.harris(edge, 20, 20)
    assert got < 0 and got.view(np.uint32) == want.view(np.uint32)
    assert abs(float(got) + 0.04 * a * a / 7140.0 ** 4) < 1e-9


def test_a_bright_square_yields_its_four_corners_and_nothing_else():
    p = K.cabi.OrbParams(2000, K.SCALE, 1, 15, 5)            # level 0 alone
    r = R.detect(p, square(), None, 20)
    assert r.per_level == [(4, 4, 4)]
    got = sorted((int(k["x"]), int(k["y"])) for k in r.kps[r.kps["octave"] == 0])
    assert got == [(70, 60), (70, 99), (119, 60), (119, 99)]
    assert (r.kps["response"] > 0).all() and (r.kps["size"] == 31).all()
    # the order is raster order, and the angle points from the corner into the square (the bright mass)
    assert [(int(k["x"]), int(k["y"])) for k in r.kps] == [(70, 60), (119, 60), (70, 99), (119, 99)]
    ang = r.kps["angle"]
    assert 0 < ang[0] < 90 and 90 < ang[1] < 180 and 270 < ang[2] < 360 and 180 < ang[3] < 270
    # without the brighter corner pixels every corner ties with two neighbours, and equal neighbours drop each other
    plain = square(corner=0)
    s = R.fast_scores(plain, 20)
    assert s[60, 70] > 0 and s[60, 70] == s[60, 71] == s[61, 70]
    assert not R.suppress(s).any()


def test_retain_best_keeps_every_tie_at_the_cut():
    assert list(R.retain_best([5, 3, 3, 3, 1], 2)) == [0, 1, 2, 3]
    assert list(R.retain_best([5, 3, 3, 3, 1], 1)) == [0]
    assert list(R.retain_best([5, 3, 3, 3, 1], 5)) == [0, 1, 2, 3, 4]
    assert list(R.retain_best([1, 2, 3], 0)) == []
    assert list(R.retain_best(np.array([0.0, -1.0, -0.0, 2.0], f32), 2)) == [0, 2, 3]     # -0.0 equals 0.0
    # in the detector: the tie scene keeps more than K in both stages of level 0, and the kept responses are one value
    r = K.model(K.tie_image())
    cand, n1, n2 = r.per_level[0]
    N = K.N_PER_LEVEL[0]
    assert cand > n1 > 2 * N and n2 > N
    resp0 = r.kps["response"][r.kps["octave"] == 0]
    assert len(resp0) == n2 and len(np.unique(resp0)) < n2
    assert len(r.kps) > K.NFEATURES


def test_three_situations_in_the_main_scene():
    for img in K.images():
        r = K.model(img)
        assert K.situations(r.per_level, K.N_PER_LEVEL) == {"both", "second", "none"}
        for (cand, n1, n2), N, l in zip(r.per_level, K.N_PER_LEVEL, range(K.NLEVELS)):
            assert n2 == (r.kps["octave"] == l).sum() and n1 >= min(cand, 2 * N) and n2 >= min(n1, N)
        # level-major, raster order within a level
        o = r.kps["octave"]
        assert (np.diff(o) >= 0).all()
        inv = D.inv_scale_factors(K.SCALE, K.NLEVELS)
        for l in range(K.NLEVELS):
            k = r.kps[o == l]
            px, py = np.rint(k["x"] * inv[l]).astype(int), np.rint(k["y"] * inv[l]).astype(int)
            key = py * 4096 + px
            assert (np.diff(key) > 0).all()


def test_mask_chain_254_passes_level_0_only_and_the_edge_of_255_erodes():
    sizes = level_sizes(K.W, K.H, K.SCALE, K.NLEVELS)
    m = R.mask_levels(K.mask_254(), sizes)
    assert (m[0] == 254).all() and not m[1].any() and not m[2].any()
    for img in K.images():
        free, masked = K.model(img), K.model(img, K.mask_254())
        assert masked.per_level[0][0] == free.per_level[0][0] and masked.per_level[1] == masked.per_level[2] == (0, 0, 0)
    pm = K.patch_mask()
    lv = R.mask_levels(pm, sizes)
    for l in (1, 2):
        assert set(np.unique(lv[l])) == {0, 255}
    plain = resize_linear_u8(pm, *sizes[1])[0]
    assert ((lv[1] == 255) == (plain == 255)).all()
    assert (plain > 0).sum() > (lv[1] > 0).sum()          # interpolated edge values, the 1-band and the 254-block are gone
    # level 2 comes from the thresholded level 1
    chained = resize_linear_u8(lv[1], *sizes[2])[0]
    assert ((chained > 254) == (lv[2] == 255)).all()
    # the 255 region loses its rim: pixels that interpolate between 255 and less are nonzero in a plain resize and 0 here,
    # and some of them touch the 255 region that stays
    rim = (plain > 0) & (plain < 255)
    assert rim.any() and not lv[1][rim].any()
    grown = np.zeros_like(rim)
    full = lv[1] == 255
    grown[1:, :] |= full[:-1, :]; grown[:-1, :] |= full[1:, :]; grown[:, 1:] |= full[:, :-1]; grown[:, :-1] |= full[:, 1:]
    assert (rim & grown).any()
    # and the detector uses them: no key point of level 0 where the mask is 0, none above level 0 where it is not 255
    for img in K.images():
        r = K.model(img, pm)
        inv = D.inv_scale_factors(K.SCALE, K.NLEVELS)
        for k in r.kps:
            l = int(k["octave"])
            px, py = int(np.rint(k["x"] * inv[l])), int(np.rint(k["y"] * inv[l]))
            assert lv[l][py, px] != 0


@pytest.mark.parametrize("axis", ["x", "y"])
def test_border_31(axis):
    """The corner of a square placed at 30 | 31 | size - 32 | size - 31 along one axis: kept from 31 to size - 32."""
    w, h = K.W, K.H
    size = w if axis == "x" else h
    for at, kept in ((30, False), (31, True), (size - 32, True), (size - 31, False)):
        if axis == "x":
            img = square(x0=at, y0=60, x1=at + 200, y1=400, corner=230) if at < size // 2 else square(x0=-200, y0=60, x1=at, y1=400, corner=0)
            if at >= size // 2:
                img[60, at] = 230
            want = (at, 60)
        else:
            img = square(x0=70, y0=at, x1=400, y1=at + 200, corner=230) if at < size // 2 else square(x0=70, y0=-200, x1=400, y1=at, corner=0)
            if at >= size // 2:
                img[at, 70] = 230
            want = (70, at)
        keep = R.suppress(R.fast_scores(img, 20))
        assert keep[want[1], want[0]]                      # a FAST survivor either way
        pos, _, _ = R.detect_level(img, None, 20, 1000)
        assert (want in pos) == kept, (axis, at, pos)


def test_a_level_of_at_most_62_px_is_empty():
    g = np.random.Generator(np.random.PCG64(5))
    for w, h, any_kp in ((62, 120, False), (120, 62, False), (63, 120, True)):
        img = g.integers(0, 256, (h, w)).astype(np.uint8)
        pos, _, counts = R.detect_level(img, None, 20, 1000)
        assert (len(pos) > 0) == any_kp
        assert all(px == 31 for px, _ in pos)
    # in a pyramid: the last level of a 100 x 80 image is 69 x 56
    p = K.cabi.OrbParams(500, K.SCALE, 3, 15, 5)
    img = g.integers(0, 256, (80, 100)).astype(np.uint8)
    r = R.detect(p, img)
    assert r.per_level[2] == (0, 0, 0) and r.per_level[0][0] > 0 and r.per_level[1][0] > 0


def test_both_size_rules_agree_and_the_round_trip_lands_on_the_pixel():
    for w, h, nl in ((K.W, K.H, K.NLEVELS), (384, 384, 8), (157, 160, 3)):
        assert R.cv_orb_level_sizes(w, h, K.SCALE, nl) == level_sizes(w, h, K.SCALE, nl)
        assert R.round_trip_ok(w, h, K.SCALE, nl)


def test_features_per_level_is_the_extractors_table():
    from orb_ref import Extractor
    for nf, nl in ((K.NFEATURES, K.NLEVELS), (2000, 8), (1000, 8)):
        e = Extractor(nf, K.SCALE, nl, 15, 5)
        assert list(e.mnFeaturesPerLevel) == R.features_per_level(nf, K.SCALE, nl)


def test_describe_at_accepts_every_detected_key_point():
    p = K.params()
    for img in K.images():
        pyr, blur = D.levels(img, p)
        kps = K.model(img).kps
        assert len(kps) > 30
        desc, angle, status = D.describe_at(p, pyr, blur, kps, D.KEEP_ANGLE)
        assert (status == D.OK).all() and desc.any(axis=1).all()
        # IC mode recomputes the angle the detector gave
        _, angle_ic, _ = D.describe_at(p, pyr, blur, kps, D.IC_ANGLE)
        assert angle_ic.view(np.uint32).tolist() == kps["angle"].view(np.uint32).tolist()
