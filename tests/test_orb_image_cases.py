"""CPU: the constructed resize / blur cases (tests/orb_image_cases.py) against the numpy model (tests/orb_image_ref.py) and
the oracle: oracle == model bit for bit on every level and every blurred level, every named wrong reading is told from the
model by the cases that name it, the hand-derivable answers hold, and the declared resize routes are the model's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import orb_image_cases as IC
import orb_image_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
model = IC.model


def differs(a, b):
    if a[0] != b[0]:
        return True
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        if (x is None) != (y is None) or (x is not None and not np.array_equal(x, y)):
            return True
    return False


@pytest.mark.parametrize("family", IC.FAMILIES)
def test_oracle_equals_model(family):
    for c in IC.CASES:
        if c.family != family or (c.group and not c.name.endswith("_a")):
            continue  # the other runs of an alignment group hold the same image in another layout
        p = O.orb_params(**c.params())
        for b in range(c.B):
            sizes, lv, bl = model(c, b)
            for l in range(c.nlevels):
                lo = O.orb_level(p, c.imgs[b], l)
                assert lo.shape == (sizes[l][1], sizes[l][0]), (c.name, l, lo.shape, sizes[l])
                np.testing.assert_array_equal(lo, lv[l], err_msg="%s level %d" % (c.name, l))
                assert c.blurred[l] == (bl[l] is not None), (c.name, l)
                if bl[l] is None:
                    continue
                bo = np.zeros_like(lo)
                O.lib().orc_gaussian_blur7(C.c_void_p(lo.ctypes.data), lo.shape[1], lo.shape[0], C.c_void_p(bo.ctypes.data))
                np.testing.assert_array_equal(bo, bl[l], err_msg="%s blurred level %d" % (c.name, l))


def test_every_variant_is_killed_by_the_cases_that_name_it():
    named = {v: [] for v in R.VARIANTS}
    for c in IC.CASES:
        for v in c.kills:
            assert v in R.VARIANTS, (c.name, v)
            assert differs(model(c), model(c, 0, v)), "%s does not tell %s from the model" % (c.name, v)
            named[v].append(c.name)
    assert all(named.values()), [v for v, n in named.items() if not n]


def test_inseparable_variants_change_no_case():
    for v in R.INSEPARABLE:
        for c in IC.CASES:
            for b in range(c.B):
                assert not differs(model(c, b), model(c, b, v)), (c.name, v)


def test_border_rules_cannot_fire_when_shrinking():
    """The reason the border readings are inseparable (orb_image_ref docstring), checked over every size pair up to 140:
    the first index is >= 0, and the second tap leaves the image only with weight 0."""
    for sn in range(1, 141):
        for dn in range(1, sn + 1):
            s, w0, w1 = R.axis_table(sn, dn, None, None, False)
            assert s.min() >= 0 and ((s + 1 <= sn - 1) | (w1 == 0)).all(), (sn, dn)


def test_literal_known_answers():
    assert [R.blur_of_constant(v) for v in (0, 100, 253, 254, 255)] == [0, 101, 255, 255, 255]
    assert (253 * 66049 + 32768) >> 16 == 255 and (254 * 66049 + 32768) >> 16 == 256 and (255 * 66049 + 32768) >> 16 == 257
    assert 255 * 257 == 65535  # the horizontal sum of a saturated row is the largest 16-bit value
    for v, want in IC.CONST_BLUR.items():
        sizes, lv, bl = model(IC.BY_NAME["const_%d" % v])
        assert sizes == [(64, 48), (53, 40)]
        for l in range(2):
            assert (lv[l] == v).all() and (bl[l] == want).all(), (v, l)
    _, lv, bl = model(IC.BY_NAME["const_255_260x45"])
    assert (lv[1] == 255).all() and (bl[0] == 255).all() and (bl[1] == 255).all()
    # an impulse of 255 in a corner: REFLECT_101 never repeats the edge pixel itself, so pixel (y, x) near the corner sees
    # the impulse exactly once, with weight k[3 - y] * k[3 - x]
    _, lv, bl = model(IC.BY_NAME["impulse_corners"])
    assert bl[0][0, 0] == (255 * 55 * 55 + 32768) >> 16 == 12
    assert bl[0][0, 1] == (255 * 55 * 49 + 32768) >> 16 == 10 and bl[0][1, 1] == (255 * 49 * 49 + 32768) >> 16 == 9
    assert bl[0][0, 3] == (255 * 55 * 18 + 32768) >> 16 == 4 and bl[0][0, 4] == 0
    # a one-pixel vertical stripe pattern 0,255,0,...: interior columns take 255 * (34 + 55 + 34) or 255 * (18 + 49 + 49 + 18)
    _, lv, bl = model(IC.BY_NAME["stripes_v"])
    assert bl[0][20, 21] == (255 * 123 * 257 + 32768) >> 16 == 123 and bl[0][20, 20] == (255 * 134 * 257 + 32768) >> 16 == 134
    # column 0 (value 0) under REFLECT_101 sees 255 at -3, -1, 1, 3: the same 134; BORDER_REFLECT would see 0,255,0 | 0,255,0,255
    assert bl[0][20, 0] == 134 and R.gaussian_blur7(lv[0], "border_reflect")[20, 0] != 134
    # level sizes of the default pyramid (DESIGN: 640x480 -> 533x400 ... 179x134) and a half-to-even tie
    assert R.level_sizes(640, 480, 1.2, 8)[1] == (533, 400) and R.level_sizes(640, 480, 1.2, 8)[7] == (179, 134)
    assert R.level_sizes(100, 80, 2.0, 7) == [(100, 80), (50, 40), (25, 20), (12, 10), (6, 5), (3, 2), (2, 1)]  # 12.5 -> 12, 2.5 -> 2


def test_declared_routes_are_the_models():
    for c in IC.CASES:
        sizes = R.level_sizes(c.w, c.h, c.scale, c.nlevels)
        got = tuple(R.resize_route(*sizes[l - 1], *sizes[l], c.aligned if l == 1 else True) for l in range(1, c.nlevels))
        assert got == c.routes, (c.name, got, c.routes)
        assert tuple(R.blurred_by_plan(*s) for s in sizes) == c.blurred, c.name
        assert c.w <= 520 and c.w >= 45 and c.h >= 45
    # the hand-over is not a function of the scale factor alone
    assert IC.ROUTES["route_131x77_1.25"] == IC.ROUTES["route_131x77_1.26"] == ("merge", "merge")
    assert IC.ROUTES["route_131x77_1.3"] == IC.ROUTES["route_131x77_2.01"] == ("rows", "rows")
    assert IC.ROUTES["route_131x77_2.5"] == ("generic", "generic") and IC.ROUTES["route_128x96_1.3334"] == ("merge",)


def test_cases_reach_every_route_height_and_width():
    al = {"generic": set(), "rows": set(), "merge": set()}    # route -> (dw, dh) on aligned sources
    unal = set()
    for c in IC.CASES:
        sizes = R.level_sizes(c.w, c.h, c.scale, c.nlevels)
        for l in range(1, c.nlevels):
            if l == 1 and not c.aligned:
                unal.add(c.routes[0])
            else:
                al[c.routes[l - 1]].add(sizes[l])
    assert unal == {"generic"}
    assert {1, 11, 12, 13, 47, 48, 49} <= {s[1] for s in al["merge"]}
    assert {7, 8, 9, 31, 32, 33} <= {s[1] for s in al["rows"]}
    for r in al:
        assert {s[0] % 4 for s in al[r]} == {0, 1, 2, 3}, r
    assert {1, 2, 3} <= {s[0] for r in al for s in al[r]}
    # every alignment group holds the five layouts, the padded ones with both fills
    for g in ("align_m", "align_r", "align_g"):
        names = [c.name[len(g) + 1:] for c in IC.CASES if c.group == g]
        assert sorted(names) == sorted(["a", "b1", "b2", "b3"] + [x + f for f in ("_00", "_ff") for x in ("c133", "c134", "c135", "d", "e")])


def test_plan_table_in_the_cpp_test_is_this_list():
    """tests/cpp/orb_plan_test.cpp carries (w, h, scale, levels) -> rowsOK / mergeOK per level as literals and holds
    orb_plan.h to them; here the same literals are held to the model's restatement (aligned source)."""
    txt = open(os.path.join(ROOT, "tests", "cpp", "orb_plan_test.cpp")).read()
    rows = re.findall(r'\{(\d+), (\d+), ([0-9.]+)f, (\d+), "([grm]*)"\}', txt)
    table = {(int(w), int(h), float(s), int(n)): r for w, h, s, n, r in rows}
    want = {}
    for c in IC.CASES:
        sizes = R.level_sizes(c.w, c.h, c.scale, c.nlevels)
        want[(c.w, c.h, float(c.scale), c.nlevels)] = "".join(R.resize_route(*sizes[l - 1], *sizes[l], True)[0] for l in range(1, c.nlevels))
    assert table == want
