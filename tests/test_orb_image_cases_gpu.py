"""GPU: the constructed resize / blur cases through fb_orb_extract_batch_dev.  Every pyramid level and every blurred level
equals the numpy model (tests/orb_image_ref.py), the resize kernel that ran is the declared one
(fb_orb_debug_resize_route), and one image handed over in five layouts -- aligned, from an odd pointer, with odd strides, as
the second image of a batch with an odd image stride, with 64 bytes of row padding; padding 0x00 and 0xFF -- gives
byte-equal levels, blurred levels, key points and descriptors."""
import numpy as np
import pytest

import hip_lib as H
import oracle_lib as O
import orb_image_cases as IC
import orb_image_ref as R

pytestmark = pytest.mark.gpu


def run(case, fill=None):
    """[(levels, blurred levels or None, key points, descriptors)] per image, and the routes of the levels >= 1."""
    orb = H.Orb(O.orb_params(**case.params()))
    try:
        out = orb.extract_batch_dev(case.buffer(fill), case.B, case.w, case.h, case.stride, case.image_stride, case.offset)
        routes = tuple(orb.resize_route(l) for l in range(1, case.nlevels))
        res = []
        for b in range(case.B):
            lv = [orb.level(b, l, case.w * case.h) for l in range(case.nlevels)]
            bl = [orb.blurred_level(b, l) if case.blurred[l] else None for l in range(case.nlevels)]
            res.append((lv, bl, out[b][0], out[b][1]))
        return res, routes
    finally:
        orb.close()


def check_against_model(case, res, routes):
    assert routes == tuple(R.ROUTE_ID[r] for r in case.routes), (case.name, routes, case.routes)
    for b in range(case.B):
        sizes, lv, bl = IC.model(case, b)
        for l in range(case.nlevels):
            assert res[b][0][l].shape == (sizes[l][1], sizes[l][0]), (case.name, l)
            np.testing.assert_array_equal(res[b][0][l], lv[l], err_msg="%s image %d level %d" % (case.name, b, l))
            if case.blurred[l]:
                np.testing.assert_array_equal(res[b][1][l], bl[l], err_msg="%s image %d blurred level %d" % (case.name, b, l))


def assert_same(a, b, what):
    for l, (x, y) in enumerate(zip(a[0], b[0])):
        np.testing.assert_array_equal(x, y, err_msg="%s level %d" % (what, l))
    for l, (x, y) in enumerate(zip(a[1], b[1])):
        if x is not None:
            np.testing.assert_array_equal(x, y, err_msg="%s blurred level %d" % (what, l))
    assert a[2].tobytes() == b[2].tobytes(), what + " key points"
    assert a[3].tobytes() == b[3].tobytes(), what + " descriptors"


@pytest.mark.parametrize("family", [f for f in IC.FAMILIES if f != "align"])
def test_levels_blur_and_route_equal_the_model(family):
    for case in IC.CASES:
        if case.family != family:
            continue
        res, routes = run(case)
        check_against_model(case, res, routes)
        if case.padded:  # the other poison: no padding byte may reach a pixel, a key point or a descriptor
            other, routes2 = run(case, 0xFF - case.fill)
            assert routes2 == routes
            for b in range(case.B):
                assert_same(res[b], other[b], "%s image %d, padding 0x%02x / 0x%02x" % (case.name, b, case.fill, 0xFF - case.fill))


def test_constant_images_blur_to_the_literal_answers():
    for v, want in IC.CONST_BLUR.items():
        res, _ = run(IC.BY_NAME["const_%d" % v])
        for l in range(2):
            assert (res[0][0][l] == v).all() and (res[0][1][l] == want).all(), (v, l)


@pytest.mark.parametrize("group", ["align_m", "align_r", "align_g"])
def test_one_image_in_five_layouts(group):
    cases = [c for c in IC.CASES if c.group == group]
    base = None
    nkp = 0
    for case in cases:
        res, routes = run(case)
        check_against_model(case, res, routes)
        mine = res[case.B - 1]          # layout (d) carries the image as the second of a batch of two
        if base is None:
            assert case.name.endswith("_a") and case.aligned
            base, nkp = mine, len(mine[2])
        else:
            assert_same(base, mine, case.name + " against the aligned run")
        # level 1 is built by k_resize from an unaligned source, by the aligned route otherwise; the levels above always by it
        assert routes[0] == (R.ROUTE_ID[cases[0].routes[0]] if case.aligned else 0) and routes[1:] == tuple(R.ROUTE_ID[r] for r in cases[0].routes[1:])
    assert nkp > 20  # k_fast and k_describe saw the same level 0 in every layout, and had something to find


def test_batch_of_three_equals_three_single_calls():
    case = IC.BY_NAME["blur_batch3"]
    res, routes = run(case)
    for b in range(3):
        single = IC.Case.__new__(IC.Case)
        single.__dict__.update(case.__dict__)
        single.imgs, single.B = case.imgs[b:b + 1], 1
        one, r1 = run(single)
        assert r1 == routes
        assert_same(res[b], one[0], "image %d of the batch against its own call" % b)
