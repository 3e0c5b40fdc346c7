"""The literal model of fb_orb_describe (tests/describe_at_ref.py) pinned on the CPU: fed with the extractor model's own key
points it reproduces the extractor model's descriptors and angles (so the new model hangs on the one fb_orb_extract is
already held to), and its position, border and level rules give the hand-derived answers."""
import numpy as np
import pytest

import describe_at_cases as K
import describe_at_ref as D
import orb_ref as R

f32 = np.float32


@pytest.fixture(scope="module")
def scene():
    p = K.params()
    img = K.image(4100)
    pyr, blur = D.levels(img, p)
    return p, pyr, blur, R.extract(p, pyr, blur)


@pytest.mark.parametrize("mode", [D.KEEP_ANGLE, D.IC_ANGLE])
def test_round_trip_reproduces_the_extractor_model(scene, mode):
    p, pyr, blur, m = scene
    kps = m["kps"].copy()
    assert len(kps) >= 100 and set(kps["octave"]) == {0, 1, 2}
    if mode == D.IC_ANGLE:
        kps["angle"] = -1.0     # IC mode owes nothing to the angle handed in
    desc, angle, status = D.describe_at(p, pyr, blur, kps, mode)
    assert (status == D.OK).all()
    np.testing.assert_array_equal(desc, m["desc"])
    np.testing.assert_array_equal(angle.view(np.uint32), m["kps"]["angle"].view(np.uint32))


def test_position_rounds_the_float_product_half_to_even():
    one = f32(1.0)
    assert D.level_position(20.5, 30.0, one, K.W, K.H) == (20, 30)
    assert D.level_position(21.5, 30.0, one, K.W, K.H) == (22, 30)
    assert D.level_position(30.0, 20.5, one, K.W, K.H) == (30, 20)
    assert D.level_position(30.0, 21.5, one, K.W, K.H) == (30, 22)
    # and through the whole model: the descriptor is the one of the rounded position
    p = K.params()
    pyr, blur = D.levels(K.image(4100), p)
    desc, _, status = D.describe_at(p, pyr, blur, K.keypoints([(20.5, 30.0, 75.0, 0), (21.5, 30.0, 75.0, 0)]), D.KEEP_ANGLE)
    assert (status == D.OK).all()
    np.testing.assert_array_equal(desc[0], D.orb_descriptor(blur[0], 20, 30, 75.0))
    np.testing.assert_array_equal(desc[1], D.orb_descriptor(blur[0], 22, 30, 75.0))
    assert not np.array_equal(desc[0], desc[1])


@pytest.mark.parametrize("mode", [D.KEEP_ANGLE, D.IC_ANGLE])
def test_border_is_the_extractors_own_range_on_every_level(mode):
    p = K.params()
    pyr, blur = D.levels(K.image(4101), p)
    cases = K.border_cases(p)
    assert {r[3] for r, _ in cases} == {0, 2}
    kps = K.keypoints([r for r, _ in cases])
    desc, angle, status = D.describe_at(p, pyr, blur, kps, mode)
    assert list(status) == [s for _, s in cases]
    ok = status == D.OK
    assert ok.sum() == len(cases) // 2 and desc[ok].any(axis=1).all() and not desc[~ok].any()
    np.testing.assert_array_equal(angle[~ok], kps["angle"][~ok])


def test_bad_octaves_and_non_finite_positions_are_refused():
    p = K.params()
    pyr, blur = D.levels(K.image(4101), p)
    cases = K.bad_input_cases(p)
    kps = K.keypoints([r for r, _ in cases])
    for mode in (D.KEEP_ANGLE, D.IC_ANGLE):
        desc, angle, status = D.describe_at(p, pyr, blur, kps, mode)
        assert list(status) == [s for _, s in cases]
        assert list(status).count(D.LEVEL) == 2 and list(status).count(D.BORDER) == 6 and list(status).count(D.OK) == 1
        assert not desc[status != D.OK].any()
        np.testing.assert_array_equal(angle[status != D.OK], kps["angle"][status != D.OK])
