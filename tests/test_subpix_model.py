"""The literal model of fb_corner_subpix (tests/subpix_ref.py) on the CPU: it finds a corner whose position is known in closed
form, every constructed scene takes the branch it is there for, and the order in which the window terms are summed does not
move a point of the test inputs (the measurement behind the GPU tests' tolerance)."""
import numpy as np
import pytest

import fishbirdeyevisualslam_amd as fb
from fishbirdeyevisualslam_amd import cabi

import subpix_ref as R

SCENES5 = R.scenes(5)


def _run(name, half=5, max_iter=40, order="serial"):
    img, pts, want = R.scenes(half)[name]
    return R.corner_subpix(img, pts, (half, half), max_iter, 1e-3, order), pts, want


def test_the_library_declares_the_entry_points():
    lib = fb.lib()
    for s in ("fb_corner_subpix", "fb_corner_subpix_dev", "fb_frame_set_bird_subpix"):
        assert hasattr(lib, s) and s in cabi.EXPORTS
    assert (R.EXIT_EPS, R.EXIT_ITER, R.EXIT_DET, R.EXIT_OUT, R.REVERTED) == (
        cabi.FB_SUBPIX_EXIT_EPS, cabi.FB_SUBPIX_EXIT_ITER, cabi.FB_SUBPIX_EXIT_DET, cabi.FB_SUBPIX_EXIT_OUT, cabi.FB_SUBPIX_REVERTED)


def test_saddle_corner_is_found():
    """I = 128 + 100 tanh((x - x0) / 2) tanh((y - y0) / 2) rounded to u8, corner (30.37, 22.71), starts up to 3 px away in each
    coordinate: every start ends nearer than it began and within 0.03 px of the corner (0.017 px is what the model reaches:
    the u8 rounding of the image, not the iteration, sets it)."""
    r, pts, _ = _run("saddle")
    x0, y0 = R.SADDLE_XY
    assert max(max(abs(p[0] - x0), abs(p[1] - y0)) for p in pts) > 2.8
    for p, q in zip(pts, r.pts):
        d0, d1 = np.hypot(p[0] - x0, p[1] - y0), np.hypot(q[0] - x0, q[1] - y0)
        assert d1 < 0.03 and (d1 < d0 or d0 < 0.03), (p, q, d0, d1)
    assert (r.exit_code == R.EXIT_EPS).all() and (r.iters >= 2).all() and (r.iters < 40).all()


@pytest.mark.parametrize("name", list(SCENES5))
def test_scene_takes_its_branch(name):
    r, pts, want = _run(name)
    assert list(r.exit_code) == list(want), (name, list(r.exit_code))
    start = np.asarray(pts, np.float32)
    if name == "flat":          # det stop in round 0, nothing moved
        assert (r.iters == 0).all() and (r.pts == start).all()
        assert all(m.det_rel == 1.0 for m in r.margins)
    if name == "border":        # the patch really hangs over the border, at the start already
        img = SCENES5[name][0]
        for p in pts:
            assert min(p[0], p[1], R.COLS - 1 - p[0], R.ROWS - 1 - p[1]) < 6
        assert (r.pts != start).any(axis=1).all()
    if name == "ramp":
        out = ((r.pts[:, 0] < 0) | (r.pts[:, 0] >= R.COLS) | (r.pts[:, 1] < 0) | (r.pts[:, 1] >= R.ROWS))
        assert list(out) == [False, False, False, True, True]     # put back / left outside
        assert (np.abs(r.pts[3:] - start[3:]) <= 5).all()
    if name == "drift":
        assert (r.pts == start).all() and r.iters[0] < 40 and r.iters[1] == 40


def test_iteration_cap():
    r, pts, _ = _run("saddle", max_iter=1)
    assert (r.exit_code == R.EXIT_ITER).all() and (r.iters == 1).all()
    assert (r.pts != np.asarray(pts, np.float32)).any()


def test_border_patch_replicates():
    """getRectSubPix over the corner of an image: rows and columns outside repeat the border pixel."""
    img = np.arange(48 * 64, dtype=np.uint32).reshape(48, 64).astype(np.uint8)
    p = R.rect_subpix(img, np.float32(1.0), np.float32(2.0), 13, 13)     # top-left corner (-5, -4)
    assert (p[:, :5] == p[:, 5:6]).all() and (p[:4] == p[4:5]).all()
    assert p[4, 5] == img[0, 0] and p[6, 7] == img[2, 2]
    q = R.rect_subpix(img, np.float32(62.5), np.float32(46.25), 13, 13)
    assert (q[:, -6:] == q[:, -6:-5]).all() and (q[-5:] == q[-5:-4]).all()


@pytest.mark.parametrize("half", [5, 2])
def test_summation_order_noise(half):
    """The measurement behind test_subpix_gpu.py's constants: every scene through the model twice, the window terms summed
    serially and in the order of a 64-lane wave.  Positions, iteration counts, exit codes and every round's err come out equal
    bit for bit on these inputs (worst position difference 0, worst relative err difference 0): the sums differ by a few
    units of 1e-16 relative and no float rounding of a centre falls that close to a tie.  Should an input ever be added that
    breaks this, the constants there have to be measured again."""
    worst_pos, worst_err = 0.0, 0.0
    for name, (img, pts, _) in R.scenes(half).items():
        a = R.corner_subpix(img, pts, (half, half), 40, 1e-3, "serial")
        b = R.corner_subpix(img, pts, (half, half), 40, 1e-3, "wave64")
        assert (a.iters == b.iters).all() and (a.exit_code == b.exit_code).all(), name
        worst_pos = max(worst_pos, float(np.abs(a.pts - b.pts).max()))
        for ta, tb in zip(a.err_trace, b.err_trace):
            worst_err = max([worst_err] + [abs(x - y) / x for x, y in zip(ta, tb) if x > 0])
    assert worst_pos == 0.0 and worst_err == 0.0
