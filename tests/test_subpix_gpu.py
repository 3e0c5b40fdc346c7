"""k_corner_subpix (fb_corner_subpix[_dev], csrc/frame.hip) against the literal model tests/subpix_ref.py on the constructed
scenes of that file: a 64 x 48 image in rows of 80 bytes, batch 2 with different n, kp_stride > n, 9 points in one image
(4 waves per workgroup x 2 + 1), half windows 5 and 2.

Tolerances (measured by tests/test_subpix_model.py::test_summation_order_noise on exactly these inputs, model summed serially
against model summed in a 64-lane wave's order):
  POS_NOISE = 0 px   worst position difference between the two orders; times 8 for the kernel's tree shape it stays 0, so the
                     floor holds: one float ulp of the coordinate, because the centre is stored as float every round.
  ERR_NOISE = 0      worst relative difference of a round's err between the two orders.  The floor used for the margin
                     exclusion is what one ulp u of a centre does to err = d^2 at the threshold d = eps: both centres of the
                     difference and both coordinates may move, 4 sqrt(2) u / eps = 0.022 for u = 2^-18 (coordinates < 64)
                     and eps = 1e-3.
A point whose model-side decision margin is below that noise (err within 2.2 % of eps^2, |det| within 1e-6 relative of its
threshold, a centre within one ulp of the image edge or of the revert bound) may differ in exit code and iteration count; at
most 1 % of a test's points may be excluded that way.  None of the scenes has such a point (the model test checks it)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fishbirdeyevisualslam_amd as fb
from fishbirdeyevisualslam_amd import cabi

import subpix_ref as R

pytestmark = pytest.mark.gpu

POS_NOISE, ERR_NOISE = 0.0, 0.0          # measured (see above)
TREE_MARGIN = 8.0
ERR_FLOOR = 4 * np.sqrt(2.0) * 2.0 ** -18 / 1e-3
DET_FLOOR = 1e-6
EPS = 1e-3
WAVES_PER_WORKGROUP = 4                  # SUBPIX_WAVES of csrc/subpix_plan.h


@functools.lru_cache(maxsize=None)
def _model(name, half, max_iter):
    img, pts, _ = R.scenes(half)[name]
    return R.corner_subpix(img, pts, (half, half), max_iter, EPS)


def _inputs(names, half, n_override=None, seed=3):
    """Two scenes as one batch: images in rows of PITCH bytes, key points with every other field and every slot beyond n set
    to recognisable junk."""
    g = np.random.Generator(np.random.PCG64(seed))
    sc = [R.scenes(half)[nm] for nm in names]
    n = np.array([len(s[1]) for s in sc], np.int32)
    if n_override is not None:
        n = np.minimum(n, np.array(n_override, np.int32))
    stride = int(max(len(s[1]) for s in sc)) + 7
    B = len(names)
    image = np.full((B, R.ROWS, R.PITCH), 0xAA, np.uint8)
    kps = np.zeros((B, stride), cabi.KP_DTYPE)
    for f in ("x", "y", "size", "angle", "response"):
        kps[f] = g.uniform(1.0, 40.0, (B, stride)).astype(np.float32)
    kps["octave"] = g.integers(0, 8, (B, stride))
    for b, (img, pts, _) in enumerate(sc):
        image[b, :, : R.COLS] = img
        p = np.asarray(pts, np.float32)
        kps["x"][b, : len(p)], kps["y"][b, : len(p)] = p[:, 0], p[:, 1]
    return image, n, kps, stride


def _args(batch, image, n, kps, iters, codes, stride, half, max_iter, over=None):
    a = cabi.CornerSubpixArgs()
    cabi.fill(a, batch=batch, kp_stride=stride, cols=R.COLS, rows=R.ROWS, pitch=R.PITCH, image_stride=R.ROWS * R.PITCH, image=image, n=n,
              kps=kps, half_win_x=half, half_win_y=half, max_iter=max_iter, eps=EPS, iters=iters, exit_code=codes)
    cabi.fill(a, **(over or {}))
    return a


def _run_dev(image, n, kps, stride, half, max_iter, over=None):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    B = len(n)
    iters, codes = np.full((B, stride), -7, np.int32), np.full((B, stride), 0xEE, np.uint8)
    d = dict(image=dev(image), n=dev(n), kps=dev(kps), iters=dev(iters), codes=dev(codes))
    a = _args(B, d["image"], d["n"], d["kps"], d["iters"], d["codes"], stride, half, max_iter, over)
    # on torch's current stream, like the uploads above: the null stream is not ordered against a non-blocking one
    rc = fb.lib().fb_corner_subpix_dev(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    back = lambda t, like: t.cpu().numpy().view(like.dtype).reshape(like.shape)
    return rc, back(d["kps"], kps), back(d["iters"], iters), back(d["codes"], codes)


def _ulp(v):
    return float(np.spacing(np.float32(abs(v))))


def _compare(names, half, max_iter, n, kps_in, kps, iters, codes):
    total = excluded = 0
    worst = 0.0
    for b, nm in enumerate(names):
        m = _model(nm, half, max_iter)
        nb = int(n[b])
        for f in ("size", "angle", "response", "octave"):
            assert kps[f][b].tobytes() == kps_in[f][b].tobytes(), (nm, f)
        assert kps[b, nb:].tobytes() == kps_in[b, nb:].tobytes(), (nm, "slots at and beyond n")
        assert (iters[b, nb:] == -7).all() and (codes[b, nb:] == 0xEE).all(), (nm, "iters / exit_code beyond n")
        for i in range(nb):
            total += 1
            mg = m.margins[i]
            tol = max(TREE_MARGIN * POS_NOISE, _ulp(m.pts[i][0]), _ulp(m.pts[i][1]))
            print("%s[%d] half %d: model (%.6f, %.6f) it %d code %d | kernel (%.6f, %.6f) it %d code %d" % (
                nm, i, half, m.pts[i][0], m.pts[i][1], m.iters[i], m.exit_code[i], kps["x"][b, i], kps["y"][b, i], iters[b, i], codes[b, i]))
            same = iters[b, i] == m.iters[i] and codes[b, i] == m.exit_code[i]
            if not same:
                near = (mg.err_rel < max(TREE_MARGIN * ERR_NOISE, ERR_FLOOR) or mg.det_rel < DET_FLOOR or mg.edge_px <= tol or mg.revert_px <= tol)
                assert near, (nm, i, "decision differs with a wide margin", mg, int(iters[b, i]), int(codes[b, i]), int(m.iters[i]), int(m.exit_code[i]))
                excluded += 1
                continue
            d = max(abs(float(kps["x"][b, i]) - float(m.pts[i][0])), abs(float(kps["y"][b, i]) - float(m.pts[i][1])))
            worst = max(worst, d)
            assert d <= tol, (nm, i, d, tol)
    assert excluded <= 0.01 * total, (excluded, total)
    print("worst position difference %.3g px over %d points, %d excluded" % (worst, total, excluded))


PAIRS = [("saddle", "flat"), ("border", "ramp"), ("drift", "saddle")]


@pytest.mark.parametrize("half", [5, 2])
@pytest.mark.parametrize("names", PAIRS)
def test_kernel_matches_model(names, half):
    assert len(R.scenes(half)["saddle"][1]) == WAVES_PER_WORKGROUP * 2 + 1     # more than one workgroup
    image, n, kps, stride = _inputs(names, half)
    assert n[0] != n[1] and stride > n.max()
    rc, out, iters, codes = _run_dev(image, n, kps, stride, half, 40)
    assert rc == 0, fb.lib().fb_last_error()
    _compare(names, half, 40, n, kps, out, iters, codes)


def test_iteration_cap_and_empty_image():
    """max_iter = 1: every moving point ends by the cap; and the second image of the batch runs with n = 0."""
    names = ("saddle", "border")
    image, n, kps, stride = _inputs(names, 5, n_override=(99, 0))
    assert list(n) == [9, 0]
    rc, out, iters, codes = _run_dev(image, n, kps, stride, 5, 1)
    assert rc == 0, fb.lib().fb_last_error()
    _compare(names, 5, 1, n, kps, out, iters, codes)
    assert (codes[0, :9] == R.EXIT_ITER).all() and (iters[0, :9] == 1).all()
    assert out[1].tobytes() == kps[1].tobytes()


def test_host_pointer_wrapper_gives_the_same_bytes():
    names = ("border", "ramp")
    image, n, kps, stride = _inputs(names, 5)
    rc, out, iters, codes = _run_dev(image, n, kps, stride, 5, 40)
    assert rc == 0, fb.lib().fb_last_error()
    hk, hi, hc = kps.copy(), np.full((2, stride), -7, np.int32), np.full((2, stride), 0xEE, np.uint8)
    a = _args(2, image, n, hk, hi, hc, stride, 5, 40)
    fb.check(fb.lib().fb_corner_subpix(C.byref(a)), "fb_corner_subpix")
    assert hk.tobytes() == out.tobytes() and hi.tobytes() == iters.tobytes() and hc.tobytes() == codes.tobytes()
    # the optional outputs left out
    hk2 = kps.copy()
    a = _args(2, image, n, hk2, None, None, stride, 5, 40)
    fb.check(fb.lib().fb_corner_subpix(C.byref(a)), "fb_corner_subpix")
    assert hk2.tobytes() == out.tobytes()


@pytest.mark.parametrize("over", [dict(half_win_x=0), dict(half_win_y=0), dict(half_win_x=9), dict(half_win_y=9), dict(pitch=R.COLS - 1),
                                  dict(image=None), dict(max_iter=0), dict(eps=-1.0)])
def test_bad_arguments_launch_nothing(over):
    image, n, kps, stride = _inputs(("saddle", "flat"), 5)
    rc, out, iters, codes = _run_dev(image, n, kps, stride, 5, 40, over)
    assert rc == cabi.FB_ERR_ARG, rc
    assert fb.lib().fb_last_error()
    assert out.tobytes() == kps.tobytes() and (iters == -7).all() and (codes == 0xEE).all()
    hk = kps.copy()
    a = _args(2, image, n, hk, None, None, stride, 5, 40, over)
    assert fb.lib().fb_corner_subpix(C.byref(a)) == cabi.FB_ERR_ARG
    assert hk.tobytes() == kps.tobytes()
