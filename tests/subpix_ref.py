"""Literal model of fb_corner_subpix: OpenCV 3's cv::cornerSubPix with no zero zone on a u8 image (imgproc/src/cornersubpix.cpp
with getRectSubPix of imgproc/src/samplers.cpp, 8u -> 32f), as include/fishbird.h restates it.  Plain and serial: one Python
loop per key point, np.float32 where OpenCV computes in float and np.float64 where it computes in double.  This file is the
contract k_corner_subpix is compared with.

    corner_subpix(image, pts, half_win, max_iter, eps, order="serial") -> Result

`order` is how the (2w+1)(2h+1) window terms of the five sums are added:
  "serial"  term 0, 1, 2, ... in row-major order, as the C loop does;
  "wave64"  64 partial sums (term k goes to partial k % 64, in ascending k), then a butterfly over the 64 partials with the
            partner distances 32, 16, 8, 4, 2, 1 -- the order a 64-lane wave with fb::wave_sum takes.
The two differ in the last bits of the sums only; the tests measure what that does to the positions.

Result.margin is, per point, how close its nearest decision came to going the other way (see Margins); a kernel that sums in
another order may legitimately decide such a point differently when the margin is within the summation noise.
"""
import collections

import numpy as np

EXIT_EPS, EXIT_ITER, EXIT_DET, EXIT_OUT, REVERTED = 0, 1, 2, 3, 4
DBL_EPSILON = 2.220446049250313e-16
F32, F64 = np.float32, np.float64

# err_rel: min over the rounds that tested `err > eps^2` of |err - eps^2| / eps^2 (inf when eps = 0 or never tested)
# det_rel: min over rounds of ||det| - DBL_EPSILON^2| / DBL_EPSILON^2
# edge_px: min over rounds of the new centre's distance to the nearest of x = 0, x = cols, y = 0, y = rows
# revert_px: min(||cI.x - cT.x| - w|, ||cI.y - cT.y| - h|) at the final rule
Margins = collections.namedtuple("Margins", "err_rel det_rel edge_px revert_px")
Result = collections.namedtuple("Result", "pts iters exit_code margins err_trace")


def window_weights(w, h):
    """mask[i][j] = exp(-y*y) * exp(-x*x) as a float product; exp taken in double and rounded to float."""
    def table(half):
        out = np.empty(2 * half + 1, F32)
        for j in range(2 * half + 1):
            x = F32(F32(j - half) / F32(half))
            out[j] = F32(np.exp(F64(-(x * x))))
        return out
    wx, wy = table(w), table(h)
    return (wy[:, None] * wx[None, :]).astype(F32)      # float32 * float32 -> float32, element by element


def rect_subpix(image, cx, cy, pw, ph):
    """getRectSubPix(image u8, Size(pw, ph), (cx, cy)) -> float32 [ph][pw]."""
    rows, cols = image.shape
    ox = F32(F32(cx) - F32(F32(pw - 1) * F32(0.5)))
    oy = F32(F32(cy) - F32(F32(ph - 1) * F32(0.5)))
    ipx, ipy = int(np.floor(ox)), int(np.floor(oy))
    a = F32(ox - F32(ipx))
    b = F32(oy - F32(ipy))
    one = F32(1.0)
    a11 = F32(F32(one - a) * F32(one - b))
    a12 = F32(a * F32(one - b))
    a21 = F32(F32(one - a) * b)
    a22 = F32(a * b)
    b1, b2 = F32(one - b), b
    sx = ipx + np.arange(pw)
    sy = ipy + np.arange(ph)
    x0, x1 = np.clip(sx, 0, cols - 1), np.clip(sx + 1, 0, cols - 1)
    y0, y1 = np.clip(sy, 0, rows - 1), np.clip(sy + 1, 0, rows - 1)
    p00 = image[np.ix_(y0, x0)].astype(F32)
    p01 = image[np.ix_(y0, x1)].astype(F32)
    p10 = image[np.ix_(y1, x0)].astype(F32)
    p11 = image[np.ix_(y1, x1)].astype(F32)
    four = ((p00 * a11 + p01 * a12) + p10 * a21) + p11 * a22     # float32 arrays: one rounding per operation, none fused
    two = p00 * b1 + p10 * b2
    border = (sx < 0) | (sx >= cols - 1)
    out = np.where(border[None, :], two, four)
    assert out.dtype == F32
    return out


def _sum(terms, order):
    """Sum of a float64 vector in the stated order."""
    if order == "serial":
        return F64(np.cumsum(terms)[-1])                 # cumsum adds left to right
    assert order == "wave64"
    n = terms.size
    padded = np.zeros((n + 63) // 64 * 64, F64)          # + 0.0 leaves a partial unchanged
    padded[:n] = terms
    v = np.cumsum(padded.reshape(-1, 64), axis=0)[-1]    # partial l = terms l, l + 64, ... in ascending order
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return F64(v[0])


def corner_subpix(image, pts, half_win, max_iter, eps, order="serial"):
    """image: uint8 [rows][cols] (a view with any row pitch); pts: [n][2] float32 (x, y); half_win: (w, h)."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2
    rows, cols = image.shape
    w, h = half_win
    ww, wh = 2 * w + 1, 2 * h + 1
    mask = window_weights(w, h).astype(F64).ravel()
    px = np.tile(np.arange(ww, dtype=F64) - w, wh)
    py = np.repeat(np.arange(wh, dtype=F64) - h, ww)
    eps2 = F64(eps) * F64(eps)
    det_thr = DBL_EPSILON * DBL_EPSILON
    pts = np.asarray(pts, F32).reshape(-1, 2)
    out = pts.copy()
    iters = np.zeros(len(pts), np.int32)
    codes = np.zeros(len(pts), np.uint8)
    margins, traces = [], []
    for k in range(len(pts)):
        tx, ty = F32(pts[k, 0]), F32(pts[k, 1])
        cx, cy = tx, ty
        it, code = 0, EXIT_EPS
        m_err = m_det = m_edge = np.inf
        trace = []
        while True:
            patch = rect_subpix(image, cx, cy, ww + 2, wh + 2)
            tgx = (patch[1:-1, 2:] - patch[1:-1, :-2]).astype(F64).ravel()      # float differences, then double
            tgy = (patch[2:, 1:-1] - patch[:-2, 1:-1]).astype(F64).ravel()
            gxx = tgx * tgx * mask
            gxy = tgx * tgy * mask
            gyy = tgy * tgy * mask
            a = _sum(gxx, order)
            b = _sum(gxy, order)
            c = _sum(gyy, order)
            bb1 = _sum(gxx * px + gxy * py, order)
            bb2 = _sum(gxy * px + gyy * py, order)
            det = F64(a * c - b * b)
            m_det = min(m_det, abs(abs(det) - det_thr) / det_thr)
            if abs(det) <= det_thr:
                code = EXIT_DET
                break
            scale = F64(1.0) / det
            nx = F32(F64(cx) + c * scale * bb1 - b * scale * bb2)
            ny = F32(F64(cy) - b * scale * bb1 + a * scale * bb2)
            dx, dy = F32(nx - cx), F32(ny - cy)
            err = F64(F32(F32(dx * dx) + F32(dy * dy)))
            trace.append(float(err))
            cx, cy = nx, ny
            m_edge = min(m_edge, abs(float(cx)), abs(float(cx) - cols), abs(float(cy)), abs(float(cy) - rows))
            if cx < 0 or cx >= cols or cy < 0 or cy >= rows:
                code = EXIT_OUT
                break
            it += 1
            if it >= max_iter:
                code = EXIT_ITER
                break
            if eps2 > 0:
                m_err = min(m_err, abs(err - eps2) / eps2)
            if not err > eps2:
                break
        ddx, ddy = abs(F32(cx - tx)), abs(F32(cy - ty))
        m_rev = min(abs(float(ddx) - w), abs(float(ddy) - h))
        if ddx > w or ddy > h:
            cx, cy = tx, ty
            code |= REVERTED
        out[k] = (cx, cy)
        iters[k] = it
        codes[k] = code
        margins.append(Margins(float(m_err), float(m_det), float(m_edge), float(m_rev)))
        traces.append(trace)
    return Result(out, iters, codes, margins, traces)


# ---- the inputs the tests share -------------------------------------------------------------------------------------------
def saddle_image(rows, cols, x0, y0, k=100.0, s=2.0):
    """I = 128 + k tanh((x - x0) / s) tanh((y - y0) / s), rounded to u8: a smoothed saddle whose corner is (x0, y0)."""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    img = 128.0 + k * np.tanh((x - x0) / s) * np.tanh((y - y0) / s)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def padded(image, pitch):
    """The image inside rows of `pitch` bytes (the padding holds 0xAA, which no read may touch); returns (buffer, view)."""
    rows, cols = image.shape
    buf = np.full((rows, pitch), 0xAA, np.uint8)
    buf[:, :cols] = image
    return buf, buf[:, :cols]


ROWS, COLS, PITCH = 48, 64, 80       # the shape every constructed scene has
SADDLE_XY = (30.37, 22.71)


def _grid():
    y, x = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    return x, y


def _u8(img):
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def scenes(half_win):
    """name -> (image u8 [ROWS][COLS], starts [(x, y)], exit codes the model gives at half window 5 (None = not pinned)).
    tests/test_subpix_model.py checks on the CPU that each scene does what it is here for; the GPU tests run the same scenes
    through the kernel.  At half window 2 the saddle is sharper and its starts nearer (the corner has to fit the window); the
    other scenes are the same inputs, there for the comparison with the model only."""
    x, y = _grid()
    out = collections.OrderedDict()
    s = 2.0 if half_win >= 4 else 0.7
    r = 3.0 if half_win >= 4 else 1.0          # starts up to r px away in each coordinate
    offs = [(-0.37, 0.29), (0.63, -0.71), (-1.37, -1.71), (2.13, 1.79), (-2.37, 2.29), (2.63, -2.71), (0.0, 0.0), (-2.87, -0.71), (0.63, 2.79)]
    out["saddle"] = (saddle_image(ROWS, COLS, SADDLE_XY[0], SADDLE_XY[1], s=s),
                     [(SADDLE_XY[0] + dx * r / 3.0, SADDLE_XY[1] + dy * r / 3.0) for dx, dy in offs], [EXIT_EPS] * len(offs))
    # saddles on a 14 px grid, the outer ones 2.4 .. 5.7 px inside each border: the replicate-border path, a start within 6 px
    # of the left, left + top, right, right + bottom, top and bottom border
    chk = _u8(128 + 100 * np.sin(np.pi * (x - 2.37) / 14.0) * np.sin(np.pi * (y - 3.71) / 14.0))
    out["border"] = (chk, [(3, 18), (2, 4), (59, 31), (59, 46), (30, 4.5), (31, 45)], [EXIT_EPS] * 6)
    out["flat"] = (np.full((ROWS, COLS), 77, np.uint8), [(20.25, 30.5), (0.5, 0.5), (63.0, 47.0)], [EXIT_DET] * 3)
    # a straight ramp edge: the normal equations are nearly singular along it and the point slides along it off the image,
    # the first three in a jump longer than the window (put back), the last two in short steps (they stay outside)
    u = (x - 32) * np.cos(0.3) + (y - 24) * np.sin(0.3)
    out["ramp"] = (_u8(128 + 12 * np.clip(u, -8, 8)), [(32, 3), (33, 45), (28, 46), (38.65, 2.5), (25.5, 45.02)],
                   [EXIT_OUT | REVERTED] * 3 + [EXIT_OUT] * 2)
    # a start between two saddles of the grid: the point walks further than the window allows and is put back
    out["drift"] = (chk, [(9, 11), (23.5, 24.5)], [EXIT_EPS | REVERTED, EXIT_ITER | REVERTED])
    return out
