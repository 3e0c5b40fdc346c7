"""Literal model of fb_orb_detect: cv::ORB's detector as include/fishbird.h restates it at fb_orb_detect_args (OpenCV 3
features2d/src/orb.cpp: computeKeyPoints, HarrisResponses, ICAngles, KeyPointsFilter::retainBest / runByImageBorder /
runByPixelsMask, and cv::FAST with nonmaxSuppression) -- TEST INFRASTRUCTURE ONLY.  OpenCV is not vendored: restated, parity
unpinned.  numpy.float32 step by step wherever the reference computes in float.  This file is the contract the kernels of
csrc/orb_detect.inc are compared with, bit for bit.

    detect(params, img, mask=None, fast_threshold=20) -> Result(kps, per_level)

`kps` is a cabi.KP_DTYPE array in output order (levels ascending, raster order within a level), untruncated; per_level[l] is
(candidates, after cut 1, after cut 2).

The seams shared with the other models are imported, not restated: cv::resize and the level sizes from tests/orb_image_ref.py,
the FAST ring, cvRound and the constructor's feature split from tests/orb_ref.py, IC_Angle from tests/describe_at_ref.py.
"""
import collections
import math

import numpy as np

from describe_at_ref import ic_angle, umax_table
from orb_image_ref import inv_scale_factors, level_sizes, pyramid, resize_linear_u8
from orb_ref import RING, cv_round

f32 = np.float32
EDGE = 31            # cv::ORB edgeThreshold
HARRIS_BLOCK = 7
HARRIS_K = f32(0.04)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])

Result = collections.namedtuple("Result", "kps per_level")


def scale_factors(scale_factor, nlevels):
    """mvScaleFactor in float32."""
    sf = [f32(1.0)]
    for _ in range(1, nlevels):
        sf.append(f32(sf[-1] * f32(scale_factor)))
    return sf


def features_per_level(nfeatures, scale_factor, nlevels):
    """mnFeaturesPerLevel (ORBextractor.cc:433-446), the formula cv::ORB's computeKeyPoints has as well."""
    factor = f32(f32(1.0) / f32(scale_factor))
    nDesired = f32(f32(f32(nfeatures) * f32(f32(1) - factor)) / f32(f32(1) - f32(math.pow(float(factor), float(nlevels)))))
    out, total = [], 0
    for _ in range(nlevels - 1):
        out.append(cv_round(nDesired))
        total += out[-1]
        nDesired = f32(nDesired * factor)
    out.append(max(nfeatures - total, 0))
    return out


def cv_orb_level_sizes(w, h, scale_factor, nlevels):
    """cv::ORB's own rule: Size(cvRound(cols / scale), cvRound(rows / scale)), scale = (float)pow(scaleFactor, l)."""
    out = []
    for l in range(nlevels):
        scale = f32(math.pow(float(f32(scale_factor)), float(l)))
        out.append((cv_round(f32(f32(w) / scale)), cv_round(f32(f32(h) / scale))))
    return out


def mask_levels(mask, sizes):
    """m_0 = mask; m_l = tozero_254(resize(m_{l-1})): resized from the already thresholded previous level."""
    out = [np.ascontiguousarray(mask)]
    for l in range(1, len(sizes)):
        m = resize_linear_u8(out[-1], sizes[l][0], sizes[l][1])[0]
        out.append(np.where(m > 254, m, 0).astype(np.uint8))
    return out


def fast_scores(img, thr):
    """The score of every pixel of a level: the largest threshold at which it passes FAST-9-16, if that is >= thr, else 0;
    0 outside [3, w - 3) x [3, h - 3).  (m = the largest over the 16 arcs and both signs of the arc's smallest difference is
    the smallest threshold at which the pixel no longer passes.)"""
    h, w = img.shape
    score = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return score
    v = img.astype(np.int32)
    c = v[3:h - 3, 3:w - 3]
    d = np.stack([v[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING])
    m = np.zeros(c.shape, np.int32)
    for e in (d, -d):
        e2 = np.concatenate([e, e[:8]])
        for s in range(16):
            m = np.maximum(m, e2[s:s + 9].min(axis=0))
    score[3:h - 3, 3:w - 3] = np.where(m > thr, m - 1, 0)
    return score


def suppress(score):
    """3x3 non-maximum suppression: kept iff positive and strictly greater than all 8 neighbours (0 outside the level)."""
    h, w = score.shape
    p = np.pad(score, 1)
    keep = score > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= score > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return keep


def harris_abc(img, px, py):
    """The integer sums of HarrisResponses at one pixel: a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy over the 7 x 7 block."""
    r = HARRIS_BLOCK // 2
    a = b = c = 0
    I = lambda y, x: int(img[y, x])
    for y in range(py - r, py + r + 1):
        for x in range(px - r, px + r + 1):
            Ix = (I(y, x + 1) - I(y, x - 1)) * 2 + (I(y - 1, x + 1) - I(y - 1, x - 1)) + (I(y + 1, x + 1) - I(y + 1, x - 1))
            Iy = (I(y + 1, x) - I(y - 1, x)) * 2 + (I(y + 1, x - 1) - I(y - 1, x - 1)) + (I(y + 1, x + 1) - I(y - 1, x + 1))
            a += Ix * Ix
            b += Iy * Iy
            c += Ix * Iy
    return a, b, c


def harris_from_abc(a, b, c):
    """((float)a*b - (float)c*c - k*((float)a+b)*((float)a+b)) * scale^4, every float operation rounded on its own."""
    s = f32(f32(1.0) / f32(f32(4 * HARRIS_BLOCK) * f32(255.0)))
    s4 = f32(f32(f32(s * s) * s) * s)
    fa, fb, fc = f32(a), f32(b), f32(c)
    det = f32(f32(fa * fb) - f32(fc * fc))
    tr = f32(fa + fb)
    return f32(f32(det - f32(f32(HARRIS_K * tr) * tr)) * s4)


def harris(img, px, py):
    return harris_from_abc(*harris_abc(img, px, py))


def retain_best(values, K):
    """KeyPointsFilter::retainBest: with more than K entries, the indices of those whose value is >= the K-th largest (every
    tie at the cut stays); K = 0 clears.  Indices in their original order."""
    values = np.asarray(values)
    n = len(values)
    if n <= K:
        return np.arange(n)
    if K == 0:
        return np.arange(0)
    cut = np.sort(values)[::-1][K - 1]
    return np.nonzero(values >= cut)[0]      # -0.0 >= 0.0 holds: compared as floats


def detect_level(img, mask_l, thr, K2):
    """One level: (positions [(px, py)] in raster order, responses, (candidates, after cut 1, after cut 2))."""
    h, w = img.shape
    if w <= 2 * EDGE or h <= 2 * EDGE:
        return [], [], (0, 0, 0)
    score = fast_scores(img, thr)
    keep = suppress(score)
    inside = np.zeros_like(keep)
    inside[EDGE:h - EDGE, EDGE:w - EDGE] = True          # runByImageBorder: EDGE <= px < w - EDGE
    keep &= inside
    if mask_l is not None:
        keep &= mask_l != 0                              # runByPixelsMask
    ys, xs = np.nonzero(keep)                            # raster order
    fast = score[ys, xs]
    i1 = retain_best(fast, 2 * K2)
    ys1, xs1 = ys[i1], xs[i1]
    resp = np.array([harris(img, int(x), int(y)) for x, y in zip(xs1, ys1)], f32)
    i2 = retain_best(resp, K2)
    pos = [(int(xs1[i]), int(ys1[i])) for i in i2]
    return pos, resp[i2], (len(ys), len(i1), len(i2))


def detect(params, img, mask=None, fast_threshold=20, levels=None):
    nl = params.nlevels
    pyr = levels if levels is not None else pyramid(img, params.scale_factor, nl)
    sizes = [(p.shape[1], p.shape[0]) for p in pyr]
    masks = mask_levels(mask, sizes) if mask is not None else [None] * nl
    N = features_per_level(params.nfeatures, params.scale_factor, nl)
    sf = scale_factors(params.scale_factor, nl)
    umax = umax_table()
    rows, per_level = [], []
    for l in range(nl):
        pos, resp, counts = detect_level(pyr[l], masks[l], fast_threshold, N[l])
        per_level.append(counts)
        for (px, py), r in zip(pos, resp):
            rows.append((f32(f32(px) * sf[l]), f32(f32(py) * sf[l]), f32(f32(31.0) * sf[l]), ic_angle(pyr[l], px, py, umax), r, l))
    kps = np.zeros(len(rows), KP_DTYPE)
    for i, r in enumerate(rows):
        kps[i] = r
    return Result(kps, per_level)


def round_trip_ok(w, h, scale_factor, nlevels):
    """cvRound(x * inv_scale_factor[l]) == px for every px (and py) a key point of level l can have."""
    sf, inv = scale_factors(scale_factor, nlevels), inv_scale_factors(scale_factor, nlevels)
    for l, (wl, hl) in enumerate(level_sizes(w, h, scale_factor, nlevels)):
        p = np.arange(EDGE, max(wl, hl) - EDGE, dtype=np.int64)
        back = np.rint((p.astype(f32) * sf[l]).astype(f32) * inv[l]).astype(np.int64)
        if not np.array_equal(back, p):
            return False
    return True
