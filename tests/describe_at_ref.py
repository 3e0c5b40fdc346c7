"""Literal model of fb_orb_describe: ORB descriptors at key points the caller supplies, as include/fishbird.h restates it at
fb_orb_describe_args (OpenCV 3's cv::ORB::compute on a given list, with ORBextractor.cc's IC_Angle :77-104 and
computeOrbDescriptor :107-147) -- TEST INFRASTRUCTURE ONLY.  Plain and serial: one Python loop per key point, np.float32 where
the reference computes in float.  This file is the contract k_describe_at is compared with, bit for bit.

    describe_at(params, pyramid, blurred, kps, angle_mode) -> (desc [n, 32] u8, angle [n] f32, status [n] u8)

pyramid[l] / blurred[l] are the raw and the blurred level l (blurred[l] may be None where the level cannot hold a key point);
`kps` is a structured array with x, y, angle, octave.  A row of `desc` whose status is not OK is zero and its `angle` is the
one handed in: the call leaves both as they were, which the caller of the model checks against its own marker.

The seams shared with the extractor's model are imported, not restated: the rBRIEF pattern, cvRound, fastAtan2 and cos / sin
from tests/orb_ref.py, the level tables, cv::resize and cv::GaussianBlur from tests/orb_image_ref.py.
"""
import math

import numpy as np

from orb_image_ref import gaussian_blur7, inv_scale_factors, pyramid
from orb_ref import EDGE_THRESHOLD, HALF_PATCH_SIZE, cos_sin, cv_round, fast_atan2, pattern

f32 = np.float32
OK, BORDER, LEVEL = 0, 1, 2
KEEP_ANGLE, IC_ANGLE = 0, 1


def levels(img, params):
    """(pyramid, blurred) of an image by the numpy models of ComputePyramid and GaussianBlur."""
    pyr = pyramid(img, params.scale_factor, params.nlevels)
    return pyr, [gaussian_blur7(p) if min(p.shape) >= 7 else None for p in pyr]


def umax_table():
    """umax of the constructor (ORBextractor.cc:452-469): the half width of the circular patch at each |v|."""
    umax = [0] * (HALF_PATCH_SIZE + 2)
    vmax = int(math.floor(f32(f32(f32(HALF_PATCH_SIZE) * np.sqrt(f32(2))) / f32(2)) + f32(1)))
    vmin = int(math.ceil(f32(f32(f32(HALF_PATCH_SIZE) * np.sqrt(f32(2))) / f32(2))))
    for v in range(vmax + 1):
        umax[v] = cv_round(math.sqrt(float(HALF_PATCH_SIZE * HALF_PATCH_SIZE) - v * v))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax[:HALF_PATCH_SIZE + 1]


def level_position(x, y, inv_scale, w, h):
    """(px, py) of a key point on a w x h level, or None when it is refused as BORDER.  The product is a float32; the range
    test is made on the rounded FLOAT, so NaN and +-inf fail it by the form of the comparison and never reach an integer."""
    fx, fy = f32(f32(x) * inv_scale), f32(f32(y) * inv_scale)
    rx, ry = np.rint(fx), np.rint(fy)       # float32 in, float32 out: to nearest, halves to even
    if not (EDGE_THRESHOLD <= rx <= w - EDGE_THRESHOLD - 1 and EDGE_THRESHOLD <= ry <= h - EDGE_THRESHOLD - 1):
        return None
    px, py = cv_round(fx), cv_round(fy)
    assert (px, py) == (int(rx), int(ry))
    return px, py


def ic_angle(image, px, py, umax):
    """IC_Angle: m_10 = sum u I, m_01 = sum v I over the rows v = -15..15 of the circular patch, |u| <= umax[|v|]."""
    R = HALF_PATCH_SIZE
    m_10 = m_01 = 0
    for v in range(-R, R + 1):
        for u in range(-umax[abs(v)], umax[abs(v)] + 1):
            val = int(image[py + v, px + u])
            m_10 += u * val
            m_01 += v * val
    return fast_atan2(f32(m_01), f32(m_10))


def orb_descriptor(blurred, px, py, angle_deg):
    """computeOrbDescriptor: 256 tests of the pattern rotated by the angle, every product and sum a float32 operation."""
    factorPI = f32(math.pi / float(f32(180.0)))
    a, b = cos_sin(f32(f32(angle_deg) * factorPI))
    # GET_VALUE(idx) for the 512 pattern points at once; float32 arrays: one rounding per product and per sum, none fused
    x, y = pattern()[:, 0].astype(f32), pattern()[:, 1].astype(f32)
    r = np.rint((x * b + y * a).astype(np.float64)).astype(np.int64)     # cvRound, element by element
    c = np.rint((x * a - y * b).astype(np.float64)).astype(np.int64)
    assert (py + r).min() >= 0 and (py + r).max() < blurred.shape[0] and (px + c).min() >= 0 and (px + c).max() < blurred.shape[1]
    val = blurred[py + r, px + c].astype(np.int32)
    # test t compares the points 2 t and 2 t + 1; byte i holds the tests 8 i .. 8 i + 7, the first in bit 0
    bits = (val[0::2] < val[1::2]).astype(np.uint8).reshape(32, 8)
    return (bits << np.arange(8, dtype=np.uint8)).sum(axis=1).astype(np.uint8)


def describe_at(params, pyramid, blurred, kps, angle_mode):
    assert angle_mode in (KEEP_ANGLE, IC_ANGLE)
    nlevels = params.nlevels
    inv = inv_scale_factors(params.scale_factor, nlevels)
    umax = umax_table()
    n = len(kps)
    desc = np.zeros((n, 32), np.uint8)
    angle = np.array(kps["angle"], f32)
    status = np.zeros(n, np.uint8)
    for i in range(n):
        l = int(kps["octave"][i])
        if l < 0 or l >= nlevels:
            status[i] = LEVEL
            continue
        h, w = pyramid[l].shape
        pos = level_position(kps["x"][i], kps["y"][i], inv[l], w, h)
        if pos is None:
            status[i] = BORDER
            continue
        px, py = pos
        if angle_mode == IC_ANGLE:
            angle[i] = ic_angle(pyramid[l], px, py, umax)
        desc[i] = orb_descriptor(blurred[l], px, py, angle[i])
        status[i] = OK
    return desc, angle, status
