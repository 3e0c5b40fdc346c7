"""cv::resize(INTER_LINEAR) and cv::GaussianBlur(7x7, sigma 2) on 8-bit images in plain numpy -- TEST INFRASTRUCTURE ONLY.

Written from the sentences of DESIGN section 2 ("PARITY UNPINNED at the OpenCV ... seams") and from ComputePyramid
(ORBextractor.cc:1107-1132, constructor tables :415-431), not from oracle/orb_oracle.cpp and not from the kernels.  It
pins kernel and oracle to a third, independent program; it does not pin either of them to OpenCV.

  level_sizes      cvRound((float)cols * mvInvScaleFactor[l]) from the ORIGINAL size (:1111-1112), float32 tables built
                   as the constructor builds them (a running product, then 1.0f / it).
  resize_linear_u8 scale = 1 / (dst / src) in double; source index float32((d + 0.5) * scale - 0.5), floor; on x an index
                   below 0 becomes (0, weight 0) and an index >= src - 1 becomes (src - 1, weight 0); on y the two row
                   indices are clamped into the image; weights cvRound((1 - f) * 2048), cvRound(f * 2048) in float32,
                   half to even; horizontal pass in int; vertical ((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16),
                   + 2, >> 2, saturated.
  gaussian_blur7   BORDER_REFLECT_101 (numpy's "reflect"), integer kernel {18,34,49,55,49,34,18} (sum 257) on each axis,
                   (sum + 2^15) >> 16, saturated.
  resize_route     which of the three resize kernels the extractor's plan takes for (source size, destination size,
                   alignment of the source), restated from this module's own xofs / yofs.

Every decision has a named wrong reading (VARIANTS); the functions run with one of them switched on.
tests/orb_image_cases.py builds the inputs that tell each from the model.

Readings that no input of the extractor can tell from the model (INSEPARABLE, implemented and run all the same):
  * `vertical_first`: both passes are exact integer sums of products with no rounding between them, so their order
    cannot change a bit.
  * `right_border_sw` (`sx >= sw` for `sx >= sw - 1`) and `no_bottom_clamp` (row sy + 1 read without the clamp; a row
    outside the image reads as 0): the extractor only shrinks (fb_orb_create demands a scale factor > 1 and a level is never
    larger than the one before it), so scale = src / dst >= 1 and the last index is
    (dst - 0.5) * scale - 0.5 = src - 1 - (scale - 1) / 2 <= src - 1, the first one (scale - 1) / 2 >= 0.  The second tap
    src - 1 + 1 is reached only at scale == 1 (or when the float32 rounding lands exactly on src - 1), and then its weight
    is exactly 0.  For the same reason the left border rule and the clamp at row 0 never fire.
"""
import numpy as np

f32 = np.float32

VARIANTS = (
    # resize
    "no_half",              # source index (d + 0.5) * scale, the `- 0.5` left out
    "scale_from_factor",    # scale = the extractor's scale factor instead of src / dst
    "size_from_previous",   # level size cvRound(previous size / scale factor) instead of from the original size
    "no_shift4",            # horizontal sums not shifted by 4 (b * r >> 20 instead of b * (r >> 4) >> 16)
    "no_plus2",             # the + 2 before the last >> 2 left out
    "weights_half_up",      # weights rounded half up instead of half to even
    # blur
    "border_reflect",       # BORDER_REFLECT (edge pixel repeated) instead of BORDER_REFLECT_101
    "kernel_256",           # a kernel that sums to 256 (centre 54)
    "no_round",             # the 2^15 rounding term left out
    "no_clamp",             # result not saturated: 257 wraps to 1
)

INSEPARABLE = (
    "right_border_sw",      # x border rule at sx >= sw; the tap at column sw reads 0
    "no_bottom_clamp",      # row sy + 1 not clamped; a row past the image reads 0
    "vertical_first",       # vertical pass before the horizontal one
)

RESIZE_VARIANTS = ("no_half", "scale_from_factor", "size_from_previous", "no_shift4", "no_plus2", "weights_half_up",
                   "right_border_sw", "no_bottom_clamp")
BLUR_VARIANTS = ("border_reflect", "kernel_256", "no_round", "no_clamp", "vertical_first")


def _check(variant):
    assert variant is None or variant in VARIANTS or variant in INSEPARABLE, variant


def cv_round_f32(v):
    """cvRound of float32 values: to the nearest integer, ties to even."""
    return np.rint(np.asarray(v, f32)).astype(np.int64)


def inv_scale_factors(scale_factor, nlevels):
    """mvInvScaleFactor (:415-431) in float32."""
    sf = [f32(1.0)]
    for _ in range(1, nlevels):
        sf.append(f32(sf[-1] * f32(scale_factor)))
    return [f32(f32(1.0) / s) for s in sf]


def level_sizes(w, h, scale_factor, nlevels, variant=None):
    """[(w_l, h_l)] of every pyramid level (:1111-1112)."""
    _check(variant)
    inv = inv_scale_factors(scale_factor, nlevels)
    out = [(int(w), int(h))]
    for l in range(1, nlevels):
        if variant == "size_from_previous":
            pw, ph = out[-1]
            out.append((int(cv_round_f32(f32(pw) * inv[1])), int(cv_round_f32(f32(ph) * inv[1]))))
        else:
            out.append((int(cv_round_f32(f32(w) * inv[l])), int(cv_round_f32(f32(h) * inv[l]))))
    return out


def _weights(f, variant):
    a0, a1 = (f32(1.0) - f) * f32(2048.0), f * f32(2048.0)
    if variant == "weights_half_up":
        return np.floor(a0.astype(np.float64) + 0.5).astype(np.int64), np.floor(a1.astype(np.float64) + 0.5).astype(np.int64)
    return cv_round_f32(a0), cv_round_f32(a1)


def axis_table(sn, dn, variant=None, scale_factor=None, x_axis=True):
    """Source index and the two 11-bit weights of every destination index along one axis."""
    if variant == "scale_from_factor":
        scale = float(f32(scale_factor))
    else:
        scale = 1.0 / (float(dn) / float(sn))
    d = np.arange(dn, dtype=np.float64)
    pos = (d + 0.5) * scale - (0.0 if variant == "no_half" else 0.5)
    fpos = pos.astype(f32)
    s = np.floor(fpos).astype(np.int64)
    f = (fpos - s.astype(f32)).astype(f32)
    if x_axis:
        lo = s < 0
        f[lo], s[lo] = 0, 0
        hi = s >= (sn if variant == "right_border_sw" else sn - 1)
        f[hi], s[hi] = 0, sn - 1
    w0, w1 = _weights(f, variant)
    return s, w0, w1


def resize_linear_u8(src, dw, dh, variant=None, scale_factor=None):
    """(dst, xofs, yofs): cv::resize(src, Size(dw, dh), INTER_LINEAR) of an 8-bit image."""
    _check(variant)
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    sh, sw = src.shape
    xofs, a0, a1 = axis_table(sw, dw, variant, scale_factor, True)
    yofs, b0, b1 = axis_table(sh, dh, variant, scale_factor, False)
    s = src.astype(np.int64)
    sp = np.pad(s, ((0, 1), (0, 1)))                       # a zero row / column for the readings that leave the image
    x0 = np.clip(xofs, 0, sw - 1)
    x1 = np.where(xofs + 1 <= sw - 1, xofs + 1, sw if variant == "right_border_sw" else sw - 1)
    x1 = np.clip(x1, 0, sw)
    h = sp[:, x0] * a0[None, :] + sp[:, x1] * a1[None, :]  # horizontal pass of every source row (+ the zero row)
    y0 = np.clip(yofs, 0, sh - 1)
    y1 = np.clip(yofs + 1, 0, sh - 1)
    if variant == "no_bottom_clamp":
        y1 = np.clip(yofs + 1, 0, sh)
    r0, r1 = h[y0, :], h[y1, :]
    if variant == "no_shift4":
        v = ((b0[:, None] * r0) >> 20) + ((b1[:, None] * r1) >> 20)
    else:
        v = ((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16)
    v = (v + (0 if variant == "no_plus2" else 2)) >> 2
    return np.clip(v, 0, 255).astype(np.uint8), xofs.astype(np.int32), yofs.astype(np.int32)


def pyramid(img, scale_factor, nlevels, variant=None):
    """The levels of ComputePyramid: level l is resized from level l - 1 to the size of level_sizes."""
    sizes = level_sizes(img.shape[1], img.shape[0], scale_factor, nlevels, variant)
    out = [np.ascontiguousarray(img)]
    for l in range(1, nlevels):
        if min(sizes[l]) < 1 or out[-1].size == 0:  # only a wrong reading of the sizes gets here: an empty level
            out.append(np.zeros((0, 0), np.uint8))
            continue
        out.append(resize_linear_u8(out[-1], sizes[l][0], sizes[l][1], variant if variant in RESIZE_VARIANTS else None, scale_factor)[0])
    return out


GAUSS7 = (18, 34, 49, 55, 49, 34, 18)


def gaussian_blur7(src, variant=None):
    """cv::GaussianBlur(src, Size(7, 7), 2, 2, BORDER_REFLECT_101) of an 8-bit image."""
    _check(variant)
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    h, w = src.shape
    k = list(GAUSS7)
    if variant == "kernel_256":
        k[3] = 54
    p = np.pad(src.astype(np.int64), 3, mode="symmetric" if variant == "border_reflect" else "reflect")
    if variant == "vertical_first":
        t = sum(k[i] * p[i:i + h, :] for i in range(7))
        s = sum(k[i] * t[:, i:i + w] for i in range(7))
    else:
        t = sum(k[i] * p[:, i:i + w] for i in range(7))
        s = sum(k[i] * t[i:i + h, :] for i in range(7))
    s = (s + (0 if variant == "no_round" else 1 << 15)) >> 16
    if variant == "no_clamp":
        return (s & 0xFF).astype(np.uint8)
    return np.minimum(s, 255).astype(np.uint8)


def blur_of_constant(c):
    """The hand-derivable answer: 257 * 257 = 66049 times the value, rounded, saturated."""
    return min(((c * 66049) + 32768) >> 16, 255)


# ------------------------------------------------------------------------------------------------------------------
# which resize kernel the plan takes (csrc/orb_plan.h: resize_rows_ok, resize_merge_ok; orb.hip: launch_resize)
# ------------------------------------------------------------------------------------------------------------------
RESIZE_ROWS, RM_ROWS, RM_SRC = 8, 12, 16
ROUTE_ID = {"generic": 0, "rows": 1, "merge": 2}


def rows_ok(xofs):
    """k_resize_rows: the taps of every group of 4 destination pixels lie inside the 12-byte window that starts at the
    group's first tap rounded down to 4, and within 8 bytes of that first tap."""
    dw = len(xofs)
    for dx4 in range(0, dw, 4):
        last = int(xofs[min(dx4 + 3, dw - 1)]) + 1
        first = int(xofs[dx4])
        if last - (first & ~3) > 11 or last - first > 7:
            return False
    return True


def merge_ok(yofs):
    """k_resize_merge: every run of RM_ROWS destination rows starts inside the image, spans at most RM_SRC source rows
    (second taps included) and no two of its rows share their first source row."""
    dh = len(yofs)
    for y0 in range(0, dh, RM_ROWS):
        y1 = min(y0 + RM_ROWS, dh) - 1
        if yofs[y0] < 0 or int(yofs[y1]) + 1 - int(yofs[y0]) > RM_SRC - 1:
            return False
        if any(yofs[y + 1] <= yofs[y] for y in range(y0, y1)):
            return False
    return True


def resize_route(src_w, src_h, dst_w, dst_h, aligned):
    """"generic", "rows" or "merge".  `aligned`: source pointer, row stride and image stride are all multiples of 4."""
    xofs = axis_table(src_w, dst_w, None, None, True)[0]
    yofs = axis_table(src_h, dst_h, None, None, False)[0]
    if not aligned or not rows_ok(xofs):
        return "generic"
    return "merge" if merge_ok(yofs) else "rows"


def blurred_by_plan(w, h):
    """The plan gives a level blur strips only if it can hold a key point (19 px of border on every side)."""
    return w >= 38 and h >= 38
