"""Constructed inputs for the resize and blur kernels of the extractor -- TEST INFRASTRUCTURE ONLY.

Every case is a tiny image (or batch) laid out in a flat byte buffer the way a caller may hand it to
fb_orb_extract_batch_dev: `offset` bytes in front (an unaligned device pointer), `stride` bytes per row, `image_stride`
bytes from image to image; everything that is not a pixel is padding and is filled with `fill`.  A case declares, as
literals, which resize kernel builds each level >= 1 (ROUTES) and which levels the plan blurs; tests/test_orb_image_cases.py
holds the declarations to orb_image_ref.resize_route and tests/cpp/orb_plan_test.cpp holds the same list to orb_plan.h.

Families (the GPU test is parametrised per family):
  routes    131x77 at the scale factors where the hand-over between the three kernels lies, 128x96 at 1.3334
  heights   destination heights around the row runs of k_resize_merge (12) and k_resize_rows (8); level widths of 1..4 px
  widths    destination widths of every residue mod 4 on every route; level-0 widths whose last 12-byte window is clamped
  content   constants, checkerboards, stripes, impulses, a ramp, saturated blocks: hand-derivable answers
  blur      blur widths around the 256-column strip, heights around the 32-row run, 38 px beside 37 px, a batch of 3
  align     one image five ways: aligned, pointer offsets 1..3, strides = 1..3 mod 4, second image of a batch whose image
            stride is not a multiple of 4, stride = width + 64; padded layouts once with 0x00 and once with 0xFF padding
"""
import numpy as np

import orb_image_ref as R


class Case:
    def __init__(self, name, family, imgs, scale, nlevels, stride=None, gap=0, offset=0, fill=0, kills=(), group=None,
                 nfeatures=300):
        imgs = np.asarray(imgs, np.uint8)
        if imgs.ndim == 2:
            imgs = imgs[None]
        self.name, self.family, self.imgs = name, family, imgs
        self.B, self.h, self.w = imgs.shape
        self.scale, self.nlevels, self.nfeatures = scale, nlevels, nfeatures
        self.stride = self.w if stride is None else stride
        self.image_stride = self.stride * self.h + gap
        self.offset, self.fill, self.kills, self.group = offset, fill, tuple(kills), group
        self.routes = ROUTES[name]              # per level >= 1
        self.blurred = BLURRED[name]            # per level
        assert len(self.routes) == nlevels - 1 and len(self.blurred) == nlevels, name

    @property
    def aligned(self):
        return (self.offset | self.stride | self.image_stride) % 4 == 0

    @property
    def padded(self):
        return self.stride > self.w or self.image_stride > self.stride * self.h or self.offset > 0

    def params(self):
        return dict(nfeatures=self.nfeatures, scale_factor=self.scale, nlevels=self.nlevels)

    def buffer(self, fill=None):
        """The flat byte buffer: `offset` bytes, then the images at their strides; padding = fill."""
        fill = self.fill if fill is None else fill
        n = self.offset + (self.B - 1) * self.image_stride + self.stride * self.h
        buf = np.full(n, fill, np.uint8)
        for b in range(self.B):
            o = self.offset + b * self.image_stride
            rows = np.lib.stride_tricks.as_strided(buf[o:], (self.h, self.w), (self.stride, 1))
            rows[...] = self.imgs[b]
        return buf


# ---- content ----
def noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def const(c, w, h):
    return np.full((h, w), c, np.uint8)


def checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return (((x + y) & 1) * 255).astype(np.uint8)


def stripes(w, h, vertical):
    y, x = np.mgrid[0:h, 0:w]
    return (((x if vertical else y) & 1) * 255).astype(np.uint8)


def impulses(w, h, points):
    a = np.zeros((h, w), np.uint8)
    for x, y in points:
        a[y % h, x % w] = 255
    return a


def ramp(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 255 // (w - 1) + y * 3) & 255).astype(np.uint8)


def blocks(w, h):
    """Saturated regions larger than the 7x7 kernel: 255 and 254 blocks on 0, touching two borders."""
    a = np.zeros((h, w), np.uint8)
    a[0:20, 0:24] = 255
    a[h - 18:h, w - 22:w] = 254
    a[14:34, 30:44] = 255
    return a


# The declared route of every level >= 1 (g generic / k_resize, r k_resize_rows, m k_resize_merge) and whether the plan
# blurs each level (1 / 0), as literals.  tests/cpp/orb_plan_test.cpp carries the aligned cases of this list.
def _decl(routes, blurred):
    return tuple({"g": "generic", "r": "rows", "m": "merge"}[c] for c in routes), tuple(c == "1" for c in blurred)


DECLARED = {
    "route_131x77_1.25": ("mm", "111"),
    "route_131x77_1.26": ("mm", "111"),
    "route_131x77_1.3": ("rr", "111"),
    "route_131x77_2": ("rr", "110"),
    "route_131x77_2.01": ("rr", "110"),
    "route_131x77_2.5": ("gg", "100"),
    "route_131x77_3": ("gg", "100"),
    "route_131x77_4": ("g", "10"),
    "route_128x96_1.3334": ("m", "11"),
    "route_131x77_1.3_sizes": ("rrr", "1110"),
    "merge_h11": ("mmmmmmm", "11000000"),
    "merge_h12": ("mmmmmm", "1000000"),
    "merge_h13": ("mmmmmm", "1100000"),
    "merge_h47": ("m", "11"),
    "merge_h48": ("m", "11"),
    "merge_h49": ("m", "11"),
    "rows_h7_w2": ("gggr", "10000"),
    "rows_h8": ("rrr", "1000"),
    "rows_h9": ("rrr", "1000"),
    "rows_h31": ("r", "10"),
    "rows_h32": ("r", "10"),
    "rows_h33": ("r", "10"),
    "tiny_levels_100x80": ("rrgmmm", "1100000"),
    "tiny_levels_100x80_8": ("rrgmmmm", "11000000"),
    "merge_w48": ("m", "11"),
    "merge_w49": ("m", "11"),
    "merge_w45": ("m", "11"),
    "merge_w47": ("m", "11"),
    "rows_w48": ("r", "10"),
    "rows_w49": ("r", "10"),
    "rows_w45": ("r", "10"),
    "rows_w46": ("r", "10"),
    "generic_w49": ("g", "10"),
    "generic_w52": ("g", "10"),
    "generic_w45": ("g", "10"),
    "generic_w47": ("g", "10"),
    "tail_w45": ("mm", "110"),
    "tail_w46": ("mm", "110"),
    "tail_w47": ("mm", "110"),
    "tail_w48": ("mm", "110"),
    "tail_w49": ("mm", "110"),
    "tail_w50": ("mm", "110"),
    "tail_w51": ("mm", "110"),
    "tail_w52": ("mm", "110"),
    "tail_w56": ("mm", "110"),
    "tail_w60": ("mm", "110"),
    "tail_w64": ("mm", "110"),
    "tail_w72": ("mm", "110"),
    "tail_w76": ("mm", "110"),
    "wide_513x45": ("m", "11"),
    "const_0": ("m", "11"),
    "const_100": ("m", "11"),
    "const_253": ("m", "11"),
    "const_254": ("m", "11"),
    "const_255": ("m", "11"),
    "const_255_260x45": ("m", "11"),
    "checker": ("m", "11"),
    "stripes_v": ("m", "11"),
    "stripes_h": ("m", "11"),
    "stripes_v_50x47": ("r", "10"),
    "stripes_h_50x47": ("r", "10"),
    "impulse_corners": ("m", "11"),
    "impulse_edges": ("m", "11"),
    "impulse_edges_51x46": ("r", "10"),
    "ramp": ("m", "11"),
    "blocks": ("m", "11"),
    "blur_w45": ("", "1"),
    "blur_w46": ("", "1"),
    "blur_w47": ("", "1"),
    "blur_w48": ("", "1"),
    "blur_w49": ("", "1"),
    "blur_w50": ("", "1"),
    "blur_w51": ("", "1"),
    "blur_w52": ("", "1"),
    "blur_w255": ("", "1"),
    "blur_w256": ("", "1"),
    "blur_w257": ("", "1"),
    "blur_w258": ("", "1"),
    "blur_w259": ("", "1"),
    "blur_w260": ("", "1"),
    "blur_w263": ("", "1"),
    "blur_w264": ("", "1"),
    "blur_w511": ("", "1"),
    "blur_w512": ("", "1"),
    "blur_w513": ("", "1"),
    "blur_h45": ("", "1"),
    "blur_h63": ("", "1"),
    "blur_h64": ("", "1"),
    "blur_h65": ("", "1"),
    "blur_h66": ("", "1"),
    "blur_h67": ("", "1"),
    "blur_h70": ("", "1"),
    "blur_h95": ("", "1"),
    "blur_h96": ("", "1"),
    "blur_h97": ("", "1"),
    "blur_38_beside_37": ("mmmmmmm", "11111110"),
    "blur_batch3": ("mmm", "1100"),
    "align_m_a": ("mm", "111"),
    "align_m_b1": ("gm", "111"),
    "align_m_b2": ("gm", "111"),
    "align_m_b3": ("gm", "111"),
    "align_m_c133_00": ("gm", "111"),
    "align_m_c134_00": ("gm", "111"),
    "align_m_c135_00": ("gm", "111"),
    "align_m_d_00": ("gm", "111"),
    "align_m_e_00": ("mm", "111"),
    "align_m_c133_ff": ("gm", "111"),
    "align_m_c134_ff": ("gm", "111"),
    "align_m_c135_ff": ("gm", "111"),
    "align_m_d_ff": ("gm", "111"),
    "align_m_e_ff": ("mm", "111"),
    "align_r_a": ("rr", "110"),
    "align_r_b1": ("gr", "110"),
    "align_r_b2": ("gr", "110"),
    "align_r_b3": ("gr", "110"),
    "align_r_c133_00": ("gr", "110"),
    "align_r_c134_00": ("gr", "110"),
    "align_r_c135_00": ("gr", "110"),
    "align_r_d_00": ("gr", "110"),
    "align_r_e_00": ("rr", "110"),
    "align_r_c133_ff": ("gr", "110"),
    "align_r_c134_ff": ("gr", "110"),
    "align_r_c135_ff": ("gr", "110"),
    "align_r_d_ff": ("gr", "110"),
    "align_r_e_ff": ("rr", "110"),
    "align_g_a": ("gg", "100"),
    "align_g_b1": ("gg", "100"),
    "align_g_b2": ("gg", "100"),
    "align_g_b3": ("gg", "100"),
    "align_g_c133_00": ("gg", "100"),
    "align_g_c134_00": ("gg", "100"),
    "align_g_c135_00": ("gg", "100"),
    "align_g_d_00": ("gg", "100"),
    "align_g_e_00": ("gg", "100"),
    "align_g_c133_ff": ("gg", "100"),
    "align_g_c134_ff": ("gg", "100"),
    "align_g_c135_ff": ("gg", "100"),
    "align_g_d_ff": ("gg", "100"),
    "align_g_e_ff": ("gg", "100"),
}
ROUTES = {k: _decl(*v)[0] for k, v in DECLARED.items()}
BLURRED = {k: _decl(*v)[1] for k, v in DECLARED.items()}

RESIZE_KILLS = ("no_half", "scale_from_factor", "no_shift4", "no_plus2")
BLUR_KILLS = ("border_reflect", "kernel_256", "no_round")


def _build():
    c = []
    # ---- routes ----
    for sf, nl in ((1.25, 3), (1.26, 3), (1.3, 3), (2.0, 3), (2.01, 3), (2.5, 3), (3.0, 3), (4.0, 2)):
        c.append(Case("route_131x77_%g" % sf, "routes", noise(11, 131, 77), sf, nl, stride=132, kills=RESIZE_KILLS))
    c.append(Case("route_128x96_1.3334", "routes", noise(12, 128, 96), 1.3334, 2, kills=RESIZE_KILLS))
    c.append(Case("route_131x77_1.3_sizes", "routes", noise(13, 131, 77), 1.3, 4, stride=132, kills=("size_from_previous",)))
    # ---- heights ----
    for name, w, h, sf, nl in (("merge_h11", 64, 51, 1.25, 8), ("merge_h12", 64, 45, 1.25, 7), ("merge_h13", 64, 48, 1.25, 7),
                               ("merge_h47", 64, 56, 1.2, 2), ("merge_h48", 64, 57, 1.2, 2), ("merge_h49", 64, 59, 1.2, 2),
                               ("rows_h7_w2", 45, 188, 2.25, 5), ("rows_h8", 64, 67, 2.0, 4), ("rows_h9", 64, 69, 2.0, 4),
                               ("rows_h31", 64, 46, 1.5, 2), ("rows_h32", 64, 48, 1.5, 2), ("rows_h33", 64, 49, 1.5, 2),
                               ("tiny_levels_100x80", 100, 80, 2.0, 7), ("tiny_levels_100x80_8", 100, 80, 2.0, 8)):
        c.append(Case(name, "heights", noise(20 + len(c), w, h), sf, nl, stride=(w + 3) & ~3))
    # ---- widths ----
    for route, sf, ws in (("merge", 1.2, (48, 49, 45, 47)), ("rows", 1.5, (48, 49, 45, 46)), ("generic", 2.5, (49, 52, 45, 47))):
        for w in ws:
            c.append(Case("%s_w%d" % (route, w), "widths", noise(40 + w, w, 64), sf, 2, stride=(w + 3) & ~3, fill=0xFF))
    for w in (45, 46, 47, 48, 49, 50, 51, 52, 56, 60, 64, 72, 76):
        c.append(Case("tail_w%d" % w, "widths", noise(60 + w, w, 48), 1.2, 3, stride=(w + 3) & ~3, fill=0xFF))
    c.append(Case("wide_513x45", "widths", noise(70, 513, 45), 1.2, 2, stride=516, fill=0xFF, kills=("weights_half_up",)))
    # ---- content ----
    for v in (0, 100, 253, 254, 255):
        c.append(Case("const_%d" % v, "content", const(v, 64, 48), 1.2, 2, kills=("no_clamp",) if v >= 254 else ()))
    c.append(Case("const_255_260x45", "content", const(255, 260, 45), 1.2, 2, kills=("no_clamp",)))
    c.append(Case("checker", "content", checker(64, 48), 1.2, 2, kills=("border_reflect", "no_half")))
    c.append(Case("stripes_v", "content", stripes(64, 48, True), 1.2, 2, kills=("border_reflect",)))
    c.append(Case("stripes_h", "content", stripes(64, 48, False), 1.2, 2, kills=("border_reflect",)))
    c.append(Case("stripes_v_50x47", "content", stripes(50, 47, True), 1.5, 2, stride=52))
    c.append(Case("stripes_h_50x47", "content", stripes(50, 47, False), 1.5, 2, stride=52))
    corners = [(0, 0), (-1, 0), (0, -1), (-1, -1)]
    edges = [(0, 20), (1, 24), (-1, 28), (-2, 32), (20, 0), (24, 1), (28, -1), (32, -2)]
    c.append(Case("impulse_corners", "content", impulses(64, 48, corners), 1.2, 2, kills=("border_reflect", "kernel_256")))
    c.append(Case("impulse_edges", "content", impulses(64, 48, edges), 1.2, 2, kills=("border_reflect",)))
    c.append(Case("impulse_edges_51x46", "content", impulses(51, 46, corners + edges), 2.0, 2, stride=52))
    c.append(Case("ramp", "content", ramp(64, 48), 1.2, 2, kills=("no_round", "no_plus2")))
    c.append(Case("blocks", "content", blocks(64, 48), 1.2, 2, kills=("no_clamp",)))
    # ---- blur ----
    for w in (45, 46, 47, 48, 49, 50, 51, 52, 255, 256, 257, 258, 259, 260, 263, 264, 511, 512, 513):
        c.append(Case("blur_w%d" % w, "blur", noise(100 + w, w, 45), 1.2, 1, kills=BLUR_KILLS if w == 257 else ()))
    for h in (45, 63, 64, 65, 66, 67, 70, 95, 96, 97):
        c.append(Case("blur_h%d" % h, "blur", noise(700 + h, 48, h), 1.2, 1, kills=BLUR_KILLS if h == 65 else ()))
    c.append(Case("blur_38_beside_37", "blur", noise(90, 45, 45), 1.027, 8, stride=48))
    c.append(Case("blur_batch3", "blur", np.stack([noise(91 + i, 64, 52) for i in range(3)]), 1.2, 4))
    # ---- align: one image five ways ----
    for tag, sf in (("m", 1.25), ("r", 2.0), ("g", 2.5)):
        img, other = noise(300, 132, 77), noise(301, 132, 77)
        g = "align_" + tag
        c.append(Case(g + "_a", "align", img, sf, 3, group=g))
        for o in (1, 2, 3):
            c.append(Case(g + "_b%d" % o, "align", img, sf, 3, offset=o, group=g))
        for fill in (0x00, 0xFF):
            f = "_ff" if fill else "_00"
            for s in (133, 134, 135):
                c.append(Case(g + "_c%d%s" % (s, f), "align", img, sf, 3, stride=s, fill=fill, group=g))
            c.append(Case(g + "_d" + f, "align", np.stack([other, img]), sf, 3, gap=2, fill=fill, group=g))
            c.append(Case(g + "_e" + f, "align", img, sf, 3, stride=132 + 64, fill=fill, group=g))
    return c


_CACHE = {}


def model(case, b=0, variant=None):
    """(sizes, levels, blurred levels or None where the plan does not blur) of image b of a case."""
    key = (case.imgs[b].tobytes(), case.w, case.scale, case.nlevels, variant)
    if key not in _CACHE:
        sizes = R.level_sizes(case.w, case.h, case.scale, case.nlevels, variant)
        lv = R.pyramid(case.imgs[b], case.scale, case.nlevels, variant)
        bv = variant if variant in R.BLUR_VARIANTS else None
        bl = [R.gaussian_blur7(x, bv) if R.blurred_by_plan(x.shape[1], x.shape[0]) else None for x in lv]
        _CACHE[key] = (sizes, lv, bl)
    return _CACHE[key]


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FAMILIES = ("routes", "heights", "widths", "content", "blur", "align")

# the literal answers of the constant images: value -> blurred value (257 * 257 = 66049; 253 is the largest value that
# reaches 255 without the clamp, 254 and 255 give 256 and 257 before it)
CONST_BLUR = {0: 0, 100: 101, 253: 255, 254: 255, 255: 255}
