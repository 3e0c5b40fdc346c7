"""fb_orb_describe[_dev] (k_describe_at, csrc/orb_describe_at.inc) against the literal model tests/describe_at_ref.py, bit for
bit: descriptors and status bytes as integers, angles as float bit patterns -- the standard tests/test_orb_cases_gpu.py holds
fb_orb_extract to; no tolerance enters.  Small scenes (160 x 120, three levels, about 200 features); the model runs on the
numpy pyramid and blur of tests/orb_image_ref.py, which the fixture checks to be the levels the handle holds.

Every output array is prefilled with a marker (descriptor bytes 0xA5, angles a NaN with a payload, status 0xEE): what the
call must not write -- refused key points, entries at or past n[b], images with n[b] = 0 -- must still hold it.  Each case
ends with an ordinary extraction on the same handle, which must give what it gave before."""
import ctypes as C

import numpy as np
import pytest

import fishbirdeyevisualslam_amd as fb
from fishbirdeyevisualslam_amd import cabi

import describe_at_cases as K
import describe_at_ref as D
import hip_lib as H

pytestmark = pytest.mark.gpu

DESC_MARK, STATUS_MARK = 0xA5, 0xEE
ANGLE_MARK = np.array([0x7FC0A5A5], np.uint32).view(np.float32)[0]
MODES = [D.KEEP_ANGLE, D.IC_ANGLE]
UNTOUCHED = ("x", "y", "size", "response", "octave")


class Scene:
    """Two different images extracted as one batch on one handle, and the numpy levels of each."""

    def __init__(self, w=K.W, h=K.H, pitch=None, image_stride=None, offset=0, seeds=(4100, 4105)):
        self.p = K.params()
        self.w, self.h, self.pitch = w, h, pitch or w
        self.image_stride = image_stride or self.pitch * h
        self.offset = offset
        self.imgs = [K.image(s, w, h) for s in seeds]
        self.buf = np.zeros(offset + len(seeds) * self.image_stride + 8, np.uint8)
        for b, im in enumerate(self.imgs):
            o = offset + b * self.image_stride
            self.buf[o: o + self.pitch * h].reshape(h, self.pitch)[:, :w] = im
        self.orb = H.Orb(self.p)
        self.out = self.extract()
        self.levels = [D.levels(im, self.p) for im in self.imgs]
        for b in range(len(seeds)):
            for l in range(self.p.nlevels):
                np.testing.assert_array_equal(self.orb.level(b, l, w * h), self.levels[b][0][l])
                np.testing.assert_array_equal(self.orb.blurred_level(b, l), self.levels[b][1][l])

    def extract(self):
        return self.orb.extract_batch_dev(self.buf, len(self.imgs), self.w, self.h, self.pitch, self.image_stride, self.offset)

    def still_extracts(self):
        again = self.extract()
        for (k0, d0), (k1, d1) in zip(self.out, again):
            assert k0.tobytes() == k1.tobytes() and d0.tobytes() == d1.tobytes()

    def images_host(self):
        return self.buf[self.offset:]


@pytest.fixture(scope="module")
def scene():
    s = Scene()
    assert all(len(k) >= 100 for k, _ in s.out) and s.out[0][0].tobytes() != s.out[1][0].tobytes()
    yield s
    s.orb.close()


def arrays(lists, stride, mode):
    """The call's arrays for per-image key-point lists: key points beyond a list, all descriptor rows and all status bytes
    hold the markers; in IC mode the angles handed in are the marker too (the mode owes nothing to them)."""
    B = len(lists)
    kps = np.zeros((B, stride), cabi.KP_DTYPE)
    kps["angle"] = ANGLE_MARK
    kps["octave"] = 1
    for b, k in enumerate(lists):
        kps[b, : len(k)] = k
        if mode == D.IC_ANGLE:
            kps["angle"][b, : len(k)] = ANGLE_MARK
    return kps, np.full((B, stride, 32), DESC_MARK, np.uint8), np.full((B, stride), STATUS_MARK, np.uint8)


def describe(scene, kps, desc, status, n, mode, host=False, images=True, batch=None, expect=cabi.FB_OK, orb=None):
    """One call on copies of the arrays; returns (kps, desc, status) after it."""
    import torch
    L = fb.lib()
    orb = orb or scene.orb
    B, stride = kps.shape
    n = np.asarray(n, np.int32)
    a = cabi.OrbDescribeArgs()
    keep = []
    if host:
        k, d, s = kps.copy(), desc.copy(), status.copy()
        img = scene.images_host()
        cabi.fill(a, n=n, kps=k, desc=d, status=s)
        if images:
            cabi.fill(a, images=img)
    else:
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
        tk, td, ts, tn = up(kps), up(desc), up(status), up(n)
        keep = [tk, td, ts, tn]
        a.n, a.kps, a.desc, a.status = tn.data_ptr(), tk.data_ptr(), td.data_ptr(), ts.data_ptr()
        if images:
            a.images = scene.orb._img.data_ptr() + scene.offset
    a.batch, a.kp_stride, a.angle_mode = (B if batch is None else batch), stride, mode
    a.stride, a.image_stride = scene.pitch, scene.image_stride
    if host:
        rc = L.fb_orb_describe(orb.h, C.byref(a))
    else:
        rc = L.fb_orb_describe_dev(orb.h, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    assert rc == expect, (rc, fb.lib().fb_last_error())
    if host:
        return k, d, s
    return (keep[0].cpu().numpy().view(cabi.KP_DTYPE).reshape(B, stride), keep[1].cpu().numpy().reshape(B, stride, 32),
            keep[2].cpu().numpy().reshape(B, stride))


def hold_to_model(scene, lists, n, mode, got, kps_in):
    """The outputs of one call against the model, image by image, markers included."""
    k1, d1, s1 = got
    for f in UNTOUCHED:
        assert k1[f].tobytes() == kps_in[f].tobytes(), f
    counts = {D.OK: 0, D.BORDER: 0, D.LEVEL: 0}
    for b in range(len(lists)):
        m = min(int(n[b]), k1.shape[1])
        pyr, blur = scene.levels[b]
        desc, angle, status = D.describe_at(scene.p, pyr, blur, kps_in[b, :m], mode)
        np.testing.assert_array_equal(s1[b, :m], status)
        ok = status == D.OK
        np.testing.assert_array_equal(d1[b, :m][ok], desc[ok])
        np.testing.assert_array_equal(k1["angle"][b, :m].view(np.uint32), angle.view(np.uint32))
        assert (d1[b, :m][~ok] == DESC_MARK).all()
        assert (d1[b, m:] == DESC_MARK).all() and (s1[b, m:] == STATUS_MARK).all()
        assert k1["angle"][b, m:].tobytes() == kps_in["angle"][b, m:].tobytes()
        for v in counts:
            counts[v] += int((status == v).sum())
    return counts


@pytest.mark.parametrize("empty", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_round_trip_returns_the_extractors_own_descriptors_and_angles(scene, mode, empty):
    lists = [k for k, _ in scene.out]
    stride = scene.orb.cap + 5
    kps, desc, status = arrays(lists, stride, mode)
    n = [len(k) for k in lists]
    n[empty] = 0
    got = describe(scene, kps, desc, status, n, mode)
    counts = hold_to_model(scene, lists, n, mode, got, kps)
    b = 1 - empty
    assert counts[D.OK] == n[b] and counts[D.BORDER] == 0
    np.testing.assert_array_equal(got[1][b, : n[b]], scene.out[b][1])
    np.testing.assert_array_equal(got[0]["angle"][b, : n[b]].view(np.uint32), scene.out[b][0]["angle"].view(np.uint32))
    assert (got[1][empty] == DESC_MARK).all() and (got[2][empty] == STATUS_MARK).all()
    scene.still_extracts()


def moved_lists(scene):
    """Every key point displaced by a fixed pseudo-random offset within +-3 px at level 0.  The seed is the first one for which
    the model's own arithmetic puts, on every level, displaced points just below AND just above a rounding boundary (the
    fraction of pt * mvInvScaleFactor within 0.05 of one half, on either side)."""
    from orb_image_ref import inv_scale_factors
    inv = inv_scale_factors(scene.p.scale_factor, scene.p.nlevels)
    for seed in range(100):
        g = np.random.Generator(np.random.PCG64(seed))
        lists, sides = [], set()
        for k, _ in scene.out:
            k = k.copy()
            k["x"] = (k["x"] + g.uniform(-3, 3, len(k)).astype(np.float32)).astype(np.float32)
            k["y"] = (k["y"] + g.uniform(-3, 3, len(k)).astype(np.float32)).astype(np.float32)
            for c in ("x", "y"):
                for v, o in zip(k[c], k["octave"]):
                    f = np.float32(v * inv[o])
                    fr = float(f) - np.floor(float(f))
                    if 0.45 <= fr < 0.5:
                        sides.add((int(o), "below"))
                    elif 0.5 < fr <= 0.55:
                        sides.add((int(o), "above"))
            lists.append(k)
        if len(sides) == 2 * scene.p.nlevels:
            return lists
    raise AssertionError("no seed puts points on both sides of a rounding boundary on every level")


@pytest.mark.parametrize("mode", MODES)
def test_moved_points_are_the_models(scene, mode):
    lists = moved_lists(scene)
    kps, desc, status = arrays(lists, scene.orb.cap, mode)
    n = [len(k) for k in lists]
    got = describe(scene, kps, desc, status, n, mode)
    counts = hold_to_model(scene, lists, n, mode, got, kps)
    assert counts[D.OK] >= 0.8 * sum(n)
    moved = sum(int((got[1][b, : n[b]] != scene.out[b][1]).any(axis=1).sum()) for b in range(2))
    assert moved >= 0.5 * sum(n)     # the descriptors are those of the new positions, not the old ones
    scene.still_extracts()


@pytest.mark.parametrize("mode", MODES)
def test_border_level_and_non_finite_inputs(scene, mode):
    cases = K.border_cases(scene.p) + K.bad_input_cases(scene.p)
    rows = K.keypoints([r for r, _ in cases])
    lists = [rows, rows[::-1].copy()]
    kps, desc, status = arrays(lists, len(rows) + 3, mode)
    if mode == D.KEEP_ANGLE:    # a finite angle for the accepted ones; the refused ones must give it back untouched
        for b in range(2):
            kps["angle"][b, : len(rows)] = lists[b]["angle"]
    n = [len(rows), len(rows) - 2]
    got = describe(scene, kps, desc, status, n, mode)
    counts = hold_to_model(scene, lists, n, mode, got, kps)
    assert list(got[2][0, : len(rows)]) == [s for _, s in cases]
    assert counts[D.LEVEL] >= 3 and counts[D.BORDER] >= 20 and counts[D.OK] >= 14
    scene.still_extracts()


def test_unaligned_raw_image_takes_the_byte_path():
    """Width 157, pitch 157, an odd image stride and a base one byte into the allocation: no image starts on a dword, so the
    level-0 raw patches of IC mode come through byte loads.  The key points are the extractor's own: IC_Angle and the
    descriptors must be what it returned."""
    s = Scene(w=157, h=K.H, pitch=157, image_stride=157 * K.H + 1, offset=1)
    try:
        lists = [k for k, _ in s.out]
        assert all((k["octave"] == 0).sum() >= 30 for k in lists)
        kps, desc, status = arrays(lists, s.orb.cap, D.IC_ANGLE)
        n = [len(k) for k in lists]
        got = describe(s, kps, desc, status, n, D.IC_ANGLE)
        counts = hold_to_model(s, lists, n, D.IC_ANGLE, got, kps)
        assert counts[D.OK] == sum(n)
        for b in range(2):
            np.testing.assert_array_equal(got[1][b, : n[b]], s.out[b][1])
            np.testing.assert_array_equal(got[0]["angle"][b, : n[b]].view(np.uint32), s.out[b][0]["angle"].view(np.uint32))
        s.still_extracts()
    finally:
        s.orb.close()


@pytest.mark.parametrize("mode", MODES)
def test_host_pointers_equal_device_pointers(scene, mode):
    lists = moved_lists(scene)
    kps, desc, status = arrays(lists, scene.orb.cap + 1, mode)
    n = [len(lists[0]), len(lists[1]) // 2]
    dev = describe(scene, kps, desc, status, n, mode)
    host = describe(scene, kps, desc, status, n, mode, host=True)
    for a, b in zip(dev, host):
        assert a.tobytes() == b.tobytes()
    assert (dev[2][1, : n[1]] == D.OK).sum() >= 0.8 * n[1] and (dev[2][1, n[1]:] == STATUS_MARK).all()
    scene.still_extracts()


def test_argument_errors_leave_nothing_written_and_the_handle_usable(scene):
    lists = [k for k, _ in scene.out]
    n = [len(k) for k in lists]
    kps, desc, status = arrays(lists, scene.orb.cap, D.KEEP_ANGLE)
    untouched = lambda got: got[1].tobytes() == desc.tobytes() and got[2].tobytes() == status.tobytes() and got[0].tobytes() == kps.tobytes()
    # a handle that has never extracted
    fresh = H.Orb(K.params())
    try:
        for host in (False, True):
            assert untouched(describe(scene, kps, desc, status, n, D.KEEP_ANGLE, host=host, expect=cabi.FB_ERR_ARG, orb=fresh))
        assert b"not extracted" in fb.lib().fb_last_error()
        out = fresh.extract_batch_dev(scene.buf, 2, scene.w, scene.h, scene.pitch, scene.image_stride)
        assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(out, scene.out))
    finally:
        fresh.close()
    # batch above the last batch
    k3, d3, s3 = arrays(lists + [lists[0]], scene.orb.cap, D.KEEP_ANGLE)
    for host in (False, True):
        got = describe(scene, k3, d3, s3, n + [n[0]], D.KEEP_ANGLE, host=host, expect=cabi.FB_ERR_ARG)
        assert got[1].tobytes() == d3.tobytes() and got[2].tobytes() == s3.tobytes()
    assert b"last extract call had 2" in fb.lib().fb_last_error()
    # IC mode without the images
    for host in (False, True):
        assert untouched(describe(scene, kps, desc, status, n, D.IC_ANGLE, host=host, images=False, expect=cabi.FB_ERR_ARG))
    assert b"needs the images" in fb.lib().fb_last_error()
    # an angle mode that is neither
    assert untouched(describe(scene, kps, desc, status, n, 2, expect=cabi.FB_ERR_ARG))
    # a smaller batch than the last one is fine
    got = describe(scene, kps[:1], desc[:1], status[:1], n[:1], D.KEEP_ANGLE)
    np.testing.assert_array_equal(got[1][0, : n[0]], scene.out[0][1])
    scene.still_extracts()
