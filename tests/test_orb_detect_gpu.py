"""fb_orb_detect[_dev] (k_det_fast, k_det_select, k_det_emit, csrc/orb_detect.inc) against the literal model
tests/orb_detect_ref.py, bit for bit: n, n_true and every field of every key point, floats as bit patterns; no tolerance enters.
Small scenes (192 x 160, three levels, 46 features, two different images: tests/orb_detect_cases.py).

The key-point array is prefilled with a marker (0xA5 bytes): entries at or past n[b] must still hold it.  Each case ends with
an ordinary extraction on the same handle, which must give what it gave before."""
import ctypes as C

import numpy as np
import pytest

import fishbirdeyevisualslam_amd as fb
from fishbirdeyevisualslam_amd import cabi

import describe_at_ref as D
import hip_lib as H
import orb_detect_cases as K

pytestmark = pytest.mark.gpu

MARK = 0xA5


class Scene:
    """Two images in one flat buffer (any pitch, image stride and base offset) and one extractor handle."""

    def __init__(self, imgs=None, pitch=None, image_stride=None, offset=0, nfeatures=K.NFEATURES):
        self.imgs = imgs if imgs is not None else K.images()
        self.h, self.w = self.imgs[0].shape
        self.pitch = pitch or self.w
        self.image_stride = image_stride or self.pitch * self.h
        self.offset = offset
        self.buf = np.zeros(offset + len(self.imgs) * self.image_stride + 8, np.uint8)
        for b, im in enumerate(self.imgs):
            o = offset + b * self.image_stride
            self.buf[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, :self.w] = im
        self.nfeatures = nfeatures
        self.orb = H.Orb(K.params(nfeatures))
        self.before = self.extract()

    def extract(self):
        return self.orb.extract_batch_dev(self.buf, len(self.imgs), self.w, self.h, self.pitch, self.image_stride, self.offset)

    def still_extracts(self):
        for (k0, d0), (k1, d1) in zip(self.before, self.extract()):
            assert k0.tobytes() == k1.tobytes() and d0.tobytes() == d1.tobytes()

    def detect(self, mask=None, thr=20, kp_stride=None, host=False, mask_pitch=None, n_true=True, expect=cabi.FB_OK):
        """One call; returns (kps [B][stride], n [B], n_true [B])."""
        import torch
        B = len(self.imgs)
        stride = kp_stride or self.orb.cap
        kps = np.full((B, stride * cabi.KP_DTYPE.itemsize), MARK, np.uint8)
        n, nt = np.full(B, -7, np.int32), np.full(B, -7, np.int32)
        a = cabi.OrbDetectArgs()
        a.batch, a.width, a.height, a.stride, a.image_stride = B, self.w, self.h, self.pitch, self.image_stride
        a.fast_threshold, a.kp_stride = thr, stride
        mbuf = None
        if mask is not None:
            mp = mask_pitch or self.w
            mbuf = np.zeros((self.h, mp), np.uint8)
            mbuf[:, :self.w] = mask
            a.mask_stride = mp
        if host:
            cabi.fill(a, images=self.buf[self.offset:], kps=kps, n=n)
            if n_true:
                cabi.fill(a, n_true=nt)
            if mbuf is not None:
                cabi.fill(a, mask=mbuf)
            rc = fb.lib().fb_orb_detect(self.orb.h, C.byref(a))
        else:
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
            self.orb._img = up(self.buf)
            tk, tn, tt = up(kps), up(n), up(nt)
            a.images, a.kps, a.n = self.orb._img.data_ptr() + self.offset, tk.data_ptr(), tn.data_ptr()
            if n_true:
                a.n_true = tt.data_ptr()
            if mbuf is not None:
                tm = up(mbuf)
                a.mask = tm.data_ptr()
            rc = fb.lib().fb_orb_detect_dev(self.orb.h, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            kps, n, nt = tk.cpu().numpy().reshape(B, -1), tn.cpu().numpy().view(np.int32), tt.cpu().numpy().view(np.int32)
        assert rc == expect, (rc, fb.lib().fb_last_error())
        return kps.view(cabi.KP_DTYPE).reshape(B, stride), n, nt


def hold_to_model(scene, got, mask=None, thr=20, with_true=True):
    """Every image of one call against the model, markers included; returns the per-level counts of the model."""
    kps, n, nt = got
    stride = kps.shape[1]
    out = []
    for b, img in enumerate(scene.imgs):
        r = K.model(img, mask, thr, scene.nfeatures)
        want = r.kps
        assert nt[b] == (len(want) if with_true else -7) and n[b] == min(len(want), stride), (b, n[b], nt[b], len(want), r.per_level)
        m = int(n[b])
        for f in cabi.KP_DTYPE.names:
            g, w_ = kps[f][b, :m], want[f][:m].astype(cabi.KP_DTYPE[f])
            assert g.tobytes() == w_.tobytes(), (b, f, np.nonzero(g.view(np.uint32) != w_.view(np.uint32))[0][:5])
        assert (kps[b, m:].view(np.uint8) == MARK).all()
        out.append(r.per_level)
    return out


@pytest.fixture(scope="module")
def scene():
    s = Scene()
    yield s
    s.orb.close()


@pytest.mark.parametrize("thr", [20, 35])
def test_three_situation_scene_at_two_thresholds(scene, thr):
    per = hold_to_model(scene, scene.detect(thr=thr), None, thr)
    if thr == 20:
        for p in per:
            assert K.situations(p, K.N_PER_LEVEL) == {"both", "second", "none"}
    scene.still_extracts()


@pytest.mark.parametrize("mask", ["patch", "254", "patch_wide_pitch"])
def test_masks(scene, mask):
    m = K.mask_254() if mask == "254" else K.patch_mask()
    got = scene.detect(mask=m, mask_pitch=K.W + 13 if mask == "patch_wide_pitch" else None)
    per = hold_to_model(scene, got, m)
    if mask == "254":
        assert all(p[0][0] > 0 and p[1] == p[2] == (0, 0, 0) for p in per)
    else:
        assert all(p[1][0] > 0 for p in per)
    # and the next call without a mask owes nothing to it
    hold_to_model(scene, scene.detect())
    scene.still_extracts()


def test_ties_straddle_both_cuts_and_truncation():
    s = Scene(imgs=[K.tie_image(), K.images()[0]])
    try:
        got = s.detect()
        per = hold_to_model(s, got)
        assert per[0][0][1] > 2 * K.N_PER_LEVEL[0] and per[0][0][2] > K.N_PER_LEVEL[0]
        assert got[2][0] > s.orb.cap == got[1][0]          # the ties overflow the recommended capacity: truncated
        wide = s.detect(kp_stride=int(got[2][0]) + 3)
        hold_to_model(s, wide)
        assert wide[1][0] == wide[2][0] == got[2][0]
        small = s.detect(kp_stride=20)
        hold_to_model(s, small)
        assert list(small[1]) == [20, 20] and (small[2] > 20).all()
        hold_to_model(s, s.detect(kp_stride=20, n_true=False), with_true=False)
        s.still_extracts()
    finally:
        s.orb.close()


def test_wide_pitch_and_unaligned_image_offset():
    imgs = [im[:, :157].copy() for im in K.images()]
    s = Scene(imgs=imgs, pitch=171, image_stride=171 * K.H + 5, offset=3)
    try:
        per = hold_to_model(s, s.detect())
        assert all(sum(c[2] for c in p) > 20 for p in per)
        m = K.patch_mask()[:, :157]
        hold_to_model(s, s.detect(mask=m, mask_pitch=161), m)
        s.still_extracts()
    finally:
        s.orb.close()


def test_host_pointers_equal_device_pointers(scene):
    for m in (None, K.patch_mask()):
        dev, host = scene.detect(mask=m), scene.detect(mask=m, host=True)
        hold_to_model(scene, host, m)
        for a, b in zip(dev, host):
            assert a.tobytes() == b.tobytes()
    scene.still_extracts()


def test_detect_then_describe_gives_the_models_descriptors(scene):
    import torch
    kps, n, _ = scene.detect()
    B, stride = kps.shape
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
    tk, tn = up(kps), up(n)
    td = torch.full((B * stride * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    ts = torch.full((B * stride,), 0xEE, dtype=torch.uint8, device="cuda")
    a = cabi.OrbDescribeArgs()
    a.batch, a.kp_stride, a.angle_mode = B, stride, cabi.FB_DESCRIBE_KEEP_ANGLE
    a.n, a.kps, a.desc, a.status = tn.data_ptr(), tk.data_ptr(), td.data_ptr(), ts.data_ptr()
    fb.check(fb.lib().fb_orb_describe_dev(scene.orb.h, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "describe")
    torch.cuda.synchronize()
    desc, status = td.cpu().numpy().reshape(B, stride, 32), ts.cpu().numpy().reshape(B, stride)
    for b, img in enumerate(scene.imgs):
        pyr, blur = D.levels(img, scene.orb.params)
        m = int(n[b])
        want, _, st = D.describe_at(scene.orb.params, pyr, blur, K.model(img).kps, D.KEEP_ANGLE)
        assert m == len(want) and (st == D.OK).all()
        np.testing.assert_array_equal(status[b, :m], st)
        np.testing.assert_array_equal(desc[b, :m], want)
        assert (desc[b, m:] == 0x5A).all() and (status[b, m:] == 0xEE).all()
    scene.still_extracts()


def test_argument_errors_and_the_empty_call(scene):
    ok = scene.detect()
    assert scene.detect(thr=0, expect=cabi.FB_ERR_ARG)[1].tolist() == [-7, -7]
    assert scene.detect(thr=256, host=True, expect=cabi.FB_ERR_ARG)[1].tolist() == [-7, -7]
    assert scene.detect(mask=K.patch_mask(), mask_pitch=K.W, expect=cabi.FB_OK)[1].tolist() != [-7, -7]
    a = cabi.OrbDetectArgs()
    assert fb.lib().fb_orb_detect(scene.orb.h, C.byref(a)) == cabi.FB_OK          # batch 0: nothing to do
    assert fb.lib().fb_orb_detect_dev(scene.orb.h, C.byref(a), None) == cabi.FB_OK
    a.batch = 1
    assert fb.lib().fb_orb_detect(scene.orb.h, C.byref(a)) == cabi.FB_ERR_ARG     # no arrays
    again = scene.detect()
    for x, y in zip(ok, again):
        assert x.tobytes() == y.tobytes()
    scene.still_extracts()
