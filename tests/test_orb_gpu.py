"""GPU parity: HIP ORBextractor (through the C-ABI) vs the CPU oracle, bit-exact."""
import ctypes as C

import numpy as np
import pytest

import fishbirdeyevisualslam_amd as fb
import hip_lib as H
import oracle_lib as O
from fishbirdeyevisualslam_amd import cabi, synth

pytestmark = pytest.mark.gpu


def _cands(orb, b, level, cap=400000):
    buf = np.zeros(cap, np.uint32)
    n = fb.lib().fb_orb_debug_candidates(orb.h, b, level, C.c_void_p(buf.ctypes.data), cap)
    assert 0 <= n <= cap
    r = buf[:n]
    return np.stack([r & 0xFFF, (r >> 12) & 0xFFF, r >> 24], 1).astype(np.int32)


def _check_image(params, img, stagewise=True, blur_where_planned=False):
    orb = H.Orb(params)
    try:
        k_h, d_h = orb.extract(img)
        if stagewise:
            for l in range(params.nlevels):
                lv_o = O.orb_level(params, img, l)
                lv_h = orb.level(0, l, img.size)
                np.testing.assert_array_equal(lv_h, lv_o, err_msg="pyramid level %d" % l)
                # (the plan gives a level that cannot hold a key point no blur strips; the oracle blurs every level)
                if not (blur_where_planned and min(lv_o.shape) < 38):
                    bl_o = np.zeros_like(lv_o)
                    O.lib().orc_gaussian_blur7(C.c_void_p(lv_o.ctypes.data), lv_o.shape[1], lv_o.shape[0], C.c_void_p(bl_o.ctypes.data))
                    bl_h = np.zeros_like(lv_o)
                    fb.check(fb.lib().fb_orb_get_blurred_level(orb.h, 0, l, C.c_void_p(bl_h.ctypes.data)), "blurred level")
                    np.testing.assert_array_equal(bl_h, bl_o, err_msg="blurred level %d" % l)
                c_o = O.orb_candidates(params, img, l)
                c_h = _cands(orb, 0, l)
                so = c_o[np.lexsort((c_o[:, 0], c_o[:, 1]))]
                sh = c_h[np.lexsort((c_h[:, 0], c_h[:, 1]))]
                np.testing.assert_array_equal(sh, so, err_msg="FAST candidates level %d" % l)
        k_o, d_o = O.orb_extract(params, img)
        assert len(k_h) == len(k_o)
        for f in ("octave", "x", "y", "response", "size", "angle"):
            np.testing.assert_array_equal(k_h[f], k_o[f], err_msg=f)
        np.testing.assert_array_equal(d_h, d_o)
        return k_o
    finally:
        orb.close()


def test_tables_match_oracle_and_known_answers():
    p = O.orb_params()
    orb = H.Orb(p)
    t_h, t_o = orb.tables(), O.orb_tables(p)
    orb.close()
    assert bytes(t_h) == bytes(t_o)
    assert list(t_h.features_per_level)[:8] == [434, 362, 302, 251, 209, 175, 145, 122]
    assert list(t_h.umax) == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


@pytest.mark.parametrize("w,h,seed", [(640, 480, 1000), (1280, 720, 1000), (512, 512, 1001), (333, 207, 5)])
def test_extract_matches_oracle(w, h, seed):
    k = _check_image(O.orb_params(), synth.synth_image(seed, w, h))
    assert len(k) > (1500 if w >= 512 else 100)


def test_extract_ini_extractor_and_sparse_images():
    # 2*nFeatures instance (Tracking.cc:133) and an almost flat image (min-threshold retries, few corners)
    _check_image(O.orb_params(nfeatures=4000), synth.synth_image(1002, 640, 480))
    flat = synth.synth_image(1003, 640, 480, n_rect=3, n_disc=2)
    _check_image(O.orb_params(), flat)
    _check_image(O.orb_params(nfeatures=300, nlevels=4), synth.synth_image(1004, 400, 300))


def test_extract_white_noise_and_constant():
    g = synth.rng(77)
    _check_image(O.orb_params(), g.integers(0, 256, (240, 320), dtype=np.uint8))
    k = _check_image(O.orb_params(), np.full((240, 320), 100, np.uint8))
    assert len(k) == 0


@pytest.mark.parametrize("scale,nlevels,nfeat", [(1.5, 5, 1200), (2.0, 4, 800), (1.1, 8, 1500)])
def test_extract_other_pyramids(scale, nlevels, nfeat):
    """Scale factors other than 1.2: the resize window logic (k_resize_rows up to scale 2, generic kernel beyond its
    12-byte window), the level tables and the per-level quotas."""
    _check_image(O.orb_params(nfeatures=nfeat, scale_factor=scale, nlevels=nlevels), synth.synth_image(1010, 800, 600))


def test_extract_4k_image():
    """3840x2160: 8820 FAST cells on level 0 (beyond the 12-bit cell index of the first quadtree key layout)."""
    _check_image(O.orb_params(nfeatures=4000), synth.synth_image(77, 3840, 2160), stagewise=False)


def test_extract_degenerate_pyramid_levels():
    """Levels too small to hold a key point (a few pixels wide) are still resized for the chain but never blurred or
    sampled; a level that rounds to 0 px is refused (cv::resize asserts on an empty Size in the reference too)."""
    img = synth.synth_image(5, 100, 80)
    _check_image(O.orb_params(nfeatures=500, scale_factor=2.0, nlevels=7), img, stagewise=True, blur_where_planned=True)
    orb = H.Orb(O.orb_params(nfeatures=500, scale_factor=2.2, nlevels=8))
    try:
        with pytest.raises(RuntimeError, match="is empty"):
            orb.extract(img)
    finally:
        orb.close()


def test_fast_phase_timers(monkeypatch):
    """fb_orb_debug_timers: with FB_FAST_DBG=20 (read when the handle sizes its workspace) the TIMED instantiation of
    k_fast runs -- same key points, and one workgroup in 16 reports its phase times; reading resets the counters."""
    img = synth.synth_image(1000, 640, 480)
    ref = H.Orb(O.orb_params())
    k0, d0 = ref.extract(img)
    t = (C.c_uint64 * 16)()
    fb.check(fb.lib().fb_orb_debug_timers(ref.h, t), "timers")
    assert list(t)[:12] == [0] * 12          # normal instantiation: nothing is timed
    ref.close()
    monkeypatch.setenv("FB_FAST_DBG", "20")
    orb = H.Orb(O.orb_params())
    try:
        k1, d1 = orb.extract(img)
        np.testing.assert_array_equal(k1, k0)
        np.testing.assert_array_equal(d1, d0)
        fb.check(fb.lib().fb_orb_debug_timers(orb.h, t), "timers")
        waves, total = t[11], t[10]
        assert waves > 0 and total > 0
        assert sum(t[i] for i in range(10)) <= total and t[2] > 0      # phases are disjoint parts of the wave; the sweep ran
        fb.check(fb.lib().fb_orb_debug_timers(orb.h, t), "timers")
        assert t[11] == 0                                              # reading reset them
    finally:
        orb.close()


def test_batch_of_72_images_matches_single_image_calls_and_the_oracle():
    # the batched entry point on a stream of the caller's, three calls back to back on the same buffers: every image of
    # the batch gives what the single-image entry point gives for it, and for three of them what the oracle gives
    import torch
    B, w, h = 72, 320, 240
    p = O.orb_params(nfeatures=500)
    imgs = np.stack([synth.synth_image(4000 + i, w, h) for i in range(B)])
    orb = H.Orb(p)
    try:
        dev = torch.device("cuda:0")
        d_img = torch.from_numpy(imgs.reshape(-1)).to(dev)
        d_kps = torch.zeros(B * orb.cap * cabi.KP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_desc = torch.zeros(B * orb.cap * 32, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(B, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream()
        for _ in range(3):  # back-to-back calls reuse the workspace
            fb.check(fb.lib().fb_orb_extract_batch_dev(orb.h, C.c_void_p(d_img.data_ptr()), B, w, h, w, C.c_size_t(w * h),
                                                       C.c_void_p(d_kps.data_ptr()), C.c_void_p(d_desc.data_ptr()),
                                                       C.c_void_p(d_n.data_ptr()), C.c_void_p(st.cuda_stream)), "extract batch")
        st.synchronize()
        n = d_n.cpu().numpy()
        kps = d_kps.cpu().numpy().view(cabi.KP_DTYPE).reshape(B, orb.cap)
        desc = d_desc.cpu().numpy().reshape(B, orb.cap, 32)
        for b in range(B):
            if b % 24 == 5:
                k1, d1 = O.orb_extract(p, imgs[b])   # the oracle itself for three of them
            else:
                k1, d1 = orb.extract(imgs[b])        # single-image entry point (one stream, pinned by the tests above)
            assert n[b] == len(k1) and n[b] > 100
            for f in ("octave", "x", "y", "response", "size", "angle"):
                np.testing.assert_array_equal(kps[b, : n[b]][f], k1[f], err_msg="image %d %s" % (b, f))
            np.testing.assert_array_equal(desc[b, : n[b]], d1)
    finally:
        orb.close()


def test_batch_extraction_can_be_captured_in_a_graph():
    # fishbird.h: the batch call only enqueues on the caller's stream once its workspace is sized, so it is legal under stream
    # capture; the replayed graph gives the same bytes
    import torch
    B, w, h = 64, 256, 192
    p = O.orb_params(nfeatures=300)
    imgs = np.stack([synth.synth_image(4200 + i, w, h) for i in range(B)])
    orb = H.Orb(p)
    try:
        dev = torch.device("cuda:0")
        d_img = torch.from_numpy(imgs.reshape(-1)).to(dev)
        d_kps = torch.zeros(B * orb.cap * cabi.KP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_desc = torch.zeros(B * orb.cap * 32, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(B, dtype=torch.int32, device=dev)

        def call(stream):
            fb.check(fb.lib().fb_orb_extract_batch_dev(orb.h, C.c_void_p(d_img.data_ptr()), B, w, h, w, C.c_size_t(w * h),
                                                       C.c_void_p(d_kps.data_ptr()), C.c_void_p(d_desc.data_ptr()),
                                                       C.c_void_p(d_n.data_ptr()), C.c_void_p(stream.cuda_stream)), "extract batch")

        st = torch.cuda.Stream()
        call(st)  # direct call (sizes the workspace, which allocates: not under capture)
        st.synchronize()
        ref = (d_n.clone(), d_kps.clone(), d_desc.clone())
        assert int(ref[0].min()) > 50
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call(torch.cuda.current_stream())
        for t in (d_n, d_kps, d_desc):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(d_n, ref[0]) and torch.equal(d_desc, ref[2]) and torch.equal(d_kps, ref[1])
    finally:
        orb.close()


@pytest.mark.parametrize("nf", [2363, 2660, 2700, 3000])
def test_single_level_with_many_features_is_extracted_or_refused_as_capacity(nf):
    # all features on one level: the quadtree's node lists approach the 160 KB of LDS.  Below the limit the result is the
    # oracle's; above it the call is refused with the documented capacity message -- never with a HIP error (the fuzz probe
    # once hit a size the host check let through and hipFuncSetAttribute refused), and the next call works
    p = O.orb_params(nfeatures=nf, nlevels=1, scale_factor=1.759)
    img = synth.synth_image(77, 501, 431)
    try:
        _check_image(p, img, stagewise=False)
    except fb.FishbirdError as e:
        assert "(-3)" in str(e) and "nfeatures too large for the LDS quadtree" in str(e), str(e)
    _check_image(O.orb_params(nfeatures=300), synth.synth_image(78, 200, 160), stagewise=False)


def test_refused_size_leaves_the_handle_usable_at_its_previous_size():
    """A call that prepare() refuses must not touch the handle: 100x80 (all eight levels >= 1 px, the last 1x1; the oracle
    accepts it), then 60x50 on the SAME handle (level 7 rounds to 0 px: refused with "is empty" after the argument checks),
    then the first image again, which must give the first result and the oracle's."""
    p = O.orb_params(nfeatures=500, scale_factor=2.0, nlevels=8)
    img = synth.synth_image(5, 100, 80)
    k_o, d_o = O.orb_extract(p, img)
    orb = H.Orb(p)
    try:
        k0, d0 = orb.extract(img)
        with pytest.raises(RuntimeError, match="is empty"):
            orb.extract(synth.synth_image(6, 60, 50))
        k1, d1 = orb.extract(img)
    finally:
        orb.close()
    assert len(k_o) > 10
    for k, d in ((k0, d0), (k1, d1)):
        assert len(k) == len(k_o)
        for f in ("octave", "x", "y", "response", "size", "angle"):
            np.testing.assert_array_equal(k[f], k_o[f], err_msg=f)
        np.testing.assert_array_equal(d, d_o)
    np.testing.assert_array_equal(k1, k0)
    np.testing.assert_array_equal(d1, d0)
