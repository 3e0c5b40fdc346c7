"""cv::cornerSubPix inside Frame construction (fb_frame_set_bird_subpix + fb_frame_extract_dev, csrc/track.hip; Frame.cc:345-352)
on the small geometry of the track-chain tests (640 x 480 front, 384 x 384 bird): with the switch on the bird key points are
the literal model (tests/subpix_ref.py) applied to the key points of a switch-off run, nothing else of the frame moves, and
mvKeysBirdCamXYZ and the bird grid are those of the refined positions; with the switch untouched, or set to 0, the handle
gives the bytes it always gave.

Positions: one float ulp of the coordinate, exit decisions as in tests/test_subpix_gpu.py (the constants and their
measurement are stated there); the bird extractor is held to 200 features so that the serial model stays quick."""
import ctypes as C

import numpy as np
import pytest

import fishbirdeyevisualslam_amd as fb
from fishbirdeyevisualslam_amd import cabi, sequence as S, track as T

import subpix_ref as R

pytestmark = pytest.mark.gpu

FRONT, BIRD = (640, 480), (384, 384)
FRONT_KEYS = ("n", "kps", "kps_un", "desc", "map_point", "outlier")


def _chain(seed):
    seq = S.Sequence(2, 1, seed=seed, front_wh=FRONT, bird_wh=BIRD, fx=250.0, fy=250.0, device="cuda:0")
    tc = T.TrackChain(2, FRONT, BIRD, K=seq.Kc, D=seq.D, bird_nfeatures=200)
    return seq, tc


def _separately(tc, kps_bird, n_bird):
    """fb_bird_keys_to_cam_dev and fb_grid_build_batch_dev on their own, on the given key points."""
    import torch
    L, p = fb.lib(), tc.params
    B, cap = tc.B, tc.cap
    dk = torch.from_numpy(kps_bird.view(np.uint8).reshape(-1).copy()).cuda()
    dn = torch.from_numpy(n_bird.copy()).cuda()
    cam = torch.zeros(B, cap, 3, dtype=torch.float32, device="cuda")
    cs = torch.zeros(B, 32 * 32 + 1, dtype=torch.int32, device="cuda")
    ci = torch.zeros(B, cap, dtype=torch.int32, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)     # the uploads above are on torch's current stream
    Tcb = (C.c_float * 12)(*list(p.Tcb))
    fb.check(L.fb_bird_keys_to_cam_dev(vp(dk), vp(dn), B, cap, p.bird_width, p.bird_height, C.c_double(p.pixel2meter),
                                       C.c_double(p.rear_axle_to_center), Tcb, vp(cam), st), "fb_bird_keys_to_cam_dev")
    g = cabi.GridGeom(0.0, 0.0, np.float32(32.0) / np.float32(p.bird_width), np.float32(32.0) / np.float32(p.bird_height), 32, 32)
    fb.check(L.fb_grid_build_batch_dev(vp(dk), vp(dn), B, cap, C.byref(g), vp(cs), vp(ci), st), "fb_grid_build_batch_dev")
    torch.cuda.synchronize()
    return cam.cpu().numpy(), cs.cpu().numpy(), ci.cpu().numpy()


def _same_grid(a, b):
    (cs_a, ci_a), (cs_b, ci_b) = a, b
    assert np.array_equal(cs_a, cs_b)
    for k in range(cs_a.shape[0]):
        assert np.array_equal(ci_a[k, : cs_a[k, -1]], ci_b[k, : cs_b[k, -1]])


@pytest.mark.parametrize("contour", [True, False])
def test_switch_on_refines_the_bird_side_only(contour):
    import torch
    seq, tc = _chain(9700)
    f, b, c = seq.render(0)
    mask = torch.from_numpy(seq.mask).cuda() if contour else None
    if not contour:
        c = None
    tc.extract(f, b, c, mask)
    off = tc.view("cur")
    tc.set_bird_subpix(5, 40, 1e-3)
    tc.extract(f, b, c, mask)
    on, grid_on = tc.view("cur"), tc.bird_grid("cur")
    bird = b.cpu().numpy()
    assert np.array_equal(on["n_bird"], off["n_bird"]) and (off["n_bird"] >= 10).all(), off["n_bird"]
    for k in FRONT_KEYS:
        assert on[k].tobytes() == off[k].tobytes(), k
    assert on["desc_bird"].tobytes() == off["desc_bird"].tobytes()
    total = excluded = moved = 0
    for s in range(2):
        nb = int(off["n_bird"][s])
        k0, k1 = off["kps_bird"][s], on["kps_bird"][s]
        for fld in ("size", "angle", "response", "octave"):
            assert k1[fld].tobytes() == k0[fld].tobytes(), fld
        assert k1[nb:].tobytes() == k0[nb:].tobytes()
        m = R.corner_subpix(bird[s], np.stack([k0["x"][:nb], k0["y"][:nb]], 1), (5, 5), 40, 1e-3)
        for i in range(nb):
            total += 1
            gx, gy, mx, my = float(k1["x"][i]), float(k1["y"][i]), float(m.pts[i][0]), float(m.pts[i][1])
            tol = max(float(np.spacing(np.float32(abs(mx)))), float(np.spacing(np.float32(abs(my)))))
            moved += (gx, gy) != (float(k0["x"][i]), float(k0["y"][i]))
            if abs(gx - mx) <= tol and abs(gy - my) <= tol:
                continue
            # a different position is a different decision somewhere: only a point whose margin is within the noise may
            mg = m.margins[i]
            assert mg.err_rel < 0.022 or mg.det_rel < 1e-6 or mg.edge_px <= tol or mg.revert_px <= tol, (s, i, (gx, gy), (mx, my), mg)
            excluded += 1
    print("contour %s: %d bird key points, %d moved, %d excluded by margin" % (contour, total, moved, excluded))
    assert excluded <= 0.01 * total and moved >= total // 2
    cam, cs, ci = _separately(tc, on["kps_bird"], on["n_bird"])
    for s in range(2):
        nb = int(on["n_bird"][s])
        assert on["bird_cam_xyz"][s, :nb].tobytes() == cam[s, :nb].tobytes()
    _same_grid(grid_on, (cs, ci))
    tc.close()


def test_switch_untouched_or_zero_changes_nothing():
    """Two handles of one chain, one never told anything, one set to 5 and back to 0: the same bytes, grid included."""
    import torch
    seq, tc = _chain(9710)
    f, b, c = seq.render(0)
    mask = torch.from_numpy(seq.mask).cuda()
    tc.set_bird_subpix(5, 40, 1e-3, frames=[tc.frames[1]])
    tc.set_bird_subpix(0, frames=[tc.frames[1]])
    views = []
    for k in (0, 1):
        tc.k = k
        tc.extract(f, b, c, mask)
        views.append((tc.view("cur"), tc.bird_grid("cur")))
    (v0, g0), (v1, g1) = views
    assert np.array_equal(v0["n"], v1["n"]) and np.array_equal(v0["n_bird"], v1["n_bird"]) and np.array_equal(v0["counts"], v1["counts"])
    for s in range(2):       # (slots beyond n are whatever the handle's memory held)
        n, nb = int(v0["n"][s]), int(v0["n_bird"][s])
        for k in ("kps", "kps_un", "desc", "map_point", "outlier"):
            assert v0[k][s, :n].tobytes() == v1[k][s, :n].tobytes(), k
        for k in ("kps_bird", "desc_bird", "bird_cam_xyz", "map_point_bird", "bird_outlier"):
            assert v0[k][s, :nb].tobytes() == v1[k][s, :nb].tobytes(), k
    _same_grid(g0, g1)
    assert fb.lib().fb_frame_set_bird_subpix(tc.frames[1], 9, 40, C.c_double(1e-3)) == cabi.FB_ERR_ARG
    assert fb.lib().fb_frame_set_bird_subpix(tc.frames[1], 5, 0, C.c_double(1e-3)) == cabi.FB_ERR_ARG
    tc.close()


def test_point_outside_the_image_is_a_key_point_without_a_cell():
    """The ramp scene leaves two points outside the image (one above, one below).  fb_grid_build_batch_dev puts them in no cell
    (PosInGridBirdview: a rounded cell index below 0 or at / beyond the grid) and fb_bird_keys_to_cam_dev still maps them."""
    import torch
    img, pts, _ = R.scenes(5)["ramp"]
    buf, _ = R.padded(img, R.PITCH)
    n = np.array([len(pts)], np.int32)
    kps = np.zeros((1, 8), cabi.KP_DTYPE)
    p = np.asarray(pts, np.float32)
    kps["x"][0, : len(p)], kps["y"][0, : len(p)] = p[:, 0], p[:, 1]
    a = cabi.CornerSubpixArgs()
    cabi.fill(a, batch=1, kp_stride=8, cols=R.COLS, rows=R.ROWS, pitch=R.PITCH, image_stride=buf.size, image=buf, n=n, kps=kps,
              half_win_x=5, half_win_y=5, max_iter=40, eps=1e-3)
    fb.check(fb.lib().fb_corner_subpix(C.byref(a)), "fb_corner_subpix")
    x, y = kps["x"][0, : len(p)], kps["y"][0, : len(p)]
    outside = (x < 0) | (x >= R.COLS) | (y < 0) | (y >= R.ROWS)
    assert list(outside) == [False, False, False, True, True]
    L = fb.lib()
    dk = torch.from_numpy(kps.view(np.uint8).reshape(-1).copy()).cuda()
    dn = torch.from_numpy(n).cuda()
    cs = torch.zeros(1, R.COLS * R.ROWS + 1, dtype=torch.int32, device="cuda")
    ci = torch.full((1, 8), -1, dtype=torch.int32, device="cuda")
    cam = torch.zeros(1, 8, 3, dtype=torch.float32, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = cabi.GridGeom(0.0, 0.0, 1.0, 1.0, R.COLS, R.ROWS)     # one cell per pixel: round(-2.19) < 0, round(48.46) >= rows
    fb.check(L.fb_grid_build_batch_dev(vp(dk), vp(dn), 1, 8, C.byref(g), vp(cs), vp(ci), st), "fb_grid_build_batch_dev")
    Tcb = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    fb.check(L.fb_bird_keys_to_cam_dev(vp(dk), vp(dn), 1, 8, R.COLS, R.ROWS, C.c_double(0.04), C.c_double(1.4), Tcb, vp(cam), st), "cam")
    torch.cuda.synchronize()
    cs, ci, cam = cs.cpu().numpy()[0], ci.cpu().numpy()[0], cam.cpu().numpy()[0]
    assert cs[-1] == 3 and sorted(ci[:3]) == [0, 1, 2]
    assert np.isfinite(cam[: len(p)]).all()
    assert np.allclose(cam[3, 0], (R.ROWS // 2 - float(y[3])) * 0.04 + 1.4, rtol=1e-6) and cam[3, 0] > (R.ROWS // 2) * 0.04 + 1.4
