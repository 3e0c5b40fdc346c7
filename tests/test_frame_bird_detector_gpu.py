"""cv::ORB's detector inside Frame construction (fb_frame_set_bird_detector + fb_frame_extract_dev, csrc/track.hip;
Frame.cc:337-355) on the small geometry of tests/test_frame_subpix_gpu.py (640 x 480 front, 384 x 384 bird, 200 bird features).

With the switch on the bird side of the frame is the composition of the models: tests/orb_detect_ref.py with the detect mask
of each image at every level -> GuidenceKeyBirdPts without a mask (the CPU oracle, orc_bird_guidance) -> cornerSubPix when that
switch is on -> tests/describe_at_ref.py with the angles kept; mvKeysBirdCamXYZ and the bird grid are those of the resulting key
points.  Key points, descriptors and status bytes are compared bit for bit.  With cornerSubPix on, the positions are held to
tests/subpix_ref.py as tests/test_frame_subpix_gpu.py holds them (one float ulp; at most 1 % of the points, whose exit decision
lies inside the summation noise, set aside), and the descriptors to the model at the positions the handle holds.
With the switch off, or never called, the frame's outputs are the bytes of a handle on which the setter was never touched."""
import ctypes as C

import numpy as np
import pytest

import fishbirdeyevisualslam_amd as fb
from fishbirdeyevisualslam_amd import cabi, synth

import describe_at_ref as D
import orb_detect_ref as DET
import subpix_ref as R
from oracle import pyoracle as O
from test_bird_guidance import make_args
from test_frame_redescribe_gpu import _bird_levels, _bird_params
from test_frame_subpix_gpu import FRONT_KEYS, _chain, _same_grid, _separately

pytestmark = pytest.mark.gpu

THR = 20


def _same_view(v0, v1):
    """The frame's outputs, byte for byte (slots beyond the counts are whatever the handle's memory held)."""
    assert np.array_equal(v0["n"], v1["n"]) and np.array_equal(v0["n_bird"], v1["n_bird"]) and np.array_equal(v0["counts"], v1["counts"])
    for s in range(len(v0["n"])):
        n, nb = int(v0["n"][s]), int(v0["n_bird"][s])
        for k in ("kps", "kps_un", "desc", "map_point", "outlier"):
            assert v0[k][s, :n].tobytes() == v1[k][s, :n].tobytes(), k
        for k in ("kps_bird", "desc_bird", "bird_cam_xyz", "map_point_bird", "bird_outlier"):
            assert v0[k][s, :nb].tobytes() == v1[k][s, :nb].tobytes(), k


def _model_bird_side(p, bird, contour, mask, cap):
    """Per image: the model's key points after detection and guidance (no cornerSubPix), truncated to the frame's capacity."""
    out = []
    for s in range(bird.shape[0]):
        det = DET.detect(p, bird[s], mask[s], THR).kps[:cap]
        a, o, _keep = make_args([contour[s]], [det.astype(cabi.KP_DTYPE)])
        assert O.lib().orc_bird_guidance(C.byref(a)) == 0
        out.append((det, o["kps_out"][0, : int(o["n_out"][0])].copy()))
        assert 10 <= len(out[-1][1]) < len(det), (len(out[-1][1]), len(det))     # the scene: the contour test drops some, not all
    return out


@pytest.fixture(scope="module")
def runs():
    import torch
    seq, tc = _chain(9700)
    f, b, c = seq.render(0)
    c = c.clone()
    c[:, : c.shape[1] // 2, : c.shape[2] // 2] = 0     # no contour in one quarter: the guidance filter has something to drop
    # one mask per image, each with a region of its own: zeros in image 0, 254 (passes level 0 only) in image 1
    mask_np = np.ascontiguousarray(seq.mask).copy()
    assert mask_np.shape == (2,) + tuple(b.shape[1:])
    mask_np[0, 100:200, 150:300] = 0
    mask_np[1, 200:330, 40:200] = 254
    mask = torch.from_numpy(mask_np).cuda()
    out = {}
    tc.extract(f, b, c, mask)
    out["off"] = (tc.view("cur"), tc.bird_grid("cur"))
    tc.set_bird_detector(True, THR)
    tc.extract(f, b, c, mask)
    out["on"] = (tc.view("cur"), tc.bird_grid("cur"), tc.bird_describe_status("cur"))
    out["sep"] = _separately(tc, out["on"][0]["kps_bird"], out["on"][0]["n_bird"])
    p = _bird_params()
    out["p"], out["levels"] = p, _bird_levels(tc, p)
    tc.set_bird_subpix(5, 40, 1e-3)
    tc.extract(f, b, c, mask)
    out["on_subpix"] = (tc.view("cur"), tc.bird_grid("cur"), tc.bird_describe_status("cur"))
    out["sep_subpix"] = _separately(tc, out["on_subpix"][0]["kps_bird"], out["on_subpix"][0]["n_bird"])
    # back to the extractor: the bytes of the first run
    tc.set_bird_subpix(0)
    tc.set_bird_detector(False)
    tc.extract(f, b, c, mask)
    out["off_again"] = (tc.view("cur"), tc.bird_grid("cur"))
    out["bird"], out["contour"], out["mask"], out["cap"] = b.cpu().numpy(), c.cpu().numpy(), mask_np, tc.cap
    out["model"] = _model_bird_side(p, out["bird"], out["contour"], out["mask"], tc.cap)
    tc.close()
    return out


def test_switch_on_is_the_composition_of_the_models(runs):
    on, grid, status = runs["on"]
    off, _ = runs["off"]
    assert np.array_equal(on["n"], off["n"])
    for s in range(2):
        for k in FRONT_KEYS[1:]:
            assert on[k][s, : on["n"][s]].tobytes() == off[k][s, : on["n"][s]].tobytes(), k
    cam, cs, ci = runs["sep"]
    for s in range(2):
        det, want = runs["model"][s]
        nb = int(on["n_bird"][s])
        assert nb == len(want), (nb, len(want), len(det))
        assert on["kps_bird"][s, :nb].tobytes() == want.tobytes()
        pyr, blur = runs["levels"][s]
        desc, _, st = D.describe_at(runs["p"], pyr, blur, want, D.KEEP_ANGLE)
        assert (st == D.OK).all()
        np.testing.assert_array_equal(status[s, :nb], st)
        np.testing.assert_array_equal(on["desc_bird"][s, :nb], desc)
        assert on["bird_cam_xyz"][s, :nb].tobytes() == cam[s, :nb].tobytes()
        # the scene: the image's own mask matters to the model, and the other image's mask would give other key points
        for other in (None, runs["mask"][1 - s]):
            assert DET.detect(runs["p"], runs["bird"][s], other, THR).kps[: runs["cap"]].tobytes() != det.tobytes()
    _same_grid(grid, (cs, ci))
    assert on["kps_bird"].tobytes() != off["kps_bird"].tobytes()


def test_switch_on_with_cornersubpix(runs):
    on, _, _ = runs["on"]
    sub, grid, status = runs["on_subpix"]
    cam, cs, ci = runs["sep_subpix"]
    total = excluded = moved = 0
    for s in range(2):
        nb = int(sub["n_bird"][s])
        assert nb == int(on["n_bird"][s])
        k0, k1 = on["kps_bird"][s, :nb], sub["kps_bird"][s, :nb]
        for fld in ("size", "angle", "response", "octave"):
            assert k1[fld].tobytes() == k0[fld].tobytes(), fld
        m = R.corner_subpix(runs["bird"][s], np.stack([k0["x"], k0["y"]], 1), (5, 5), 40, 1e-3)
        for i in range(nb):
            total += 1
            gx, gy, mx, my = float(k1["x"][i]), float(k1["y"][i]), float(m.pts[i][0]), float(m.pts[i][1])
            tol = max(float(np.spacing(np.float32(abs(mx)))), float(np.spacing(np.float32(abs(my)))))
            moved += (gx, gy) != (float(k0["x"][i]), float(k0["y"][i]))
            if abs(gx - mx) <= tol and abs(gy - my) <= tol:
                continue
            mg = m.margins[i]
            assert mg.err_rel < 0.022 or mg.det_rel < 1e-6 or mg.edge_px <= tol or mg.revert_px <= tol, (s, i, (gx, gy), (mx, my), mg)
            excluded += 1
        pyr, blur = runs["levels"][s]
        desc, _, st = D.describe_at(runs["p"], pyr, blur, k1, D.KEEP_ANGLE)
        np.testing.assert_array_equal(status[s, :nb], st)
        ok = st == D.OK
        assert ok.sum() >= 0.9 * nb
        np.testing.assert_array_equal(sub["desc_bird"][s, :nb][ok], desc[ok])
        assert sub["bird_cam_xyz"][s, :nb].tobytes() == cam[s, :nb].tobytes()
    _same_grid(grid, (cs, ci))
    assert excluded <= 0.01 * total and moved >= total // 2


def test_switch_off_again_gives_the_first_bytes(runs):
    (v0, g0), (v1, g1) = runs["off"], runs["off_again"]
    _same_view(v0, v1)
    _same_grid(g0, g1)


def test_switch_never_called_or_set_to_the_default_changes_nothing():
    """Two handles of one chain, one never told anything, one set to CVORB and back: the same bytes, grid included."""
    import torch
    seq, tc = _chain(9710)
    f, b, c = seq.render(0)
    mask = torch.from_numpy(np.ascontiguousarray(seq.mask)).cuda()
    told = tc.frames[1]
    tc.set_bird_detector(True, 33, frames=[told])
    tc.set_bird_detector(False, frames=[told])
    views = []
    for k in (0, 1):
        tc.k = k
        tc.extract(f, b, c, mask)
        views.append((tc.view("cur"), tc.bird_grid("cur")))
    (v0, g0), (v1, g1) = views
    _same_view(v0, v1)
    _same_grid(g0, g1)
    assert (v0["n_bird"] >= 10).all()
    # argument checks of the setter
    L = fb.lib()
    assert L.fb_frame_set_bird_detector(told, 2, 20) == cabi.FB_ERR_ARG
    assert L.fb_frame_set_bird_detector(told, cabi.FB_BIRD_DETECT_CVORB, 0) == cabi.FB_ERR_ARG
    assert L.fb_frame_set_bird_detector(told, cabi.FB_BIRD_DETECT_CVORB, 256) == cabi.FB_ERR_ARG
    assert L.fb_frame_set_bird_detector(told, cabi.FB_BIRD_DETECT_ORBEXTRACTOR, 0) == cabi.FB_OK
    tc.close()
