"""extractorBird->compute at the refined bird positions inside Frame construction (fb_frame_set_bird_redescribe +
fb_frame_set_bird_subpix + fb_frame_extract_dev, csrc/track.hip; Frame.cc:345-355) on the scenes and handles of
tests/test_frame_subpix_gpu.py: with both switches on the bird descriptors are the literal model (tests/describe_at_ref.py,
angles kept) at the refined positions and nothing else of the frame moves; with cornerSubPix off the switch changes no byte.

The model reads the bird extractor's own pyramid and blurred levels (fb_orb_get_level / fb_orb_get_blurred_level), as
tests/test_orb_cases_gpu.py does.  Descriptors and status bytes are compared as integers: no tolerance enters.  The refined
positions themselves are held to tests/subpix_ref.py by tests/test_frame_subpix_gpu.py, within one ulp and with the few
points whose exit decision lies inside the summation noise set aside; here the descriptors are compared with the model at
the positions the handle holds (every point), and with the model at the positions of tests/subpix_ref.py wherever both
round to the same pixel of the level (all but at most 1 % of the points, the share that test sets aside)."""
import ctypes as C

import numpy as np
import pytest

import fishbirdeyevisualslam_amd as fb
from fishbirdeyevisualslam_amd import cabi, synth

import describe_at_ref as D
import hip_lib as H
import subpix_ref as R
from orb_image_ref import inv_scale_factors
from test_frame_subpix_gpu import FRONT_KEYS, _chain, _same_grid

pytestmark = pytest.mark.gpu

BIRD_KEYS = ("n_bird", "kps_bird", "bird_cam_xyz", "map_point_bird", "bird_outlier")


def _bird_params():
    p = cabi.OrbParams(**synth.ORB_DEFAULT)
    p.nfeatures = 200
    return p


def _bird_levels(tc, p):
    """[(pyramid, blurred)] per sequence: the levels the bird extractor holds from its last call."""
    o = H.Orb.__new__(H.Orb)
    o.h = tc.orb_b
    out = []
    for s in range(tc.B):
        pyr = [o.level(s, l, tc.bw * tc.bh) for l in range(p.nlevels)]
        out.append((pyr, [o.blurred_level(s, l) if min(pyr[l].shape) >= 38 else None for l in range(p.nlevels)]))
    return out


@pytest.fixture(scope="module")
def runs():
    import torch
    seq, tc = _chain(9700)
    f, b, c = seq.render(0)
    mask = torch.from_numpy(seq.mask).cuda()
    out = {}
    tc.extract(f, b, c, mask)
    out["off"] = (tc.view("cur"), tc.bird_grid("cur"))
    tc.set_bird_subpix(5, 40, 1e-3)
    tc.extract(f, b, c, mask)
    out["subpix"] = (tc.view("cur"), tc.bird_grid("cur"))
    tc.set_bird_redescribe(True)
    tc.extract(f, b, c, mask)
    out["both"] = (tc.view("cur"), tc.bird_grid("cur"))
    out["status"] = tc.bird_describe_status("cur")
    p = _bird_params()
    out["p"], out["levels"], out["bird"] = p, _bird_levels(tc, p), b.cpu().numpy()
    tc.close()
    return out


def test_both_switches_describe_at_the_refined_positions(runs):
    (off, _), (sub, grid_sub), (both, grid_both) = runs["off"], runs["subpix"], runs["both"]
    p = runs["p"]
    inv = inv_scale_factors(p.scale_factor, p.nlevels)
    for k in FRONT_KEYS + BIRD_KEYS:     # bird key points, mvKeysBirdCamXYZ and everything of the front side: the same bytes
        assert both[k].tobytes() == sub[k].tobytes(), k
    _same_grid(grid_both, grid_sub)
    assert sub["desc_bird"].tobytes() == off["desc_bird"].tobytes()     # cornerSubPix alone leaves the descriptors
    total = differ_model = differ_gpu = other_pixel = 0
    for s in range(2):
        nb = int(both["n_bird"][s])
        assert nb >= 10
        k = both["kps_bird"][s, :nb]
        pyr, blur = runs["levels"][s]
        desc, _, status = D.describe_at(p, pyr, blur, k, D.KEEP_ANGLE)
        ok = status == D.OK
        np.testing.assert_array_equal(both["desc_bird"][s, :nb][ok], desc[ok])
        # a refused point keeps the descriptor of its unrefined position, at its index
        np.testing.assert_array_equal(both["desc_bird"][s, :nb][~ok], off["desc_bird"][s, :nb][~ok])
        assert both["desc_bird"][s, nb:].tobytes() == sub["desc_bird"][s, nb:].tobytes()
        # the same at the positions tests/subpix_ref.py gives for the key points of the switch-off run
        k0 = off["kps_bird"][s, :nb]
        m = R.corner_subpix(runs["bird"][s], np.stack([k0["x"], k0["y"]], 1), (5, 5), 40, 1e-3)
        km = k0.copy()
        km["x"], km["y"] = m.pts[:, 0], m.pts[:, 1]
        desc_m, _, status_m = D.describe_at(p, pyr, blur, km, D.KEEP_ANGLE)
        for i in range(nb):
            total += 1
            s_inv = inv[int(k["octave"][i])]
            same_pixel = all(np.rint(np.float32(a * s_inv)) == np.rint(np.float32(c * s_inv)) or (np.isnan(a) and np.isnan(c))
                             for a, c in ((k["x"][i], km["x"][i]), (k["y"][i], km["y"][i])))
            if not same_pixel:
                other_pixel += 1
                continue
            assert status_m[i] == status[i]
            if status_m[i] == D.OK:
                np.testing.assert_array_equal(both["desc_bird"][s, i], desc_m[i])
                differ_model += not np.array_equal(desc_m[i], off["desc_bird"][s, i])
        differ_gpu += int((both["desc_bird"][s, :nb] != off["desc_bird"][s, :nb]).any(axis=1).sum())
    print("%d bird key points, %d re-described differently (model: %d), %d set aside" % (total, differ_gpu, differ_model, other_pixel))
    assert other_pixel <= 0.01 * total
    assert differ_model >= 1 and differ_gpu >= 1     # the scene is one where the model says re-describing matters


def test_status_download_is_the_models(runs):
    both, _ = runs["both"]
    seen = set()
    for s in range(2):
        nb = int(both["n_bird"][s])
        pyr, blur = runs["levels"][s]
        _, _, status = D.describe_at(runs["p"], pyr, blur, both["kps_bird"][s, :nb], D.KEEP_ANGLE)
        np.testing.assert_array_equal(runs["status"][s, :nb], status)
        seen |= set(int(v) for v in status)
    assert D.OK in seen


def test_without_subpix_the_switch_changes_nothing():
    import torch
    seq, tc = _chain(9710)
    f, b, c = seq.render(0)
    mask = torch.from_numpy(seq.mask).cuda()
    tc.extract(f, b, c, mask)
    v0, g0 = tc.view("cur"), tc.bird_grid("cur")
    tc.set_bird_redescribe(True)
    tc.extract(f, b, c, mask)
    v1, g1 = tc.view("cur"), tc.bird_grid("cur")
    for k in v0:
        assert v0[k].tobytes() == v1[k].tobytes(), k
    _same_grid(g0, g1)
    st = np.zeros((tc.B, tc.cap), np.uint8)
    rc = fb.lib().fb_frame_download_bird_describe_status(tc.cur, C.c_void_p(st.ctypes.data), None)
    assert rc == cabi.FB_ERR_ARG and b"did not re-describe" in fb.lib().fb_last_error()
    # off again, then cornerSubPix alone: the descriptors stay those of the unrefined positions, as before the switch existed
    tc.set_bird_redescribe(False)
    tc.set_bird_subpix(5, 40, 1e-3)
    tc.extract(f, b, c, mask)
    v2 = tc.view("cur")
    assert v2["desc_bird"].tobytes() == v0["desc_bird"].tobytes() and v2["kps_bird"].tobytes() != v0["kps_bird"].tobytes()
    tc.close()
