"""The constructed extractor cases (tests/orb_cases.py) through fb_orb_extract and fb_orb_extract_batch_dev, held to the
literal model (tests/orb_ref.py) fed with HIP's own pyramid levels and blurred levels: FAST candidates as a set per level,
key points (x, y, size, angle, response as float32 bit patterns, octave) and descriptors in output order.  Everything is
integers, bytes or bit patterns: every comparison is equality.

Both instantiations of k_octree run: 1024 threads in this process (nlevels * batch <= 512 for every call here) and 256
threads in a fresh child process started with FB_OCT_WIDE_MAX=0 (read once per process)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fishbirdeyevisualslam_amd as fb
import hip_lib as H
import orb_cases as K
import orb_cases_hip as G
import orb_ref as R
from fishbirdeyevisualslam_amd import cabi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = K.cases()
BATCH_SLOTS = [(bname, b) for bname, p, imgs in K.batches() for b in range(len(imgs))]
_MODEL = {}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{"nt1024": results of this process, "nt256": results of the child process}"""
    out_path = str(tmp_path_factory.mktemp("orb_cases") / "child.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "orb_cases_child.py"), out_path], env=dict(os.environ, FB_OCT_WIDE_MAX="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    return {"nt1024": G.collect(), "nt256": dict(np.load(out_path))}


def model_on_hip_levels(res, name, p):
    pyr, blur = G.model_inputs(res, name, p.nlevels)
    key = (name, tuple(a.tobytes() for a in pyr), tuple(None if a is None else a.tobytes() for a in blur))
    if key not in _MODEL:
        _MODEL[key] = R.extract(p, pyr, blur)
    return _MODEL[key]


def hold_to_model(res, name, p, img):
    np.testing.assert_array_equal(res[name + "_level0"], img, err_msg="level 0 is the image")
    m = model_on_hip_levels(res, name, p)
    for l in range(p.nlevels):
        c = m["candidates"][l]
        np.testing.assert_array_equal(res["%s_cand%d" % (name, l)], c[np.lexsort((c[:, 0], c[:, 1]))], err_msg="candidates, level %d" % l)
    k = res[name + "_kps"].view(cabi.KP_DTYPE)
    assert len(k) == len(m["kps"]), (len(k), len(m["kps"]))
    for f in ("octave", "x", "y", "response", "size", "angle"):
        np.testing.assert_array_equal(k[f].view(np.uint32), m["kps"][f].view(np.uint32), err_msg=f)
    np.testing.assert_array_equal(res[name + "_desc"], m["desc"])
    return m


@pytest.mark.parametrize("nt", ["nt1024", "nt256"])
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_through_fb_orb_extract(runs, c, nt):
    m = hold_to_model(runs[nt], c.name, c.p, c.img)
    assert c.branch(m), (c.name, "the branch, on HIP's levels")


@pytest.mark.parametrize("nt", ["nt1024", "nt256"])
@pytest.mark.parametrize("bname,b", BATCH_SLOTS, ids=["%s_%d" % s for s in BATCH_SLOTS])
def test_batch_slot_through_fb_orb_extract_batch_dev(runs, bname, b, nt):
    p, imgs = next((p, imgs) for n, p, imgs in K.batches() if n == bname)
    m = hold_to_model(runs[nt], "%s_%d" % (bname, b), p, imgs[b])
    if imgs[b].max() == imgs[b].min():
        assert len(m["kps"]) == 0   # the empty image between two full ones
    else:
        assert len(m["kps"]) > 0


def test_both_instantiations_agree_byte_for_byte(runs):
    a, b = runs["nt1024"], runs["nt256"]
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_plan_limit_is_the_largest_nfeatures_accepted():
    """orb_cases.octree_max_nfeatures() is the edge: the case `n_at_plan_limit` ran with it; one more is refused with the
    quadtree's capacity error, and the refusal is an error, not a shorter answer."""
    c = K.by_name("n_at_plan_limit")
    assert c.p.nfeatures == K.octree_max_nfeatures(320, 300)
    orb = H.Orb(K.params(c.p.nfeatures + 1))
    try:
        with pytest.raises(fb.FishbirdError, match="LDS quadtree"):
            orb.extract(c.img)
    finally:
        orb.close()
