"""k_blur by level range and the optional side-stream schedule of the batched extractor.

By default the pyramid is blurred in one launch on the caller's stream.  Calls of FB_ORB_SIDE_MIN images or more blur it
on a side stream of the handle, in the groups of levels that FB_ORB_BLUR_CUTS names, each group behind the resize of its
last level.  Both must give the oracle's bytes.  The two settings are read once per process, so the scenarios that force
the fork on for a batch of 2 and cut the pyramid into one launch per level run in ONE child process; its results are
shared by the tests below.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hip_lib as H
import oracle_lib as O
import orb_blur_schedule_common as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _oracle_blurred(params, img, level):
    lv = O.orb_level(params, img, level)
    bl = np.zeros_like(lv)
    O.lib().orc_gaussian_blur7(C.c_void_p(lv.ctypes.data), lv.shape[1], lv.shape[0], C.c_void_p(bl.ctypes.data))
    return bl


@pytest.fixture(scope="module")
def forked(tmp_path_factory):
    """Results of the child process (schedule forced on at batch 2, one blur launch per level) and of the same calls in
    this process, where a batch of 2 stays on the caller's stream."""
    import torch
    out_path = str(tmp_path_factory.mktemp("blur_schedule") / "child.npz")
    env = dict(os.environ, FB_ORB_SIDE_MIN="1", FB_ORB_BLUR_CUTS="0xFE")
    r = subprocess.run([sys.executable, os.path.join(HERE, "orb_blur_schedule_child.py"), out_path], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    child = dict(np.load(out_path))
    p = S.params()
    sets = [S.image_set(k) for k in range(2)]
    h, w = sets[0].shape[1:]
    dev = torch.device("cuda:0")
    here = []
    orb = H.Orb(p)
    try:
        st = torch.cuda.Stream()
        for k in range(2):
            d_img = torch.from_numpy(sets[k].reshape(-1)).to(dev)
            out = S.alloc_outputs(orb, S.B, dev)
            torch.cuda.synchronize()
            S.extract_batch(orb, d_img, S.B, w, h, out, st)
            st.synchronize()
            here.append(S.host(out, orb.cap))
    finally:
        orb.close()
    return {"child": child, "here": here, "sets": sets, "params": p}


@pytest.mark.parametrize("w,h", S.SIZES)
def test_level_range_launches_give_the_whole_pyramid_launch_and_the_oracle(forked, w, h):
    """One k_blur launch per level (child process) against the single launch over [0, nlevels) (this process) and the
    oracle's gaussian_blur7: every blurred level that holds key points byte for byte, and the key points and descriptors
    computed from them.  75 x 61: levels narrower than a 256-column strip, every strip has reflected rows; 260 x 70: a
    second column strip of 4 columns (clamped 12-byte window); 512 x 96: two full column strips."""
    p, child, name = forked["params"], forked["child"], "size%dx%d" % (w, h)
    imgs = S.size_images(w, h)
    orb = H.Orb(p)
    try:
        k1, d1 = orb.extract(imgs[1])
        whole = S.blurred_levels(orb, 0, p.nlevels)
    finally:
        orb.close()
    assert len(whole) >= 2
    assert sorted(whole) == sorted(int(k.rsplit("blur", 1)[1]) for k in child if k.startswith(name + "_blur"))
    for l, buf in whole.items():
        ref = _oracle_blurred(p, imgs[1], l)
        np.testing.assert_array_equal(child["%s_blur%d" % (name, l)], ref, err_msg="level %d: level-range launch vs oracle" % l)
        np.testing.assert_array_equal(buf, ref, err_msg="level %d: whole-pyramid launch vs oracle" % l)
    n = child[name + "_n"]
    for b in range(S.B):
        k_o, d_o = O.orb_extract(p, imgs[b])
        assert n[b] == len(k_o)
        np.testing.assert_array_equal(child[name + "_desc"][b, : n[b]], d_o)
        np.testing.assert_array_equal(child[name + "_kps"][b, : n[b]].reshape(-1), k_o.view(np.uint8).reshape(-1))
    np.testing.assert_array_equal(d1, child[name + "_desc"][1, : n[1]])
    np.testing.assert_array_equal(k1.view(np.uint8).reshape(-1), child[name + "_kps"][1, : n[1]].reshape(-1))


def _same(child, name, ref):
    for key, r in zip(("_n", "_kps", "_desc"), ref):
        np.testing.assert_array_equal(child[name + key], r, err_msg=name + key)


def test_forked_schedule_at_batch_2_equals_the_unforked_run_and_the_oracle(forked):
    p, child = forked["params"], forked["child"]
    for k in range(2):
        n, kps, desc = forked["here"][k]
        assert n.min() > 50
        _same(child, "iso%d" % k, forked["here"][k])
        for b in range(S.B):
            k_o, d_o = O.orb_extract(p, forked["sets"][k][b])
            assert n[b] == len(k_o)
            np.testing.assert_array_equal(kps[b, : n[b]].reshape(-1), k_o.view(np.uint8).reshape(-1))
            np.testing.assert_array_equal(desc[b, : n[b]], d_o)
    # the per-level launches themselves: blurred levels of the second image of the batch
    blurred = sorted(int(k[4:]) for k in child if k.startswith("blur"))   # (level 7 is too small to hold key points)
    assert blurred == list(range(7))
    for l in blurred:
        np.testing.assert_array_equal(child["blur%d" % l], _oracle_blurred(p, forked["sets"][0][1], l), err_msg="level %d" % l)


def test_blurred_buffer_is_reused_across_back_to_back_calls(forked):
    """8 calls on one handle and one stream, alternating two image sets, synchronised once at the end: the blur of call
    k + 1 must not overwrite what k_describe of call k still reads (every side-stream launch waits for an event of the
    caller's stream recorded behind that k_describe)."""
    for i in range(8):
        _same(forked["child"], "seq%d" % i, forked["here"][i % 2])


def test_level_0_blur_has_read_the_images_when_the_call_returns_to_the_stream(forked):
    """The caller overwrites its images on the same stream right behind the call: the level-0 blur on the side stream is
    joined before k_describe, so everything the call reads of the images lies before the overwrite."""
    _same(forked["child"], "overwritten", forked["here"][0])
