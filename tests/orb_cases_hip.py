"""Shared by test_orb_cases_gpu.py and its child process: every case of orb_cases.py through fb_orb_extract and every
batch through fb_orb_extract_batch_dev, with what the comparison needs (key points, descriptors, FAST candidates, HIP's own
pyramid levels and blurred levels) gathered into one dict of arrays."""
import ctypes as C

import numpy as np

import fishbirdeyevisualslam_amd as fb
import hip_lib as H
import orb_cases as K
from fishbirdeyevisualslam_amd import cabi

MIN_BLURRED = 38   # a level narrower or lower than 2 * EDGE_THRESHOLD holds no key point and gets no blurred copy


def _levels(orb, b, nlevels, res, name):
    for l in range(nlevels):
        lv = orb.level(b, l, 1 << 20)
        res["%s_level%d" % (name, l)] = lv
        if min(lv.shape) >= MIN_BLURRED:
            bl = np.zeros_like(lv)
            fb.check(fb.lib().fb_orb_get_blurred_level(orb.h, b, l, C.c_void_p(bl.ctypes.data)), "blurred level")
            res["%s_blur%d" % (name, l)] = bl
        buf = np.zeros(1 << 16, np.uint32)
        n = fb.lib().fb_orb_debug_candidates(orb.h, b, l, C.c_void_p(buf.ctypes.data), len(buf))
        assert 0 <= n <= len(buf), n
        r = buf[:n]
        c = np.stack([r & 0xFFF, (r >> 12) & 0xFFF, r >> 24], 1).astype(np.int32)
        res["%s_cand%d" % (name, l)] = c[np.lexsort((c[:, 0], c[:, 1]))]


def collect():
    import torch
    res = {}
    for c in K.cases():
        orb = H.Orb(c.p)
        try:
            k, d = orb.extract(c.img)
            res[c.name + "_kps"], res[c.name + "_desc"] = k.view(np.uint8).reshape(-1), d
            _levels(orb, 0, c.p.nlevels, res, c.name)
        finally:
            orb.close()
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()
    for bname, p, imgs in K.batches():
        assert len(imgs) <= 8
        stack = np.stack(imgs)
        nb, h, w = stack.shape
        orb = H.Orb(p)
        try:
            d_img = torch.from_numpy(stack.reshape(-1)).to(dev)
            d_kps = torch.zeros(nb * orb.cap * cabi.KP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_desc = torch.zeros(nb * orb.cap * 32, dtype=torch.uint8, device=dev)
            d_n = torch.zeros(nb, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            fb.check(fb.lib().fb_orb_extract_batch_dev(orb.h, C.c_void_p(d_img.data_ptr()), nb, w, h, w, C.c_size_t(w * h),
                                                       C.c_void_p(d_kps.data_ptr()), C.c_void_p(d_desc.data_ptr()),
                                                       C.c_void_p(d_n.data_ptr()), C.c_void_p(st.cuda_stream)), "extract batch")
            st.synchronize()
            n = d_n.cpu().numpy()
            kps = d_kps.cpu().numpy().reshape(nb, orb.cap, cabi.KP_DTYPE.itemsize)
            desc = d_desc.cpu().numpy().reshape(nb, orb.cap, 32)
            for b in range(nb):
                name = "%s_%d" % (bname, b)
                res[name + "_kps"], res[name + "_desc"] = kps[b, :n[b]].reshape(-1).copy(), desc[b, :n[b]].copy()
                _levels(orb, b, p.nlevels, res, name)
        finally:
            orb.close()
    return res


def model_inputs(res, name, nlevels):
    pyr = [res["%s_level%d" % (name, l)] for l in range(nlevels)]
    blur = [res.get("%s_blur%d" % (name, l)) for l in range(nlevels)]
    return pyr, blur
