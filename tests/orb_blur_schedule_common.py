"""Shared by test_orb_blur_schedule_gpu.py and its child process: the inputs and the batched device call."""
import ctypes as C

import numpy as np

import fishbirdeyevisualslam_amd as fb
from fishbirdeyevisualslam_amd import cabi, synth
from oracle import pyoracle as O

B = 2                # images per call of the forced-fork scenarios
WH = (160, 120)      # 8 levels at scale 1.2: levels 0 .. 6 hold key points, level 7 (45 x 33) is too small to be blurred
MIN_BLURRED = 38     # a level narrower or lower than 2 * EDGE_THRESHOLD gets no blur strips


SIZES = [(75, 61), (260, 70), (512, 96)]   # level-range launches: see test_orb_blur_schedule_gpu.py


def size_images(w, h):
    return np.stack([synth.synth_image(8300 + i, w, h) for i in range(B)])


def blurred_levels(orb, b, nlevels):
    """{level: blurred level of image b of the last call}, for the levels large enough to hold key points"""
    out = {}
    for l in range(nlevels):
        lw, lh = level_size(orb, l)
        if min(lw, lh) >= MIN_BLURRED:
            buf = np.zeros((lh, lw), np.uint8)
            fb.check(fb.lib().fb_orb_get_blurred_level(orb.h, b, l, C.c_void_p(buf.ctypes.data)), "blurred level")
            out[l] = buf
    return out


def params():
    return O.orb_params(nfeatures=300)


def image_set(k):
    return np.stack([synth.synth_image(8100 + 10 * k + i, *WH) for i in range(B)])


def alloc_outputs(orb, batch, dev):
    import torch
    return (torch.zeros(batch * orb.cap * cabi.KP_DTYPE.itemsize, dtype=torch.uint8, device=dev),
            torch.zeros(batch * orb.cap * 32, dtype=torch.uint8, device=dev),
            torch.zeros(batch, dtype=torch.int32, device=dev))


def extract_batch(orb, d_img, batch, w, h, out, stream):
    d_kps, d_desc, d_n = out
    fb.check(fb.lib().fb_orb_extract_batch_dev(orb.h, C.c_void_p(d_img.data_ptr()), batch, w, h, w, C.c_size_t(w * h),
                                               C.c_void_p(d_kps.data_ptr()), C.c_void_p(d_desc.data_ptr()),
                                               C.c_void_p(d_n.data_ptr()), C.c_void_p(stream.cuda_stream)), "extract batch")


def host(out, cap):
    """(n, key points [batch, cap, bytes], descriptors [batch, cap, 32]) on the host, everything behind n[b] zeroed"""
    d_kps, d_desc, d_n = out
    n = d_n.cpu().numpy()
    batch = len(n)
    kps = d_kps.cpu().numpy().reshape(batch, cap, cabi.KP_DTYPE.itemsize).copy()
    desc = d_desc.cpu().numpy().reshape(batch, cap, 32).copy()
    for b in range(batch):
        kps[b, n[b]:] = 0
        desc[b, n[b]:] = 0
    return n, kps, desc


def store(res, name, out, cap):
    res[name + "_n"], res[name + "_kps"], res[name + "_desc"] = host(out, cap)


def level_size(orb, level):
    w, h = C.c_int(0), C.c_int(0)
    fb.check(fb.lib().fb_orb_get_level(orb.h, 0, level, None, C.byref(w), C.byref(h)), "fb_orb_get_level")
    return w.value, h.value
