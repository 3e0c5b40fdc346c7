"""fb_orb_detect_dev beside fb_orb_extract_batch_dev on ONE handle, on a 384 x 384 bird image (the size of the track-chain
tests; 8 levels, 2000 features = the reference's cv::ORB::create(2000)): time per call from stream events around REPS back-to-back calls after
warm-up, B = 1 and B = 256, and the per-kernel split of the detect call from the library's own event brackets (fb_prof_enable:
every kernel on the caller's stream; the brackets add event records between the launches, so the parts add up to more than
the call).  usage: python profiles/probes/orb_detect_probe.py [out.json]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import fishbirdeyevisualslam_amd as fb
from fishbirdeyevisualslam_amd import cabi, synth

L = fb.lib()
W = H = 384


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def kernel_split(fn, reps):
    fb.check(L.fb_prof_enable(1), "prof"); fb.check(L.fb_prof_only(None), "only"); fb.check(L.fb_prof_reset(), "reset")
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = (cabi.ProfEntry * 64)()
    n = L.fb_prof_report(out, 64)
    L.fb_prof_enable(0)
    return {x.name.decode(): 1e3 * x.total_ms / reps for x in out[:n] if x.launches}


res = {}
for B in (1, 256):
    p = cabi.OrbParams(2000, 1.2, 8, 20, 7)
    h = C.c_void_p()
    fb.check(L.fb_orb_create(C.byref(p), C.byref(h)), "create")
    L.fb_orb_capacity.restype = C.c_int
    cap = L.fb_orb_capacity(C.byref(p))
    img = torch.from_numpy(np.stack([synth.synth_image(1500 + i % 8, W, H) for i in range(B)])).cuda()
    kps = torch.zeros(B * cap * cabi.KP_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    n = torch.zeros(B, dtype=torch.int32, device="cuda")
    nt = torch.zeros(B, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    extract = lambda: fb.check(L.fb_orb_extract_batch_dev(h, C.c_void_p(img.data_ptr()), B, W, H, W, C.c_size_t(W * H), C.c_void_p(kps.data_ptr()),
                                                          C.c_void_p(desc.data_ptr()), C.c_void_p(n.data_ptr()), st), "extract")
    a = cabi.OrbDetectArgs()
    a.batch, a.width, a.height, a.stride, a.image_stride = B, W, H, W, W * H
    a.images, a.fast_threshold, a.kp_stride = img.data_ptr(), 20, cap
    a.kps, a.n, a.n_true = kps.data_ptr(), n.data_ptr(), nt.data_ptr()
    detect = lambda: fb.check(L.fb_orb_detect_dev(h, C.byref(a), st), "detect")
    reps = 200 if B == 1 else 20
    for _ in range(3):
        extract(); detect()
    r = {"extract_us": timed(extract, reps), "detect_us": timed(detect, reps)}
    r["detect_key_points_per_image"] = float(n.float().mean().item())
    r["detect_untruncated_per_image"] = float(nt.float().mean().item())
    extract()
    torch.cuda.synchronize()
    r["extract_key_points_per_image"] = float(n.float().mean().item())
    r["detect_kernels_us"] = kernel_split(detect, 20 if B == 1 else 5)
    res["B=%d" % B] = r
    L.fb_orb_destroy(h)
print(json.dumps(res))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
