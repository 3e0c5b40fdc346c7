"""k_describe_at alone, beside k_describe, on the bird image of the benchmark (512 x 512, 1000 features): per-launch time from
the library's own event brackets (fb_prof_only), B = 1 and B = 256, angles kept and IC_Angle.  The key points are the
extractor's own output, so every one of them is accepted.  usage: python profiles/probes/describe_at_probe.py [out.json]"""
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
W = H = 512
REPS = 200


def prof(name, fn, reps):
    fb.check(L.fb_prof_enable(1), "prof"); fb.check(L.fb_prof_only(name.encode()), "only"); fb.check(L.fb_prof_reset(), "reset")
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = (cabi.ProfEntry * 64)()
    n = L.fb_prof_report(out, 64)
    L.fb_prof_enable(0)
    e = [x for x in out[:n] if x.name.decode() == name][0]
    return 1e3 * e.total_ms / e.launches, e.launches


res = {}
for B in (1, 256):
    p = cabi.OrbParams(**synth.ORB_DEFAULT)
    p.nfeatures = 1000
    h = C.c_void_p()
    fb.check(L.fb_orb_create(C.byref(p), C.byref(h)), "create")
    L.fb_orb_capacity.restype = C.c_int
    cap = L.fb_orb_capacity(C.byref(p))
    img = torch.from_numpy(np.stack([synth.synth_image(1500 + i % 8, W, H) for i in range(B)])).cuda()
    kps = torch.zeros(B * cap * cabi.KP_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    status = torch.zeros(B * cap, dtype=torch.uint8, device="cuda")
    n = torch.zeros(B, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    extract = lambda: fb.check(L.fb_orb_extract_batch_dev(h, C.c_void_p(img.data_ptr()), B, W, H, W, C.c_size_t(W * H), C.c_void_p(kps.data_ptr()),
                                                          C.c_void_p(desc.data_ptr()), C.c_void_p(n.data_ptr()), st), "extract")
    for _ in range(3):
        extract()
    torch.cuda.synchronize()
    r = {"key_points_per_image": float(n.float().mean().item())}
    r["k_describe_us"], _ = prof("k_describe", extract, 30 if B > 1 else REPS)
    want = desc.clone()
    for mode, tag in ((cabi.FB_DESCRIBE_KEEP_ANGLE, "keep"), (cabi.FB_DESCRIBE_IC_ANGLE, "ic")):
        a = cabi.OrbDescribeArgs()
        a.batch, a.kp_stride, a.angle_mode = B, cap, mode
        a.n, a.kps, a.desc, a.status = n.data_ptr(), kps.data_ptr(), desc.data_ptr(), status.data_ptr()
        a.images, a.stride, a.image_stride = img.data_ptr(), W, W * H
        call = lambda: fb.check(L.fb_orb_describe_dev(h, C.byref(a), st), "describe")
        for _ in range(5):
            call()
        r["k_describe_at_%s_us" % tag], _ = prof("k_describe_at", call, REPS)
        torch.cuda.synchronize()
        assert torch.equal(desc, want), "the round trip must give the extractor's descriptors"
    res["B=%d" % B] = r
    L.fb_orb_destroy(h)
print(json.dumps(res))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
