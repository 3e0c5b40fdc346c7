"""k_fast list lengths on the bench's images (B = 64, 1280x720 + 512x512): how many cells list 0, 1-64, 65-128 and more
pixels at iniThFAST (list A), and how long the minThFAST-only list (B) of the redone cells is.  Needs the probe build:
    FB_BUILD_DEFS=-DFB_FAST_LISTHIST python -m fishbirdeyevisualslam_amd.build --force
Prints one JSON object (committed as profiles/r04_fast_list_lengths.json)."""
import sys, json, ctypes as C
sys.path.insert(0, '.')
import numpy as np, torch
import fishbirdeyevisualslam_amd as fb
from fishbirdeyevisualslam_amd import synth
from fishbirdeyevisualslam_amd.pipeline import FramePipeline
B = 64
f = np.stack([synth.synth_image(1000 + i, 1280, 720) for i in range(B)])
b = np.stack([synth.synth_image(1500 + i, 512, 512) for i in range(B)])
pipe = FramePipeline(B)
pipe.set_images(f, b)
L = fb.lib()
assert hasattr(L, "fb_orb_debug_list_hist"), "not the FB_FAST_LISTHIST build"
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
pipe.extract(s); torch.cuda.synchronize()
out = {"batch": B, "bin": "bin k = lists of 8k-7 .. 8k entries, bin 0 = empty, bin 63 = 497 and more"}
for which, orb in (("front", pipe.orb_f), ("bird", pipe.orb_b)):
    t = (C.c_uint64 * 128)()
    fb.check(L.fb_orb_debug_list_hist(orb, t), "hist")   # reset
    pipe.extract(s); torch.cuda.synchronize()
    fb.check(L.fb_orb_debug_list_hist(orb, t), "hist")
    for name, h in (("A", list(t[:64])), ("B_redone", list(t[64:]))):
        n = max(sum(h), 1)
        mean = sum((8 * k - 3.5 if k else 0) * c for k, c in enumerate(h)) / n
        out["%s_%s" % (which, name)] = {"cells": sum(h), "empty": h[0], "1_64": sum(h[1:9]), "65_128": sum(h[9:17]), "129_256": sum(h[17:33]),
                                        "over_256": sum(h[33:]), "mean_len_approx": round(mean, 1), "hist": h}
print(json.dumps(out))
