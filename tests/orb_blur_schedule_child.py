"""Child process of test_orb_blur_schedule_gpu.py: batched ORB extraction with the side-stream blur schedule forced on.

    python orb_blur_schedule_child.py OUT.npz

The caller sets FB_ORB_SIDE_MIN=1 (every batched call forks) and FB_ORB_BLUR_CUTS=0xFE (one blur launch per level);
both are read once per process, hence the process.  Everything is written to OUT.npz and judged by the caller.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import hip_lib as H  # noqa: E402
import orb_blur_schedule_common as S  # noqa: E402


def main(out_path):
    assert os.environ.get("FB_ORB_SIDE_MIN") == "1"
    dev = torch.device("cuda:0")
    p = S.params()
    sets = [S.image_set(k) for k in range(2)]
    B, (h, w) = S.B, sets[0].shape[1:]
    res = {}
    orb = H.Orb(p)
    try:
        st = torch.cuda.Stream()
        d_sets = [torch.from_numpy(s.reshape(-1)).to(dev) for s in sets]

        def outputs(n=1):
            o = [S.alloc_outputs(orb, B, dev) for _ in range(n)]
            torch.cuda.synchronize()  # (zeroed on torch's stream, written on `st`)
            return o

        def call(d_img, out):
            S.extract_batch(orb, d_img, B, w, h, out, st)

        # isolated calls, one per image set, each followed by a synchronisation; blurred levels of the first
        for k in range(2):
            out = outputs()[0]
            call(d_sets[k], out)
            st.synchronize()
            S.store(res, "iso%d" % k, out, orb.cap)
            if k == 0:
                for l, buf in S.blurred_levels(orb, 1, p.nlevels).items():
                    res["blur%d" % l] = buf
        # 8 back-to-back calls on one handle and one stream, alternating the sets, one synchronisation at the end
        outs = outputs(8)
        for i in range(8):
            call(d_sets[i % 2], outs[i])
        st.synchronize()
        for i in range(8):
            S.store(res, "seq%d" % i, outs[i], orb.cap)
        # the caller overwrites its images on the same stream right behind the call
        d_img = d_sets[0].clone()
        torch.cuda.synchronize()
        out = outputs()[0]
        call(d_img, out)
        with torch.cuda.stream(st):
            d_img.copy_(d_sets[1])
            d_img.fill_(0)
        st.synchronize()
        S.store(res, "overwritten", out, orb.cap)
    finally:
        orb.close()
    # the level-range launches at sizes that take the kernel's other paths (a handle per size)
    for (sw, sh) in S.SIZES:
        orb = H.Orb(p)
        try:
            out = S.alloc_outputs(orb, B, dev)
            torch.cuda.synchronize()
            S.extract_batch(orb, torch.from_numpy(S.size_images(sw, sh).reshape(-1)).to(dev), B, sw, sh, out, st)
            st.synchronize()
            S.store(res, "size%dx%d" % (sw, sh), out, orb.cap)
            for l, buf in S.blurred_levels(orb, 1, p.nlevels).items():
                res["size%dx%d_blur%d" % (sw, sh, l)] = buf
        finally:
            orb.close()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main(sys.argv[1])
