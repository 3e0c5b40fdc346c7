"""Latency of fb_optimize_sim3_dev (event-bracketed medians after warm-up) for (a) one candidate with 150 kept
correspondences, (b) 3 candidates x 150, (c) one candidate whose kept count is the stride; beside it fb_sim3_solver_dev and
fb_match_sim3_dev on problems of the same size, as the scale of the neighbours.  Writes profiles/opt_sim3_probe.json.

    python profiles/probes/opt_sim3_probe.py [out.json]
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fishbirdeyevisualslam_amd as fb  # noqa: E402
from fishbirdeyevisualslam_amd import cabi, kf_problems as KP, opt_sim3_problem as OP, problems as P, sim3_problem as SP, synth  # noqa: E402

WARM, REPS = 10, 50


def dev(v):
    return torch.from_numpy(np.ascontiguousarray(v.view(np.uint8) if v.dtype in (cabi.KP_DTYPE, cabi.SIM3_CORR_DTYPE) else v).copy()).to("cuda:0")


def timed(fn, reset=None):
    st = torch.cuda.current_stream()
    ts = []
    for i in range(WARM + REPS):
        if reset:
            reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        if i >= WARM:
            ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def optimize_case(seed, n_corr, **kw):
    lib = fb.lib()
    p = OP.make_problem(seed, n_corr, **kw)
    a, out, keep = OP.optimize_args(p)
    hold = {}
    for sub, field, key in OP.INPUT_FIELDS:
        hold[key] = dev(keep[key])
        cabi.fill(a if sub is None else getattr(a, sub), **{field: hold[key]})
    for k in OP.OUTPUT_FIELDS:
        hold[k] = dev(out[k])
        cabi.fill(a, **{k: hold[k]})
    m0 = hold["matches12"].clone()
    lib.fb_optimize_sim3_workspace.restype = C.c_size_t
    ws = torch.empty(max(lib.fb_optimize_sim3_workspace(a.n_cand, a.kf1.kf_stride), 16), dtype=torch.uint8, device="cuda:0")
    cabi.fill(a, workspace=ws, workspace_bytes=ws.numel())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        rc = lib.fb_optimize_sim3_dev(C.byref(a), st)
        assert rc == 0, lib.fb_last_error()
    med, mn = timed(run, reset=lambda: hold["matches12"].copy_(m0))  # (the call edits matches12: every repetition starts alike)
    torch.cuda.synchronize()
    return dict(us_median=med, us_min=mn, n_inliers=hold["n_inliers"].cpu().tolist(), n_bad=hold["n_bad"].cpu().tolist())


def neighbours(seed, n_corr, n1, n2):
    """fb_sim3_solver_dev (300 hypotheses per candidate) and fb_match_sim3_dev (one candidate) at the same sizes"""
    import oracle_lib as O
    lib = fb.lib()
    p = SP.make_problem(seed, n_corr, n1=n1, n2=n2, outlier_share=0.1, pixel_noise=0.3, plants=False)
    a, out, keep = SP.solver_args(p)
    hold = []
    for sub, field, key in SP.INPUT_FIELDS:
        if key in keep:
            t = dev(keep[key]); hold.append(t)
            cabi.fill(a if sub is None else getattr(a, sub), **{field: t})
    for k in SP.OUTPUT_FIELDS:
        t = dev(out[k]); hold.append(t)
        cabi.fill(a, **{k: t})
    lib.fb_sim3_solver_workspace.restype = C.c_size_t
    ws = torch.empty(max(lib.fb_sim3_solver_workspace(a.n_cand, n1), 16), dtype=torch.uint8, device="cuda:0")
    cabi.fill(a, workspace=ws, workspace_bytes=ws.numel())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    solver = timed(lambda: lib.fb_sim3_solver_dev(C.byref(a), st))
    q = KP.make_sim3_problem(seed, n1, n2, min(n1, n2) * 2 // 3)
    geom = P.grid_geom(synth.front_grid_geom(KP.W, KP.H))
    g1 = P.build_grid_host([q["kps1"]], geom, O.grid_build, n1)
    g2 = P.build_grid_host([q["kps2"]], geom, O.grid_build, n2)
    a2, o2, (kk1, kk2, mk1, mk2, k2) = KP.sim3_args([q], g1, g2)
    for struct, arrays in ((a2.kf1, kk1), (a2.kf2, kk2), (a2.mp1, mk1), (a2.mp2, mk2), (a2, k2), (a2, o2)):
        for k, v in arrays.items():
            t = dev(v); hold.append(t)
            cabi.fill(struct, **{k: t})
    match = timed(lambda: lib.fb_match_sim3_dev(C.byref(a2), st))
    return dict(sim3_solver_us_median=solver[0], match_sim3_us_median=match[0])


def main():
    res = dict(device=torch.cuda.get_device_name(0), warmup=WARM, reps=REPS, cases={})
    res["cases"]["a_1x150"] = optimize_case(501, [150], n1=400, n2=400, n_outliers=[10])
    res["cases"]["b_3x150"] = optimize_case(502, [150, 150, 150], n1=700, n2=400, n_outliers=[10, 10, 10])
    res["cases"]["c_1x400_stride"] = optimize_case(503, [400], n1=400, n2=400, n_outliers=[20])
    res["neighbours_1_candidate_400_features"] = neighbours(504, [150], 400, 400)
    res["neighbours_3_candidates_700_features"] = neighbours(505, [150, 150, 150], 700, 400)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "opt_sim3_probe.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
