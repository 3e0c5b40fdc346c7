"""fb_sim3_solver_dev on one problem of 12 candidates, about 800 correspondences and 300 hypotheses each.

    python profiles/probes/sim3_solver_probe.py [--out profiles/sim3_solver_probe.json]
        whole call: HIP events around one call, median of 50 after 10 warm-ups; and the compiled CPU restatement
        (tests/cpp/sim3_solver_ref.cpp) on one core for the same table.  The restatement is a port without the reference's
        per-point cv::Mat allocations, but it keeps a log per iteration: an estimate of the reference's order of magnitude,
        not a bound on either side.
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/probes/sim3_solver_probe.py --calls 20
        per kernel: 20 calls and nothing else, for the kernel statistics of one profiler run.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cpu_leg(p):
    """-> (ms, the restatement's table).  The compiled class alone: solvers built beforehand, iterate(300) until bNoMore (one
    call per return, a few dozen in all).  It still does the restatement's own bookkeeping per iteration (razor figures, a copy
    of the inlier vector into its log)."""
    import sim3_solver_ref as R
    R.lib()
    tab = R.full_table(p)
    solvers = [R.Solver(p, c) for c in range(p["C"])]
    for S in solvers:
        S.SetRansacParameters(p["ransac_prob"], p["min_inliers"], p["max_iterations"])
    t0 = time.perf_counter()
    for S in solvers:
        while not S.iterate(300)[1]:
            pass
    return (time.perf_counter() - t0) * 1e3, tab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_solver_probe.json"))
    ap.add_argument("--calls", type=int, default=0, help="only run this many calls (for a profiler run)")
    ap.add_argument("--cpu-only", action="store_true", help="only the CPU restatement's leg (needs no device); printed, not written")
    opt = ap.parse_args()
    if opt.cpu_only:
        from fishbirdeyevisualslam_amd import sim3_problem as SP
        print(json.dumps(dict(cpu_restatement_one_core_ms=cpu_leg(SP.make_problem(41, [800 + 7 * c for c in range(12)], n1=2000, n2=2000,
                                                                                   outlier_share=0.4, pixel_noise=0.3))[0])))
        return
    import torch
    import fishbirdeyevisualslam_amd as fb
    from fishbirdeyevisualslam_amd import cabi, sim3_problem as SP
    p = SP.make_problem(41, [800 + 7 * c for c in range(12)], n1=2000, n2=2000, outlier_share=0.4, pixel_noise=0.3)
    a, out, keep = SP.solver_args(p)
    dev = torch.device("cuda:0")
    hold = {}
    for sub, field, key in SP.INPUT_FIELDS:
        if key in keep:
            v = keep[key]
            hold[key] = torch.from_numpy(np.ascontiguousarray(v.view(np.uint8) if v.dtype == cabi.KP_DTYPE else v).copy()).to(dev)
            cabi.fill(a if sub is None else getattr(a, sub), **{field: hold[key]})
    for k in SP.OUTPUT_FIELDS:
        v = out[k]
        hold[k] = torch.from_numpy(np.ascontiguousarray(v.view(np.uint8) if v.dtype == cabi.SIM3_CORR_DTYPE else v).copy()).to(dev)
        cabi.fill(a, **{k: hold[k]})
    lib = fb.lib()
    lib.fb_sim3_solver_workspace.restype = C.c_size_t
    wsb = lib.fb_sim3_solver_workspace(a.n_cand, a.kf1.kf_stride)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    cabi.fill(a, workspace=ws, workspace_bytes=wsb)
    st = torch.cuda.current_stream()

    def call():
        rc = lib.fb_sim3_solver_dev(C.byref(a), C.c_void_p(st.cuda_stream))
        assert rc == 0, lib.fb_last_error()

    if opt.calls:
        for _ in range(opt.calls):
            call()
        torch.cuda.synchronize()
        return
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    cpu_ms, tab = cpu_leg(p)
    res = dict(problem="make_problem(41, 12 candidates, N = 800..877, n1 = n2 = 2000, 40 % outliers)",
               hypotheses=int(sum(t["n_hyp_done"] for t in tab)), correspondences=[int(t["N"]) for t in tab],
               device_call_ms_median=float(np.median(ms)), device_call_ms_min=float(np.min(ms)),
               cpu_restatement_one_core_ms=cpu_ms,
               note="compiled restatement, iterate(300) until bNoMore; no per-point cv::Mat allocations as in the reference, but with the "
                    "restatement's per-iteration log")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    json.dump(res, open(opt.out, "w"), indent=1)


if __name__ == "__main__":
    main()
