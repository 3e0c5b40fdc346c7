"""Times fb_create_new_map_points_dev on make_new_points_problem(seed, n_nb=20, 2000, 2000): whole call (device
synchronisation, warm-ups), per kernel (fb_prof_*), and the CPU restatement (tests/new_points_ref.py) on one core.

    python3 profiles/probes/new_points_probe.py [OUT.json] [--no-cpu]

Run under `rocprofv3 --kernel-trace --stats -- python3 profiles/probes/new_points_probe.py --no-cpu` for the kernel table."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fishbirdeyevisualslam_amd as fb  # noqa: E402
from fishbirdeyevisualslam_amd import bow_problem as BP, cabi  # noqa: E402


def main():
    out_path = next((a for a in sys.argv[1:] if a.endswith(".json")), None)
    dev = torch.device("cuda:0")
    p = BP.make_new_points_problem(41, n_nb=20, n1=2000, n2=2000)
    a, out, (keep, k1, k2) = BP.new_points_args(p)
    d = {}
    for k, v in list(keep.items()) + list(out.items()):
        if k == "nb_mp_start":
            continue
        d[k] = torch.from_numpy(np.ascontiguousarray(v.view(np.uint8) if v.dtype == cabi.KP_DTYPE else v).copy()).to(dev)
        cabi.fill(a, **{k: d[k]})
    for fv, kk in ((a.fv1, k1), (a.fv2, k2)):
        for name, arr in zip(("n_nodes", "node_ids", "node_start", "items"), kk):
            d[id(fv), name] = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
            cabi.fill(fv, **{name: d[id(fv), name]})
    lib = fb.lib()
    lib.fb_create_new_map_points_workspace.restype = C.c_size_t
    wsb = lib.fb_create_new_map_points_workspace(a.n_nb, a.kf1_stride)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    cabi.fill(a, workspace=ws, workspace_bytes=wsb)
    has1, has2 = d["has_mp1"].clone(), d["has_mp2"].clone()
    s = torch.cuda.current_stream()

    def call():
        d["has_mp1"].copy_(has1)  # in/out: every timed call starts from the same state
        d["has_mp2"].copy_(has2)
        fb.check(lib.fb_create_new_map_points_dev(C.byref(a), C.c_void_p(s.cuda_stream)), "new points")

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    # whole call: events around the call alone (the two in/out resets are outside)
    reps, ms = 50, []
    for _ in range(reps):
        d["has_mp1"].copy_(has1)
        d["has_mp2"].copy_(has2)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fb.check(lib.fb_create_new_map_points_dev(C.byref(a), C.c_void_p(s.cuda_stream)), "new points")
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    # wall clock per call including the host side (synchronised)
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
        torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps * 1e3
    lib.fb_prof_enable(1)
    lib.fb_prof_reset()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    ents = (cabi.ProfEntry * 64)()
    n = lib.fb_prof_report(ents, 64)
    lib.fb_prof_enable(0)
    kern = {ents[i].name.decode(): ents[i].total_ms / ents[i].launches for i in range(n)}
    res = dict(problem="make_new_points_problem(41, n_nb=20, 2000, 2000)", n_new=int(d["n_new"].item()),
               call_ms_median=float(np.median(ms)), call_ms_min=float(np.min(ms)), call_wall_ms_synchronised=wall,
               kernels_ms=kern, nb_skipped=int(d["nb_skipped"].sum().item()))
    if "--no-cpu" not in sys.argv:
        import new_points_ref as R
        os.environ.setdefault("OMP_NUM_THREADS", "1")
        R.create_new_map_points(p)
        t0 = time.perf_counter()
        R.create_new_map_points(p)
        res["cpu_restatement_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
