"""fb_covis_search_in_neighbors_dev for a key frame of 2000 features with 20 first neighbours and their second neighbours,
against the host route it replaces: one host-pointer fb_fuse_search per target with the literal model's commit
(tests/search_in_neighbors_ref.py) between them.

    python profiles/probes/search_in_neighbors_probe.py [reps]

The device call is timed with events around the whole call, warm-up excluded, on a fresh copy of the map each repetition
(the call edits it); the copy is made outside the events.  Four figures: the call with the exact target count, with
n_targets = 120 (the cost of idle launches), with th = 0 (nothing is committed: the difference is the serial walk's share),
and the host route.  Writes profiles/search_in_neighbors_probe.json and prints it."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from fishbirdeyevisualslam_amd import kf_problems as KP, lib, problems as P, synth  # noqa: E402
from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceMap  # noqa: E402
import covis_ref as CR  # noqa: E402
import loop_fuse_ref as LR  # noqa: E402
import search_in_neighbors_cases as SC  # noqa: E402
import search_in_neighbors_ref as SR  # noqa: E402
from map_correct_ref import set_pose  # noqa: E402

K, S, CUR, CAP = 24, 2000, 23, 120


def xyz(j, depth=10.0):
    u, v = 160.0 + 20.0 * (j % 50), 20.0 + 17.0 * (j // 50)
    return np.array([(u - KP.W / 2.0) / KP.FX * depth, (v - KP.H / 2.0) / KP.FY * depth, depth])


def scene():
    """2000 sites 20 px apart, two map points per site; key frames 0 .. 9 hold the first, 10 .. 22 the second, cur a mix; a
    feature is empty with probability 0.3"""
    g = np.random.default_rng(5)
    D = g.integers(0, 256, (S, 32)).astype(np.uint8)
    point_site = list(range(S)) * 2
    feats = []
    for k in range(K):
        r, pick = g.random(S), g.integers(0, 2, S)
        feats.append([(j, -1 if r[j] < 0.3 else (j + S * int(pick[j]) if k == CUR else j + S * (k >= 10))) for j in g.permutation(S).tolist()])
    c = SC.site_map(K, S, feats, point_site, kf_order=g.permutation(K) * 5 + 2, xyz=xyz, D=D)
    w, gr = LR.World(c), CR.Graph(K, c["kf_order"])
    m = CR.Map(w.kf_n, w.kf_mp, w.kf_octave, w.mp_bad, w.obs_mp, w.obs_kf, w.obs_idx, w.kf_order)
    order = sorted(range(K), key=gr.key)
    for s in order:
        gr.update_connections(m, s)
    return c, gr, order, SR.fuse_targets(gr, CUR, c["kf_bad"], 20, 5)


def device_ms(c, order, n_launch, th, reps, warm=2):
    target = KP.kf_target([dict(kf_kps=c["kf_keys_un"][0], kf_desc=c["kf_desc"][0])], "kf_", np.zeros((1, 64 * 48 + 1), np.int32),
                          np.zeros((1, S), np.int32))[0]
    n_mp, new_edge_cap = len(c["mp_bad"]), 8 * S
    times = []
    for r in range(warm + reps):
        G = CovisibilityGraph(K)                                           # the call ends with UpdateConnections(cur): a fresh graph too
        m = DeviceMap(c, obs_spare=new_edge_cap)
        t, fuse = G.point_fuse_arrays(m, c["kf_bad"], c["kf_desc"], c["mp_desc"], c["mp_found"], c["mp_visible"], replaced_cap=n_mp)
        rt, refresh = G.refresh_arrays(m, c["kf_Tcw"], c["kf_bad"], c["kf_desc"], c["scale_factors"], c["mp_xw"], c["mp_ref_kf"], c["mp_normal"],
                                       c["mp_min_dist"], c["mp_max_dist"], c["mp_desc"])
        G.update_connections(m, order)
        G.reserve_search_in_neighbors(n_mp, m.n_obs, new_edge_cap, S, CAP, n_mp, 64 * 48)
        d_n, d_t = G.fuse_targets(CUR, c["kf_bad"], 20, 5, target_cap=CAP)
        torch.cuda.synchronize()
        n_real = int(d_n.cpu()[0])
        n = n_real if n_launch is None else n_launch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = G.search_in_neighbors(m, fuse, refresh, target, CUR, S, n, d_n, d_t, c["kf_keys_un"], new_edge_cap, n_mp, th=th)
        e1.record()
        torch.cuda.synchronize()
        if r >= warm:
            times.append(e0.elapsed_time(e1))
        if r + 1 < warm + reps:
            G.close()
    res = dict(ms=float(np.median(times)), n_targets=n_real, n_launch=n, n_fused=out["n_fused"].cpu().numpy()[:n + 1].tolist(),
               n_added=int(out["n_added"].cpu()[0]), n_replaced=int(t["d_n_replaced"].cpu()[0]), errors=G.error_count())
    G.close()
    return res


def host_search(w, c, slot, points, valid, th):
    """a host-pointer fb_fuse_search on the model's state: the gather, the grid and the round trip of the host route"""
    import oracle_lib as O
    n = int(w.kf_n[slot])
    lp = np.clip(np.asarray(points, np.int64), 0, w.n_mp - 1)
    pose = np.asarray(w.kf_Tcw[slot], np.float32)
    prob = dict(kf_kps=np.ascontiguousarray(c["kf_keys_un"][slot][:n]), kf_desc=np.ascontiguousarray(w.kf_desc[slot][:n]), pose=pose,
                Ow=np.asarray(set_pose(pose)[1], np.float32).reshape(3), mp_valid=np.asarray(valid, np.uint8), mp_xw=w.mp_xw[lp], mp_normal=w.normal[lp],
                mp_max_dist=w.max_dist[lp], mp_min_dist=w.min_dist[lp], mp_desc=w.desc[lp])
    cs, ci = P.build_grid_host([prob["kf_kps"]], P.grid_geom(synth.front_grid_geom(KP.W, KP.H)), O.grid_build, max(n, 1))
    a, out, keep = KP.fuse_args([prob], cs, ci, th=th)
    assert lib().fb_fuse_search(C.byref(a)) == 0
    return [int(b) if v else -1 for b, v in zip(out["best_idx"][0][:len(lp)], valid)]


def host_ms(c, gr, targets):
    w = LR.World(c)
    t0 = time.perf_counter()
    out = SR.search_in_neighbors(w, gr, c, CUR, S, targets, new_edge_cap=8 * S, search=host_search)
    return (time.perf_counter() - t0) * 1e3, out.n_fused


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    c, gr, order, targets = scene()
    exact = device_ms(c, order, None, 3.0, reps)
    idle = device_ms(c, order, CAP, 3.0, reps)
    empty = device_ms(c, order, None, 0.0, reps)
    host, host_fused = host_ms(c, gr, targets)
    fixed = 3 + 1 + 2 * 7 + 1 + 6 + 1 + 1 + 6 + 1 + 2      # memsets, begin, two index builds, step 3, step 5, refresh, UpdateConnections
    res = dict(key_frames=K, features=S, n_targets=exact["n_targets"], device_ms=exact["ms"], device_ms_120_launches=idle["ms"],
               device_ms_nothing_to_commit=empty["ms"], walk_share=(exact["ms"] - empty["ms"]) / exact["ms"] if exact["ms"] else None,
               host_route_ms=host, n_fused=sum(exact["n_fused"]), n_added=exact["n_added"], n_replaced=exact["n_replaced"], errors=exact["errors"],
               same_n_fused=exact["n_fused"] == host_fused, same_with_idle_launches=idle["n_fused"][:exact["n_targets"]] == exact["n_fused"][:-1],
               calls_per_fuse=4, enqueued_exact=4 * (exact["n_targets"] + 1) + fixed, enqueued_120=4 * (CAP + 1) + fixed,
               device_beats_host=exact["ms"] < host)
    with open(os.path.join(ROOT, "profiles", "search_in_neighbors_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
