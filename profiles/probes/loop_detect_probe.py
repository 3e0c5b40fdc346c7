"""fb_covis_detect_loop_dev, fb_covis_loop_map_points_dev and fb_covis_loop_connections_dev against the host route each
replaces (download the list, the literal model's walk of tests/loop_detect_ref.py, upload the result), on the same inputs.

    python profiles/probes/loop_detect_probe.py [reps]

max_keyframes = 4096.  Consistency: 64 candidates against 64 previous groups (every candidate consistent with one of them),
and, for the quadratic ranking of k_dl_emit and the K workgroups of k_dl_hit, 4096 candidates against 4096 groups.  Loop
points and LoopConnections: a current key frame with 29 neighbours (a set of 30), 20 points shared with each, and 16 points
per neighbour shared with a key frame across the loop.  The device calls are timed with events around the C call alone, on
preallocated outputs, warm-up excluded, median of `reps`; the graph is put back before every repetition of LoopConnections
(the call edits it), outside the events.  The host routes are wall time including their copies.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from fishbirdeyevisualslam_amd import cabi, lib  # noqa: E402
from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceMap, _p, _stream  # noqa: E402
import covis_ref as CR  # noqa: E402
import loop_detect_cases as LD  # noqa: E402
import loop_detect_ref as LR  # noqa: E402

K, N_CAND, SPACING, LINKS, N_SET = 4096, 64, 8, 3, 30
# launches per call, read off covis_loop.inc / covis.hip (memsets included)
LAUNCHES = dict(detect_loop=4, loop_map_points=8, loop_connections=12)


def i32(x, n=None):
    t = torch.tensor(list(x), dtype=torch.int32, device="cuda")
    if n is not None and t.numel() < n:
        t = torch.cat([t, torch.full((n - t.numel(),), -1, dtype=torch.int32, device="cuda")])
    return t


def device_ms(call, reps, warm=2, before=None):
    times = []
    for r in range(warm + reps):
        if before:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if r >= warm:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def host_ms(route, reps, before=None):
    times = []
    for _ in range(reps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        route()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def consistency(reps):
    """a chain of 512 key frames, each linked to the 3 on either side; the candidates are every 8th, so their groups are
    disjoint and each is consistent with exactly the group it pushed the call before"""
    G, g = CovisibilityGraph(K), CR.Graph(K)
    n_active = N_CAND * SPACING
    for a in range(n_active):
        for d in range(1, LINKS + 1):
            for b in (a - d, a + d):
                if 0 <= b < n_active:
                    G.add_connection(a, b, 30 - d)
                    g.add_connection(a, b, 30 - d)
    cands = list(range(0, n_active, SPACING))
    d_n, d_c = i32([len(cands)]), i32(cands, K)
    n_enough, enough, header = i32([0]), i32([], K), i32([0, 0])

    def call():
        assert lib().fb_covis_detect_loop_dev(G.h, _p(d_n), _p(d_c), 3, _p(n_enough), _p(enough), _p(header), _stream()) == 0
    call()                                            # 64 groups with counter 0
    dev = device_ms(call, reps)
    groups = G.loop_groups()
    cg = LR.ConsistencyGroups(3)

    def route():
        n = int(d_n.cpu()[0])
        lst = d_c.cpu().numpy()[:n].tolist()
        en = cg.detect(g, lst)
        out = i32(en, K)                              # the upload
        return out
    route()
    host = host_ms(route, reps)
    same = sorted(s for s, _ in groups) == sorted(sorted(s) for s, _ in cg.groups) and len(groups) == N_CAND
    # every slot a candidate: 4096 groups, then 4096 candidates against them
    d_n2, d_c2 = i32([K]), i32(range(K))
    call2 = lambda: lib().fb_covis_detect_loop_dev(G.h, _p(d_n2), _p(d_c2), 3, _p(n_enough), _p(enough), _p(header), _stream())
    G.clear()
    call2()
    full = device_ms(call2, reps)
    n_groups_full = int(header.cpu()[0])
    G.close()
    return dict(detect_loop_device_ms=dev, detect_loop_host_route_ms=host, detect_loop_groups=len(groups), detect_loop_same_groups=same,
                detect_loop_4096x4096_device_ms=full, detect_loop_4096x4096_groups=n_groups_full)


def loop_scene():
    cur, nbs, far = 100, list(range(101, 101 + N_SET - 1)), list(range(2000, 2000 + N_SET - 1))
    shared = [(cur, b, 20) for b in nbs] + [(b, f, 16) for b, f in zip(nbs, far)]
    c = LD.make_map(K, shared=shared)
    ops = [op for j, b in enumerate(nbs) for op in LD.both(cur, b, 20 + j)]
    return c, ops, cur, nbs


def points_and_connections(reps):
    c, ops, cur, nbs = loop_scene()
    m, ref = DeviceMap(c), LD.ref_map(c)
    G = CovisibilityGraph(K)
    state = {}

    def reset():
        G.clear()
        for _, a, b, w in ops:
            G.add_connection(a, b, w)
        state["g"] = LD.model_graph(K, ops, ref.kf_order)
    reset()
    # mvpLoopMapPoints of the current key frame (its ordered vector is the 29 neighbours)
    cap = m.n_mp
    n_loop, loop_mp, over = i32([0]), i32([], cap), i32([0])
    lp_call = lambda: lib().fb_covis_loop_map_points_dev(G.h, C.byref(m.c), cur, cap, _p(n_loop), _p(loop_mp), _p(over), _stream())
    lp_dev = device_ms(lp_call, reps)
    got_points = loop_mp.cpu().numpy()[:int(n_loop.cpu()[0])].tolist()

    def lp_route():
        n, sl, _ = G.ordered(cur)                     # the download of the list the host walks
        lst = sl.cpu().numpy()[:int(n.cpu()[0])].tolist()
        assert lst == state["g"].get_vector_covisible_keyframes(cur)
        return i32(LR.loop_map_points(state["g"], ref, cur), cap)
    lp_host = host_ms(lp_route, reps)
    same_points = got_points == LR.loop_map_points(state["g"], ref, cur)
    # LoopConnections over the ordered vector followed by the current key frame
    members = state["g"].get_vector_covisible_keyframes(cur) + [cur]
    d_set, d_n_set = i32(members), i32([len(members)])
    lc_cap = N_SET * 64
    out = dict(n_counter=i32([], N_SET), front=i32([], N_SET), off=i32([], N_SET + 1), slots=i32([], lc_cap), header=i32([0, 0]))
    a = cabi.LoopConnectionsArgs()
    cabi.fill(a, set_cap=N_SET, d_n_set=d_n_set, d_set=d_set, d_n_counter=out["n_counter"], d_front=out["front"], lc_cap=lc_cap,
              d_lc_off=out["off"], d_lc_slots=out["slots"], d_header=out["header"])
    lc_call = lambda: lib().fb_covis_loop_connections_dev(G.h, C.byref(m.c), C.byref(a), _stream())
    lc_dev = device_ms(lc_call, reps, before=reset)
    off = out["off"].cpu().numpy().tolist()
    flat = out["slots"].cpu().numpy().tolist()
    got_rows = [flat[off[j]:off[j + 1]] for j in range(N_SET)]
    rows = {}

    def lc_route():
        n = int(d_n_set.cpu()[0])
        lst = d_set.cpu().numpy()[:n].tolist()
        rows["r"], _, _ = LR.loop_connections(state["g"], ref, lst)
        o = np.cumsum([0] + [len(r) for r in rows["r"]])
        return i32(o), i32([x for r in rows["r"] for x in r], lc_cap)
    lc_host = host_ms(lc_route, reps, before=reset)
    G.close()
    return dict(loop_map_points_device_ms=lp_dev, loop_map_points_host_route_ms=lp_host, loop_points=len(got_points), loop_points_same=same_points,
                loop_connections_device_ms=lc_dev, loop_connections_host_route_ms=lc_host, loop_connections_total=int(out["header"].cpu()[0]),
                loop_connections_same=got_rows == rows["r"], map_points=m.n_mp, map_edges=m.n_obs)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    res = dict(max_keyframes=K, candidates=N_CAND, set_members=N_SET, reps=reps, launches_per_call=LAUNCHES)
    res.update(consistency(reps))
    res.update(points_and_connections(reps))
    print(json.dumps(res))
