"""Generators of the bird-map tests (tests/test_covis_bird.py asserts their branch coverage on the CPU,
tests/test_covis_bird_gpu.py runs them on the device).  Test infrastructure: the package never imports it."""
import numpy as np

import bird_map_ref as R


def make_bird_problem(seed, K, used, bird_stride=64, n_points=150, obs=(2, 7), n_global=0, bad_frac=0.1, tomb_frac=0.05):
    """A bird map over the slots `used` (at least 8 of them) of a K-slot handle.  The last five used slots are special:
      lone      no bird point at all: empty counter, parent -1, a middle frame id        -> the search finds a key frame
      orphan    only erased edges and bad points, the smallest frame id, parent -1       -> the search finds nothing
      thin      shares exactly one point with two others: non-empty counter, empty list  -> the search, from the list branch
      id0       mnId == 0: parent -1, first set, a non-empty list                        -> the return at :516
      twin      holds one shared point at two features                                   -> a weight of 2 from one point
    The others hold random points (obs[0] .. obs[1]-1 observers each), n_global points that every one of them holds, and
    start from mixed parent / first states."""
    rng = np.random.default_rng(seed)
    used = [int(s) for s in used]
    assert len(used) >= 8
    regular, (lone, orphan, thin, id0, twin) = used[:-5], used[-5:]
    BS = bird_stride
    kf_nb = np.zeros(K, np.int32)
    kf_mpb = np.full((K, BS), -1, np.int32)
    mpb_bad, edges = [], []

    def new_point(bad=False):
        mpb_bad.append(1 if bad else 0)
        return len(mpb_bad) - 1

    def hold(kf, p, edge=True):
        i = int(kf_nb[kf])
        assert i < BS
        kf_mpb[kf, i] = p
        kf_nb[kf] = i + 1
        if edge:
            edges.append([p, kf, i])

    for _ in range(n_global):
        p = new_point()
        for kf in regular + [id0]:
            hold(kf, p)
    for _ in range(n_points):
        free = [kf for kf in regular + [id0] if kf_nb[kf] < BS - (10 if kf == regular[0] else 6)]   # room for the special points
        if len(free) < obs[0]:
            break
        p = new_point(rng.random() < bad_frac)
        for kf in rng.choice(free, min(int(rng.integers(obs[0], obs[1])), len(free)), replace=False):
            hold(int(kf), p)
    # a weight tie for regular[0]: two more key frames that share exactly three fresh points with it (and nothing else new)
    for other in regular[1:3]:
        for _ in range(3):
            p = new_point()
            hold(regular[0], p); hold(other, p)
    # thin: one point with each of two regular key frames
    for other in regular[:2]:
        p = new_point()
        hold(thin, p); hold(other, p)
    # twin: one point of regular[3], held at two features of twin (one observation edge, as a std::map has one entry)
    p = new_point()
    hold(regular[3], p); hold(twin, p); hold(twin, p, edge=False)
    # orphan: a bad point shared with regular[0], and a good one whose every other edge is erased
    p = new_point(bad=True)
    hold(orphan, p); hold(regular[0], p)
    p = new_point()
    hold(orphan, p)
    hold(regular[1], p)
    edges[-1][1] = -1                                  # tombstone: regular[1] still holds the point, the observation is gone
    e = np.asarray(edges, np.int32).reshape(-1, 3)
    live = np.flatnonzero(e[:, 1] >= 0)
    protect = set(np.flatnonzero(np.isin(e[:, 0], np.arange(len(mpb_bad) - 11, len(mpb_bad)))).tolist())
    for i in rng.choice(live, int(len(live) * tomb_frac), replace=False):
        if int(i) not in protect:
            e[i, 1] = -1
    e = e[rng.permutation(len(e))]
    kf_order = (rng.permutation(K).astype(np.uint64) * np.uint64(64) + np.uint64(0x7F0000000000))
    frame_id = np.zeros(K, np.int32)
    ids = rng.permutation(len(used) - 1) * 3 + 10
    for s, f in zip([u for u in used if u != orphan], ids):
        frame_id[s] = f
    frame_id[orphan] = 4                               # the smallest: nothing lies strictly between 0 and it
    frame_id[regular[-1]] = frame_id[regular[-2]]      # equal ids: the smaller kf_order wins
    in_map = np.zeros(K, np.uint8)
    in_map[used] = 1
    in_map[regular[4 % len(regular)]] = 0              # a key frame that is not in the map never wins
    parent = np.full(K, -1, np.int32)
    linked = np.zeros(K, np.uint8)
    first = np.ones(K, np.uint8)
    for j, s in enumerate(regular):
        mode = j % 4
        if mode == 1:
            parent[s], linked[s], first[s] = regular[(j + 1) % len(regular)], 1, 0     # settled: nothing changes
        elif mode == 2:
            parent[s], linked[s], first[s] = regular[(j + 2) % len(regular)], 1, 1     # a parent, first still set: replaced
        elif mode == 3:
            first[s] = 0                                                                # no parent, first cleared: set
    return dict(K=K, used=used, bird_stride=BS, kf_nb=kf_nb, kf_mpb=kf_mpb, mpb_bad=np.asarray(mpb_bad, np.uint8),
                bobs_mpb=e[:, 0].copy(), bobs_kf=e[:, 1].copy(), bobs_idx=e[:, 2].copy(), kf_order=kf_order, frame_id=frame_id,
                in_map=in_map, parent=parent, linked=linked, first=first, id0=id0,
                special=dict(lone=lone, orphan=orphan, thin=thin, id0=id0, twin=twin))


def tables_of(p):
    return R.BirdTables(p["kf_nb"], p["kf_mpb"], p["mpb_bad"], p["bobs_mpb"], p["bobs_kf"], p["bobs_idx"])


def graph_of(p):
    return R.BirdGraph(p["K"], p["kf_order"], p["parent"], p["linked"], p["first"])


def front_counter(p, slots, seed=3):
    """a stand-in for the front call's d_n_counter: zero for about a third of the queries, and for `lone`"""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 3, len(slots)).astype(np.int32)
    for q, s in enumerate(slots):
        if s == p["special"]["lone"]:
            n[q] = 0
    return n


def inject_out_of_range(p, seed=9):
    """-> (dirty copy, clean copy, number of injected entries): kf_mpb entries >= n_mpb in unused cells, and appended edges whose
    point, key frame or feature index is out of range.  The clean copy is what the model sees."""
    rng = np.random.default_rng(seed)
    dirty = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    n_mpb, K, BS = len(p["mpb_bad"]), p["K"], p["bird_stride"]
    n = 0
    for kf in p["used"][:4]:
        i = int(dirty["kf_nb"][kf])
        if i < BS:
            dirty["kf_mpb"][kf, i] = n_mpb + int(rng.integers(0, 5))
            dirty["kf_nb"][kf] = i + 1
            n += 1
    bad_edges = [[n_mpb, p["used"][0], 0], [-1, p["used"][1], 1], [0, K, 0], [1, K + 7, 2], [2, p["used"][2], BS], [3, p["used"][0], -1]]
    n += len(bad_edges)
    be = np.asarray(bad_edges, np.int32)
    for k, c in (("bobs_mpb", 0), ("bobs_kf", 1), ("bobs_idx", 2)):
        dirty[k] = np.concatenate([p[k], be[:, c]])
    clean = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in dirty.items()}
    for kf in p["used"][:4]:
        row = clean["kf_mpb"][kf]
        row[row >= n_mpb] = -1
    clean["bobs_kf"][len(p["bobs_kf"]):] = -1
    clean["bobs_mpb"][len(p["bobs_kf"]):] = 0
    return dirty, clean, n


def make_local_problem(seed, K=40, steps=30, bird_stride=48, mpb_order=True):
    """`steps` key frames along a path that leaves the 5 m ball of its start and comes back into it.  Consecutive key frames
    share a few bird points (a member stays only while it is the first holder of 10); every fourth brings fewer than 10 new ones; two sit far outside on a detour.  kf_Tcw has a
    rotation, so the centre is not just -t.  -> dict with the tables, kf_Tcw, kf_ow (= the derived centres) and the slot of
    every step."""
    rng = np.random.default_rng(seed)
    BS = bird_stride
    slots = [int(s) for s in rng.permutation(K)[:steps]]
    t = np.linspace(0.0, 2.0 * np.pi, steps, endpoint=False)
    centre = np.stack([4.5 * (1.0 - np.cos(t)), 3.0 * np.sin(t), 0.05 * np.sin(3 * t)], 1)
    centre[steps // 2] += [30.0, 0.0, 0.0]
    centre[steps // 2 + 1] += [0.0, -25.0, 0.0]
    kf_Tcw = np.zeros((K, 12), np.float32)
    kf_Tcw[:, [0, 5, 10]] = 1.0
    for j, s in enumerate(slots):
        a = 0.3 * j
        Rcw = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        T = np.zeros((3, 4))
        T[:, :3], T[:, 3] = Rcw, -Rcw @ centre[j]
        kf_Tcw[s] = T.astype(np.float32).reshape(12)
    kf_ow = np.stack([R.camera_centre(kf_Tcw[s]) for s in range(K)]).astype(np.float32)
    kf_nb = np.zeros(K, np.int32)
    kf_mpb = np.full((K, BS), -1, np.int32)
    n_mpb, prev = 0, []
    for j, s in enumerate(slots):
        n_new = int(rng.integers(3, 9)) if j % 4 == 3 else int(rng.integers(11, 20))
        pts = list(rng.choice(prev, min(len(prev), int(rng.integers(2, 7))), replace=False)) if prev else []
        pts += list(range(n_mpb, n_mpb + n_new))
        n_mpb += n_new
        if j % 5 == 2:
            pts.append(pts[0])                         # a point held at two features counts once
        row = np.full(BS, -1, np.int32)
        cells = np.sort(rng.choice(BS, len(pts), replace=False))
        row[cells] = rng.permutation(np.asarray(pts, np.int32))
        kf_mpb[s] = row
        kf_nb[s] = BS if j % 2 else int(cells[-1]) + 1
        prev = [int(x) for x in set(pts)]
    order = (rng.permutation(n_mpb).astype(np.uint64) * np.uint64(16) + np.uint64(0x560000000000)) if mpb_order else None
    return dict(K=K, bird_stride=BS, slots=slots, kf_Tcw=kf_Tcw, kf_ow=kf_ow, kf_nb=kf_nb, kf_mpb=kf_mpb,
                mpb_bad=(rng.random(n_mpb) < 0.2).astype(np.uint8), bobs_mpb=np.zeros(0, np.int32), bobs_kf=np.zeros(0, np.int32),
                bobs_idx=np.zeros(0, np.int32), kf_order=np.arange(K, dtype=np.uint64), mpb_order=order, n_mpb=n_mpb)


def run_local_model(p, mpb_order=None, kf_ow=None):
    """the model over the whole sequence -> (model, [(local_kf, local_mpb) after every AddKeyFrame])"""
    T = tables_of(p)
    m = R.LocalBirdMap(mpb_order)
    ow = p["kf_ow"] if kf_ow is None else kf_ow
    out = []
    for s in p["slots"]:
        m.add_keyframe(T, ow, s)
        out.append((list(m.local_kf), list(m.local_mpb)))
    return m, out
