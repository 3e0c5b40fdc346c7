"""Synthetic problems + C-ABI argument builders for the vocabulary-gated matchers (M5 SearchByBoW,
M7 SearchForTriangulation).  No vocabulary file ships with the reference, so the
DBoW2::FeatureVector of a frame is synthesised deterministically: NodeId = (desc[0] mod 10)*10 + desc[1] mod 10,
feature indices appended in keypoint order exactly like FeatureVector::addFeature."""
import numpy as np

from . import cabi, synth
from .cabi import fill


def feature_vector(desc):
    """-> (node_ids ascending, node_start, items) for one frame."""
    node = (desc[:, 0].astype(np.int64) % 10) * 10 + desc[:, 1].astype(np.int64) % 10
    order = np.argsort(node, kind="stable")
    ids, counts = np.unique(node, return_counts=True)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return ids.astype(np.uint32), start, order.astype(np.int32)


def _fv_struct(fvs, node_stride, item_stride):
    B = len(fvs)
    n = np.array([len(f[0]) for f in fvs], np.int32)
    ids = np.zeros((B, node_stride), np.uint32)
    st = np.zeros((B, node_stride + 1), np.int32)
    it = np.zeros((B, item_stride), np.int32)
    for b, (i, s, t) in enumerate(fvs):
        ids[b, : len(i)] = i
        st[b, : len(s)] = s
        st[b, len(s):] = s[-1]
        it[b, : len(t)] = t
    v = cabi.FeatureVector()
    fill(v, node_stride=node_stride, item_stride=item_stride, n_nodes=n, node_ids=ids, node_start=st, items=it)
    return v, (n, ids, st, it)


def make_bow_problem(seed, n_kf=1500, n_f=1500, share_prefix=True):
    """KeyFrame vs Frame: 70% of the frame features are noisy copies of keyframe features.  Copies keep the first
    two descriptor bytes so that they fall into the same synthetic vocabulary node (true matches exist)."""
    g = synth.rng(seed)
    kf = synth.random_keypoints(g, n_kf, 640, 480)
    kd = synth.random_descriptors(g, n_kf)
    src = g.integers(0, n_kf, n_f)
    f = synth.random_keypoints(g, n_f, 640, 480)
    fd = synth.random_descriptors(g, n_f)
    is_copy = g.random(n_f) < 0.7
    cp = synth.flip_bits(g, kd[src[is_copy]], p=0.04)
    if share_prefix:
        cp[:, :2] = kd[src[is_copy], :2]
    fd[is_copy] = cp
    f["angle"][is_copy] = np.mod(kf["angle"][src[is_copy]] - 25.0 + g.normal(0, 4.0, int(is_copy.sum())), 360.0).astype(np.float32)
    return dict(kf_kps=kf, kf_desc=kd, kf_has_mp=(g.random(n_kf) < 0.6).astype(np.uint8), f_kps=f, f_desc=fd)


def make_contended_bow_problem(seed, n_q, n_t):
    """make_bow_problem with the roles swapped: the n_q query (key-frame side) features are noisy copies of the n_t candidate
    features, so some 0.7 * n_q / n_t queries want each candidate and all but the first of them find it taken."""
    p = make_bow_problem(seed, n_t, n_q)
    g = synth.rng(seed + 3)
    return dict(kf_kps=p["f_kps"], kf_desc=p["f_desc"], kf_has_mp=(g.random(n_q) < 0.6).astype(np.uint8),
                f_kps=p["kf_kps"], f_desc=p["kf_desc"])


def queries_kept_in_registers():
    """k_match_bow_t keeps the per-query data of up to QPT * BOW_THREADS queries in registers and re-derives it every round
    for more: two paths through the claim rounds, and a test of them needs a query count on either side."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "match_bow.hip")).read()
    return int(re.search(r"constexpr int QPT = (\d+);", src).group(1)) * int(re.search(r"constexpr int BOW_THREADS = (\d+);", src).group(1))


def bow_args(problems, nnratio=0.7, check_ori=1):
    B = len(problems)
    ks = max(len(p["kf_kps"]) for p in problems)
    fs = max(len(p["f_kps"]) for p in problems)
    stack = lambda key, n, dt, tail=(): np.stack([np.concatenate([p[key], np.zeros((n - len(p[key]),) + tail, dt)]) for p in problems])
    keep = dict(n_kf=np.array([len(p["kf_kps"]) for p in problems], np.int32), kf_kps=stack("kf_kps", ks, cabi.KP_DTYPE),
                kf_desc=stack("kf_desc", ks, np.uint8, (32,)), kf_has_mp=stack("kf_has_mp", ks, np.uint8),
                n_f=np.array([len(p["f_kps"]) for p in problems], np.int32), f_kps=stack("f_kps", fs, cabi.KP_DTYPE),
                f_desc=stack("f_desc", fs, np.uint8, (32,)))
    kfv, k1 = _fv_struct([feature_vector(p["kf_desc"]) for p in problems], 100, ks)
    ffv, k2 = _fv_struct([feature_vector(p["f_desc"]) for p in problems], 100, fs)
    out = dict(match_f_to_kf=np.full((B, fs), -7, np.int32), nmatches=np.full(B, -7, np.int32))
    a = cabi.BowArgs()
    fill(a, batch=B, kf_stride=ks, f_stride=fs, **keep, **out)
    a.kf_fv, a.f_fv = kfv, ffv
    fill(a.matcher, nnratio=nnratio, check_orientation=check_ori)
    return a, out, (keep, k1, k2)


def make_triangulation_problem(seed, n1=1500, n2=1500, w=640, h=480, fx=400.0, fy=400.0):
    """Two keyframes of a static scene: KF2 features are projections of KF1's back-projected features under a
    known relative pose, so that the epipolar constraint holds for true matches (plus outliers)."""
    g = synth.rng(seed)
    cx, cy = w / 2.0, h / 2.0
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    T1 = synth.random_pose(g)
    D = np.eye(4)
    D[:3, :3] = synth.so3_exp(g.normal(0, 0.03, 3))
    D[:3, 3] = [0.6, 0.05, 0.1]
    T2 = D @ T1
    k1 = synth.random_keypoints(g, n1, w, h, margin=20)
    d1 = synth.random_descriptors(g, n1)
    z = g.uniform(3.0, 25.0, n1)
    Xc1 = np.stack([(k1["x"] - cx) / fx * z, (k1["y"] - cy) / fy * z, z], 1)
    Xw = (T1[:3, :3].T @ (Xc1 - T1[:3, 3]).T).T
    Xc2 = (T2[:3, :3] @ Xw.T).T + T2[:3, 3]
    u2 = Xc2[:, 0] / Xc2[:, 2] * fx + cx
    v2 = Xc2[:, 1] / Xc2[:, 2] * fy + cy
    src = g.integers(0, n1, n2)
    k2 = synth.random_keypoints(g, n2, w, h, margin=20)
    d2 = synth.random_descriptors(g, n2)
    is_copy = g.random(n2) < 0.7
    k2["x"][is_copy] = (u2[src[is_copy]] + g.normal(0, 0.7, int(is_copy.sum()))).astype(np.float32)
    k2["y"][is_copy] = (v2[src[is_copy]] + g.normal(0, 0.7, int(is_copy.sum()))).astype(np.float32)
    k2["octave"][is_copy] = k1["octave"][src[is_copy]]
    cp = synth.flip_bits(g, d1[src[is_copy]], p=0.04)
    cp[:, :2] = d1[src[is_copy], :2]
    d2[is_copy] = cp
    # F12 = K^-T [t12]x R12 K^-1 with x1' F12 x2 = 0  (LocalMapping::ComputeF12, LocalMapping.cc:560-577)
    R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
    R12 = R1 @ R2.T
    t12 = -R1 @ R2.T @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = np.linalg.inv(K).T @ tx @ R12 @ np.linalg.inv(K)
    Cw1 = -R1.T @ t1
    return dict(kps1=k1, desc1=d1, has_mp1=(g.random(n1) < 0.3).astype(np.uint8), kps2=k2, desc2=d2,
                has_mp2=(g.random(n2) < 0.3).astype(np.uint8), F12=F12.astype(np.float32).reshape(9), Cw1=Cw1.astype(np.float32),
                R2w=R2.astype(np.float32).reshape(9), t2w=t2.astype(np.float32), fx=fx, fy=fy, cx=cx, cy=cy)


def triangulation_args(problems, nnratio=0.6, check_ori=0):
    B = len(problems)
    p0 = problems[0]
    s1 = max(len(p["kps1"]) for p in problems)
    s2 = max(len(p["kps2"]) for p in problems)
    stack = lambda key, n, dt, tail=(): np.stack([np.concatenate([p[key], np.zeros((n - len(p[key]),) + tail, dt)]) for p in problems])
    keep = dict(n1=np.array([len(p["kps1"]) for p in problems], np.int32), kps1=stack("kps1", s1, cabi.KP_DTYPE),
                desc1=stack("desc1", s1, np.uint8, (32,)), has_mp1=stack("has_mp1", s1, np.uint8),
                n2=np.array([len(p["kps2"]) for p in problems], np.int32), kps2=stack("kps2", s2, cabi.KP_DTYPE),
                desc2=stack("desc2", s2, np.uint8, (32,)), has_mp2=stack("has_mp2", s2, np.uint8),
                F12=np.stack([p["F12"] for p in problems]), Cw1=np.stack([p["Cw1"] for p in problems]),
                R2w=np.stack([p["R2w"] for p in problems]), t2w=np.stack([p["t2w"] for p in problems]))
    fv1, k1 = _fv_struct([feature_vector(p["desc1"]) for p in problems], 100, s1)
    fv2, k2 = _fv_struct([feature_vector(p["desc2"]) for p in problems], 100, s2)
    out = dict(matches12=np.full((B, s1), -7, np.int32), nmatches=np.full(B, -7, np.int32))
    a = cabi.TriangulationArgs()
    sf, _, sig2, _ = synth.scale_tables()
    fill(a, batch=B, kf1_stride=s1, kf2_stride=s2, fx=p0["fx"], fy=p0["fy"], cx=p0["cx"], cy=p0["cy"],
         scale_factors=[float(x) for x in sf], level_sigma2=[float(x) for x in sig2], **keep, **out)
    a.fv1, a.fv2 = fv1, fv2
    fill(a.matcher, nnratio=nnratio, check_orientation=check_ori)
    return a, out, (keep, k1, k2)


def make_vocabulary(seed, k=10, L=3, stop_frac=0.05):
    """Complete k-ary tree of depth L in BFS node order (node 0 = root), random node descriptors (every node = its parent
    with a quarter of the bits flipped, so that the descent is meaningful), idf-like leaf weights.  k = 10, L = 6 is the
    shape of the stock ORB vocabulary (1.1 M nodes); built level by level so that it takes seconds, not minutes."""
    g = synth.rng(seed)
    n_nodes = sum(k ** l for l in range(L + 1))
    first_leaf = sum(k ** l for l in range(L))
    child_start = np.minimum(np.arange(n_nodes + 1, dtype=np.int64), first_leaf) * k
    child_start = child_start.astype(np.int32)
    children = np.arange(1, n_nodes, dtype=np.int32)
    desc = np.zeros((n_nodes, 32), np.uint8)
    desc[0] = synth.random_descriptors(g, 1)[0]
    lo = 1
    for l in range(1, L + 1):
        hi = lo + k ** l
        for c0 in range(lo, hi, 65536):   # bounded scratch: 65536 x 256 random numbers at a time
            c1 = min(hi, c0 + 65536)
            parents = (np.arange(c0, c1) - 1) // k
            desc[c0:c1] = synth.flip_bits(g, desc[parents], p=0.25)
        lo = hi
    weights = np.zeros(n_nodes, np.float64)
    weights[first_leaf:] = g.uniform(0.5, 9.0, n_nodes - first_leaf)
    weights[first_leaf:][g.random(n_nodes - first_leaf) < stop_frac] = 0.0   # stopped words
    word_ids = np.full(n_nodes, -1, np.int32)
    word_ids[first_leaf:] = np.arange(n_nodes - first_leaf)
    keep = dict(child_start=child_start, children=children, descriptors=desc, weights=weights, word_ids=word_ids)
    v = cabi.Vocabulary()
    fill(v, n_nodes=n_nodes, L=L, **keep)
    return v, keep, first_leaf


# ---- LocalMapping::CreateNewMapPoints -------------------------------------------------------------------------------
def _project(T, X, fx, fy, cx, cy):
    Xc = X @ T[:3, :3].T + T[:3, 3]
    return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1), Xc[:, 2]


def make_new_points_problem(seed, n_nb=20, n1=2000, n2=2000, w=640, h=480, fx=400.0, fy=400.0, pixel_noise=0.5, plants=True):
    """One static scene, a current key frame (KF1) and n_nb covisible neighbours that see overlapping subsets of it, with pixel
    noise, outliers, existing map points (has_mp*) and synthetic feature vectors (feature_vector()).  KF1 feature i observes
    scene point i (truth["xw"][i]; NaN for outliers).  With plants=True it also holds (indices in truth["plants"]):
      short   a neighbour whose baseline / median depth is below 0.01 (n_nb >= 3)
      far     points thousands of metres away (cos parallax > 0.9998)
      behind  points in front of KF1 but behind neighbour `behind_nb` (which moved forward past them)
      chi2    KF1 octave 0 / neighbour 0 octave 7, the neighbour-0 copy 6 px off the epipolar line (inside M7's 7 px band)
      scale   KF1 octave 0 / neighbour 0 octave 7 on the exact projection (ratioOctave ~ 0.28)
      chi2 and scale points are also seen, correctly, by neighbour `second_nb`
      dup     pairs of KF1 features on one scene point: both match the same neighbour slot (many-to-one)"""
    g = synth.rng(seed)
    cx, cy = w / 2.0, h / 2.0
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    sf, _, _, _ = synth.scale_tables()
    T1 = synth.random_pose(g)
    R1, t1 = T1[:3, :3], T1[:3, 3]
    Ow1 = -R1.T @ t1
    kps1 = synth.random_keypoints(g, n1, w, h, margin=20)
    # scene point of every KF1 feature (noiseless pixel, depth)
    z = g.uniform(3.0, 25.0, n1)
    n_plant = min(n1 // 10, 200) if plants else 0
    npl = n_plant // 5
    sl = dict(far=np.arange(0, npl), behind=np.arange(npl, 2 * npl), chi2=np.arange(2 * npl, 3 * npl), scale=np.arange(3 * npl, 4 * npl),
              dup=np.arange(4 * npl, 5 * npl))
    base = n1 - n_plant
    for k in sl:
        sl[k] = sl[k] + base
    z[sl["far"]] = g.uniform(3000.0, 6000.0, npl)
    # behind: neighbour `behind_nb` sits 3 m ahead of KF1; the points lie 1-2 m in front of KF1
    z[sl["behind"]] = g.uniform(1.0, 2.0, npl)
    kps1["octave"][sl["chi2"]] = 0
    kps1["octave"][sl["scale"]] = 0
    uv_true = np.stack([kps1["x"].astype(np.float64), kps1["y"].astype(np.float64)], 1)
    Xc1 = np.stack([(uv_true[:, 0] - cx) / fx * z, (uv_true[:, 1] - cy) / fy * z, z], 1)
    Xw = (R1.T @ (Xc1 - t1).T).T
    # dup: the second feature of a pair re-observes the scene point of the first (features base+4npl.. pair with ..+npl/2)
    half = npl // 2
    d0, d1 = sl["dup"][:half], sl["dup"][half:2 * half]
    Xw[d1] = Xw[d0]
    uv1 = _project(T1, Xw, fx, fy, cx, cy)[0]
    n1_noise = g.normal(0, pixel_noise, (n1, 2)) if pixel_noise > 0 else np.zeros((n1, 2))
    kps1["x"] = (uv1[:, 0] + n1_noise[:, 0]).astype(np.float32)
    kps1["y"] = (uv1[:, 1] + n1_noise[:, 1]).astype(np.float32)
    kps1["octave"][d1] = kps1["octave"][d0]
    scene_desc = synth.random_descriptors(g, n1)
    scene_desc[d1] = scene_desc[d0]
    desc1 = synth.flip_bits(g, scene_desc, p=0.03)
    desc1[:, :2] = scene_desc[:, :2]
    outlier1 = g.random(n1) < 0.12
    outlier1[base:] = False
    desc1[outlier1] = synth.random_descriptors(g, int(outlier1.sum()))
    has_mp1 = (g.random(n1) < 0.3).astype(np.uint8)
    has_mp1[base:] = 0
    truth_xw = Xw.copy()
    truth_xw[outlier1] = np.nan
    short_nb = 2 if (plants and n_nb >= 3) else -1
    behind_nb = 1 if (plants and n_nb >= 2) else -1
    second_nb = 3 if n_nb > 3 else n_nb - 1
    nbs = []
    for b in range(n_nb):
        D = np.eye(4)
        D[:3, :3] = synth.so3_exp(g.normal(0, 0.04, 3))
        dirn = g.normal(0, 1, 3)
        dirn[2] *= 0.3
        D[:3, 3] = dirn / np.linalg.norm(dirn) * g.uniform(0.4, 1.6)
        if b == short_nb:
            D[:3, :3] = np.eye(3)
            D[:3, 3] = [0.02, 0.0, 0.0]
        if b == behind_nb:
            D[:3, :3] = np.eye(3)
            D[:3, 3] = [-0.5, 0.1, -3.0]  # camera centre 3 m ahead of KF1 (tcw2 = tcw1 - c)
        T2 = D @ T1
        uv2, z2 = _project(T2, Xw, fx, fy, cx, cy)
        inside = (uv2[:, 0] > 10) & (uv2[:, 0] < w - 10) & (uv2[:, 1] > 10) & (uv2[:, 1] < h - 10)
        vis = inside & (z2 > 0) & (g.random(n1) < 0.5)
        if plants:
            vis[base:] = False
            vis[sl["far"]] = inside[sl["far"]] & (z2[sl["far"]] > 0)
            vis[d0] = inside[d0] & (z2[d0] > 0) & (b % 2 == 0)
            if b == behind_nb:
                vis[sl["behind"]] = inside[sl["behind"]]
            if b in (0, second_nb):
                vis[sl["chi2"]] = inside[sl["chi2"]] & (z2[sl["chi2"]] > 0)
                vis[sl["scale"]] = inside[sl["scale"]] & (z2[sl["scale"]] > 0)
        src = np.nonzero(vis)[0]
        n_copy = min(len(src), int(0.75 * n2))
        keep_plant = src[src >= base]
        rest = src[src < base]
        src = np.concatenate([keep_plant, g.permutation(rest)[: max(n_copy - len(keep_plant), 0)]])
        n_copy = len(src)
        k2 = synth.random_keypoints(g, n2, w, h, margin=20)
        d2 = synth.random_descriptors(g, n2)
        slot = g.permutation(n2)[:n_copy]
        noise2 = g.normal(0, pixel_noise, (n_copy, 2)) if pixel_noise > 0 else np.zeros((n_copy, 2))
        px = uv2[src] + noise2
        oc = kps1["octave"][src].copy()
        if plants and b == 0:
            # chi2 / scale plants: octave 7 here; chi2 ones 6 px off the epipolar line of the KF1 feature
            R2, t2 = T2[:3, :3], T2[:3, 3]
            R12 = R1 @ R2.T
            t12 = -R1 @ R2.T @ t2 + t1
            tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
            F12 = np.linalg.inv(K).T @ tx @ R12 @ np.linalg.inv(K)
            for j, s_ in enumerate(src):
                if s_ in set(sl["chi2"]) or s_ in set(sl["scale"]):
                    oc[j] = 7
                    px[j] = uv2[s_]
                if s_ in set(sl["chi2"]):
                    l = np.array([kps1["x"][s_], kps1["y"][s_], 1.0]) @ F12
                    nrm = l[:2] / np.linalg.norm(l[:2])
                    px[j] = px[j] + 6.0 * nrm
        k2["x"][slot] = px[:, 0].astype(np.float32)
        k2["y"][slot] = px[:, 1].astype(np.float32)
        k2["octave"][slot] = oc
        cp = synth.flip_bits(g, scene_desc[src], p=0.03)
        cp[:, :2] = scene_desc[src, :2]
        d2[slot] = cp
        has2 = (g.random(n2) < 0.3).astype(np.uint8)
        is_plant_slot = np.zeros(n2, bool)
        is_plant_slot[slot[src >= base]] = True
        has2[is_plant_slot] = 0
        # the neighbour's map points (ComputeSceneMedianDepth input): the scene point of a copy slot, else a point in front
        owner = np.full(n2, -1)
        owner[slot] = src
        mps = []
        for s_ in np.nonzero(has2)[0]:
            if owner[s_] >= 0:
                mps.append(Xw[owner[s_]])
            else:
                zz = g.uniform(3.0, 25.0)
                xc = np.array([(k2["x"][s_] - cx) / fx * zz, (k2["y"][s_] - cy) / fy * zz, zz])
                mps.append(T2[:3, :3].T @ (xc - T2[:3, 3]))
        if not mps:
            mps.append(Xw[0])
        nbs.append(dict(kps=k2, desc=d2, has_mp=has2, T=T2, mp_xw=np.asarray(mps, np.float32).reshape(-1, 3),
                        before=np.uint8(g.random() < 0.5), owner=owner))
    sf_, _, sig2, _ = synth.scale_tables()
    return dict(kps1=kps1, desc1=desc1, has_mp1=has_mp1, Tcw1=synth.to12(T1), nbs=nbs, fx=fx, fy=fy, cx=cx, cy=cy,
                scale_factors=sf_, level_sigma2=sig2, n_levels=8, scale_factor=1.2,
                truth=dict(xw=truth_xw, T1=T1, plants=dict(sl, dup_pairs=np.stack([d0, d1], 1)), short_nb=short_nb, behind_nb=behind_nb,
                           second_nb=second_nb))


def new_points_args(prob, n_nb=None, kf1_stride=None, kf2_stride=None):
    """-> (cabi.NewPointsArgs with host pointers, out dict, keepalive).  n_nb: use the first n_nb neighbours only."""
    nbs = prob["nbs"][: (len(prob["nbs"]) if n_nb is None else n_nb)]
    B = len(nbs)
    n1 = len(prob["kps1"])
    s1 = kf1_stride or max(n1, 1)
    s2 = kf2_stride or max([len(x["kps"]) for x in nbs] + [1])
    pad = lambda a, n, tail=(), dt=None: np.concatenate([a, np.zeros((n - len(a),) + tail, dt or a.dtype)])
    kps2 = np.stack([pad(x["kps"], s2) for x in nbs]) if B else np.zeros((1, s2), cabi.KP_DTYPE)
    desc2 = np.stack([pad(x["desc"], s2, (32,)) for x in nbs]) if B else np.zeros((1, s2, 32), np.uint8)
    has2 = np.stack([pad(x["has_mp"], s2) for x in nbs]) if B else np.zeros((1, s2), np.uint8)
    starts = np.concatenate([[0], np.cumsum([len(x["mp_xw"]) for x in nbs])]).astype(np.int32)
    mp_xw = np.concatenate([x["mp_xw"] for x in nbs]) if B else np.zeros((1, 3), np.float32)
    keep = dict(n1=np.array([n1], np.int32), kps1=pad(prob["kps1"], s1), desc1=pad(prob["desc1"], s1, (32,)),
                Tcw1=np.ascontiguousarray(prob["Tcw1"], np.float32),
                n2=np.array([len(x["kps"]) for x in nbs] or [0], np.int32), kps2=kps2, desc2=desc2,
                Tcw2=np.stack([synth.to12(x["T"]) for x in nbs]) if B else np.zeros((1, 12), np.float32),
                nb_mp_start=starts, nb_mp_xw=np.ascontiguousarray(mp_xw, np.float32),
                nb_before_kf1=np.array([x["before"] for x in nbs] or [0], np.uint8))
    out = dict(has_mp1=pad(prob["has_mp1"], s1).copy(), has_mp2=has2.copy(), n_new=np.full(1, -7, np.int32),
               xw=np.zeros((s1, 3), np.float32), normal=np.zeros((s1, 3), np.float32), max_dist=np.zeros(s1, np.float32),
               min_dist=np.zeros(s1, np.float32), desc=np.zeros((s1, 32), np.uint8), idx1=np.full(s1, -7, np.int32),
               nb=np.full(s1, -7, np.int32), idx2=np.full(s1, -7, np.int32), kf1_new=np.full(s1, -7, np.int32),
               kf2_new=np.full((max(B, 1), s2), -7, np.int32), nb_matches=np.full(max(B, 1), -7, np.int32),
               nb_new=np.full(max(B, 1), -7, np.int32), nb_skipped=np.full(max(B, 1), -7, np.int32))
    fv1, k1 = _fv_struct([feature_vector(prob["desc1"])], 100, s1)
    fv2, k2 = _fv_struct([feature_vector(x["desc"]) for x in nbs] or [feature_vector(np.zeros((1, 32), np.uint8))], 100, s2)
    a = cabi.NewPointsArgs()
    fill(a, n_nb=B, kf1_stride=s1, kf2_stride=s2, fx=prob["fx"], fy=prob["fy"], cx=prob["cx"], cy=prob["cy"],
         scale_factors=[float(x) for x in prob["scale_factors"]] + [1.0] * (cabi.FB_MAX_LEVELS - len(prob["scale_factors"])),
         level_sigma2=[float(x) for x in prob["level_sigma2"]] + [1.0] * (cabi.FB_MAX_LEVELS - len(prob["level_sigma2"])),
         n_levels=prob["n_levels"], scale_factor=prob["scale_factor"], **keep, **out)
    a.fv1, a.fv2 = fv1, fv2
    fill(a.matcher, nnratio=0.6, check_orientation=0)
    return a, out, (keep, k1, k2)
