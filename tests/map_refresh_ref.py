"""A literal Python restatement of the per-point side of LocalMapping, written from the reference (not from the kernels) on
dict-of-observations points.  Test infrastructure: the package never imports it.

    MapPoint::AddObservation (monocular)                 src/MapPoint.cc:98-109
    MapPoint::SetBadFlag                                 src/MapPoint.cc:151-168
    MapPoint::GetFoundRatio                              src/MapPoint.cc:236-240
    MapPoint::ComputeDistinctiveDescriptors              src/MapPoint.cc:242-307
    MapPoint::UpdateNormalAndDepth                       src/MapPoint.cc:330-371
    LocalMapping::ProcessNewKeyFrame, the point loop     src/LocalMapping.cc:158-179
    LocalMapping::MapPointCulling                        src/LocalMapping.cc:207-228

Every loop runs serially in the reference's order; std::map<KeyFrame*, size_t> iterates ascending kf_order.  The seams are
those of map_correct_ref (cv::norm in double, Mat / scalar as a product with the float reciprocal, SetPose).
"""
import numpy as np

from map_correct_ref import cv_norm, set_pose

f32 = np.float32
NORMAL_DEPTH, DESCRIPTOR = 1, 2


class World:
    """The map as the reference holds it: mObservations per point next to the arrays of the case c (see
    covis_problem.make_refresh_problem).  `edges` keeps the edge list itself so that the edits can be compared."""

    def __init__(self, c):
        self.K, self.S = np.asarray(c["kf_mp"]).shape
        self.n_mp = len(c["mp_bad"])
        self.kf_order = [int(x) for x in c["kf_order"]]
        self.kf_n = np.array(c["kf_n"], np.int32)
        self.kf_mp = np.array(c["kf_mp"], np.int32)
        self.kf_octave = np.array(c["kf_octave"], np.uint8)
        self.kf_Tcw = np.array(c["kf_Tcw"], f32).reshape(-1, 12)
        self.kf_bad = np.array(c["kf_bad"], np.uint8)
        self.kf_desc = np.array(c["kf_desc"], np.uint8).reshape(self.K, self.S, 32)
        self.scale = np.array(c["scale_factors"], f32)
        self.mp_bad = np.array(c["mp_bad"], np.uint8)
        self.mp_xw = np.array(c["mp_xw"], f32).reshape(-1, 3)
        self.mp_ref_kf = np.array(c["mp_ref_kf"], np.int32)
        self.normal = np.array(c["mp_normal"], f32).reshape(-1, 3)
        self.min_dist, self.max_dist = np.array(c["mp_min_dist"], f32), np.array(c["mp_max_dist"], f32)
        self.desc = np.array(c["mp_desc"], np.uint8).reshape(-1, 32)
        self.obs_mp, self.obs_kf, self.obs_idx = (np.array(c[k], np.int32) for k in ("obs_mp", "obs_kf", "obs_idx"))
        self.errors = 0
        self.obs = [dict() for _ in range(self.n_mp)]                                                  # mp -> {kf: (idx, edge)}
        for e, (mp, kf, idx) in enumerate(zip(self.obs_mp.tolist(), self.obs_kf.tolist(), self.obs_idx.tolist())):
            if kf < 0:
                continue
            if kf >= self.K or mp < 0 or mp >= self.n_mp or idx < 0 or idx >= self.S:
                self.errors += 1
                continue
            self.obs[mp][kf] = (idx, e)

    def key(self, kf):
        return (self.kf_order[kf], kf)

    def map_order(self, d):
        return sorted(d, key=self.key)                                                                 # a std::map<KeyFrame*, ..>

    def centre(self, kf):
        return set_pose(self.kf_Tcw[kf])[1]


def update_normal_and_depth(w, mp):                                                                    # MapPoint.cc:330-371
    if w.mp_bad[mp]:                                                                                   # :338
        return
    observations = {kf: v[0] for kf, v in w.obs[mp].items()}
    if not observations:                                                                               # :345
        return
    pRefKF = int(w.mp_ref_kf[mp])
    if pRefKF < 0 or pRefKF >= w.K:
        w.errors += 1
        return
    Pos = w.mp_xw[mp].copy()
    normal, n = np.zeros(3, f32), 0
    for pKF in w.map_order(observations):                                                              # :350
        normali = (Pos - w.centre(pKF)).astype(f32)
        normal = (normal + normali * f32(1.0 / cv_norm(normali))).astype(f32)
        n += 1
    PC = (Pos - w.centre(pRefKF)).astype(f32)
    dist = f32(cv_norm(PC))
    level = int(w.kf_octave[pRefKF, observations.get(pRefKF, 0)])                                      # :361: operator[] inserts 0
    if level >= len(w.scale):
        w.errors += 1
        return
    w.max_dist[mp] = f32(dist * w.scale[level])                                                        # :367-369
    w.min_dist[mp] = f32(w.max_dist[mp] / w.scale[len(w.scale) - 1])
    w.normal[mp] = (normal * f32(1.0 / n)).astype(f32)


def descriptor_distance(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def distinctive_choice(vDescriptors):
    """:272-301 -> BestIdx"""
    N = len(vDescriptors)
    Distances = [[0] * N for _ in range(N)]
    for i in range(N):
        for j in range(i + 1, N):
            Distances[i][j] = Distances[j][i] = descriptor_distance(vDescriptors[i], vDescriptors[j])
    BestMedian, BestIdx = 2 ** 31 - 1, 0
    for i in range(N):
        vDists = sorted(Distances[i])
        median = vDists[int(0.5 * (N - 1))]
        if median < BestMedian:
            BestMedian, BestIdx = median, i
    return BestIdx


def compute_distinctive_descriptors(w, mp):                                                            # MapPoint.cc:242-307
    if w.mp_bad[mp]:                                                                                   # :251
        return
    observations = w.obs[mp]
    if not observations:
        return
    vDescriptors = [w.kf_desc[pKF, observations[pKF][0]] for pKF in w.map_order(observations) if not w.kf_bad[pKF]]   # :261-267
    if not vDescriptors:
        return
    w.desc[mp] = vDescriptors[distinctive_choice(vDescriptors)]


def refresh_points(w, points=None, what=NORMAL_DEPTH | DESCRIPTOR):
    for mp in (range(w.n_mp) if points is None else points):
        mp = int(mp)
        if mp < 0 or mp >= w.n_mp:
            w.errors += 1
            continue
        if what & NORMAL_DEPTH:
            update_normal_and_depth(w, mp)
        if what & DESCRIPTOR:
            compute_distinctive_descriptors(w, mp)


def process_new_keyframe(w, slot, n_features, recent):
    """LocalMapping.cc:158-179 for the key frame in `slot`; the edge list grows by the block [n_obs, n_obs + n_features): the
    new edges in the order they were added, then tombstones.  -> the number of new edges; `recent` is appended to."""
    base = len(w.obs_kf)
    block = np.full((3, n_features), -1, np.int32)
    n_added = 0
    if int(w.kf_n[slot]) != n_features:                                                                # the contract of the call
        w.errors += 1
    else:
        for i in range(n_features):                                                                    # :160
            pMP = int(w.kf_mp[slot, i])
            if pMP < 0:                                                                                # :163
                continue
            if pMP >= w.n_mp:
                w.errors += 1
                continue
            if w.mp_bad[pMP]:                                                                          # :165
                continue
            if slot not in w.obs[pMP]:                                                                 # :167
                w.obs[pMP][slot] = (i, base + n_added)                                                 # AddObservation
                block[:, n_added] = (pMP, slot, i)
                n_added += 1
                update_normal_and_depth(w, pMP)
                compute_distinctive_descriptors(w, pMP)
            else:
                recent.append(pMP)                                                                     # :175
    w.obs_mp, w.obs_kf, w.obs_idx = (np.concatenate([a, b]) for a, b in zip((w.obs_mp, w.obs_kf, w.obs_idx), block))
    return n_added


def set_bad_flag(w, mp, erased):                                                                       # MapPoint.cc:151-168
    w.mp_bad[mp] = 1
    obs, w.obs[mp] = w.obs[mp], {}
    for pKF in w.map_order(obs):
        idx, e = obs[pKF]
        w.kf_mp[pKF, idx] = -1                                                                         # EraseMapPointMatch(idx)
        w.obs_kf[e] = -1
        erased.append((pKF, mp, idx, e))


def map_point_culling(w, recent, cur_kf_id, first_kf_id, found, visible, n_th_obs=2):
    """LocalMapping.cc:207-228 -> (the list afterwards, the points that got SetBadFlag, the erased edges as rows)"""
    kept, culled, erased = [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for pMP in recent:
            pMP = int(pMP)
            if pMP < 0 or pMP >= w.n_mp:
                w.errors += 1
                continue
            age = int(cur_kf_id) - int(first_kf_id[pMP])
            if w.mp_bad[pMP]:                                                                          # :210
                continue
            elif f32(found[pMP]) / f32(visible[pMP]) < f32(0.25):                                      # :214
                set_bad_flag(w, pMP, erased)
                culled.append(pMP)
            elif age >= 2 and len(w.obs[pMP]) <= n_th_obs:                                             # :219
                set_bad_flag(w, pMP, erased)
                culled.append(pMP)
            elif age >= 3:                                                                             # :224
                continue
            else:
                kept.append(pMP)
    return kept, culled, erased
