"""A literal Python restatement of the bird side of the reference's key-frame graph and of its local bird map, written from
the reference text (not from the kernels) as the model the device is compared with.  Test infrastructure: the package never
imports it.

    KeyFrame::UpdateBirdConnections                               src/KeyFrame.cc:418-562
    KeyFrame::AddChild                                            :704-716
    Map::AddKeyFrame, the bird block                              src/Map.cc:41-46
    Map::UpdateLocalBirdMap                                       :97-153

A key frame is a slot and a bird point an index; std::map<KeyFrame*, ..> / std::set<MapPointBird*> iterate ascending
pointer, which is (kf_order[slot], slot) / (mpb_order[index], index) here.  `counters` records which branches ran.
"""
import math
from collections import Counter

import numpy as np

TH = 2   # KeyFrame.cc:483


class BirdTables:
    """The bird side of fb_covis_kf_tables as numpy arrays."""

    def __init__(self, kf_nb, kf_mpb, mpb_bad, bobs_mpb, bobs_kf, bobs_idx):
        self.kf_nb, self.kf_mpb, self.mpb_bad = np.asarray(kf_nb), np.asarray(kf_mpb), np.asarray(mpb_bad)
        self.bobs_mpb, self.bobs_kf, self.bobs_idx = np.asarray(bobs_mpb), np.asarray(bobs_kf), np.asarray(bobs_idx)
        self.K, self.BS = self.kf_mpb.shape
        self.n_mpb = len(self.mpb_bad)

    def observations(self):
        """MapPointBird::mObservations of every point: index -> {kf: idx}; erased (bobs_kf < 0) edges are not there"""
        obs = [dict() for _ in range(self.n_mpb)]
        for p, kf, idx in zip(self.bobs_mpb.tolist(), self.bobs_kf.tolist(), self.bobs_idx.tolist()):
            if kf < 0:
                continue
            obs[p][kf] = idx
        return obs


class BirdGraph:
    """mvpBirdConnectedKeyFrames (+ the weights :512 computes), mpParent, mspChildrens and mbFirstConnection of every key frame."""

    def __init__(self, K, kf_order, parent=None, linked=None, first=None):
        self.K = K
        self.kf_order = [int(x) for x in kf_order]
        self.bird_connected = [[] for _ in range(K)]
        self.bird_weights = [[] for _ in range(K)]
        self.parent = [-1] * K if parent is None else [int(x) for x in parent]
        self.first = [True] * K if first is None else [bool(x) for x in first]
        self.children = [set() for _ in range(K)]
        if linked is not None:
            for c in range(K):
                if linked[c] and self.parent[c] >= 0:
                    self.children[self.parent[c]].add(c)
        self.counters = Counter()
        self.errors = 0   # the places where the reference reads an uninitialised pointer

    def key(self, slot):
        return (self.kf_order[slot], slot)

    def linked(self):
        return [1 if self.parent[c] >= 0 and c in self.children[self.parent[c]] else 0 for c in range(self.K)]

    def _nearest_earlier(self, a, frame_id, in_map):
        """:453-465 / :535-547 over mpMap->GetAllKeyFrames() (a std::set<KeyFrame*>: ascending pointer); None = nearKF is
        never assigned"""
        near, near_idx = None, 0
        for kf in sorted((s for s in range(self.K) if in_map[s]), key=self.key):
            if frame_id[kf] > near_idx and frame_id[kf] < frame_id[a]:
                near_idx, near = frame_id[kf], kf
        return near

    def _set_parent(self, a, p):
        self.parent[a] = p                 # mpParent = ..
        self.children[p].add(a)            # mpParent->AddChild(this)
        self.first[a] = False              # mbFirstConnection = false

    def _search(self, a, frame_id, in_map):
        self.counters["search_taken"] += 1
        near = self._nearest_earlier(a, frame_id, in_map)
        if near is None:                   # the reference dereferences the uninitialised nearKF
            self.counters["search_finds_nothing"] += 1
            self.errors += 1
            return
        self._set_parent(a, near)

    def update_bird_connections(self, T, obs, a, now_state, id0_slot=-1, frame_id=None, in_map=None):
        """UpdateBirdConnections(nowState) of key frame a -> (KFcounter.size(), front of the list afterwards or -1)"""
        KFcounter = {}
        for i in range(int(T.kf_nb[a])):                                                      # :428-445
            p = int(T.kf_mpb[a][i])
            if p == -1 or T.mpb_bad[p]:
                continue
            for kf in sorted(obs[p], key=self.key):
                if kf == a:
                    continue
                KFcounter[kf] = KFcounter.get(kf, 0) + 1
        if not KFcounter:                                                                     # :447-480
            self.counters["empty_counter"] += 1
            if now_state >= 3 and self.parent[a] == -1:
                self._search(a, frame_id, in_map)
            return 0, (self.bird_connected[a][0] if self.bird_connected[a] else -1)
        vPairs = []
        for kf in sorted(KFcounter, key=self.key):                                            # :487-493
            if KFcounter[kf] >= TH:
                vPairs.append((KFcounter[kf], self.key(kf), kf))
        vPairs.sort()                                                                         # :499
        lKFs, lWs = [], []
        for w, _, kf in vPairs:                                                               # :502-506
            lKFs.insert(0, kf)
            lWs.insert(0, w)
        self.bird_connected[a], self.bird_weights[a] = lKFs, lWs                              # :511-512
        if not lKFs:
            self.counters["list_empty_after_threshold"] += 1
        if self.parent[a] == -1 or self.first[a]:                                             # :514
            if a == id0_slot:                                                                 # :516-517
                self.counters["id0_return"] += 1
            elif lKFs:                                                                        # :519-529
                self._set_parent(a, lKFs[0])
            elif now_state >= 3:                                                              # :533-557
                self._search(a, frame_id, in_map)
        return len(KFcounter), (lKFs[0] if lKFs else -1)

    def run_batch(self, T, slots, n_counter, now_state, id0_slot=-1, frame_id=None, in_map=None):
        """The calls UpdateConnections makes for the batch (:701 when the front counter is non-empty, :608-609 otherwise), in
        list order -> (n_bird_counter, bird_front) lists"""
        obs = T.observations()
        out = []
        for q, a in enumerate(slots):
            if (n_counter is None or n_counter[q] != 0) or now_state >= 3:
                out.append(self.update_bird_connections(T, obs, a, now_state, id0_slot, frame_id, in_map))
            else:
                out.append((0, self.bird_connected[a][0] if self.bird_connected[a] else -1))
        return [o[0] for o in out], [o[1] for o in out]


def camera_centre(Tcw):
    """KeyFrame::GetCameraCenter() from a row-major 3x4 float Tcw the way the device derives it: -Rcw^T tcw with the
    products and the sum in double, rounded to float once"""
    T = np.asarray(Tcw, np.float32).reshape(12)
    ow = np.zeros(3, np.float32)
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += float(T[k * 4 + r]) * float(T[k * 4 + 3])
        ow[r] = np.float32(-s)
    return ow


def distance(ref, cur):
    """cv::norm(refTw - curTw, cv::NORM_L2) of CV_32F: the difference in float, the squares summed in double in order"""
    d = np.asarray(ref, np.float32) - np.asarray(cur, np.float32)
    s = 0.0
    for c in range(3):
        s += float(d[c]) * float(d[c])
    return math.sqrt(s)


class LocalBirdMap:
    """Map::localKFbird, curTw and localMapPointBirds."""

    def __init__(self, mpb_order=None):
        self.local_kf = []
        self.local_mpb = []
        self.mpb_order = None if mpb_order is None else [int(x) for x in mpb_order]
        self.counters = Counter()

    def pkey(self, p):
        return (p if self.mpb_order is None else self.mpb_order[p], p)

    def add_keyframe(self, T, ow, slot):                                                      # Map.cc:41-46
        self.local_kf.insert(0, slot)
        self.cur = np.asarray(ow[slot], np.float32)
        self.update_local_bird_map(T, ow)

    def update_local_bird_map(self, T, ow):                                                   # :97-153
        s = set()
        kept, kept_points, near_points = [], set(), set()
        for kf in list(self.local_kf):
            dis = distance(ow[kf], self.cur)
            if dis > 5:                                                                       # :106-109
                self.counters["far_member"] += 1
                continue
            pMP_sum = 0
            mine = set()
            for i in range(int(T.kf_nb[kf])):                                                 # :114-125
                p = int(T.kf_mpb[kf][i])
                if p == -1:
                    continue
                mine.add(p)
                if self.pkey(p) not in s:
                    s.add(self.pkey(p))
                    pMP_sum += 1
            near_points |= mine
            if pMP_sum < 10:                                                                  # :127-128
                self.counters["member_dropped_below_10"] += 1
            else:
                kept.append(kf)
                kept_points |= mine
        self.counters["point_only_from_dropped_member"] += len(near_points - kept_points)
        self.local_kf = kept
        self.local_mpb = [p for _, p in sorted(s)]                                            # :134-143
