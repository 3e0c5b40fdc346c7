"""A literal Python restatement of the reference's covisibility graph and KeyFrameCulling, written from the reference
(not from the kernels) as the model the device is compared with.  Test infrastructure: the package never imports it.

    KeyFrame::AddConnection / UpdateBestCovisibles / getters      src/KeyFrame.cc:179-270
    KeyFrame::UpdateConnections (graph part)                      :564-663
    KeyFrame::SetBadFlag (graph part)                             :785-808
    KeyFrame::EraseConnection                                     :885-899
    LocalMapping::KeyFrameCulling                                 src/LocalMapping.cc:656-729
    MapPoint::EraseObservation / Observations                     src/MapPoint.cc:111-137, 145-149

A key frame is a slot; std::map<KeyFrame*, ..> and std::set<KeyFrame*> iterate ascending pKF, which is kf_order[slot] here.
"""
import numpy as np

TH = 15   # KeyFrame.cc:621


class Map:
    """The caller's map (fb_covis_map) as numpy arrays."""

    def __init__(self, kf_n, kf_mp, kf_octave, mp_bad, obs_mp, obs_kf, obs_idx, kf_order):
        self.kf_n, self.kf_mp, self.kf_octave = np.asarray(kf_n), np.asarray(kf_mp), np.asarray(kf_octave)
        self.mp_bad = np.asarray(mp_bad)
        self.obs_mp, self.obs_kf, self.obs_idx = np.asarray(obs_mp), np.asarray(obs_kf), np.asarray(obs_idx)
        self.kf_order = [int(x) for x in kf_order]
        self.K, self.S = self.kf_mp.shape
        self.n_mp = len(self.mp_bad)

    def key(self, slot):
        return (self.kf_order[slot], slot)

    def observations(self):
        """MapPoint::mObservations of every point: mp -> {kf: idx}.  Erased (obs_kf < 0) and out-of-range edges are not there."""
        obs = [dict() for _ in range(self.n_mp)]
        for mp, kf, idx in zip(self.obs_mp.tolist(), self.obs_kf.tolist(), self.obs_idx.tolist()):
            if kf < 0 or kf >= self.K or mp < 0 or mp >= self.n_mp or idx < 0 or idx >= self.S:
                continue
            obs[mp][kf] = idx
        return obs


class Graph:
    """mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights of every key frame."""

    def __init__(self, K, kf_order=None):
        self.K = K
        self.kf_order = list(range(K)) if kf_order is None else [int(x) for x in kf_order]
        self.clear()

    def clear(self):
        self.weights = [dict() for _ in range(self.K)]
        self.ordered = [[] for _ in range(self.K)]
        self.ordered_w = [[] for _ in range(self.K)]

    def key(self, slot):
        return (self.kf_order[slot], slot)

    def _map_order(self, d):
        return sorted(d, key=self.key)   # iteration order of a std::map<KeyFrame*, ..>

    def _set_ordered(self, a, vPairs):
        vPairs.sort()                     # sort(vPairs.begin(), vPairs.end()) of pair<int, KeyFrame*>   (:202, :648)
        lKFs, lWs = [], []
        for w, _, kf in vPairs:
            lKFs.insert(0, kf)            # push_front                                                  (:205-209, :651-655)
            lWs.insert(0, w)
        self.ordered[a], self.ordered_w[a] = lKFs, lWs

    def update_best_covisibles(self, a):                                                               # :194-213
        self._set_ordered(a, [(w, self.key(b), b) for b, w in self.weights[a].items()])

    def add_connection(self, a, b, weight):                                                            # :179-192
        if b not in self.weights[a]:
            self.weights[a][b] = weight
        elif self.weights[a][b] != weight:
            self.weights[a][b] = weight
        else:
            return
        self.update_best_covisibles(a)

    def erase_connection(self, a, b):                                                                  # :885-899
        if b in self.weights[a]:
            del self.weights[a][b]
            self.update_best_covisibles(a)

    def update_connections(self, m, a):
        """KeyFrame::UpdateConnections of slot a (:564-663) -> (KFcounter.size(), mvpOrderedConnectedKeyFrames.front() or -1)"""
        obs = m.observations()
        KFcounter = {}
        for i in range(int(m.kf_n[a])):                                                                # :580
            mp = int(m.kf_mp[a, i])
            if mp < 0 or mp >= m.n_mp:                                                                 # :584 (NULL; out of range is skipped)
                continue
            if m.mp_bad[mp]:                                                                           # :587
                continue
            for kf in obs[mp]:
                if kf == a:                                                                            # :594
                    continue
                KFcounter[kf] = KFcounter.get(kf, 0) + 1
        if not KFcounter:                                                                              # :604-612
            return 0, (self.ordered[a][0] if self.ordered[a] else -1)
        nmax, pKFmax, vPairs = 0, None, []
        for kf in self._map_order(KFcounter):                                                          # :625
            w = KFcounter[kf]
            if w > nmax:
                nmax, pKFmax = w, kf
            if w >= TH:
                vPairs.append((w, self.key(kf), kf))
                self.add_connection(kf, a, w)
        if not vPairs:                                                                                 # :639-643
            vPairs.append((nmax, self.key(pKFmax), pKFmax))
            self.add_connection(pKFmax, a, nmax)
        self.weights[a] = dict(KFcounter)                                                              # :661
        self._set_ordered(a, vPairs)
        return len(KFcounter), self.ordered[a][0]

    def erase_keyframe(self, slot):
        """The graph part of KeyFrame::SetBadFlag (:797-798, :807-808)"""
        for b in self._map_order(self.weights[slot]):
            self.erase_connection(b, slot)
        self.weights[slot] = {}
        self.ordered[slot], self.ordered_w[slot] = [], []

    # ---- getters -------------------------------------------------------------------------------------------------------
    def get_vector_covisible_keyframes(self, a):                                                       # :230-234
        return list(self.ordered[a])

    def get_best_covisibility_keyframes(self, a, N):                                                   # :236-244
        return list(self.ordered[a][:N])

    def get_covisibles_by_weight(self, a, w):                                                          # :246-261
        if not self.ordered[a]:
            return []
        ws = self.ordered_w[a]
        it = next((i for i, x in enumerate(ws) if w > x), len(ws))   # upper_bound(.., w, weightComp): the first x with w > x
        if it == len(ws):
            return []
        return list(self.ordered[a][:it])

    def get_connected_keyframes(self, a):                                                              # :221-228 (a std::set)
        return self._map_order(self.weights[a])

    def get_weight(self, a, b):                                                                        # :263-270
        return self.weights[a].get(b, 0)

    def kfdb_rows(self, n=10):
        rows = np.full((self.K, n), -1, np.int32)
        for a in range(self.K):
            best = self.get_best_covisibility_keyframes(a, n)
            rows[a, :len(best)] = best
        return rows


def keyframe_culling(g, m, cur, id0=-1, not_erase=None, apply_effects=True):
    """LocalMapping::KeyFrameCulling (LocalMapping.cc:656-729) -> dict(slots, n_redundant, n_mps, culled, mp_bad_after).
    The map and the graph are not modified: SetBadFlag()'s effects on later key frames are kept in copies.
    apply_effects=False judges every key frame on the unchanged map (what the call would give without those effects)."""
    obs = m.observations()
    nObs = [len(o) for o in obs]                       # MapPoint::Observations(), monocular
    bad = [bool(b) for b in m.mp_bad]
    out = dict(slots=[], n_redundant=[], n_mps=[], culled=[])
    for pKF in g.get_vector_covisible_keyframes(cur):                                                  # :662-664
        out["slots"].append(pKF)
        if pKF == id0:                                                                                 # :667
            for k in ("n_redundant", "n_mps", "culled"):
                out[k].append(0)
            continue
        thObs, nRedundantObservations, nMPs = 3, 0, 0
        N = int(m.kf_n[pKF])
        for i in range(N):
            mp = int(m.kf_mp[pKF, i])
            if mp < 0 or mp >= m.n_mp or bad[mp]:                                                      # :678-680
                continue
            nMPs += 1
            if nObs[mp] > thObs:                                                                       # :689
                scaleLevel = int(m.kf_octave[pKF, i])
                n = 0
                for pKFi in sorted(obs[mp], key=m.key):
                    if pKFi == pKF:
                        continue
                    if int(m.kf_octave[pKFi, obs[mp][pKFi]]) <= scaleLevel + 1:                        # :701
                        n += 1
                        if n >= thObs:
                            break
                if n >= thObs:
                    nRedundantObservations += 1
        cull = float(nRedundantObservations) > 0.9 * nMPs                                              # :717
        out["n_redundant"].append(nRedundantObservations)
        out["n_mps"].append(nMPs)
        out["culled"].append(int(cull))
        if not cull or not apply_effects or (not_erase is not None and not_erase[pKF]):               # KeyFrame.cc:790-794
            continue
        for i in range(N):                                                                             # KeyFrame.cc:800-802
            mp = int(m.kf_mp[pKF, i])
            if mp < 0 or mp >= m.n_mp:
                continue
            if pKF in obs[mp]:                                                                         # MapPoint.cc:116
                del obs[mp][pKF]
                nObs[mp] -= 1
                if nObs[mp] <= 2:                                                                      # MapPoint.cc:129-136
                    bad[mp] = True
                    obs[mp] = {}                                                                       # MapPoint::SetBadFlag
    out["mp_bad_after"] = np.array(bad, np.uint8)
    return out
