"""A literal Python restatement of the reference's key frame spanning tree and Tracking::UpdateLocalMap, written from the
reference (not from the kernels) on top of covis_ref's graph model.  Test infrastructure: the package never imports it.

    KeyFrame::UpdateConnections, the mbFirstConnection block        src/KeyFrame.cc:665-690
    AddChild / EraseChild / ChangeParent / GetChilds / GetParent     :704-741
    KeyFrame::SetBadFlag (tree part)                                 :810-868
    Tracking::UpdateLocalKeyFrames / UpdateLocalPoints               src/Tracking.cc:2095-2229

std::set<KeyFrame*> and std::map<KeyFrame*, ..> iterate ascending pKF: kf_order[slot] here (Graph.key).
"""
import numpy as np

import covis_ref as R

MAX_EXPAND = 80                                                                                        # Tracking.cc:2175


class Tree:
    """mpParent, mspChildrens, mbFirstConnection of every key frame, next to a covis_ref.Graph."""

    def __init__(self, g):
        self.g = g
        self.errors = 0
        self.clear()

    def clear(self):
        K = self.g.K
        self.parent = [-1] * K
        self.childs = [set() for _ in range(K)]
        self.first = [True] * K

    def add_child(self, a, c):                                                                         # :704-716
        self.childs[a].add(c)

    def erase_child(self, a, c):                                                                       # :718-722
        self.childs[a].discard(c)

    def change_parent(self, c, p):                                                                     # :724-729
        self.parent[c] = p
        self.add_child(p, c)

    def get_childs(self, a):                                                                           # :731-735 (a std::set)
        return sorted(self.childs[a], key=self.g.key)

    def get_parent(self, a):
        return self.parent[a]

    def set_state(self, parent, linked, first):
        self.clear()
        for c, (p, l, f) in enumerate(zip(parent, linked, first)):
            self.parent[c] = int(p)
            if l and p >= 0:
                self.childs[int(p)].add(c)
            self.first[c] = bool(f)

    def state(self):
        """(parent, linked, first) as the device keeps them: linked[c] = c is in mspChildrens of parent[c]"""
        K = self.g.K
        linked = [1 if self.parent[c] >= 0 and c in self.childs[self.parent[c]] else 0 for c in range(K)]
        return np.array(self.parent, np.int32), np.array(linked, np.uint8), np.array([int(f) for f in self.first], np.uint8)

    def update_connections(self, m, a, id0=-1, now_state4=False, frame_id=None, in_map=None):
        """KeyFrame::UpdateConnections of slot a with the spanning tree (:564-690) -> (KFcounter.size(), front)"""
        n, front = self.g.update_connections(m, a)
        if n == 0:                                                                                     # :604-612 returned
            return n, front
        if self.first[a] and a != id0:                                                                 # :665
            pKFt = front                                                                               # :667
            if now_state4 and frame_id[pKFt] > frame_id[a]:                                            # :669
                nearIDx = 0
                for pKF in sorted((s for s in range(self.g.K) if in_map[s]), key=self.g.key):          # Map::GetAllKeyFrames: a std::set
                    if frame_id[pKF] > nearIDx and frame_id[pKF] < frame_id[a]:                        # :679
                        nearIDx = frame_id[pKF]
                        pKFt = pKF
            self.parent[a] = pKFt                                                                      # :687-689
            self.add_child(pKFt, a)
            self.first[a] = False
        return n, front

    def set_bad_flag(self, slot, kf_bad):
        """The spanning tree part of KeyFrame::SetBadFlag (:810-868)"""
        g = self.g
        mpParent = self.parent[slot]
        if mpParent < 0:                                                                               # the reference dereferences it
            self.errors += 1
            return
        sParentCandidates = {mpParent}                                                                 # :811-812
        mspChildrens = self.childs[slot]
        while mspChildrens:                                                                            # :816
            bContinue, mx, pC, pP = False, -1, None, None
            for pKF in sorted(mspChildrens, key=g.key):                                                # :824
                if kf_bad[pKF]:
                    continue
                for conn in g.get_vector_covisible_keyframes(pKF):                                     # :831-832
                    for cand in sorted(sParentCandidates, key=g.key):
                        if conn == cand:                                                               # :836
                            w = g.get_weight(pKF, conn)
                            if w > mx:                                                                 # :839
                                pC, pP, mx, bContinue = pKF, conn, w, True
            if bContinue:                                                                              # :851-856
                self.change_parent(pC, pP)
                sParentCandidates.add(pC)
                mspChildrens.discard(pC)
            else:
                break
        for c in sorted(mspChildrens, key=g.key):                                                      # :862-866
            self.change_parent(c, mpParent)
        self.erase_child(mpParent, slot)                                                               # :868


def list_limit(K):
    """No list the device produces is longer: voters <= K, with an expansion <= 80 + 3"""
    return max(K, MAX_EXPAND + 4)


def update_local_map(tree, m, n, map_point, kf_bad, local_kf, ref_kf, cap_kf=None, cap_mp=None, obs=None):
    """Tracking::UpdateLocalMap for one frame: n = N, map_point = mvpMapPoints (a list, modified in place), local_kf /
    ref_kf = mvpLocalKeyFrames / mpReferenceKF as they come in.  -> dict(local_kf, n_local_kf, local_mp, n_local_mp, ref_kf,
    n_voters, overflow, errors); the lists are cut at the capacities as the device cuts them."""
    g = tree.g
    K = g.K
    obs = m.observations() if obs is None else obs
    errors = 0
    cap_kf = list_limit(K) if cap_kf is None else cap_kf
    cap_mp = m.n_mp if cap_mp is None else cap_mp
    mvpLocalKeyFrames = list(local_kf)
    # ---- UpdateLocalKeyFrames (:2121-2229)
    keyframeCounter = {}
    for i in range(min(max(int(n), 0), len(map_point))):                                               # :2125
        mp = int(map_point[i])
        if mp < 0:
            continue
        if mp >= m.n_mp:
            errors += 1
            continue
        if not m.mp_bad[mp]:                                                                           # :2130
            for kf in obs[mp]:
                keyframeCounter[kf] = keyframeCounter.get(kf, 0) + 1
        else:
            map_point[i] = -1                                                                          # :2138
    carried = not keyframeCounter
    if not carried:                                                                                    # :2143
        mx, pKFmax = 0, None
        mvpLocalKeyFrames = []
        marks = set()                                                                                  # mnTrackReferenceForFrame == mnId
        for pKF in sorted(keyframeCounter, key=g.key):                                                 # :2153
            if kf_bad[pKF]:
                continue
            if keyframeCounter[pKF] > mx:
                mx, pKFmax = keyframeCounter[pKF], pKF
            mvpLocalKeyFrames.append(pKF)
            marks.add(pKF)
        for it in range(len(mvpLocalKeyFrames)):                                                       # :2172: itEndKF is taken here
            if len(mvpLocalKeyFrames) > MAX_EXPAND:                                                    # :2175
                break
            pKF = mvpLocalKeyFrames[it]
            for pNeighKF in g.get_best_covisibility_keyframes(pKF, 10):                                # :2180
                if not kf_bad[pNeighKF]:
                    if pNeighKF not in marks:
                        mvpLocalKeyFrames.append(pNeighKF)
                        marks.add(pNeighKF)
                        break
            for pChildKF in tree.get_childs(pKF):                                                      # :2196
                if not kf_bad[pChildKF]:
                    if pChildKF not in marks:
                        mvpLocalKeyFrames.append(pChildKF)
                        marks.add(pChildKF)
                        break
            pParent = tree.get_parent(pKF)                                                             # :2211
            if pParent >= 0:
                if pParent not in marks:
                    mvpLocalKeyFrames.append(pParent)
                    marks.add(pParent)
                    break                                                                              # :2218 leaves the outer for
        if pKFmax is not None:                                                                         # :2224
            ref_kf = pKFmax
    # ---- UpdateLocalPoints (:2095-2118) on what fitted
    walk = mvpLocalKeyFrames[:min(cap_kf, list_limit(K))]
    mvpLocalMapPoints, seen = [], set()
    for pKF in walk:
        if pKF < 0 or pKF >= K:                                                                        # (a carried-over entry out of range)
            errors += 1
            continue
        for i in range(min(max(int(m.kf_n[pKF]), 0), m.S)):
            mp = int(m.kf_mp[pKF, i])
            if mp < 0:
                continue
            if mp >= m.n_mp:
                errors += 1
                continue
            if mp in seen:                                                                             # :2109
                continue
            if not m.mp_bad[mp]:
                mvpLocalMapPoints.append(mp)
                seen.add(mp)
    n_kf = len(mvpLocalKeyFrames)
    return dict(local_kf=mvpLocalKeyFrames[:cap_kf], n_local_kf=n_kf, local_mp=mvpLocalMapPoints[:cap_mp], n_local_mp=len(mvpLocalMapPoints),
                ref_kf=ref_kf, n_voters=len(keyframeCounter), carried=carried,
                overflow=int((not carried and n_kf > cap_kf) or len(mvpLocalMapPoints) > cap_mp), errors=errors)
