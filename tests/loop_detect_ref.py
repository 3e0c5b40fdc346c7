"""A literal Python restatement of three passages of the reference's LoopClosing, written from the reference (not from the
kernels) as the model the device is compared with.  Test infrastructure: the package never imports it.

    LoopClosing::DetectLoop, the consistency groups               src/LoopClosing.cc:147-153, :155-228
    LoopClosing::ComputeSim3, mvpLoopMapPoints                    :355-375
    LoopClosing::CorrectLoop, LoopConnections                     :571-589

A key frame is a slot; the graph and the map are those of tests/covis_ref.py.
"""


class ConsistencyGroups:
    """mvConsistentGroups: a list of (set of slots, consistency counter)."""

    def __init__(self, consistency_th=3):
        self.th = consistency_th                       # mnCovisibilityConsistencyTh
        self.groups = []

    def detect(self, g, candidates):
        """DetectLoop from :147 on, for vpCandidateKFs = candidates -> mvpEnoughConsistentCandidates"""
        if not candidates:                                                                             # :147-153
            self.groups = []
            return []
        enough = []                                                                                    # :159
        vCurrentConsistentGroups = []
        vbConsistentGroup = [False] * len(self.groups)
        for pCandidateKF in candidates:                                                                # :163
            spCandidateGroup = set(g.get_connected_keyframes(pCandidateKF))                            # :167
            spCandidateGroup.add(pCandidateKF)                                                         # :168
            bEnoughConsistent = False
            bConsistentForSomeGroup = False
            for iG in range(len(self.groups)):                                                         # :172
                sPreviousGroup = self.groups[iG][0]
                bConsistent = False
                for kf in spCandidateGroup:                                                            # :177
                    if kf in sPreviousGroup:
                        bConsistent = True
                        bConsistentForSomeGroup = True
                        break
                if bConsistent:                                                                        # :187
                    nPreviousConsistency = self.groups[iG][1]
                    nCurrentConsistency = nPreviousConsistency + 1
                    if not vbConsistentGroup[iG]:                                                      # :191
                        vCurrentConsistentGroups.append((set(spCandidateGroup), nCurrentConsistency))
                        vbConsistentGroup[iG] = True
                    if nCurrentConsistency >= self.th and not bEnoughConsistent:                       # :197
                        enough.append(pCandidateKF)
                        bEnoughConsistent = True
            if not bConsistentForSomeGroup:                                                            # :206
                vCurrentConsistentGroups.append((set(spCandidateGroup), 0))
        self.groups = vCurrentConsistentGroups                                                         # :214
        return enough


def loop_map_points(g, m, matched):
    """:355-375 -> mvpLoopMapPoints as point indices (a kf_mp entry >= n_mp is skipped, as everywhere in fb_covis_map)"""
    vpLoopConnectedKFs = g.get_vector_covisible_keyframes(matched)                                     # :356
    vpLoopConnectedKFs.append(matched)                                                                 # :357
    out, mark = [], set()                              # mnLoopPointForKF == mpCurrentKF->mnId
    for pKF in vpLoopConnectedKFs:
        for i in range(int(m.kf_n[pKF])):                                                              # :363
            mp = int(m.kf_mp[pKF, i])
            if mp < 0 or mp >= m.n_mp:                                                                 # :366
                continue
            if not m.mp_bad[mp] and mp not in mark:                                                    # :368
                out.append(mp)
                mark.add(mp)
    return out


def loop_connections(g, m, connected_kfs, snapshot_before_batch=False):
    """:571-589 on the graph g (modified) -> (rows, n_counter, front): rows[j] = LoopConnections[pKFi] of member j in the
    std::set's order.  snapshot_before_batch=True is NOT the reference: vpPreviousNeighbors of every member is taken
    before the first UpdateConnections (what a batched implementation would give if it ignored the order of :576-579)."""
    before = {kf: g.get_vector_covisible_keyframes(kf) for kf in connected_kfs if 0 <= kf < g.K}
    rows, n_counter, front = [], [], []
    for pKFi in connected_kfs:                                                                         # :573
        if pKFi < 0 or pKFi >= g.K:                    # never used as an index
            rows.append([]); n_counter.append(0); front.append(-1)
            continue
        vpPreviousNeighbors = before[pKFi] if snapshot_before_batch else g.get_vector_covisible_keyframes(pKFi)   # :576
        n, f = g.update_connections(m, pKFi)                                                           # :579
        lc = set(g.get_connected_keyframes(pKFi))                                                      # :580
        for kf in vpPreviousNeighbors:                                                                 # :581-584
            lc.discard(kf)
        for kf in connected_kfs:                                                                       # :585-588
            lc.discard(kf)
        rows.append(sorted(lc, key=g.key))
        n_counter.append(n)
        front.append(f)
    return rows, n_counter, front
