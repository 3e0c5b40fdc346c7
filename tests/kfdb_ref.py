"""A literal restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc), of L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) and of DetectLoop's reference-score loop (src/LoopClosing.cc:127-141):
per-key-frame objects with the six query members, a real inverted file of lists, the reference's loops in the reference's
order.  Python floats are the doubles, numpy.float32 is every `float` variable.  The device is held to this bit for bit."""
from bisect import bisect_left

import numpy as np

F32 = np.float32


class BowVector:
    """std::map<WordId, WordValue> as two parallel ascending lists."""

    def __init__(self, ids=(), vals=()):
        self.ids = [int(x) for x in ids]
        self.vals = [float(x) for x in vals]
        assert all(a < b for a, b in zip(self.ids, self.ids[1:])), "word ids must be strictly ascending"

    def __len__(self):
        return len(self.ids)


def l1_score(v1, v2):
    """L1Scoring::score(v1, v2) -> double"""
    i, j, n1, n2 = 0, 0, len(v1.ids), len(v2.ids)
    score = 0.0
    while i != n1 and j != n2:
        vi, wi = v1.vals[i], v2.vals[j]
        if v1.ids[i] == v2.ids[j]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif v1.ids[i] < v2.ids[j]:
            i = bisect_left(v1.ids, v2.ids[j])  # v1.lower_bound(v2_it->first)
        else:
            j = bisect_left(v2.ids, v1.ids[i])
    score = -score / 2.0
    return score


class KeyFrame:
    def __init__(self, slot, bow):
        self.slot = slot
        self.mBowVec = bow
        self.mnLoopQuery = 0          # KeyFrame.cc:35
        self.mnLoopWords = 0
        self.mLoopScore = F32(0.0)    # uninitialised in the reference; defined as 0
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F32(0.0)


class KeyFrameDatabase:
    def __init__(self, max_keyframes):
        self.K = max_keyframes
        self.clear()

    def clear(self):
        """KeyFrameDatabase::clear as Tracking::Reset uses it: the key frames themselves are deleted too."""
        self.mvInvertedFile = {}
        self.kf = [KeyFrame(s, BowVector()) for s in range(self.K)]
        self.inside = [False] * self.K

    def add(self, slot, ids, vals):
        assert not self.inside[slot]
        pKF = self.kf[slot] = KeyFrame(slot, BowVector(ids, vals))
        for w in pKF.mBowVec.ids:
            self.mvInvertedFile.setdefault(w, []).append(pKF)
        self.inside[slot] = True

    def erase(self, slot):
        assert self.inside[slot]
        pKF = self.kf[slot]
        for w in pKF.mBowVec.ids:
            lKFs = self.mvInvertedFile[w]
            for k, other in enumerate(lKFs):
                if other is pKF:
                    del lKFs[k]
                    break
        self.inside[slot] = False

    def _neighbours(self, covis, slot):
        return [self.kf[int(s)] for s in covis[slot] if 0 <= int(s) < self.K]

    def _finish(self, info, lAccScoreAndMatch, bestAccScore, words, score):
        minScoreToRetain = F32(0.75) * bestAccScore
        spAlreadyAddedKF = set()
        out = []
        dup = 0
        for acc, pKFi in lAccScoreAndMatch:
            if acc > minScoreToRetain:
                if pKFi.slot not in spAlreadyAddedKF:
                    out.append(pKFi.slot)
                    spAlreadyAddedKF.add(pKFi.slot)
                else:
                    dup += 1
        info.update(candidates=out, duplicates_removed=dup, acc=[(a, k.slot) for a, k in lAccScoreAndMatch])
        return self._state(info, words, score)

    def _state(self, info, words, score):
        info.setdefault("candidates", [])
        info["common_words"] = np.array([getattr(k, words) for k in self.kf], np.int32)
        info["scores"] = np.array([getattr(k, score) for k in self.kf], np.float32)
        return info

    def detect_relocalization_candidates(self, query_id, ids, vals, covis):
        F = BowVector(ids, vals)
        lKFsSharingWords = []
        for w in F.ids:
            for pKFi in self.mvInvertedFile.get(w, ()):
                if pKFi.mnRelocQuery != query_id:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = query_id
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        info = dict(n_sharing=len(lKFsSharingWords), max_common_words=0, n_scored=0, listed=[k.slot for k in lKFsSharingWords],
                    below_threshold=0, self_best=0, neighbour_best=0, below_min_score=0)
        if not lKFsSharingWords:
            return self._state(info, "mnRelocWords", "mRelocScore")
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        nscores = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                nscores += 1
                si = F32(l1_score(F, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
            else:
                info["below_threshold"] += 1
        info.update(max_common_words=maxCommonWords, n_scored=nscores)
        if not lScoreAndMatch:
            return self._state(info, "mnRelocWords", "mRelocScore")
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in self._neighbours(covis, pKFi.slot):
                if pKF2.mnRelocQuery != query_id:
                    continue
                accScore = F32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            info["self_best" if pBestKF is pKFi else "neighbour_best"] += 1
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._finish(info, lAccScoreAndMatch, bestAccScore, "mnRelocWords", "mRelocScore")

    def detect_loop_candidates(self, query_id, ids, vals, min_score, connected, covis):
        minScore = F32(min_score)
        pKF = BowVector(ids, vals)
        spConnectedKeyFrames = set(int(s) for s in connected)
        lKFsSharingWords = []
        for w in pKF.ids:
            for pKFi in self.mvInvertedFile.get(w, ()):
                if pKFi.mnLoopQuery != query_id:
                    pKFi.mnLoopWords = 0
                    if pKFi.slot not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = query_id
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        info = dict(n_sharing=len(lKFsSharingWords), max_common_words=0, n_scored=0, listed=[k.slot for k in lKFsSharingWords],
                    below_threshold=0, self_best=0, neighbour_best=0, below_min_score=0)
        if not lKFsSharingWords:
            return self._state(info, "mnLoopWords", "mLoopScore")
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnLoopWords > maxCommonWords:
                maxCommonWords = k.mnLoopWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        nscores = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                nscores += 1
                si = F32(l1_score(pKF, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
                else:
                    info["below_min_score"] += 1
            else:
                info["below_threshold"] += 1
        info.update(max_common_words=maxCommonWords, n_scored=nscores)
        if not lScoreAndMatch:
            return self._state(info, "mnLoopWords", "mLoopScore")
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in self._neighbours(covis, pKFi.slot):
                if pKF2.mnLoopQuery == query_id and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            info["self_best" if pBestKF is pKFi else "neighbour_best"] += 1
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._finish(info, lAccScoreAndMatch, bestAccScore, "mnLoopWords", "mLoopScore")

    def min_score(self, ids, vals, slots, skip=None):
        """LoopClosing.cc:127-141 -> (scores float32 per list entry, minScore)"""
        cur = BowVector(ids, vals)
        minScore = F32(1)
        scores = []
        for i, s in enumerate(slots):
            score = F32(l1_score(cur, self.kf[int(s)].mBowVec))
            scores.append(score)
            if skip is not None and skip[i]:
                continue
            if score < minScore:
                minScore = score
        return np.array(scores, np.float32), minScore
