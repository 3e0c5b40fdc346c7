"""ORBextractor.cc restated literally in plain Python, from the reference text alone -- TEST INFRASTRUCTURE ONLY.

One object per ExtractorNode and per KeyPoint, a real list with front insertion, `numpy.float32` scalars wherever the
reference has `float`.  Line numbers are those of ORBextractor.cc.  Restated: the constructor tables (:410-470), the cell
loop of ComputeKeyPointsOctTree (:765-848), DivideNode (:481-537), DistributeOctTree (:539-763), IC_Angle and
computeOrbDescriptor (:77-147) and the assembly of operator() (:1076-1104).

Taken as given ("PARITY UNPINNED"): the pyramid levels and their blurred copies are INPUTS (they come
from the side under test, so cv::resize and cv::GaussianBlur never enter a comparison), and three small seams are written
here from DESIGN's sentences: cv::FAST on a cell (`fast_cell`), cvRound (`cv_round`, half to even) and fastAtan2 / cos /
sin (`fast_atan2`, `cos_sin`).  The rBRIEF pattern is a number table; it is read from the repository's data table
(oracle/orb_pattern.inc, whose sha256 is stated there).

The (size, pointer) sort of :684 breaks ties by heap address in the reference; as DESIGN section 2 restates it, a node
created later counts as the larger pointer.

Every decision has a named wrong variant (VARIANTS); `extract(..., variant=name)` runs the model with that one decision
misread.  tests/orb_cases.py builds the inputs that tell each of them from the model.

Where the reference itself has no defined answer:
  * nIni == 0 (a level more than twice as high as wide): `hX` is a division by zero and `vpIniNodes[kp.pt.x/hX]` indexes an
    empty vector (:545, :569).  The model returns no key points for such a level, as product and oracle do.
Variants that no constructible input can separate, and why they are not in VARIANTS:
  * the row `continue` at -6 and the column `continue` at -3 (:794, :803 with each other's constant): a cell window that
    starts at iniX is clamped to maxBorderX, and cv::FAST tests nothing in a window narrower than 7.  The column test skips
    exactly the windows of width <= 6; with -3 it would keep those of width 4..6, which yield nothing.  The row test skips
    the windows of height <= 3; with -6 it would also skip those of height 4..6, which yield nothing either.  Both
    misreadings are kept as INSEPARABLE and run: they change the trace's skipped-cell count and no key point.
  * `maxY > maxBorderY` against `>=` in the clamp of :796 / :805: both give min(maxY, maxBorderY).
  * `pt *= scale` on level 0 too (:1095 without its `if`): mvScaleFactor[0] is exactly 1.0f and x * 1.0f == x for every
    float, so the misreading computes the reference's result.  What CAN be told apart is the scaling left out above
    level 0 (`scale_missing`).
  * the order of the four `push_front`s against any other order WITH the same response maxima: list order is visible only
    as output order, which every case compares, so it needs no variant of its own.
"""
import math
import os
import re

import numpy as np

f32 = np.float32
PATCH_SIZE, HALF_PATCH_SIZE, EDGE_THRESHOLD = 31, 15, 19   # :72-74

VARIANTS = (
    "nini_floor",               # :543 nIni by truncation
    "nini_half_even",           # :543 nIni by round-half-to-even
    "bounds_rounded",           # :555-556 node bounds rounded instead of truncated
    "split_le",                 # :515/:517/:522 `<=` at the split line
    "floor_halves",             # :483-484 floor instead of ceil
    "finish_gt_n",              # :669/:730/:734 `> N` for `>= N`
    "expand_ge_n",              # :673 `>= N` for `> N`
    "sort_tie_oldest_first",    # :684-685 equal sizes walked oldest node first
    "no_break",                 # :730-731 without the break
    "best_ge",                  # :752 `>=`: the last maximum wins
    "best_tie_raster",          # :752 ties of the best by raster order of the level, not vToDistributeKeys order
    "second_fast_below_count",  # :812 second FAST when the first found fewer than 2, not none
    "fast_merged",              # :812-816 both thresholds' results merged
    "scale_missing",            # :1095-1101 `pt *= scale` left out above level 0
)

# Misreadings that are implemented like the variants but that no input can tell from the model (module docstring);
# tests/test_orb_cases.py asserts that they change no case, the trace's skipped-cell count aside.
INSEPARABLE = (
    "row_continue_6",           # :794 `iniY >= maxBorderY-6`
    "col_continue_3",           # :803 `iniX >= maxBorderX-3`
)


# ------------------------------------------------------------------------------------------------------------------
# seams
# ------------------------------------------------------------------------------------------------------------------
def cv_round(v):
    """cvRound: to nearest, halves to even."""
    return int(np.rint(np.float64(v)))


_P1 = f32(0.9997878412794807) * f32(180.0 / math.pi)
_P3 = f32(-0.3258083974640975) * f32(180.0 / math.pi)
_P5 = f32(0.1555786518463281) * f32(180.0 / math.pi)
_P7 = f32(-0.04432655554792128) * f32(180.0 / math.pi)
_EPS = f32(2.220446049250313e-16)


def fast_atan2(y, x):
    """cv::fastAtan2(float y, float x): degrees in [0, 360), 7th-order odd polynomial, every operation in float32."""
    y, x = f32(y), f32(x)
    ax, ay = f32(abs(x)), f32(abs(y))
    if ax >= ay:
        c = f32(ay / f32(ax + _EPS))
        c2 = f32(c * c)
        a = f32(f32(f32(f32(f32(f32(f32(_P7 * c2) + _P5) * c2) + _P3) * c2) + _P1) * c)
    else:
        c = f32(ax / f32(ay + _EPS))
        c2 = f32(c * c)
        a = f32(f32(90.0) - f32(f32(f32(f32(f32(f32(f32(_P7 * c2) + _P5) * c2) + _P3) * c2) + _P1) * c))
    if x < 0:
        a = f32(f32(180.0) - a)
    if y < 0:
        a = f32(f32(360.0) - a)
    return a


def cos_sin(angle):
    """cos / sin of a float: the double function rounded once to float."""
    return f32(math.cos(float(angle))), f32(math.sin(float(angle)))


# the 16 ring pixels of FAST-9-16 (dx, dy), clockwise from (0, 3)
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
        (-3, 1), (-2, 2), (-1, 3))


def fast_cell(sub, thr):
    """cv::FAST(sub, thr, nonmaxSuppression=true) -> [(x, y, score)] in raster order, coordinates inside `sub`.

    A pixel at least 3 px inside passes at threshold t iff 9 contiguous ring pixels are all brighter than v + t or all
    darker than v - t.  m = max over the 16 arcs (both signs) of the arc's smallest difference is the smallest t at
    which it no longer passes, so it passes at thr iff m > thr and its score, the largest passing threshold, is m - 1.
    Kept: a passing pixel whose score is strictly larger than the scores of its 8 neighbours in this call (0 for a
    neighbour that does not pass at thr or lies in the rim)."""
    h, w = sub.shape
    if h < 7 or w < 7:
        return []
    v = sub.astype(np.int32)
    c = v[3:h - 3, 3:w - 3]
    d = np.stack([v[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING])
    m = np.zeros(c.shape, np.int32)
    for e in (d, -d):
        e2 = np.concatenate([e, e[:8]])
        for s in range(16):
            m = np.maximum(m, e2[s:s + 9].min(axis=0))
    passes = m > thr
    score = np.zeros((h - 4, w - 4), np.int32)   # one pixel of zeros around the tested interior
    score[1:-1, 1:-1] = np.where(passes, m - 1, 0)
    s0 = score[1:-1, 1:-1]
    keep = passes.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= s0 > score[1 + dy:score.shape[0] - 1 + dy, 1 + dx:score.shape[1] - 1 + dx]
    ys, xs = np.nonzero(keep)
    return [(int(x) + 3, int(y) + 3, int(s0[y, x])) for y, x in zip(ys, xs)]


_PATTERN = None


def pattern():
    """bit_pattern_31_ as 512 (x, y) points (:150-408, :448-450)."""
    global _PATTERN
    if _PATTERN is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "orb_pattern.inc")
        text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        v = np.array([int(t) for t in re.findall(r"-?\d+", text)], np.int32)
        assert v.size == 1024
        _PATTERN = v.reshape(512, 2)
    return _PATTERN


# ------------------------------------------------------------------------------------------------------------------
# the reference's objects
# ------------------------------------------------------------------------------------------------------------------
class KeyPoint:
    __slots__ = ("x", "y", "size", "angle", "response", "octave", "seq")

    def __init__(self, x, y, size, response):
        self.x, self.y, self.size, self.response = f32(x), f32(y), f32(size), f32(response)
        self.angle, self.octave = f32(-1), 0
        self.seq = -1    # position in vToDistributeKeys (bookkeeping of the model, not a member of cv::KeyPoint)

    def copy(self):
        k = KeyPoint(self.x, self.y, self.size, self.response)
        k.angle, k.octave, k.seq = self.angle, self.octave, self.seq
        return k


class ExtractorNode:
    _created = 0
    divided = []   # (width, height, points) of every node DivideNode was called on: trace only

    def __init__(self):
        self.UL = self.UR = self.BL = self.BR = (0, 0)
        self.vKeys = []
        self.bNoMore = False
        ExtractorNode._created += 1
        self.address = ExtractorNode._created   # stands for the heap address: a later node is the larger pointer

    def DivideNode(self, n1, n2, n3, n4, variant=None):   # :481-537
        half = math.floor if variant == "floor_halves" else math.ceil
        ExtractorNode.divided.append((self.UR[0] - self.UL[0], self.BR[1] - self.UL[1], len(self.vKeys)))
        halfX = int(half(f32(f32(self.UR[0] - self.UL[0]) / f32(2))))
        halfY = int(half(f32(f32(self.BR[1] - self.UL[1]) / f32(2))))
        n1.UL = self.UL
        n1.UR = (self.UL[0] + halfX, self.UL[1])
        n1.BL = (self.UL[0], self.UL[1] + halfY)
        n1.BR = (self.UL[0] + halfX, self.UL[1] + halfY)
        n2.UL = n1.UR
        n2.UR = self.UR
        n2.BL = n1.BR
        n2.BR = (self.UR[0], self.UL[1] + halfY)
        n3.UL = n1.BL
        n3.UR = n1.BR
        n3.BL = self.BL
        n3.BR = (n1.BR[0], self.BL[1])
        n4.UL = n3.UR
        n4.UR = n2.BR
        n4.BL = n3.BR
        n4.BR = self.BR
        less = (lambda a, b: a <= b) if variant == "split_le" else (lambda a, b: a < b)
        for kp in self.vKeys:
            if less(kp.x, f32(n1.UR[0])):
                if less(kp.y, f32(n1.BR[1])):
                    n1.vKeys.append(kp)
                else:
                    n3.vKeys.append(kp)
            elif less(kp.y, f32(n1.BR[1])):
                n2.vKeys.append(kp)
            else:
                n4.vKeys.append(kp)
        for n in (n1, n2, n3, n4):
            if len(n.vKeys) == 1:
                n.bNoMore = True


def c_round(v):
    """C round(): half away from zero."""
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


class Extractor:
    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, variant=None):   # :410-470
        assert variant is None or variant in VARIANTS or variant in INSEPARABLE, variant
        self.variant = variant
        self.nfeatures, self.scaleFactor, self.nlevels = int(nfeatures), f32(scaleFactor), int(nlevels)
        self.iniThFAST, self.minThFAST = int(iniThFAST), int(minThFAST)
        self.mvScaleFactor = [f32(1.0)] * nlevels
        self.mvLevelSigma2 = [f32(1.0)] * nlevels
        for i in range(1, nlevels):
            self.mvScaleFactor[i] = f32(self.mvScaleFactor[i - 1] * self.scaleFactor)
            self.mvLevelSigma2[i] = f32(self.mvScaleFactor[i] * self.mvScaleFactor[i])
        self.mvInvScaleFactor = [f32(f32(1.0) / s) for s in self.mvScaleFactor]
        self.mvInvLevelSigma2 = [f32(f32(1.0) / s) for s in self.mvLevelSigma2]
        self.mnFeaturesPerLevel = [0] * nlevels
        factor = f32(f32(1.0) / self.scaleFactor)
        nDesired = f32(f32(f32(self.nfeatures) * f32(f32(1) - factor)) / f32(f32(1) - f32(math.pow(float(factor), float(nlevels)))))
        sumFeatures = 0
        for level in range(nlevels - 1):
            self.mnFeaturesPerLevel[level] = cv_round(nDesired)
            sumFeatures += self.mnFeaturesPerLevel[level]
            nDesired = f32(nDesired * factor)
        self.mnFeaturesPerLevel[nlevels - 1] = max(self.nfeatures - sumFeatures, 0)
        self.pattern = pattern()
        umax = [0] * (HALF_PATCH_SIZE + 2)
        vmax = int(math.floor(f32(f32(f32(HALF_PATCH_SIZE) * np.sqrt(f32(2))) / f32(2)) + f32(1)))
        vmin = int(math.ceil(f32(f32(f32(HALF_PATCH_SIZE) * np.sqrt(f32(2))) / f32(2))))
        hp2 = float(HALF_PATCH_SIZE * HALF_PATCH_SIZE)
        for v in range(vmax + 1):
            umax[v] = cv_round(math.sqrt(hp2 - v * v))
        v0 = 0
        for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
            while umax[v0] == umax[v0 + 1]:
                v0 += 1
            umax[v] = v0
            v0 += 1
        self.umax = umax[:HALF_PATCH_SIZE + 1]
        self.trace = []

    # ---- :539-763 ----
    def DistributeOctTree(self, vToDistributeKeys, minX, maxX, minY, maxY, N, level, tr):
        V = self.variant
        ratio = f32(f32(maxX - minX) / f32(maxY - minY))
        if V == "nini_floor":
            nIni = int(ratio)
        elif V == "nini_half_even":
            nIni = cv_round(ratio)
        else:
            nIni = c_round(ratio)
        tr["nIni"] = nIni
        ExtractorNode.divided = tr["divided"] = []
        tr["rounds"] = []
        tr["exit"] = None
        tr["best_pos"] = []
        if nIni < 1:
            return []    # undefined in the reference (module docstring)
        hX = f32(f32(maxX - minX) / f32(nIni))
        lNodes = []
        vpIniNodes = []
        bound = (lambda v: cv_round(v)) if V == "bounds_rounded" else (lambda v: int(v))
        for i in range(nIni):
            ni = ExtractorNode()
            ni.UL = (bound(f32(hX * f32(i))), 0)
            ni.UR = (bound(f32(hX * f32(i + 1))), 0)
            ni.BL = (ni.UL[0], maxY - minY)
            ni.BR = (ni.UR[0], maxY - minY)
            lNodes.append(ni)
            vpIniNodes.append(ni)
        for kp in vToDistributeKeys:
            vpIniNodes[int(f32(kp.x / hX))].vKeys.append(kp)
        i = 0
        while i < len(lNodes):
            if len(lNodes[i].vKeys) == 1:
                lNodes[i].bNoMore = True
                i += 1
            elif not lNodes[i].vKeys:
                del lNodes[i]
            else:
                i += 1
        tr["ini_sizes"] = [len(n.vKeys) for n in vpIniNodes]
        at_least = (lambda s: s > N) if V == "finish_gt_n" else (lambda s: s >= N)
        bFinish = False
        vSizeAndPointerToNode = []

        def add_children(children):
            """:621-660 / :691-726: push_front each child that holds points; remember the expandable ones."""
            n_exp = 0
            for n in children:
                if len(n.vKeys) > 0:
                    lNodes.insert(0, n)
                    if len(n.vKeys) > 1:
                        n_exp += 1
                        vSizeAndPointerToNode.append((len(n.vKeys), n))
            return n_exp

        guard = 0
        while not bFinish:
            guard += 1
            if guard > 200:
                tr["exit"] = "guard"
                break
            prevSize = len(lNodes)
            nToExpand = 0
            vSizeAndPointerToNode.clear()
            i = 0
            while i < len(lNodes):
                lit = lNodes[i]
                if lit.bNoMore:
                    i += 1
                    continue
                ch = [ExtractorNode() for _ in range(4)]
                lit.DivideNode(*ch, variant=V)
                before = len(lNodes)
                nToExpand += add_children(ch)
                i += len(lNodes) - before     # the children went in front of `lit`
                del lNodes[i]                 # lit = lNodes.erase(lit)
            tr["rounds"].append(dict(phase="full", size=len(lNodes), nToExpand=nToExpand))
            if at_least(len(lNodes)) or len(lNodes) == prevSize:
                bFinish = True
                tr["exit"] = "size>=N" if at_least(len(lNodes)) else "size==prevSize"
            elif (len(lNodes) + nToExpand * 3 >= N) if V == "expand_ge_n" else (len(lNodes) + nToExpand * 3 > N):
                while not bFinish:
                    guard += 1
                    if guard > 200:
                        tr["exit"] = "guard"
                        bFinish = True
                        break
                    prevSize = len(lNodes)
                    vPrev = list(vSizeAndPointerToNode)
                    vSizeAndPointerToNode.clear()
                    if V == "sort_tie_oldest_first":
                        vPrev.sort(key=lambda sp: (sp[0], -sp[1].address))
                    else:
                        vPrev.sort(key=lambda sp: (sp[0], sp[1].address))
                    n_split, broke = 0, False
                    for j in range(len(vPrev) - 1, -1, -1):
                        node = vPrev[j][1]
                        ch = [ExtractorNode() for _ in range(4)]
                        node.DivideNode(*ch, variant=V)
                        add_children(ch)
                        for q, n in enumerate(lNodes):
                            if n is node:
                                del lNodes[q]
                                break
                        n_split += 1
                        if at_least(len(lNodes)) and V != "no_break":
                            broke = True
                            break
                    tr["rounds"].append(dict(phase="sorted", size=len(lNodes), expandable=len(vPrev), split=n_split, broke=broke,
                                             top_sizes=[s for s, _ in vPrev[::-1][:8]]))
                    if at_least(len(lNodes)) or len(lNodes) == prevSize:
                        bFinish = True
                        tr["exit"] = "size>=N" if at_least(len(lNodes)) else "size==prevSize"
        # :741-760 retain the best point in each node
        vResultKeys = []
        for lit in lNodes:
            vNodeKeys = lit.vKeys
            pKP = vNodeKeys[0]
            maxResponse = pKP.response
            pos = 0
            for k in range(1, len(vNodeKeys)):
                r = vNodeKeys[k].response
                if V == "best_ge":
                    better = r >= maxResponse
                elif V == "best_tie_raster":
                    better = r > maxResponse or (r == maxResponse and (vNodeKeys[k].y, vNodeKeys[k].x) < (pKP.y, pKP.x))
                else:
                    better = r > maxResponse
                if better:
                    pKP = vNodeKeys[k]
                    maxResponse = r
                    pos = k
            ties = sum(1 for kp in vNodeKeys if kp.response == maxResponse)
            tr["best_pos"].append((pos, len(vNodeKeys), ties))
            vResultKeys.append(pKP.copy())
        return vResultKeys

    # ---- :765-848 ----
    def ComputeKeyPointsOctTree(self, pyramid):
        V = self.variant
        allKeypoints = [[] for _ in range(self.nlevels)]
        self.candidates = [[] for _ in range(self.nlevels)]
        W = f32(30)
        for level in range(self.nlevels):
            img = pyramid[level]
            rows, cols = img.shape
            tr = dict(level=level, cells_skipped=0, cells_redone=0, cells=0)
            self.trace.append(tr)
            minBorderX = EDGE_THRESHOLD - 3
            minBorderY = minBorderX
            maxBorderX = cols - EDGE_THRESHOLD + 3
            maxBorderY = rows - EDGE_THRESHOLD + 3
            vToDistributeKeys = []
            width = f32(maxBorderX - minBorderX)
            height = f32(maxBorderY - minBorderY)
            nCols = int(f32(width / W))
            nRows = int(f32(height / W))
            tr["grid"] = (nCols, nRows)
            if nCols < 1 or nRows < 1:
                # width / nCols divides by zero in the reference (:786); no cell, no candidate, and DistributeOctTree is
                # given an empty vector
                nCols = nRows = 0
                wCell = hCell = 0
            else:
                wCell = int(math.ceil(f32(width / f32(nCols))))
                hCell = int(math.ceil(f32(height / f32(nRows))))
            tr["cell"] = (wCell, hCell)
            for i in range(nRows):
                iniY = f32(minBorderY + i * hCell)
                maxY = f32(iniY + f32(hCell + 6))
                if iniY >= maxBorderY - (6 if V == "row_continue_6" else 3):
                    tr["cells_skipped"] += nCols
                    continue
                if maxY > maxBorderY:
                    maxY = f32(maxBorderY)
                for j in range(nCols):
                    iniX = f32(minBorderX + j * wCell)
                    maxX = f32(iniX + f32(wCell + 6))
                    if iniX >= maxBorderX - (3 if V == "col_continue_3" else 6):
                        tr["cells_skipped"] += 1
                        continue
                    if maxX > maxBorderX:
                        maxX = f32(maxBorderX)
                    tr["cells"] += 1
                    sub = img[int(iniY):int(maxY), int(iniX):int(maxX)]
                    vKeysCell = fast_cell(sub, self.iniThFAST)
                    if V == "fast_merged":
                        have = set((x, y) for x, y, _ in vKeysCell)
                        vKeysCell = vKeysCell + [k for k in fast_cell(sub, self.minThFAST) if (k[0], k[1]) not in have]
                    elif (len(vKeysCell) < 2) if V == "second_fast_below_count" else (not vKeysCell):
                        tr["cells_redone"] += 1
                        vKeysCell = fast_cell(sub, self.minThFAST)
                    for (x, y, s) in vKeysCell:
                        kp = KeyPoint(f32(x), f32(y), 7, s)
                        kp.x = f32(kp.x + f32(j * wCell))
                        kp.y = f32(kp.y + f32(i * hCell))
                        kp.seq = len(vToDistributeKeys)
                        vToDistributeKeys.append(kp)
            self.candidates[level] = [(int(k.x) + minBorderX, int(k.y) + minBorderY, int(k.response)) for k in vToDistributeKeys]
            tr["candidates"] = len(vToDistributeKeys)
            if maxBorderY - minBorderY <= 0 or maxBorderX - minBorderX <= 0:
                tr.update(nIni=0, rounds=[], exit=None, best_pos=[])
                keypoints = []
            else:
                keypoints = self.DistributeOctTree(vToDistributeKeys, minBorderX, maxBorderX, minBorderY, maxBorderY,
                                                   self.mnFeaturesPerLevel[level], level, tr)
            tr["N"] = self.mnFeaturesPerLevel[level]
            tr["keypoints"] = len(keypoints)
            scaledPatchSize = int(f32(f32(PATCH_SIZE) * self.mvScaleFactor[level]))
            for kp in keypoints:
                kp.x = f32(kp.x + f32(minBorderX))
                kp.y = f32(kp.y + f32(minBorderY))
                kp.octave = level
                kp.size = f32(scaledPatchSize)
            allKeypoints[level] = keypoints
        for level in range(self.nlevels):
            for kp in allKeypoints[level]:
                kp.angle = self.IC_Angle(pyramid[level], kp.x, kp.y)
        return allKeypoints

    # ---- :77-104 ----
    def IC_Angle(self, image, ptx, pty):
        """m_10 = sum u * I, m_01 = sum v * I over the rows v = -15..15 of the circular patch, |u| <= umax[|v|]; the
        reference pairs the rows +v and -v, which is the same integer sum."""
        cy, cx = cv_round(pty), cv_round(ptx)
        R = HALF_PATCH_SIZE
        patch = image[cy - R:cy + R + 1, cx - R:cx + R + 1].astype(np.int64)
        assert patch.shape == (2 * R + 1, 2 * R + 1)
        v, u = np.mgrid[-R:R + 1, -R:R + 1]
        inside = np.abs(u) <= np.array(self.umax)[np.abs(v)]
        m_10 = int((u * patch * inside).sum())
        m_01 = int((v * patch * inside).sum())
        return fast_atan2(f32(m_01), f32(m_10))

    # ---- :107-147 ----
    def computeOrbDescriptor(self, kpt, img):
        factorPI = f32(math.pi / float(f32(180.0)))
        angle = f32(f32(kpt.angle) * factorPI)
        a, b = cos_sin(angle)
        cy, cx = cv_round(kpt.y), cv_round(kpt.x)
        # GET_VALUE(idx) for the 512 pattern points at once: every product and sum is a float32 operation of its own
        px, py = self.pattern[:, 0].astype(f32), self.pattern[:, 1].astype(f32)
        r = np.rint((px * b + py * a).astype(np.float64)).astype(np.int64)
        c = np.rint((px * a - py * b).astype(np.float64)).astype(np.int64)
        val = img[cy + r, cx + c].astype(np.int32)
        assert (cy + r).min() >= 0 and (cx + c).min() >= 0
        bits = (val[0::2] < val[1::2]).astype(np.uint8).reshape(32, 8)
        return (bits << np.arange(8, dtype=np.uint8)).sum(axis=1).astype(np.uint8)

    # ---- :1043-1105; ComputePyramid and GaussianBlur are the caller's ----
    def __call__(self, pyramid, blurred):
        """pyramid[level]: mvImagePyramid[level] (the level without its border; every read stays inside it).
        blurred[level]: the same after GaussianBlur, or None where the side under test has none.
        Returns (key points, descriptors [n, 32]) in output order."""
        allKeypoints = self.ComputeKeyPointsOctTree(pyramid)
        _keypoints, descriptors = [], []
        for level in range(self.nlevels):
            keypoints = allKeypoints[level]
            if len(keypoints) == 0:
                continue
            workingMat = blurred[level]
            for kp in keypoints:
                descriptors.append(self.computeOrbDescriptor(kp, workingMat))
            if level != 0 and self.variant != "scale_missing":
                scale = self.mvScaleFactor[level]
                for kp in keypoints:
                    kp.x = f32(kp.x * scale)
                    kp.y = f32(kp.y * scale)
            _keypoints.extend(keypoints)
        desc = np.stack(descriptors) if descriptors else np.zeros((0, 32), np.uint8)
        return _keypoints, desc


def extract(params, pyramid, blurred, variant=None):
    """params: anything with nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast.  Returns a dict:
    kps (structured array x, y, size, angle, response, octave), desc, candidates (per level, [(x, y, response)] in
    vToDistributeKeys order, level coordinates), trace (per level), tables."""
    e = Extractor(params.nfeatures, params.scale_factor, params.nlevels, params.ini_th_fast, params.min_th_fast, variant)
    kps, desc = e(pyramid, blurred)
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
    out = np.zeros(len(kps), dt)
    for i, k in enumerate(kps):
        out[i] = (k.x, k.y, k.size, k.angle, k.response, k.octave)
    return dict(kps=out, desc=desc, candidates=[np.array(c, np.int32).reshape(-1, 3) for c in e.candidates], trace=e.trace,
                features_per_level=list(e.mnFeaturesPerLevel), umax=list(e.umax), scale_factor=list(e.mvScaleFactor))


def levels_needed(params, pyramid):
    """Which levels can hold a key point at all (a blurred copy is asked for only there)."""
    return [l for l in range(params.nlevels) if min(pyramid[l].shape) >= 2 * EDGE_THRESHOLD]
