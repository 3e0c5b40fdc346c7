"""Literal model of the per-frame matchers, written from the reference alone (src/ORBmatcher.cc, src/Frame.cc,
src/Converter.cc), one statement per reference statement, in plain Python.  It does not look at the oracle or at the
kernels: where the three agree, two independent readings of the reference agree.

  M2  SearchByProjection(F, vpMapPoints, th)            ORBmatcher.cc:46-130, RadiusByViewingCos :132-138
  M3  SearchByProjection(CurrentFrame, LastFrame, th)   ORBmatcher.cc:1329-1471 (bMono = true)
  M5  SearchByBoW(KeyFrame, Frame)                      ORBmatcher.cc:160-289
  M6  SearchByBoW(KeyFrame, KeyFrame)                   ORBmatcher.cc:523-656
  M8  BirdviewMatch, isProject = 0                      ORBmatcher.cc:1602-1760
  M9  BirdMapPointMatch                                 ORBmatcher.cc:1763-1902
      ComputeThreeMaxima                                ORBmatcher.cc:1905-1946
      GetFeaturesInArea / ..Birdview, PosInGrid         Frame.cc:493-626

Arithmetic: what the reference computes in `float` is computed in np.float32 scalars, one rounding per operation; what it
promotes to `double` (a float compared with a double literal, `1.0/z`, the Frame statics that are `double`) is computed in
Python floats.  Products of cv::Mat_<float> accumulate in double and round once per element (OpenCV's gemm for CV_32F).

`variant` names ONE decision that is restated differently (VARIANTS); None is the reference.  The variants exist only so
that tests/matcher_edge_cases.py can show that each constructed case bites: they are the mistakes a restatement makes.

Things the model shows and does not "fix":
  * factor = 1.0f/HISTO_LENGTH, so bin = round(rot/30): only bins 0..12 of the 30 are ever filled;
  * GetFeaturesInAreaBirdview walks ix < nMaxCellX, iy < nMaxCellY (exclusive), GetFeaturesInArea walks inclusive;
  * BirdviewMatch pushes to the rotation histogram even when the ratio test failed, and emits DMatches and
    BirdMapPointMatch confirms inliers for vnMatches12[i] > 0 only (current index 0 never counts);
  * BirdMapPointMatch builds no rotation histogram at all: mbCheckOrientation changes nothing there.

Decisions without a variant, because no input separates the two readings:
  * pt.x<0 / pt.y<0 at :1807 against <=0: BaseXY2BirdPixel is birdviewCols/2 - p.y*meter2pixel in double, rounded to float;
    it is 0.0f only if the double is (all but) exactly 0, and no float p.y (p.x) within 2000 steps of 32/25.1 gives that;
  * a tie for the best distance in M5, M6, M8, M9 with nnratio < 1: best == second, so the ratio test fails whoever won.
    The tie cases therefore pass nnratio = 1.5, which the entry points accept, and there the winner shows.
"""
import math

import numpy as np

F = np.float32
TH_HIGH = 100        # ORBmatcher.cc:38
TH_LOW = 50          # :39
HISTO_LENGTH = 30    # :40
INT_MAX = 2 ** 31 - 1

VARIANTS = (
    "th_high_strict",        # bestDist<=TH_HIGH          -> <            (:119, :1427)
    "th_low_strict",         # bestDist<=TH_LOW           -> <            (:229, :1702, :1850)
    "th_low_m6_inclusive",   # bestDist1<TH_LOW           -> <=           (:599)
    "ratio_inclusive",       # the ratio comparison gains / loses its `=`  (:121, :231, :601, :1704, :1852)
    "ratio_ignores_level",   # bestLevel==bestLevel2 &&   dropped         (:121)
    "ratio_in_double",       # mfNNratio*bestDist2 kept in double instead of rounded to float
    "bin_floor",             # round(rot*factor)          -> floor
    "bin_half_down",         # round(): halves away from zero -> halves towards zero
    "neg_rot_no_wrap",       # if(rot<0.0) rot+=360.0f    dropped
    "maxima_in_double",      # 0.1f*(float)max1 kept in double instead of rounded to float (:1937, :1942)
    "maxima_tie_last",       # s>max1                     -> >=           (:1914)
    "maxima_tie_last2",      # s>max2                     -> >=           (:1923)
    "maxima_tie_last3",      # s>max3                     -> >=           (:1930)
    "radius_inclusive",      # fabs(distx)<r && fabs(disty)<r -> <=       (Frame.cc:539, :619)
    "bounds_inclusive",      # pt.x>=birdviewCols, pt.y>=birdviewRows -> > (:1807)
    "bounds_exclusive",      # u<mnMinX || u>mnMaxX, v<mnMinY || v>mnMaxY -> <=, >= (:1374-1377), one rule: the bound is in
    "level_window_wide",     # the level window of the call site one level wider at each open end
    "tie_last_wins",         # dist<bestDist              -> <=           (:103, :217, :587, :1420, :1690, :1838)
    "viewcos_in_float",      # viewCos>0.998 (double literal) -> compared as float (:134)
    "bird_cells_inclusive",  # ix < nMaxCellX, iy < nMaxCellY -> <=  (Frame.cc:595, :597)
)


def _is(variant, name):
    assert variant is None or variant in VARIANTS, variant
    return variant == name


# ---- small pieces ----------------------------------------------------------------------------------------------------
def descriptor_distance(a, b):
    """:1951-1967 counts the bits of a ^ b over 8 words."""
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def c_round(x):
    """C round(): halves away from zero.  x is a float promoted to double."""
    x = float(x)
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def _to_int(x):
    """(int) of a double that came from floor/ceil."""
    return int(x)


def rot_bin(angle1, angle2, variant=None):
    """:239-244 (the same five lines at :608-613, :1434-1439, :1714-1719)."""
    factor = F(F(1.0) / F(HISTO_LENGTH))              # const float factor = 1.0f/HISTO_LENGTH
    rot = F(F(angle1) - F(angle2))                    # float rot = kp.angle-F.mvKeys[bestIdxF].angle
    if float(rot) < 0.0 and not _is(variant, "neg_rot_no_wrap"):   # if(rot<0.0)
        rot = F(rot + F(360.0))                       # rot+=360.0f
    x = F(rot * factor)                               # rot*factor is a float
    if _is(variant, "bin_floor"):
        b = int(math.floor(float(x)))
    elif _is(variant, "bin_half_down"):
        b = int(math.copysign(math.ceil(abs(float(x)) - 0.5), float(x)))
    else:
        b = c_round(x)                                # int bin = round(rot*factor)
    if b == HISTO_LENGTH:                             # if(bin==HISTO_LENGTH) bin=0
        b = 0
    if variant is None:
        assert 0 <= b < HISTO_LENGTH                  # assert(bin>=0 && bin<HISTO_LENGTH)
    return b % HISTO_LENGTH


def three_maxima(sizes, variant=None):
    """ComputeThreeMaxima :1905-1946 on the bin sizes -> (ind1, ind2, ind3)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i in range(len(sizes)):
        s = int(sizes[i])
        if s > max1 or (_is(variant, "maxima_tie_last") and s == max1):       # :1914
            max3 = max2; max2 = max1; max1 = s
            ind3 = ind2; ind2 = ind1; ind1 = i
        elif s > max2 or (_is(variant, "maxima_tie_last2") and s == max2):    # :1923
            max3 = max2; max2 = s
            ind3 = ind2; ind2 = i
        elif s > max3 or (_is(variant, "maxima_tie_last3") and s == max3):    # :1930
            max3 = s
            ind3 = i
    if _is(variant, "maxima_in_double"):
        lim = float(F(0.1)) * float(max1)
    else:
        lim = float(F(F(0.1) * F(max1)))              # 0.1f*(float)max1; the int on the left converts to float (exact here)
    if float(F(max2)) < lim:                          # :1937
        ind2 = -1
        ind3 = -1
    elif float(F(max3)) < lim:                        # :1942
        ind3 = -1
    return ind1, ind2, ind3


def _hist():
    return [[] for _ in range(HISTO_LENGTH)]


def _kept_bins(hist, variant):
    return three_maxima([len(h) for h in hist], variant)


# ---- grids (Frame.cc:381-411, :493-626) ---------------------------------------------------------------------------------
def build_grid(kps, geom):
    """AssignFeaturesToGrid with PosInGrid / PosInGridBirdview: mGrid[posX][posY] in key-point order."""
    grid = {}
    for i in range(len(kps)):
        px = c_round(F(F(F(kps["x"][i]) - F(geom["min_x"])) * F(geom["inv_w"])))      # :550 / :562
        py = c_round(F(F(F(kps["y"][i]) - F(geom["min_y"])) * F(geom["inv_h"])))      # :551 / :563
        if px < 0 or px >= geom["cols"] or py < 0 or py >= geom["rows"]:              # :554 / :566
            continue
        grid.setdefault((px, py), []).append(i)
    return grid


def features_in_area(kps, grid, geom, x, y, r, min_level=-1, max_level=-1, bird=False, variant=None):
    """GetFeaturesInArea :493-546 (bird=False) / GetFeaturesInAreaBirdview :572-626 (bird=True; its min is 0)."""
    x, y, r = F(x), F(y), F(r)
    out = []
    mx, my, iw, ih = F(geom["min_x"]), F(geom["min_y"]), F(geom["inv_w"]), F(geom["inv_h"])
    cols, rows = geom["cols"], geom["rows"]
    lo_x = max(0, _to_int(math.floor(float(F(F(F(x - mx) - r) * iw)))))               # :498 / :577
    if lo_x >= cols:
        return out
    hi_x = min(cols - 1, _to_int(math.ceil(float(F(F(F(x - mx) + r) * iw)))))         # :502 / :581
    if hi_x < 0:
        return out
    lo_y = max(0, _to_int(math.floor(float(F(F(F(y - my) - r) * ih)))))               # :506 / :585
    if lo_y >= rows:
        return out
    hi_y = min(rows - 1, _to_int(math.ceil(float(F(F(F(y - my) + r) * ih)))))         # :510 / :589
    if hi_y < 0:
        return out
    check_levels = (min_level > 0) or (max_level >= 0)                                # :514 / :593
    exclusive = bird and not _is(variant, "bird_cells_inclusive")
    end_x, end_y = (hi_x, hi_y) if exclusive else (hi_x + 1, hi_y + 1)                # :595,:597 `<`; :516,:518 `<=`
    for ix in range(lo_x, end_x):
        for iy in range(lo_y, end_y):
            for j in grid.get((ix, iy), ()):
                if check_levels:
                    if kps["octave"][j] < min_level:
                        continue
                    if max_level >= 0:
                        if kps["octave"][j] > max_level:
                            continue
                dx = F(F(kps["x"][j]) - x)
                dy = F(F(kps["y"][j]) - y)
                if _is(variant, "radius_inclusive"):
                    ok = abs(dx) <= r and abs(dy) <= r
                else:
                    ok = abs(dx) < r and abs(dy) < r                                  # :539 / :619
                if ok:
                    out.append(j)
    return out


def _matmul_f32(A, B):
    """cv::Mat_<float> product: double accumulation, one rounding per element."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    return (A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)


def _transform(R, t, X):
    """R*X+t as two cv::Mat expressions: the product rounds to float, then the float sum."""
    return (_matmul_f32(R, np.asarray(X, np.float32).reshape(3, 1)).reshape(3) + np.asarray(t, np.float32)).astype(np.float32)


# ---- M2 ------------------------------------------------------------------------------------------------------------
def radius_by_viewing_cos(view_cos, variant=None):
    if _is(variant, "viewcos_in_float"):
        big = F(view_cos) > F(0.998)
    else:
        big = float(F(view_cos)) > 0.998          # :134 the float is promoted to the double literal
    return F(2.5) if big else F(4.0)


def search_by_projection_points(p, geom, scale_factors, th=1.0, nnratio=0.8, variant=None):
    """M2 :46-130 -> dict(match_cur_to_mp, nmatches)."""
    kps, n_cur = p["cur_kps"], len(p["cur_kps"])
    grid = build_grid(kps, geom)
    holder = [None] * n_cur                               # F.mvpMapPoints: None, "entry" (held on entry), or an iMP
    held_obs = [bool(x) for x in p["cur_blocked"]]        # ...->Observations()>0 of what the slot holds
    nmatches = 0
    b_factor = float(F(th)) != 1.0                        # :50
    for i in range(len(p["mp_desc"])):
        if not p["mp_track"][i]:                          # :55-59
            continue
        lvl = int(p["mp_level"][i])                       # :61
        r = radius_by_viewing_cos(p["mp_view_cos"][i], variant)   # :64
        if b_factor:
            r = F(r * F(th))                              # :67
        hi = lvl + 1 if _is(variant, "level_window_wide") else lvl
        cand = features_in_area(kps, grid, geom, p["mp_proj"][i][0], p["mp_proj"][i][1], F(r * F(scale_factors[lvl])),
                                lvl - 1, hi, variant=variant)     # :70
        if not cand:
            continue
        best, best_lvl, best2, best_lvl2, best_idx = 256, -1, 256, -1, -1
        for j in cand:
            if held_obs[j]:                               # :88-90
                continue
            d = descriptor_distance(p["mp_desc"][i], p["cur_desc"][j])
            if d < best or (_is(variant, "tie_last_wins") and d == best):     # :103
                best2 = best; best = d
                best_lvl2 = best_lvl; best_lvl = int(kps["octave"][j])
                best_idx = j
            elif d < best2:                               # :111
                best_lvl2 = int(kps["octave"][j]); best2 = d
        if best < TH_HIGH or (best == TH_HIGH and not _is(variant, "th_high_strict")):   # :119
            if _is(variant, "ratio_in_double"):
                lim = float(F(nnratio)) * best2
            else:
                lim = float(F(F(nnratio) * F(best2)))     # mfNNratio*bestDist2: float * int -> float
            over = float(F(best)) >= lim if _is(variant, "ratio_inclusive") else float(F(best)) > lim
            same = True if _is(variant, "ratio_ignores_level") else best_lvl == best_lvl2
            if same and over:                             # :121
                continue
            holder[best_idx] = i                          # :124
            held_obs[best_idx] = bool(p["mp_obs_pos"][i])
            nmatches += 1
    m = np.array([-1 if h is None else h for h in holder], np.int32).reshape(n_cur)
    return dict(match_cur_to_mp=m, nmatches=nmatches)


# ---- M3 ------------------------------------------------------------------------------------------------------------
def search_by_projection_frame(p, geom, scale_factors, th=15.0, check_ori=1, variant=None):
    """M3 :1329-1471 with bMono = true -> dict(match_cur_to_last, nmatches, hist, kept)."""
    kps, n_cur = p["cur_kps"], len(p["cur_kps"])
    grid = build_grid(kps, geom)
    hist = _hist()
    T = np.asarray(p["Tcw"], np.float32).reshape(3, 4)
    Rcw, tcw = T[:, :3], T[:, 3]
    fx, fy, cx, cy = F(p["fx"]), F(p["fy"]), F(p["cx"]), F(p["cy"])
    min_x, min_y, max_x, max_y = F(0.0), F(0.0), F(p["w"]), F(p["h"])
    holder = [None] * n_cur
    held_obs = [bool(x) for x in p["cur_blocked"]]
    nmatches = 0
    for i in range(len(p["last_xw"])):
        if not p["last_valid"][i]:                        # :1356-1358
            continue
        xc3 = _transform(Rcw, tcw, p["last_xw"][i])       # :1362
        xc, yc = F(xc3[0]), F(xc3[1])
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            invzc = F(np.float64(1.0) / np.float64(xc3[2]))   # :1366 const float invzc = 1.0/z
            if invzc < 0:                                 # :1368
                continue
            u = F(F(F(fx * xc) * invzc) + cx)             # :1371
            v = F(F(F(fy * yc) * invzc) + cy)             # :1372
        if _is(variant, "bounds_exclusive"):
            if u <= min_x or u >= max_x or v <= min_y or v >= max_y:
                continue
        else:
            if u < min_x or u > max_x:                    # :1374
                continue
            if v < min_y or v > max_y:                    # :1376
                continue
        assert not (np.isnan(u) or np.isnan(v)), "a NaN projection reaches (int)floor(NaN): undefined in the reference"
        octv = int(p["last_octave"][i])                   # :1379
        radius = F(F(th) * F(scale_factors[octv]))        # :1382
        w = 2 if _is(variant, "level_window_wide") else 1
        cand = features_in_area(kps, grid, geom, u, v, radius, octv - w, octv + w, variant=variant)   # :1391
        if not cand:
            continue
        best, best_idx = 256, -1
        for j in cand:
            if held_obs[j]:                               # :1404-1406
                continue
            d = descriptor_distance(p["last_desc"][i], p["cur_desc"][j])
            if d < best or (_is(variant, "tie_last_wins") and d == best):    # :1420
                best = d
                best_idx = j
        if best < TH_HIGH or (best == TH_HIGH and not _is(variant, "th_high_strict")):    # :1427
            holder[best_idx] = i                          # :1429
            held_obs[best_idx] = bool(p["last_obs_pos"][i])
            nmatches += 1
            if check_ori:
                hist[rot_bin(p["last_angle"][i], kps["angle"][best_idx], variant)].append(best_idx)   # :1434-1441
    kept = None
    if check_ori:
        kept = _kept_bins(hist, variant)                  # :1455
        for b in range(HISTO_LENGTH):
            if b not in kept:                             # :1459
                for j in hist[b]:
                    holder[j] = None                      # :1463
                    nmatches -= 1
    m = np.array([-1 if h is None else h for h in holder], np.int32).reshape(n_cur)
    return dict(match_cur_to_last=m, nmatches=nmatches, hist=[len(h) for h in hist], kept=kept)


# ---- M5 / M6 -----------------------------------------------------------------------------------------------------------
def _walk_feature_vectors(fv1, fv2):
    """The merge of two DBoW2::FeatureVector maps (:181-265): yields the item lists of every shared node id, ascending."""
    ids1, st1, it1 = fv1
    ids2, st2, it2 = fv2
    a = b = 0
    while a < len(ids1) and b < len(ids2):
        if ids1[a] == ids2[b]:
            yield it1[st1[a]:st1[a + 1]], it2[st2[b]:st2[b + 1]]
            a += 1
            b += 1
        elif ids1[a] < ids2[b]:
            while a < len(ids1) and ids1[a] < ids2[b]:    # lower_bound
                a += 1
        else:
            while b < len(ids2) and ids2[b] < ids1[a]:
                b += 1


def _ratio_passes_float(best1, best2, nnratio, variant):
    """static_cast<float>(bestDist1)<mfNNratio*static_cast<float>(bestDist2)  (:231, :601)."""
    if _is(variant, "ratio_in_double"):
        lim = float(F(nnratio)) * float(best2)
    else:
        lim = float(F(F(nnratio) * F(best2)))
    return float(F(best1)) <= lim if _is(variant, "ratio_inclusive") else float(F(best1)) < lim


def search_by_bow(p, kf_fv, f_fv, nnratio=0.7, check_ori=1, variant=None):
    """M5 :160-289 -> dict(match_f_to_kf, nmatches, hist, kept)."""
    n_f = len(p["f_kps"])
    slot = [None] * n_f                                   # vpMapPointMatches
    hist = _hist()
    nmatches = 0
    for items_kf, items_f in _walk_feature_vectors(kf_fv, f_fv):
        for ikf in items_kf:
            ikf = int(ikf)
            if not p["kf_has_mp"][ikf]:                   # :194-198
                continue
            best1, best_f, best2 = 256, -1, 256
            for jf in items_f:
                jf = int(jf)
                if slot[jf] is not None:                  # :210
                    continue
                d = descriptor_distance(p["kf_desc"][ikf], p["f_desc"][jf])
                if d < best1 or (_is(variant, "tie_last_wins") and d == best1):     # :217
                    best2 = best1; best1 = d; best_f = jf
                elif d < best2:
                    best2 = d
            if best1 < TH_LOW or (best1 == TH_LOW and not _is(variant, "th_low_strict")):     # :229
                if _ratio_passes_float(best1, best2, nnratio, variant):                       # :231
                    slot[best_f] = ikf
                    if check_ori:
                        hist[rot_bin(p["kf_kps"]["angle"][ikf], p["f_kps"]["angle"][best_f], variant)].append(best_f)
                    nmatches += 1
    kept = None
    if check_ori:
        kept = _kept_bins(hist, variant)
        for b in range(HISTO_LENGTH):
            if b in kept:                                 # :278
                continue
            for j in hist[b]:
                slot[j] = None
                nmatches -= 1
    m = np.array([-1 if h is None else h for h in slot], np.int32).reshape(n_f)
    return dict(match_f_to_kf=m, nmatches=nmatches, hist=[len(h) for h in hist], kept=kept)


def search_by_bow_kf(p, fv1, fv2, nnratio=0.75, check_ori=1, variant=None):
    """M6 :523-656 -> dict(matches12, nmatches, hist, kept)."""
    n1, n2 = len(p["kps1"]), len(p["kps2"])
    m12 = [None] * n1                                     # vpMatches12
    matched2 = [False] * n2                               # vbMatched2
    hist = _hist()
    nmatches = 0
    for items1, items2 in _walk_feature_vectors(fv1, fv2):
        for i1 in items1:
            i1 = int(i1)
            if not p["has_mp1"][i1]:                      # :560-563
                continue
            best1, best_idx2, best2 = 256, -1, 256
            for i2 in items2:
                i2 = int(i2)
                if matched2[i2] or not p["has_mp2"][i2]:  # :577-581
                    continue
                d = descriptor_distance(p["desc1"][i1], p["desc2"][i2])
                if d < best1 or (_is(variant, "tie_last_wins") and d == best1):     # :587
                    best2 = best1; best1 = d; best_idx2 = i2
                elif d < best2:
                    best2 = d
            if best1 < TH_LOW or (best1 == TH_LOW and _is(variant, "th_low_m6_inclusive")):   # :599 strict
                if _ratio_passes_float(best1, best2, nnratio, variant):                       # :601
                    m12[i1] = best_idx2
                    matched2[best_idx2] = True
                    if check_ori:
                        hist[rot_bin(p["kps1"]["angle"][i1], p["kps2"]["angle"][best_idx2], variant)].append(i1)
                    nmatches += 1
    kept = None
    if check_ori:
        kept = _kept_bins(hist, variant)
        for b in range(HISTO_LENGTH):
            if b in kept:
                continue
            for i1 in hist[b]:
                m12[i1] = None
                nmatches -= 1
    m = np.array([-1 if h is None else h for h in m12], np.int32).reshape(n1)
    return dict(matches12=m, nmatches=nmatches, hist=[len(h) for h in hist], kept=kept)


# ---- M8 / M9 -----------------------------------------------------------------------------------------------------------
def _bird_ratio_passes(best, best2, nnratio, variant):
    """bestDist<(float)bestDist2*mfNNratio (:1704, :1852): the int on the left converts to float."""
    if _is(variant, "ratio_in_double"):
        lim = float(F(best2)) * float(F(nnratio))
    else:
        lim = float(F(F(best2) * F(nnratio)))
    return float(F(best)) <= lim if _is(variant, "ratio_inclusive") else float(F(best)) < lim


def birdview_match(p, geom, window=10, nnratio=0.9, check_ori=1, variant=None):
    """M8 :1602-1760, isProject = 0 -> dict(match_ref_to_cur, match_dist, nmatches, n_dmatches, hist, kept)."""
    cur, ref = p["cur_kps"], p["ref_kps"]
    grid = build_grid(cur, geom)
    hist = _hist()
    m21 = [-1] * len(cur)
    m12 = [-1] * len(ref)
    dist12 = [INT_MAX] * len(ref)
    nmatches = 0
    for i1 in range(len(ref)):
        level1 = int(ref["octave"][i1])                   # :1632
        if level1 > 0:                                    # :1658
            continue
        hi = level1 + 1 if _is(variant, "level_window_wide") else level1
        cand = features_in_area(cur, grid, geom, ref["x"][i1], ref["y"][i1], F(window), level1, hi, bird=True,
                                variant=variant)          # :1661
        if not cand:
            continue
        best, best2, best_idx = INT_MAX, INT_MAX, -1
        for j in cand:
            d = descriptor_distance(p["ref_desc"][i1], p["cur_desc"][j])
            if d < best or (_is(variant, "tie_last_wins") and d == best):    # :1690
                best2 = best; best = d; best_idx = j
            elif d < best2:
                best2 = d
        if best < TH_LOW or (best == TH_LOW and not _is(variant, "th_low_strict")):      # :1702
            if _bird_ratio_passes(best, best2, nnratio, variant):                         # :1704
                m21[best_idx] = i1
                m12[i1] = best_idx
                dist12[i1] = best
                nmatches += 1
            if check_ori:                                 # :1712 outside the ratio test
                hist[rot_bin(ref["angle"][i1], cur["angle"][best_idx], variant)].append(i1)
    kept = None
    if check_ori:
        kept = _kept_bins(hist, variant)
        for b in range(HISTO_LENGTH):
            if b in kept:
                continue
            for idx1 in hist[b]:
                if m12[idx1] >= 0:                        # :1742
                    m21[m12[idx1]] = -1
                    m12[idx1] = -1
                    nmatches -= 1
    n_dm = sum(1 for x in m12 if x > 0)                   # :1755 `> 0`
    return dict(match_ref_to_cur=np.array(m12, np.int32).reshape(len(ref)), match_dist=np.array(dist12, np.int64).reshape(len(ref)),
                nmatches=nmatches, n_dmatches=n_dm, hist=[len(h) for h in hist], kept=kept)


def bird_mappoint_match(p, geom, window=10, filter_size=0.05, nnratio=0.9, meter2pixel=25.1, rear_axle_to_center=1.393,
                        prefill=-1, variant=None):
    """M9 :1763-1902 -> dict(match_cur_to_ref, ninliers)."""
    cur = p["cur_kps"]
    grid = build_grid(cur, geom)
    n_ref = len(p["ref_xw"])
    m21 = [-1] * len(cur)
    m12 = [-1] * n_ref
    Tcw = np.vstack([np.asarray(p["Tcw"], np.float32).reshape(3, 4), np.array([[0, 0, 0, 1]], np.float32)])
    Tbc = np.vstack([np.asarray(p["Tbc"], np.float32)[:3, :4], np.array([[0, 0, 0, 1]], np.float32)])
    Tbw = _matmul_f32(Tbc, Tcw)                           # :1784
    cols, rows = int(p["cols"]), int(p["rows"])
    for i1 in range(n_ref):
        if not p["ref_valid"][i1]:                        # :1794
            continue
        lp = _transform(Tbw[:3, :3], Tbw[:3, 3], p["ref_xw"][i1])    # :1800
        if abs(float(lp[2])) > 0.2:                       # :1802 double literal
            continue
        ptx = F(cols // 2 - float(lp[1]) * meter2pixel)                            # Converter.cc:307 (double statics)
        pty = F(rows // 2 - (float(lp[0]) - rear_axle_to_center) * meter2pixel)    # Converter.cc:308
        if _is(variant, "bounds_inclusive"):
            out = ptx < 0 or ptx > cols or pty < 0 or pty > rows
        else:
            out = ptx < 0 or ptx >= cols or pty < 0 or pty >= rows                # :1807
        if out:
            continue
        cand = features_in_area(cur, grid, geom, ptx, pty, F(window), bird=True, variant=variant)   # :1810
        if not cand:
            continue
        best, best2, best_idx = INT_MAX, INT_MAX, -1
        for j in cand:
            d = descriptor_distance(p["ref_desc"][i1], p["cur_desc"][j])
            if d < best or (_is(variant, "tie_last_wins") and d == best):    # :1838
                best2 = best; best = d; best_idx = j
            elif d < best2:
                best2 = d
        if best < TH_LOW or (best == TH_LOW and not _is(variant, "th_low_strict")):      # :1850
            if _bird_ratio_passes(best, best2, nnratio, variant):                         # :1852
                m21[best_idx] = i1
                m12[i1] = best_idx
    out_m = [prefill] * len(cur)                          # CurF.mvpMapPointsBird as it came in
    inliers = 0
    R, t = Tcw[:3, :3], Tcw[:3, 3]
    for i1 in range(n_ref):
        if m12[i1] > 0:                                   # :1871 `> 0`
            pc = _transform(R, t, p["ref_xw"][i1])        # :1879
            diff = (pc - np.asarray(p["cur_cam_xyz"][m12[i1]], np.float32)).astype(np.float32)
            dis = math.sqrt(float((diff.astype(np.float64) ** 2).sum()))          # :1881 cv::norm, double
            if dis < float(F(filter_size)):               # :1889
                out_m[m12[i1]] = i1
                inliers += 1
    return dict(match_cur_to_ref=np.array(out_m, np.int32).reshape(len(cur)), ninliers=inliers)
