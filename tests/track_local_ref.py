"""A literal model of the map-point bookkeeping between the first tracking stage and SearchLocalPoints, written from the
reference (src/Tracking.cc) and from nothing else: the "Discard outliers" loops of TrackWithMotionModel (:1358-1376) and
TrackReferenceKeyFrame (:1222-1241), and the two loops of SearchLocalPoints (:1950-1984).  One Python object per MapPoint
with the reference's own members; plain loops, one statement per reference statement.

The model does the bookkeeping only.  Frame::isInFrustum and ORBmatcher::SearchByProjection are numeric and are pinned by
their own tests (orc_in_frustum, orc_match_projection_points); tests/track_local_cases.py composes them with this model.
"""


class MapPoint:
    """The members of MapPoint the two functions touch (MapPoint.h: mnLastFrameSeen, mbTrackInView, mbBad, nObs)."""

    def __init__(self, idx, bad, nObs):
        self.idx = idx
        self.bad = bool(bad)
        self.nObs = int(nObs)
        self.mnLastFrameSeen = -1   # no frame has this id
        self.mbTrackInView = False

    def isBad(self):
        return self.bad

    def Observations(self):
        return self.nObs


def make_points(bad, obs_pos, n):
    """The map of one sequence: MapPoint objects for the table rows 0 .. n-1 (obs_pos: Observations() > 0 as 0 / 1)."""
    return [MapPoint(i, bad[i], obs_pos[i]) for i in range(int(n))]


def refresh(points, bad, obs_pos):
    """The other threads changed the map (SetBadFlag, AddObservation): the members Tracking only reads."""
    for p in points:
        p.bad = bool(bad[p.idx])
        p.nObs = int(obs_pos[p.idx])


def discard_outliers(points, map_point, outlier, N, frame_id, nmatches, gate_min=0, mark=True):
    """Tracking.cc:1358-1376 == :1222-1241.  map_point[i] = table row or -1 (NULL), outlier[i] = mvbOutlier[i], N = the
    frame's key-point count, nmatches = the matcher's return value.  gate_min: `if (nmatches < gate_min) return false`
    in front of the optimisation (:1351 / :1212), i.e. the loop does not run.
    mark=False leaves out the two lines on pMP (the variant that forgets the marks; only for comparison).
    Returns (map_point, outlier, nmatches, nmatchesMap) as new lists / ints; the marks land on `points`."""
    mvpMapPoints = [points[int(i)] if int(i) >= 0 else None for i in map_point]
    mvbOutlier = [bool(o) for o in outlier]
    nmatchesMap = 0
    if not (gate_min > 0 and nmatches < gate_min):
        for i in range(N):
            if mvpMapPoints[i]:
                if mvbOutlier[i]:
                    pMP = mvpMapPoints[i]
                    mvpMapPoints[i] = None
                    mvbOutlier[i] = False
                    if mark:
                        pMP.mbTrackInView = False
                        pMP.mnLastFrameSeen = frame_id
                    nmatches -= 1
                elif mvpMapPoints[i].Observations() > 0:
                    nmatchesMap += 1
    return [p.idx if p else -1 for p in mvpMapPoints], [int(o) for o in mvbOutlier], nmatches, nmatchesMap


def marked_ids(points, frame_id):
    """The points whose mnLastFrameSeen is this frame's id."""
    return {p.idx for p in points if p.mnLastFrameSeen == frame_id}


def search_local_points(points, map_point, N, local, frame_id):
    """Tracking.cc:1950-1984 without the isInFrustum call itself.  local = mvpLocalMapPoints as table rows (None = the whole
    table in row order); an entry that names no row of the table is no entry of the reference's pointer list.
    Returns (map_point after the first loop, candidates) where candidates = [(position in local, row), ...] in list order:
    the entries that reach mCurrentFrame.isInFrustum(pMP, 0.5)."""
    mvpMapPoints = [points[int(i)] if int(i) >= 0 else None for i in map_point]
    for i in range(len(mvpMapPoints)):   # the iterator runs over the whole vector; slots >= N hold NULL
        pMP = mvpMapPoints[i]
        if pMP:
            if pMP.isBad():
                mvpMapPoints[i] = None
            else:
                pMP.mnLastFrameSeen = frame_id
                pMP.mbTrackInView = False
    rows = range(len(points)) if local is None else [int(x) for x in local]
    candidates = []
    for j, row in enumerate(rows):
        if row < 0 or row >= len(points):
            continue
        pMP = points[row]
        if pMP.mnLastFrameSeen == frame_id:
            continue
        if pMP.isBad():
            continue
        candidates.append((j, row))
    return [p.idx if p else -1 for p in mvpMapPoints], candidates


def blocked_slots(points, map_point):
    """What SearchByProjection(F, vpMapPoints, th) tests per key point before it takes it (ORBmatcher.cc:88-90):
    F.mvpMapPoints[idx] && F.mvpMapPoints[idx]->Observations() > 0."""
    return [1 if int(i) >= 0 and points[int(i)].Observations() > 0 else 0 for i in map_point]
