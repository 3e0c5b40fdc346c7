"""Discard outliers -> SearchLocalPoints on the CPU oracle's granular steps against the literal model of
tests/track_local_ref.py (Tracking.cc:1358-1376, :1222-1241, :1947-1997): a point the first stage dropped carries
mnLastFrameSeen == mCurrentFrame.mnId and is neither re-projected, nor counted in nToMatch, nor re-matched in that frame.
Everything compared is an integer and must be equal.  The scenario and what it contains: tests/track_local_cases.py."""
import numpy as np

import track_local_cases as TC
import track_local_ref as R

_VIEWS = {}


def _views(gate_min=0, two_stages=False):
    key = (gate_min, two_stages)
    if key not in _VIEWS:
        _VIEWS[key] = TC.run_oracle(TC.scenario(), gate_min=gate_min, two_stages=two_stages)
    return _VIEWS[key]


def test_scenario_holds_every_kind_and_discriminates():
    sc = TC.scenario()
    views = _views()
    for b in range(TC.B):
        kd, out, mp = sc["kinds"][b], views["pose"]["outlier"][b], views["pose"]["map_point"][b]
        nmap = int(sc["M"]["n"][b])
        listed = set(sc["lm"][0][b, : sc["lm"][1][b]].tolist())
        for s, X, t in kd["a"]:   # stage 1 flagged it, it is listed
            assert out[s] == 1 and mp[s] == X and X in listed, (b, "a", s, X)
        for s, X, t in kd["b"]:
            assert out[s] == 1 and mp[s] == X and X not in listed, (b, "b", s, X)
        for s, t, X in kd["c"]:
            assert out[s] == 0 and out[t] == 1 and mp[s] == X and mp[t] == X, (b, "c", s, t, X)
        for s, X in kd["d"] + kd["e0"] + kd["e1"]:
            assert out[s] == 0 and mp[s] == X and X in listed, (b, "d/e", s, X)
        assert all(sc["M_after"]["bad"][b, X] and not sc["M"]["bad"][b, X] for _, X in kd["d"])
        assert all(sc["M"]["obs_pos"][b, X] == 0 for _, X in kd["e0"]) and all(sc["M"]["obs_pos"][b, X] == 1 for _, X in kd["e1"])
        assert any(x < 0 for x in kd["g"]) and any(x == nmap for x in kd["g"]) and any(x > nmap for x in kd["g"])
        held = set(mp[mp >= 0].tolist())
        assert len(listed - held - set(kd["g"])) > 50   # (f)
    print("one stage:", TC.check_discriminates(sc, views))
    print("two stages:", TC.check_discriminates(sc, _views(two_stages=True), two_stages=True))


def test_oracle_steps_against_the_model():
    sc, views = TC.scenario(), _views()
    for b in range(TC.B):
        e = TC.expected(sc, views, b)
        TC.compare(views, e, b, "discard", "oracle")
        TC.compare(views, e, b, "local", "oracle")


def test_marked_points_never_come_back():
    sc = TC.scenario()
    for two in (False, True):
        views = _views(two_stages=two)
        for b in range(TC.B):
            e = TC.expected(sc, views, b, two_stages=two)
            N = int(views["local"]["n"][b])
            held = set(views["local"]["map_point"][b, :N].tolist())
            # (c): the point's other slot still holds it -- the mark only keeps it out of the search
            kept = {X for _, _, X in sc["kinds"][b]["c"]}
            assert e["marked"] and not (e["marked"] - kept) & held, (two, b, sorted((e["marked"] - kept) & held))
            assert kept <= held and kept <= e["marked"]


def test_marks_of_two_discards_in_one_frame_both_count():
    """The slots of (a) are filled again and dropped again with other points: both generations stay out of the search."""
    sc, views = TC.scenario(), _views(two_stages=True)
    for b in range(TC.B):
        e = TC.expected(sc, views, b, two_stages=True)
        first, again = {X for _, X, _ in sc["kinds"][b]["a"]}, {Y for _, Y in sc["second"][b]}
        assert first <= e["marked"] and again <= e["marked"], (b, first, again, e["marked"])
        for stage in ("discard", "discard2", "local"):
            TC.compare(views, e, b, stage, "oracle, two stages")


def test_gated_discard_leaves_no_marks():
    """`if (nmatches < 20) return false` in front of the loop (here every sequence: no matcher ran, the counter reads 0): nothing
    is dropped and nothing is marked, so the flagged points are still held when SearchLocalPoints runs."""
    sc, views = TC.scenario(), _views(gate_min=20)
    for b in range(TC.B):
        e = TC.expected(sc, views, b, gate_min=20)
        assert not e["marked"]
        N = int(views["pose"]["n"][b])
        assert np.array_equal(views["discard"]["map_point"][b, :N], views["pose"]["map_point"][b, :N])
        assert np.array_equal(views["discard"]["outlier"][b, :N], views["pose"]["outlier"][b, :N])
        TC.compare(views, e, b, "discard", "oracle, gated")
        TC.compare(views, e, b, "local", "oracle, gated")


# ---- drives: the oracle composite, each discard loop a call of its own, against the model ---------------------------------------
def _check_drive(drive, sc, tag, loops):
    figures = []
    for k, fr in enumerate(drive):
        for b in range(TC.B):
            e = TC.model_drive_frame(sc, fr["stages"], b)
            for loop in loops:
                TC.compare(fr["stages"], e, b, loop + "_discard", "%s, frame %d" % (tag, k + 1))
            got = {n: int(fr["view"]["counts"][TC.CNT[n], b]) for n in ("TO_MATCH", "LOCAL_MATCHES")}
            assert got == {n: e[n] for n in got}, (tag, k + 1, b, got, e["TO_MATCH"], e["LOCAL_MATCHES"])
            figures.append((k + 1, b, e))
    return figures


def test_drive_points_the_first_stage_drops_stay_out():
    """Two tracked frames (TrackWithMotionModel + TrackLocalMap) on a map with 8 listed points per sequence moved 10 px: M3
    (th = 15) matches them in frame 1, the pose optimisation flags them, the loop marks them, SearchLocalPoints skips them."""
    sc = TC.fused_scenario()
    drive = TC.run_oracle_drive(sc)
    figures = _check_drive(drive, sc, "drive", ("motion",))
    for b in range(TC.B):
        k, _, e = [f for f in figures if f[1] == b][0]          # frame 1
        naive = TC.model_drive_frame(sc, drive[0]["stages"], b, marks="none")
        assert e["TO_MATCH"] < naive["TO_MATCH"], (b, e["TO_MATCH"], naive["TO_MATCH"])
        hit = set(sc["moved"][b]) & e["marked"]["motion"]
        print("sequence", b, "moved ids marked in frame 1:", len(hit), "of", len(sc["moved"][b]), "nToMatch", e["TO_MATCH"], "without marks", naive["TO_MATCH"])
        # the edits matter: moved points are among the dropped ones, a search without marks would take them up again, this one does not
        assert hit and hit <= naive["candidates"] and not hit & e["candidates"], (b, hit)


def test_fall_back_frame_marks_of_both_stages_count():
    """Tracking.cc:531-540: TrackWithMotionModel, then TrackReferenceKeyFrame, then TrackLocalMap in one frame.  Sequence 0's
    motion-model stage fails after its discard loop in frame 1 (a yaw error in the odometry increment); the marks of that loop
    and of the reference stage's loop both keep their points out of SearchLocalPoints."""
    sc = TC.fused_scenario()
    drive = TC.run_oracle_drive(sc, TC.FALLBACK_MODES, TC.FALLBACK_YAW)
    c = drive[0]["stages"]["motion_discard"]["counts"]
    assert c[TC.CNT["PROJ_MATCHES"], 0] >= 20 and c[TC.CNT["MATCHES_MAP"], 0] < 10, c[:5, 0]      # the loop ran, the stage failed
    c = drive[0]["stages"]["reference_discard"]["counts"]
    assert c[TC.CNT["BOW_MATCHES"], 0] >= 15 and c[TC.CNT["MATCHES_MAP"], 0] >= 10, c[:13, 0]     # the fall-back succeeded
    for k, b, e in _check_drive(drive, sc, "fall-back", ("motion", "reference")):
        assert e["marked"]["motion"] and e["marked"]["reference"], (k, b)
        for only in ("none", "motion", "reference"):
            other = TC.model_drive_frame(sc, drive[k - 1]["stages"], b, marks=only)
            assert e["TO_MATCH"] < other["TO_MATCH"], (k, b, only, e["TO_MATCH"], other["TO_MATCH"])
        assert not (e["marked"]["motion"] | e["marked"]["reference"]) & e["candidates"]
    # taking the loops apart changes nothing: the composite calls give the same frames
    whole = TC.run_oracle_composite(sc, TC.FALLBACK_MODES, TC.FALLBACK_YAW)
    for fr, v in zip(drive, whole):
        for name in ("map_point", "outlier", "map_point_bird", "Tcw", "counts"):
            assert np.array_equal(fr["view"][name], v[name]), name


# ---- the model itself on five points ---------------------------------------------------------------------------------
def _five(bad=(0, 0, 0, 0, 0), obs=(1, 1, 0, 1, 1)):
    return R.make_points(bad, obs, 5)


def test_model_discard_marks_and_counts():
    pts = _five()
    #             slot: 0  1  2  3   4  5
    mp, out = [0, 1, 2, -1, 3, -1], [0, 1, 0, 1, 1, 0]     # slot 3 is flagged but holds nothing
    mp2, out2, nm, nmm = R.discard_outliers(pts, mp, out, 6, frame_id=7, nmatches=4)
    assert mp2 == [0, -1, 2, -1, -1, -1] and out2 == [0, 0, 0, 1, 0, 0]
    assert nm == 2 and nmm == 1                            # point 2 has no observations
    assert R.marked_ids(pts, 7) == {1, 3} and R.marked_ids(pts, 8) == set()
    mp3, cand = R.search_local_points(pts, mp2, 6, [4, 3, 9, 1, -1, 0, 2], frame_id=7)
    assert mp3 == mp2 and cand == [(0, 4)]                 # 3 and 1 marked, 0 and 2 held, 9 and -1 name nothing
    assert R.blocked_slots(pts, mp3) == [1, 0, 0, 0, 0, 0]


def test_model_only_the_first_n_slots_and_the_gate():
    pts = _five()
    mp, out = [0, 1, 2], [1, 1, 1]
    mp2, out2, nm, nmm = R.discard_outliers(pts, mp, out, 2, frame_id=1, nmatches=2)
    assert mp2 == [-1, -1, 2] and out2 == [0, 0, 1] and nm == 0 and R.marked_ids(pts, 1) == {0, 1}
    pts = _five()
    mp2, out2, nm, nmm = R.discard_outliers(pts, mp, out, 3, frame_id=1, nmatches=2, gate_min=15)
    assert mp2 == mp and out2 == out and nm == 2 and nmm == 0 and not R.marked_ids(pts, 1)


def test_model_second_discard_adds_marks_and_new_frame_forgets():
    pts = _five()
    R.discard_outliers(pts, [0, -1], [1, 0], 2, frame_id=3, nmatches=1)
    R.discard_outliers(pts, [4, 2], [1, 0], 2, frame_id=3, nmatches=2)     # the same slot, another point
    assert R.marked_ids(pts, 3) == {0, 4}
    mp, cand = R.search_local_points(pts, [-1, 2], 2, None, frame_id=3)
    assert cand == [(1, 1), (3, 3)]
    mp, cand = R.search_local_points(pts, [-1, 2], 2, None, frame_id=4)   # the next frame: the marks are stale
    assert cand == [(0, 0), (1, 1), (3, 3), (4, 4)]


def test_model_bad_points_and_duplicates():
    pts = _five(bad=(0, 0, 0, 1, 0))
    # point 3 is bad and held: dropped from the frame, not marked, skipped as bad; point 0 held twice, one slot flagged
    mp, out, nm, nmm = R.discard_outliers(pts, [0, 0, 3], [0, 1, 0], 3, frame_id=2, nmatches=3)
    assert mp == [0, -1, 3] and nm == 2 and nmm == 2
    mp, cand = R.search_local_points(pts, mp, 3, [3, 0, 1], frame_id=2)
    assert mp == [0, -1, -1] and cand == [(2, 1)] and pts[3].mnLastFrameSeen != 2
    naive = _five(bad=(0, 0, 0, 1, 0))
    R.discard_outliers(naive, [1, 0], [1, 0], 2, frame_id=2, nmatches=2, mark=False)
    assert not R.marked_ids(naive, 2)
    assert R.search_local_points(naive, [-1, 0], 2, [3, 0, 1], frame_id=2)[1] == [(2, 1)]
