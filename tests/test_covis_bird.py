"""The bird-map model (tests/bird_map_ref.py) against answers derived by hand, and the branch coverage of the generators the
GPU test uses (tests/bird_map_cases.py): asserted here, without a GPU, so the GPU test cannot pass by never reaching a branch."""
import numpy as np
import pytest

import bird_map_cases as CS
import bird_map_ref as R


def _tables(K, BS, holds, edges, bad=()):
    """holds: {kf: [point per feature]}, edges: [(point, kf, idx)]"""
    n_mpb = 1 + max([p for row in holds.values() for p in row if p >= 0] + [e[0] for e in edges])
    kf_nb = np.zeros(K, np.int32)
    kf_mpb = np.full((K, BS), -1, np.int32)
    for kf, row in holds.items():
        kf_nb[kf] = len(row)
        kf_mpb[kf, :len(row)] = row
    mpb_bad = np.zeros(n_mpb, np.uint8)
    mpb_bad[list(bad)] = 1
    e = np.asarray(edges, np.int32).reshape(-1, 3)
    return R.BirdTables(kf_nb, kf_mpb, mpb_bad, e[:, 0], e[:, 1], e[:, 2])


def _auto_edges(holds):
    seen, edges = set(), []
    for kf, row in holds.items():
        for i, p in enumerate(row):
            if p >= 0 and (p, kf) not in seen:
                seen.add((p, kf))
                edges.append((p, kf, i))
    return edges


def test_three_keyframes_by_eye():
    # kf0 holds points 0 1 2 3, kf1 holds 0 1 2, kf2 holds 2 3 and the bad point 4 (which kf0 holds too)
    holds = {0: [0, 1, 2, 3, 4], 1: [0, 1, 2], 2: [2, 3, 4]}
    T = _tables(3, 8, holds, _auto_edges(holds), bad=[4])
    g = R.BirdGraph(3, [30, 10, 20])
    nc, fr = g.run_batch(T, [0, 1, 2], None, 1, id0_slot=0)
    # kf0: {kf1: 3, kf2: 2} -> [kf1, kf2]; kf1: {kf0: 3, kf2: 1} -> [kf0]; kf2: {kf0: 2, kf1: 1} -> [kf0]
    assert nc == [2, 2, 2] and fr == [1, 0, 0]
    assert g.bird_connected == [[1, 2], [0], [0]] and g.bird_weights == [[3, 2], [3], [2]]
    assert g.parent == [-1, 0, 0] and g.first == [True, False, False] and g.linked() == [0, 1, 1]   # kf0 is mnId 0: the return at :516
    assert g.counters["id0_return"] == 1 and g.errors == 0


def test_point_held_twice_counts_twice():
    holds = {0: [5, -1, 5], 1: [5]}
    T = _tables(2, 4, holds, _auto_edges(holds))
    g = R.BirdGraph(2, [1, 2])
    nc, fr = g.run_batch(T, [0, 1], None, 1)
    assert g.bird_connected[0] == [1] and g.bird_weights[0] == [2]      # one shared point, walked at two features
    assert g.bird_connected[1] == [] and nc == [1, 1] and fr == [1, -1]  # kf1 walks it once: weight 1 < th, and no pKFmax fallback
    assert g.counters["list_empty_after_threshold"] == 1
    assert g.parent == [1, -1]                                           # state 1: kf1 stays without a parent


def test_weight_tie_descending_kf_order():
    holds = {0: [0, 1, 2, 3, 4, 5], 1: [0, 1], 2: [2, 3], 3: [4, 5]}
    T = _tables(4, 8, holds, _auto_edges(holds))
    g = R.BirdGraph(4, [5, 70, 90, 80])
    g.run_batch(T, [0], None, 1)
    assert g.bird_connected[0] == [2, 3, 1] and g.bird_weights[0] == [2, 2, 2]   # sort ascending by (w, pKF), then push_front
    assert g.parent[0] == 2


def test_empty_counter_and_the_search():
    holds = {0: [], 1: [0, 1], 2: [0, 1], 3: [0, 1]}
    T = _tables(4, 4, holds, _auto_edges(holds))
    fid, in_map = [9, 4, 7, 7], [1, 1, 1, 1]
    g = R.BirdGraph(4, [40, 30, 20, 10])
    assert g.run_batch(T, [0], [0], 1, -1, fid, in_map) == ([0], [-1]) and g.parent[0] == -1    # does not act
    assert g.run_batch(T, [0], [0], 3, -1, fid, in_map) == ([0], [-1])
    assert g.parent[0] == 3 and g.first[0] is False and 0 in g.children[3]   # id 7 twice: the smaller kf_order (slot 3) wins
    g = R.BirdGraph(4, [40, 30, 20, 10])
    g.run_batch(T, [0], None, 4, -1, [4, 4, 7, 0], in_map)                   # nothing strictly between 0 and 4
    assert g.parent[0] == -1 and g.errors == 1 and g.counters["search_finds_nothing"] == 1
    g = R.BirdGraph(4, [40, 30, 20, 10], parent=[2, -1, -1, -1], linked=[1, 0, 0, 0], first=[1, 1, 1, 1])
    g.run_batch(T, [0], None, 4, -1, fid, in_map)                            # a parent is there: :449 does not search
    assert g.parent[0] == 2 and g.first[0] is True and g.counters["search_taken"] == 0


def _one_member(ow_other, n_points=12):
    holds = {0: list(range(n_points)), 1: list(range(100, 100 + n_points))}
    T = _tables(2, 16, holds, [])
    ow = np.array([ow_other, [0.0, 0.0, 0.0]], np.float32)
    m = R.LocalBirdMap()
    m.add_keyframe(T, ow, 0)
    m.add_keyframe(T, ow, 1)
    return m


def test_distance_exactly_five_is_kept_one_float_step_further_is_not():
    m = _one_member([3.0, 4.0, 0.0])
    assert R.distance([3.0, 4.0, 0.0], [0, 0, 0]) == 5.0
    assert m.local_kf == [1, 0] and len(m.local_mpb) == 24 and m.counters["far_member"] == 0
    far = [3.0, float(np.nextafter(np.float32(4.0), np.float32(5.0))), 0.0]
    assert R.distance(far, [0, 0, 0]) > 5.0
    m = _one_member(far)
    assert m.local_kf == [1] and m.local_mpb == list(range(100, 112)) and m.counters["far_member"] == 1


def test_near_member_with_nine_new_points_is_dropped_but_its_points_stay():
    holds = {0: list(range(12)), 1: list(range(3, 21))}     # kf0 holds 0..11, kf1 holds 3..20
    T = _tables(2, 24, holds, [])
    ow = np.zeros((2, 3), np.float32)
    m = R.LocalBirdMap()
    m.add_keyframe(T, ow, 1)
    m.add_keyframe(T, ow, 0)       # list [0, 1]: kf0 is the first holder of 12 points, kf1 of the 9 points 12..20 only
    assert m.local_kf == [0] and m.local_mpb == list(range(21))
    assert m.counters["member_dropped_below_10"] == 1 and m.counters["point_only_from_dropped_member"] == 9


def test_local_points_follow_the_set_order():
    holds = {0: list(range(10))}
    T = _tables(1, 16, holds, [])
    order = [50, 40, 90, 10, 20, 80, 70, 60, 30, 0]
    m = R.LocalBirdMap(order)
    m.add_keyframe(T, np.zeros((1, 3), np.float32), 0)
    assert m.local_mpb == [9, 3, 4, 8, 1, 0, 7, 6, 5, 2]


def test_camera_centre_is_minus_Rt_t():
    a = 0.7
    Rcw = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    c = np.array([1.5, -2.0, 0.25])
    T = np.zeros((3, 4)); T[:, :3] = Rcw; T[:, 3] = -Rcw @ c
    assert np.allclose(R.camera_centre(T.astype(np.float32).reshape(12)), c, atol=1e-6)


UPDATE_CASES = {"a": dict(seed=11, K=12, used=list(range(12)), n_points=150),
                "b": dict(seed=12, K=4096, used=[0, 4095] + list(range(100, 4000, 103))[:38], n_points=300),
                "c": dict(seed=13, K=300, used=list(range(300)), n_points=700, n_global=4, obs=(2, 5))}


@pytest.mark.parametrize("name", sorted(UPDATE_CASES))
def test_update_generator_reaches_every_branch(name):
    p = CS.make_bird_problem(**UPDATE_CASES[name])
    T = CS.tables_of(p)
    total = {}
    for state in (1, 3, 4):
        g = CS.graph_of(p)
        g.run_batch(T, p["used"], CS.front_counter(p, p["used"]), state, p["id0"], p["frame_id"], p["in_map"])
        for k, v in g.counters.items():
            total[k] = total.get(k, 0) + v
        if state == 1:
            assert g.counters["search_taken"] == 0
    for k in ("empty_counter", "search_taken", "search_finds_nothing", "list_empty_after_threshold", "id0_return"):
        assert total.get(k, 0) > 0, k
    g = CS.graph_of(p)
    g.run_batch(T, p["used"], None, 3, p["id0"], p["frame_id"], p["in_map"])
    sp = p["special"]
    assert g.bird_weights[sp["twin"]] == [2] and g.bird_connected[sp["thin"]] == []
    assert g.parent[sp["orphan"]] == -1 and g.parent[sp["lone"]] >= 0 and g.parent[sp["id0"]] == -1
    replaced = [s for s in p["used"] if p["parent"][s] >= 0 and p["first"][s] and g.parent[s] != p["parent"][s]]
    assert replaced, "a parent that is replaced while mbFirstConnection is still set"
    ties = [a for a in p["used"] if len(set(g.bird_weights[a])) < len(g.bird_weights[a])]
    assert ties, "weight ties"
    if name == "a":
        assert 120 <= T.n_mpb <= 200 and 400 <= len(p["bobs_kf"]) <= 750
    if name == "c":
        assert max(len(l) for l in g.bird_connected) > 256
    if name == "b":
        assert g.bird_connected[0] and g.bird_connected[4095]


def test_local_generator_reaches_every_branch():
    p = CS.make_local_problem(21)
    m, out = CS.run_local_model(p, p["mpb_order"])
    for k in ("far_member", "member_dropped_below_10", "point_only_from_dropped_member"):
        assert m.counters[k] > 0, k
    sizes = [len(kfs) for kfs, _ in out]
    assert max(sizes) >= 4 and any(b < a for a, b in zip(sizes, sizes[1:]))
    first = p["slots"][0]
    assert first in out[2][0] and first not in out[len(out) // 2 - 2][0], "the path leaves the ball of its start"
    assert any(len(pts) > 40 for _, pts in out)
    held_bad = [pt for _, pts in out for pt in pts if p["mpb_bad"][pt]]
    assert held_bad, "bad points are listed: :117 has no isBad test"


def test_out_of_range_injection_counts():
    p = CS.make_bird_problem(**UPDATE_CASES["a"])
    dirty, clean, n = CS.inject_out_of_range(p)
    assert n == 10
    g1, g2 = CS.graph_of(p), CS.graph_of(clean)
    g1.run_batch(CS.tables_of(p), p["used"], None, 1)
    g2.run_batch(CS.tables_of(clean), p["used"], None, 1)
    assert g1.bird_connected == g2.bird_connected     # the clean copy is the original map again
