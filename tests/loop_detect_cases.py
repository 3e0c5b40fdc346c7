"""Constructed cases for the consistency groups, mvpLoopMapPoints and LoopConnections (tests/loop_detect_ref.py is the model,
tests/test_loop_detect.py checks the model against the answers written here, tests/test_loop_detect_gpu.py the device against
the model).  Every answer is known by construction and stated in the case's docstring.

A graph is set up by `ops`: ("add", a, b, w) = a->AddConnection(b, w) (every entry of a changed row becomes a member of its
ordered vector) and ("update", pre_map, [slots]) = UpdateConnections on a map (entries below 15 stay non-members).
"""
import numpy as np

import covis_ref as CR


def make_map(K, shared=(), rows=None, n_mp=None, bad=(), kf_order=None, S=None):
    """shared: ((a, b, n), ..): n points seen by key frames a and b each.  rows: {kf: [point or -1, ..]} explicit kf_mp rows,
    written behind the shared points; an edge is made for every row entry in [0, n_mp)."""
    held = {k: [] for k in range(K)}
    nxt = 0
    for a, b, n in shared:
        for _ in range(n):
            held[a].append(nxt); held[b].append(nxt)
            nxt += 1
    for kf, r in (rows or {}).items():
        held[kf].extend(r)
    n_mp = max([nxt] + [p + 1 for r in (rows or {}).values() for p in r if p < 90]) if n_mp is None else n_mp
    S = max([1] + [len(v) for v in held.values()]) if S is None else S
    kf_mp = np.full((K, S), -1, np.int32)
    kf_n = np.zeros(K, np.int32)
    obs = []
    for kf, v in held.items():
        kf_n[kf] = len(v)
        kf_mp[kf, :len(v)] = v
        obs += [(p, kf, i) for i, p in enumerate(v) if 0 <= p < n_mp]
    mp_bad = np.zeros(n_mp, np.uint8)
    mp_bad[list(bad)] = 1
    o = np.array(obs, np.int32).reshape(-1, 3)
    return dict(K=K, kf_n=kf_n, kf_mp=kf_mp, kf_octave=np.zeros((K, S), np.uint8), mp_bad=mp_bad, obs_mp=o[:, 0].copy(), obs_kf=o[:, 1].copy(),
                obs_idx=o[:, 2].copy(), kf_order=np.arange(K, dtype=np.uint64) + 100 if kf_order is None else np.asarray(kf_order, np.uint64))


def ref_map(c):
    return CR.Map(*[c[k] for k in ("kf_n", "kf_mp", "kf_octave", "mp_bad", "obs_mp", "obs_kf", "obs_idx", "kf_order")])


def model_graph(K, ops, kf_order=None):
    g = CR.Graph(K, kf_order)
    for op in ops:
        if op[0] == "add":
            g.add_connection(op[1], op[2], op[3])
        else:
            m = ref_map(op[1])
            for s in op[2]:
                g.update_connections(m, s)
    return g


def both(a, b, w):
    return [("add", a, b, w), ("add", b, a, w)]


# ---- consistency groups: dict(K, ops, calls=[(candidates, th), ..], expect=[(enough, [(slots, counter), ..]), ..]) ------------
def dl_no_previous():
    """No previous group: every candidate pushes its group with counter 0 and none is enough.  Rows: 0 <-> 1; 5 has none."""
    return dict(K=8, ops=both(0, 1, 20), calls=[([0, 5], 3)], expect=[([], [([0, 1], 0), ([5], 0)])])


def dl_zero_clears():
    """Zero candidates clear a non-empty state (:147-153)."""
    return dict(K=8, ops=both(0, 1, 20), calls=[([0], 3), ([], 3)], expect=[([], [([0, 1], 0)]), ([], [])])


def dl_two_candidates_one_group():
    """Candidates 2 and 3 (2 <-> 3) are both consistent with the one previous group {2, 3}: the first pushes, once; with
    th = 1 both are enough (0 + 1 >= 1)."""
    return dict(K=8, ops=both(2, 3, 20), calls=[([2], 1), ([2, 3], 1)], expect=[([], [([2, 3], 0)]), ([2, 3], [([2, 3], 1)])])


def dl_one_candidate_two_groups():
    """Candidate 2 (row {1, 5}) is consistent with both previous groups {0, 1} (counter 1) and {4, 5} (counter 0): its group
    is pushed twice, with counters 2 and 1, in the order of the groups."""
    ops = both(0, 1, 20) + both(4, 5, 20) + [("add", 2, 1, 16), ("add", 2, 5, 16)]
    return dict(K=8, ops=ops, calls=[([0], 3), ([0, 4], 3), ([2], 3)],
                expect=[([], [([0, 1], 0)]), ([], [([0, 1], 1), ([4, 5], 0)]), ([], [([1, 2, 5], 2), ([1, 2, 5], 1)])])


def dl_taken_group_still_enough():
    """The only previous group {2, 3} (counter 1) is taken by candidate 2; candidate 3 is consistent with nothing else: it
    pushes nothing, yet 1 + 1 >= 2 makes it enough."""
    return dict(K=8, ops=both(2, 3, 20), calls=[([2], 2), ([2], 2), ([2, 3], 2)],
                expect=[([], [([2, 3], 0)]), ([], [([2, 3], 1)]), ([2, 3], [([2, 3], 2)])])


def dl_through_candidate_itself():
    """Row 0 holds 6, row 6 is empty.  The previous group {0, 6} and the group {6} of candidate 6 share the candidate only."""
    return dict(K=8, ops=[("add", 0, 6, 5)], calls=[([0], 3), ([6], 3)], expect=[([], [([0, 6], 0)]), ([], [([6], 1)])])


def dl_through_non_member_entry():
    """UpdateConnections(0) on a map where 0 shares 16 points with 1 and 2 with key frame 2: row 0 = {1: 16 (member), 2: 2
    (below 15: an entry, not a member)}, row 2 stays empty.  The previous group {2} and the group {0, 1, 2} of candidate 0
    share slot 2 only."""
    pre = make_map(8, shared=((0, 1, 16), (0, 2, 2)))
    return dict(K=8, ops=[("update", pre, [0])], calls=[([2], 3), ([0], 3)], expect=[([], [([2], 0)]), ([], [([0, 1, 2], 1)])])


def dl_k70(s):
    """K = 70 (three words, the last partly used; two ballots of 64).  Rows 0 and 1 both hold slot s and nothing else: the
    groups {0, s} and {1, s} share s only.  s = 31, 32, 63, 64, 69: either side of a word and of a ballot, and the last slot."""
    return dict(K=70, ops=[("add", 0, s, 3), ("add", 1, s, 3)], calls=[([0], 3), ([1], 3)],
                expect=[([], [([0, s], 0)]), ([], [([1, s], 1)])])


def dl_four_calls():
    """The same candidate four times with th = 3: counters 0, 1, 2, 3; enough only on the fourth call (2 + 1 >= 3)."""
    return dict(K=8, ops=both(2, 3, 20), calls=[([2], 3)] * 4,
                expect=[([], [([2, 3], 0)]), ([], [([2, 3], 1)]), ([], [([2, 3], 2)]), ([2], [([2, 3], 3)])])


def dl_cap_too_small():
    """cap_groups = 2 and three disjoint candidates: overflow, the first two groups are kept.  The next call works on those."""
    return dict(K=8, ops=[], cap_groups=2, calls=[([0, 4, 6], 3), ([4], 3)], overflow=[1, 0],
                expect=[([], [([0], 0), ([4], 0)]), ([], [([4], 1)])])


def dl_candidate_out_of_range():
    """Candidates 9 and -1 of K = 8 are skipped and counted; 0 and 4 are handled as usual."""
    return dict(K=8, ops=[], calls=[([0, 9, -1, 4], 3)], errors=2, expect=[([], [([0], 0), ([4], 0)])])


def detect_cases():
    cs = [dl_no_previous, dl_zero_clears, dl_two_candidates_one_group, dl_one_candidate_two_groups, dl_taken_group_still_enough,
          dl_through_candidate_itself, dl_through_non_member_entry, dl_four_calls, dl_cap_too_small, dl_candidate_out_of_range]
    out = [(f.__name__, f()) for f in cs]
    return out + [("dl_k70_%d" % s, dl_k70(s)) for s in (31, 32, 63, 64, 69)]


# ---- mvpLoopMapPoints: dict(map, ops, matched, expect, errors) --------------------------------------------------------------
LP_OPS = [("add", 0, 2, 30), ("add", 0, 1, 20)]   # GetVectorCovisibleKeyFrames(0) = [2, 1]


def lp_first_holder_wins():
    """The list is [2, 1, 0].  Point 11 is held by 2 and 1, point 12 by 2 and 0: both are taken at key frame 2."""
    return dict(map=make_map(8, rows={2: [12, 11], 1: [10, 11], 0: [12, 13]}), ops=LP_OPS, matched=0, expect=[12, 11, 10, 13])


def lp_bad_point():
    """Point 11 is bad: left out."""
    return dict(map=make_map(8, rows={2: [12, 11], 1: [10, 11], 0: [12, 13]}, bad=[11]), ops=LP_OPS, matched=0, expect=[12, 10, 13])


def lp_null_feature():
    """Feature 1 of key frame 2 holds no point."""
    return dict(map=make_map(8, rows={2: [12, -1, 11], 1: [10, 11], 0: [12, 13]}), ops=LP_OPS, matched=0, expect=[12, 11, 10, 13])


def lp_entry_out_of_range():
    """kf_mp[1][1] = 99 >= n_mp = 14: skipped and counted."""
    return dict(map=make_map(8, rows={2: [12, 11], 1: [10, 99], 0: [12, 13]}), ops=LP_OPS, matched=0, expect=[12, 11, 10, 13], errors=1)


def lp_empty_ordered_vector():
    """The matched key frame has no ordered vector: only its own points."""
    return dict(map=make_map(8, rows={2: [12, 11], 1: [10, 11], 0: [12, 13]}), ops=[], matched=0, expect=[12, 13])


def points_cases():
    cs = [lp_first_holder_wins, lp_bad_point, lp_null_feature, lp_entry_out_of_range, lp_empty_ordered_vector]
    return [(f.__name__, f()) for f in cs]


# ---- LoopConnections: dict(map, ops, set, expect rows, n_counter, front[, naive rows]) --------------------------------------
def lc_new_link_outside():
    """0 <-> 1 before; the fused map adds 16 points shared by 0 and 5.  Member 1: {0} minus its neighbour 0: empty.  Member
    0: {1, 5} minus its neighbour 1: {5}."""
    return dict(map=make_map(8, shared=((0, 1, 20), (0, 5, 16))), ops=both(0, 1, 20), set=[1, 0], expect=[[], [5]],
                n_counter=[1, 2], front=[0, 1])


def lc_previous_neighbour_excluded():
    """0 has the neighbours 1 and 5 before (5 is not in the list handed in); 6 is new with 15 points: only 6 is reported."""
    return dict(map=make_map(8, shared=((0, 1, 20), (0, 5, 16), (0, 6, 15))), ops=both(0, 1, 20) + both(0, 5, 16), set=[1, 0],
                expect=[[], [6]], n_counter=[1, 3], front=[0, 1])


def lc_set_members_excluded():
    """List [1, 2, 0], no rows before.  1 shares 20 points with 0 and 15 with 2, 2 shares 3 with 6.  Member 1: {0, 2} are in the
    list.  Its update adds 1 to row 2, so at 2's turn 1 is a neighbour and in the list; 6 is a below-threshold entry of the
    new row 2, not a neighbour, not in the list: reported.  Member 0: {1}: in the list."""
    return dict(map=make_map(8, shared=((1, 0, 20), (1, 2, 15), (2, 6, 3))), ops=[], set=[1, 2, 0], expect=[[], [6], []],
                n_counter=[2, 2, 1], front=[0, 1, 1])


def lc_entry_becomes_member_before_turn():
    """Before: UpdateConnections(2) on a map where 2 shares 3 points with 6 and 20 with 7: row 2 = {6: 3 (entry, not a member),
    7: 20 (member)}.  The fused map adds 16 points shared by 1 and 2.  List [1, 2, 0].  Member 1's update calls
    2->AddConnection(1, 16): row 2 changes and its ordered vector is rebuilt from EVERY entry, so 6 is a neighbour of 2 at
    2's turn: LoopConnections[2] = {1, 6, 7} - {7, 1, 6} = {}.  A snapshot taken before the batch has {7} only and reports 6."""
    pre = make_map(8, shared=((2, 6, 3), (2, 7, 20)))
    return dict(map=make_map(8, shared=((2, 6, 3), (2, 7, 20), (1, 2, 16))), ops=[("update", pre, [2])], set=[1, 2, 0],
                expect=[[], [], []], naive=[[], [6], []], n_counter=[1, 3, 0], front=[2, 7, -1])


def lc_empty_counter_keeps_row():
    """Row 3 = {6: 3 (entry), 7: 20 (member)} before; in the new map key frame 3 holds no point: the counter is empty, the
    row stays, and its non-member entry 6 is reported."""
    pre = make_map(8, shared=((3, 6, 3), (3, 7, 20)))
    return dict(map=make_map(8, shared=((0, 1, 20),)), ops=[("update", pre, [3])], set=[3, 0], expect=[[6], [1]], n_counter=[0, 1],
                front=[7, 1])


def lc_order_is_kf_order():
    """kf_order descends with the slot: the new links 5, 6, 7 of key frame 0 come out as 7, 6, 5.  (The front of the ordered
    vector is the largest kf_order among the equal weights: 5.)"""
    order = [900 - 10 * k for k in range(8)]
    return dict(map=make_map(8, shared=((0, 5, 16), (0, 6, 16), (0, 7, 16)), kf_order=order), ops=[], set=[0], expect=[[7, 6, 5]],
                n_counter=[3], front=[5])


def connections_cases():
    cs = [lc_new_link_outside, lc_previous_neighbour_excluded, lc_set_members_excluded, lc_entry_becomes_member_before_turn,
          lc_empty_counter_keeps_row, lc_order_is_kf_order]
    return [(f.__name__, f()) for f in cs]
