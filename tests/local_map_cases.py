"""Hand-built maps for the spanning tree and Tracking::UpdateLocalMap, one per quirk of the reference, with the answers worked
out by hand.  tests/test_local_map.py checks the model against them, tests/test_local_map_gpu.py the device."""
import numpy as np

from fishbirdeyevisualslam_amd import covis_problem as P


def make(pairs, frame, conns=(), parents=(), kf_bad=(), bad_points=(), local_in=(), ref_in=-1, K=8, S=40, order=None, want=None):
    """pairs: [(n points, [observing key frames])]; frame: mvpMapPoints as (pair, point) or None; conns: AddConnection(a, b, w);
    parents: ChangeParent(c, p) in order; bad_points: (pair, point) turned bad"""
    b = P.MapBuilder(K, S, 0)
    made = [b.shared(n, kfs) for n, kfs in pairs]
    order = list(range(100, 100 + K)) if order is None else order
    arr = b.arrays(order, shuffle=False)
    for pr, pt in bad_points:
        arr["mp_bad"][made[pr][pt]] = 1
    bad = np.zeros(K, np.uint8)
    bad[list(kf_bad)] = 1
    return dict(K=K, S=S, arr=arr, made=made, order=order, conns=list(conns), parents=list(parents), kf_bad=bad,
                frame=[-1 if f is None else made[f[0]][f[1]] for f in frame], local_in=list(local_in), ref_in=ref_in, want=want or {})


def local_map_cases():
    c = {}
    # kf_order puts slot 1 before slot 0.  A is seen by 0, B by 1.  The frame holds A at two features: 0 gets 2 votes, 1 gets 1
    c["double_vote"] = make([(1, [0]), (1, [1])], [(0, 0), (0, 0), (1, 0)], order=[200, 100, 300, 400, 500, 600, 700, 800],
                            want=dict(local_kf=[1, 0], ref_kf=0, n_voters=2, local_mp=[1, 0]))
    # one vote each: strict > in ascending kf_order keeps the first, slot 1
    c["pkfmax_tie"] = make([(1, [0]), (1, [1])], [(0, 0), (1, 0)], order=[200, 100, 300, 400, 500, 600, 700, 800],
                           want=dict(local_kf=[1, 0], ref_kf=1, n_voters=2))
    # slot 2 has the most votes and is bad: counted in keyframeCounter, not listed, not pKFmax
    c["bad_voter"] = make([(3, [2]), (1, [0]), (2, [1])], [(0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (2, 1)], kf_bad=[2],
                          want=dict(local_kf=[0, 1], ref_kf=1, n_voters=3, local_mp=[3, 4, 5]))
    # voter 0 has 12 neighbours (weights 30 .. 19 for slots 1 .. 12); the first ten are bad, so none of the ten is taken and
    # the good eleventh is never looked at
    c["bad_neighbours_occupy_places"] = make([(1, [0])], [(0, 0)], conns=[(0, s, 31 - s) for s in range(1, 13)], kf_bad=range(1, 11), K=14,
                                             want=dict(local_kf=[0], ref_kf=0, n_voters=1))
    # voters 0 and 1.  0 takes its neighbour 2 and then its parent 3, which ends the whole loop: 1's neighbour 4 is never added
    c["parent_break"] = make([(1, [0]), (1, [1])], [(0, 0), (1, 0)], conns=[(0, 2, 20), (1, 4, 20)], parents=[(0, 3)],
                             want=dict(local_kf=[0, 1, 2, 3], ref_kf=0, n_voters=2))
    # voter 0: neighbour 2 is taken in (a); 2 is also its first child and its parent.  (b) takes the next child 3; (c) finds the
    # parent marked, so there is no break and voter 1 still takes its neighbour 4.
    c["same_step_exclusion"] = make([(1, [0]), (1, [1])], [(0, 0), (1, 0)], conns=[(0, 2, 20), (1, 4, 20)],
                                    parents=[(2, 0), (3, 0), (0, 2)], want=dict(local_kf=[0, 1, 2, 3, 4], ref_kf=0, n_voters=2))
    # a bad parent is taken (no isBad test at :2211-2219) and a bad child is not
    c["bad_parent_taken"] = make([(1, [0])], [(0, 0)], parents=[(0, 3), (5, 0)], kf_bad=[3, 5],
                                 want=dict(local_kf=[0, 3], ref_kf=0, n_voters=1))
    # the only point of the frame is bad: it is cleared, the counter is empty, the list that came in stays (with the bad key
    # frame 2 in it, whose points are still collected: UpdateLocalPoints has no isBad test) and so does mpReferenceKF
    c["empty_counter"] = make([(1, [0]), (2, [2]), (1, [1, 2])], [(0, 0), None], bad_points=[(0, 0)], kf_bad=[2], local_in=[2, 1], ref_in=6,
                              want=dict(local_kf=[2, 1], ref_kf=6, n_voters=0, local_mp=[1, 2, 3], map_point=[-1, -1]))
    return c


def expansion_limit_case(n_voters=80):
    """80 voters (slots 0 .. 79), each with one point; voter 0 has a neighbour (100) and a child (125), every voter has a neighbour:
    after the first step the list holds 82 key frames and the second step's test ends the loop."""
    K = 128
    conns = [(v, 100 + v % 20, 20) for v in range(n_voters)]
    want = list(range(n_voters)) + ([100, 125] if n_voters <= 80 else [])         # more than 80 voters: the first test ends the loop
    return make([(1, [v]) for v in range(n_voters)], [(v, 0) for v in range(n_voters)], conns=conns, parents=[(125, 0)], K=K, S=8,
                want=dict(local_kf=want, ref_kf=0, n_voters=n_voters))
