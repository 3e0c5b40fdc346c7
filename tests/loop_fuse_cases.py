"""The cases of test_loop_fuse.py and test_loop_fuse_gpu.py: hand-built maps (map_refresh_cases.tiny) whose answers the tests
write out, and generated maps the device is compared with the literal model on.  Each case is made once and never
modified: the tests copy what they edit.  A case is (map dict, operation), operation = ("replace", from, to) or
("loop_fuse", cur, matched)."""
import functools

import numpy as np

from fishbirdeyevisualslam_amd import covis_problem as CP
from map_refresh_cases import bits, tiny


def counted(c, found=None, visible=None):
    n = len(c["mp_bad"])
    c["mp_found"] = np.arange(1, n + 1, dtype=np.int32) if found is None else np.asarray(found, np.int32)
    c["mp_visible"] = (10 * np.arange(1, n + 1)).astype(np.int32) if visible is None else np.asarray(visible, np.int32)
    return c


def described(c):
    """every feature its own descriptor: key frame k, feature i has the bits (8 * k + i) .. up to 8 * k + 7 set"""
    for k in range(c["K"]):
        for i in range(c["S"]):
            c["kf_desc"][k, i] = bits(*range((8 * k + i) % 256, (8 * k + 8) % 256 or 256)) if i < 8 else bits(k % 256)
    return c


def to_already_observed():
    """point 0 -> point 1; key frame 1 holds both: its slot of 0 is nulled and that edge dropped, key frame 0's goes over"""
    return described(counted(tiny(3, 4, [{0: 0, 1: 1}, {1: 2, 2: 0}]))), ("replace", [0], [1])


def same_from_twice():
    """0 -> 1, then 0 -> 2: the second finds no edges, adds found / visible again, mp_replaced = 2"""
    return described(counted(tiny(3, 4, [{0: 0}, {1: 0}, {2: 0}]))), ("replace", [0, 0], [1, 2])


def from_is_to():
    return described(counted(tiny(2, 2, [{0: 0}, {1: 0}]))), ("replace", [1, -1, 0], [1, 0, 0])


def chain():
    """a = 0 -> b = 1, then b -> c = 2; c is in key frame 1 already, where a was too"""
    return described(counted(tiny(4, 2, [{0: 0, 1: 0}, {2: 0}, {1: 1, 3: 0}]))), ("replace", [0, 1], [1, 2])


def out_of_range():
    return described(counted(tiny(2, 2, [{0: 0}, {1: 0}]))), ("replace", [2, 0, 0, 1], [0, 2, -1, 0])


def loop_point_already_in_cur():
    """cur = 2, 4 features.  Point 0 observes cur at feature 2 and is matched at the empty feature 0: kf_mp written, no edge.
    Point 1 is matched at the empty features 1 and 3: the first adds, the second returns early.  Feature 2 keeps point 0."""
    c = described(counted(tiny(3, 4, [{0: 0, 2: 2}, {1: 0}])))
    return c, ("loop_fuse", 2, [0, 1, -1, 1])


def loop_replace_and_add():
    """cur = 1: feature 0 holds point 0, matched to point 2 (Replace 0 -> 2); feature 1 is empty, matched to point 3 (add);
    feature 2 holds point 1, matched to point 2 again: 2 is in key frame 1 by then, so the slot is nulled"""
    c = described(counted(tiny(3, 4, [{0: 1, 1: 0}, {1: 2, 2: 1}, {0: 0}, {2: 0}])))
    return c, ("loop_fuse", 1, [2, 3, 2, -1])


def loop_wrong_n():
    c = described(counted(tiny(3, 4, [{0: 1, 1: 0}, {0: 0}])))
    c["kf_n"] = np.array([4, 3, 4], np.int32)
    return c, ("loop_fuse", 1, [1, 1, -1, -1])


def more_than_a_wave():
    """stride 2, 72 key frames: point 0 has 70 observers and is replaced by point 1 that has 40, 38 of them in common; then
    point 1, with 72 observers by then, goes on to point 2, which key frame 71 holds already"""
    K = 72
    a = {k: 0 for k in range(70)}
    b = {k: 1 for k in range(35, 72)}
    b.update({k: 1 for k in range(3)})
    c = tiny(K, 2, [a, b, {71: 0}], kf_order=(np.arange(K)[::-1] * 7 + 3))
    g = np.random.default_rng(5)
    c["kf_desc"] = g.integers(0, 256, (K, 2, 32)).astype(np.uint8)
    c["kf_desc"][::3] = c["kf_desc"][0]                                                               # ties in the medians
    return counted(c), ("replace", [0, 1], [1, 2])


def many_pairs(n=1100):
    """more pairs than a workgroup has threads: point i -> point n + (i % 7); the first 12 have an edge"""
    obs = [({i % 4: i // 4} if i < 12 else {}) for i in range(n)] + [({3: 3} if j == 0 else {}) for j in range(7)]
    c = described(counted(tiny(4, 4, obs)))
    return c, ("replace", list(range(n)), [n + (i % 7) for i in range(n)])


def exactly_k_edges():
    """K = 2: point 0 has exactly K live edges and goes to point 1 that has none (both moved), which, with K gained edges,
    goes to point 2 that has K of its own (both dropped).  No error: K + 1 edges is one (overflow_replace)."""
    return described(counted(tiny(2, 4, [{0: 0, 1: 0}, {}, {0: 1, 1: 1}]))), ("replace", [0, 1], [1, 2])


def one_key_frame():
    """K = 1 (one word of bits, two keys), S = 2: 0 -> 1 drops the edge and nulls the slot; 1 -> 2 moves 1's edge to a point
    that had none"""
    return described(counted(tiny(1, 2, [{0: 0}, {0: 1}, {}]))), ("replace", [0, 1], [1, 2])


def rank_32():
    """K = 33, S = 2, kf_order descending so that slot 0 has rank 32 (the one bit of the second word) and slot 1 rank 31.
    0 -> 1: `to` is observed by slot 0 only, `from` by slots 0 and 1: the rank-32 edge is dropped, the rank-31 one moved.
    1 -> 2: `to` is observed by slot 2 (rank 30) only, so both edges of 1 move: a bit left over in the second word would drop one"""
    K = 33
    c = tiny(K, 2, [{0: 0, 1: 0}, {0: 1}, {2: 0}], kf_order=(K - np.arange(K)) * 3)
    return described(counted(c)), ("replace", [0, 1], [1, 2])


def ping_pong():
    """a = 0 -> b = 1, b -> a, a -> b: edge 0 (a's at entry) goes to b, comes home to a (the index's row finds it: not linked
    again), goes to b again; b's own two come home in the third pair"""
    return described(counted(tiny(3, 4, [{0: 0, 1: 0}, {1: 1, 2: 0}]))), ("replace", [0, 1, 0], [1, 0, 1])


def bad_to_then_from():
    """point 1 is bad at entry: 0 -> 1 fills it and skips its refresh; 1 -> 2 takes its own edge and the gained one"""
    c = described(counted(tiny(3, 4, [{0: 0}, {1: 0}, {2: 0}])))
    c["mp_bad"][1] = 1
    return c, ("replace", [0, 1], [1, 2])


def bad_observers():
    """key frames 0 and 1 are bad.  0 -> 1: `to` ends with observers 0 and 1 only, the descriptor stays; 2 -> 3: `to` ends
    with 0, 1 and the good key frame 2, the descriptor is that one's"""
    return described(counted(tiny(3, 4, [{0: 0}, {1: 0}, {0: 1, 2: 1}, {1: 1}], kf_bad=(0, 1)))), ("replace", [0, 2], [1, 3])


def gained_edges_only():
    """point 1 has no edge at entry: 0 -> 1 hands it the two of point 0 (another row of the index), then 1 -> 2, where 2 is in
    key frame 1 already"""
    return described(counted(tiny(3, 4, [{0: 0, 1: 0}, {}, {1: 1}]))), ("replace", [0, 1], [1, 2])


def loop_two_adds():
    """loop_replace_and_add with point 4 matched at the empty feature 3: two replacements, two adds (the log-cut case)"""
    c = described(counted(tiny(3, 4, [{0: 1, 1: 0}, {1: 2, 2: 1}, {0: 0}, {2: 0}, {2: 2}])))
    return c, ("loop_fuse", 1, [2, 3, 2, 4])


HAND = (to_already_observed, same_from_twice, from_is_to, chain, out_of_range, loop_point_already_in_cur, loop_replace_and_add,
        loop_wrong_n, more_than_a_wave, many_pairs, exactly_k_edges, one_key_frame, rank_32, ping_pong, bad_to_then_from,
        bad_observers, gained_edges_only, loop_two_adds)


# ---- a repeated (mp, kf) edge: more live edges than key frames -------------------------------------------------------------------
def with_extra_edges(c, extra):
    """a copy of the map c with the edges extra = [(mp, kf, idx)] appended to the edge list, kf_mp left as it is: the map's
    precondition broken by hand (the model's dict of observations cannot hold them)"""
    c = dict(c)
    for k, col in (("obs_mp", 0), ("obs_kf", 1), ("obs_idx", 2)):
        c[k] = np.concatenate([c[k], np.array([e[col] for e in extra], np.int32)])
    return c


def world_beside_extra_edges(c, extra):
    """the model's World of the well-formed map c, with the edges of with_extra_edges(c, extra) in its edge arrays only: the
    model never sees them, they stay as they came, and edge numbers are those of the malformed map"""
    import loop_fuse_ref as LR
    w = LR.World(c)
    m = with_extra_edges(c, extra)
    w.obs_mp, w.obs_kf, w.obs_idx, w.home = m["obs_mp"].copy(), m["obs_kf"].copy(), m["obs_idx"].copy(), m["obs_mp"].copy()
    return w


OVERFLOW_EXTRA = [(0, 0, 1)]


def overflow_map():
    """K = 2: point 0 gets the edges (kf 0, 0), (kf 1, 0) and, appended by hand, (kf 0, 1): three live edges.  Points 1, 2, 3
    are well formed; 2 -> 3 moves 2's edge of key frame 0 and drops the one of key frame 1"""
    return described(counted(tiny(2, 4, [{0: 0, 1: 0}, {0: 2, 1: 1}, {0: 3, 1: 3}, {1: 2}])))


def overflow_replace():
    """-> (malformed map, operation, the expected World): 0 -> 1 and 1 -> 0 are skipped whole and counted, 2 -> 3 is what the
    model gives without the extra edge"""
    import loop_fuse_ref as LR
    good = overflow_map()
    w = world_beside_extra_edges(good, OVERFLOW_EXTRA)
    LR.replace_points(w, [2], [3])
    w.errors += 2
    return with_extra_edges(good, OVERFLOW_EXTRA), ("replace", [0, 1, 2], [1, 0, 3]), w


LOOP_OVERFLOW_EXTRA = [(0, 0, 1), (0, 0, 2)]


def overflow_loop_fuse():
    """K = 2, S = 4, cur = 1 is empty.  Point 0 has the edges (kf 0, 0) and, appended by hand, (kf 0, 1), (kf 0, 2): three live
    edges, none to cur (with one to cur the outcome would be that of AddObservation's early return).  It is matched at
    feature 1, the good point 1 at feature 2.  Contract (fishbird.h): kf_mp[1][1] = 0 is written, no edge is made, no refresh
    is done, one error; feature 2 then adds as the model does.  -> (malformed map, operation, the expected World)"""
    import loop_fuse_ref as LR
    good = described(counted(tiny(2, 4, [{0: 0}, {0: 3}])))
    w = world_beside_extra_edges(good, LOOP_OVERFLOW_EXTRA)
    LR.loop_fuse(w, 1, 4, [-1, -1, 1, -1])
    w.kf_mp[1, 1] = 0
    w.errors += 1
    return with_extra_edges(good, LOOP_OVERFLOW_EXTRA), ("loop_fuse", 1, [-1, 0, 1, -1]), w


GEN_SEED = 11


@functools.lru_cache(maxsize=None)
def generated_map(seed=GEN_SEED):
    return CP.make_refresh_problem(seed=seed, K=8, S=64, n_mp=190, counts=(), pool=8)


def generated_replace(seed=GEN_SEED):
    """120 random pairs over the generated map: repeats of a from, chains, self pairs, NULLs and two entries out of range"""
    c = generated_map(seed)
    n = len(c["mp_bad"])
    g = np.random.default_rng(seed + 1)
    frm, to = g.integers(0, n, 120), g.integers(0, n, 120)
    frm[10:20] = to[0:10]                                                                              # chains
    frm[30:34] = frm[26:30]                                                                            # the same from again
    to[40] = frm[40]
    frm[50:53] = -1
    frm[60], to[61] = n + 2, n
    return c, ("replace", frm.astype(np.int32).tolist(), to.astype(np.int32).tolist())


def generated_loop_fuse(seed=GEN_SEED):
    """cur = 3 of the generated map, every third feature matched: to a random point, to the point of another key frame, to a
    point that observes cur already, one point at two features, one entry out of range"""
    c = generated_map(seed)
    n, S, cur = len(c["mp_bad"]), c["S"], 3
    g = np.random.default_rng(seed + 2)
    matched = np.full(S, -1, np.int32)
    in_cur = [int(p) for p in c["kf_mp"][cur] if p >= 0]
    for i in range(0, S, 3):
        r = (i // 3) % 4
        matched[i] = int(g.integers(0, n)) if r < 2 else (in_cur[i % len(in_cur)] if r == 2 else int(c["kf_mp"][(cur + 1) % c["K"], i]))
    matched[4], matched[7] = matched[0], matched[0]
    matched[10] = n + 1
    return c, ("loop_fuse", cur, matched.tolist())


def all_cases():
    return [(f.__name__, f()) for f in HAND] + [("generated_replace", generated_replace()), ("generated_loop_fuse", generated_loop_fuse())]


# ---- SearchAndFuse ---------------------------------------------------------------------------------------------------------------
SAF_SET = (2, 5, 6)


@functools.lru_cache(maxsize=None)
def search_and_fuse_scene(seed=GEN_SEED, per_kf=20):
    """A generated scene from kf_problems: three key frames of 64 features (slots 2, 5, 6 of 8), each with 20 loop points that
    project into it (kf_problems.make_kf_points_problem, sim3).  Every third feature of a set key frame holds a point of its
    own (every second of those bad); the loop points are observed by key frames 0 and 1.  Loop point 3 * j + 1 is a copy of
    3 * j for j < 4 in every group: both win one feature.  -> (map dict, set slots, Scw rows, loop points)"""
    from fishbirdeyevisualslam_amd import kf_problems as KP
    K, S = 8, 64
    probs = [KP.make_kf_points_problem(seed * 10 + k, S, per_kf, True) for k in range(len(SAF_SET))]
    n_loop = per_kf * len(SAF_SET)
    obs = [{0: i, 1: (i * 7) % S} if i % 2 == 0 else {0: i} for i in range(n_loop)]
    own = []
    for slot in SAF_SET:
        for i in range(0, S, 3):
            own.append({slot: i, 7: len(own) % S} if len(own) < S else {slot: i})
    c = tiny(K, S, obs + own, kf_order=[50, 20, 70, 10, 80, 30, 60, 40], n_levels=8)
    g = np.random.default_rng(seed)
    c["kf_desc"] = g.integers(0, 256, (K, S, 32)).astype(np.uint8)
    c["kf_keys_un"] = np.zeros((K, S), probs[0]["kf_kps"].dtype)
    n_mp = len(c["mp_bad"])
    c["mp_xw"], c["mp_normal"] = np.zeros((n_mp, 3), np.float32), np.zeros((n_mp, 3), np.float32)
    c["mp_min_dist"], c["mp_max_dist"] = np.zeros(n_mp, np.float32), np.zeros(n_mp, np.float32)
    c["mp_desc"] = g.integers(0, 256, (n_mp, 32)).astype(np.uint8)
    scw = []
    for k, (slot, p) in enumerate(zip(SAF_SET, probs)):
        c["kf_keys_un"][slot], c["kf_desc"][slot] = p["kf_kps"], p["kf_desc"]
        sl = slice(k * per_kf, (k + 1) * per_kf)
        for key in ("mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc"):
            c[key][sl] = p[key]
        for j in range(4):                                                                             # same-feature collisions
            for key in ("mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc"):
                c[key][k * per_kf + 3 * j + 1] = c[key][k * per_kf + 3 * j]
        scw.append(p["pose"])
    c["mp_bad"][n_loop::2] = 1                                                                         # pMPinKF bad
    return counted(c), list(SAF_SET), np.stack(scw).astype(np.float32), list(range(n_loop))


# ---- SearchAndFuse: two set key frames that see the same thing ------------------------------------------------------------------
SHARED_SET = (5, 2)


@functools.lru_cache(maxsize=None)
def shared_view_scene(seed=GEN_SEED, n_loop=12):
    """search_and_fuse_scene with two set key frames (slots 5 and 2, in that order) that have the same key points, descriptors
    and Scw row, and 12 loop points: every loop point that matches in the first matches in the second.  Loop points 3 * j + 1
    and 3 * j + 2 are copies of 3 * j for j < 3: in the first key frame the first of three adds, the other two get it as rep;
    in the second key frame the second adds, holding the first's edges (one of them made in this call), and the third
    replaces it, which moves those edges again.  -> (map dict, set slots, Scw rows, loop points)"""
    from fishbirdeyevisualslam_amd import kf_problems as KP
    K, S = 8, 64
    p = KP.make_kf_points_problem(seed * 10 + 7, S, n_loop, True)
    obs = [{0: i, 1: (i * 7) % S} if i % 2 == 0 else {0: i} for i in range(n_loop)]
    own = []
    for slot in SHARED_SET:
        for i in range(0, S, 3):
            own.append({slot: i, 7: len(own) % S})
    c = tiny(K, S, obs + own, kf_order=[50, 20, 70, 10, 80, 30, 60, 40], n_levels=8)
    g = np.random.default_rng(seed + 3)
    c["kf_desc"] = g.integers(0, 256, (K, S, 32)).astype(np.uint8)
    c["kf_keys_un"] = np.zeros((K, S), p["kf_kps"].dtype)
    n_mp = len(c["mp_bad"])
    c["mp_xw"], c["mp_normal"] = np.zeros((n_mp, 3), np.float32), np.zeros((n_mp, 3), np.float32)
    c["mp_min_dist"], c["mp_max_dist"] = np.zeros(n_mp, np.float32), np.zeros(n_mp, np.float32)
    c["mp_desc"] = g.integers(0, 256, (n_mp, 32)).astype(np.uint8)
    for slot in SHARED_SET:
        c["kf_keys_un"][slot], c["kf_desc"][slot] = p["kf_kps"], p["kf_desc"]
    for key in ("mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc"):
        c[key][:n_loop] = p[key]
        for j in range(3):
            c[key][3 * j + 1] = c[key][3 * j + 2] = c[key][3 * j]
    for i, o in enumerate(obs):                                                                        # a loop point looks the same from its observers:
        for kf, idx in o.items():                                                                      # a refreshed descriptor still matches
            c["kf_desc"][kf, idx] = c["mp_desc"][i]
    c["mp_bad"][n_loop::2] = 1                                                                         # pMPinKF bad
    return counted(c), list(SHARED_SET), np.stack([p["pose"], p["pose"]]).astype(np.float32), list(range(n_loop))


def shared_view_bad_entries():
    """the shared view with set slots [5, -1, 8, 2] (two out of range), a loop point out of range appended and the entry of
    feature 1 of slot 2 set to n_mp"""
    c, slots, scw, loop = shared_view_scene()
    c = dict(c, kf_mp=c["kf_mp"].copy())
    n_mp = len(c["mp_bad"])
    c["kf_mp"][2, 1] = n_mp
    return c, [5, -1, 8, 2], np.stack([scw[0]] * 4), loop + [n_mp + 3]


SHORT_KEPT = 11


def shared_view_short(n=40):
    """the shared view with kf_n = 40 < S for both set key frames, and their features permuted so that every feature the search
    returns for a loop point in the full scene sits at 40 or later, the one of loop point 11 apart: the descriptors that would
    win are not part of the key frame.  Loop point 11 also stands at feature 50 of slot 5: past kf_n, so it is not one of
    GetMapPoints() and stays valid"""
    import loop_fuse_ref as LR
    c, slots, scw, loop = shared_view_scene()
    w, log = LR.World(c), []

    def recorded(*a):
        log.append(LR.oracle_search(*a))
        return log[-1]
    LR.search_and_fuse(w, c, slots, scw, loop, search=recorded)
    S, kept = c["S"], log[0][SHORT_KEPT]
    won = sorted({b for row in log for b in row if b >= 0 and b != kept})
    assert kept >= 0 and 0 < len(won) <= S - n
    perm = np.array([kept] + [i for i in range(S) if i not in won and i != kept] + won)               # new position -> old feature
    c = dict(c, kf_n=c["kf_n"].copy(), kf_keys_un=c["kf_keys_un"].copy(), kf_desc=c["kf_desc"].copy(), kf_mp=c["kf_mp"].copy())
    for slot in slots:
        c["kf_keys_un"][slot], c["kf_desc"][slot] = c["kf_keys_un"][slot][perm], c["kf_desc"][slot][perm]
        c["kf_n"][slot] = n
        c["kf_mp"][slot, 0] = -1                                                                       # the kept feature is empty
    c["kf_mp"][5, 50] = SHORT_KEPT
    return c, slots, scw, loop


SAF_OVERFLOW_POINT = 11
SAF_OVERFLOW_EXTRA = [(SAF_OVERFLOW_POINT, 0, 20 + j) for j in range(8)]


def shared_view_overflow():
    """the shared view with loop point 11 (one edge, wins the empty feature 14 in both set key frames) given eight more edges
    by hand: nine live edges at K = 8.  Contract (fishbird.h): kf_mp[slot][14] = 11 is written and counts in nFused, no edge
    is made, one error per key frame; every other loop point goes as the model says.  The model gets there by believing the
    point is in both set key frames already (AddObservation's early return).  -> (malformed map, slots, Scw, loop, expected
    World, expected nFused)"""
    import loop_fuse_ref as LR
    c, slots, scw, loop = shared_view_scene()
    w = world_beside_extra_edges(c, SAF_OVERFLOW_EXTRA)
    for slot in slots:
        w.obs[SAF_OVERFLOW_POINT][slot] = (0, -1)
    n_fused = LR.search_and_fuse(w, c, slots, scw, loop)
    w.errors += len(slots)
    return with_extra_edges(c, SAF_OVERFLOW_EXTRA), slots, scw, loop, w, n_fused
