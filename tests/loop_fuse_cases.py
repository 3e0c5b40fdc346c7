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


HAND = (to_already_observed, same_from_twice, from_is_to, chain, out_of_range, loop_point_already_in_cur, loop_replace_and_add,
        loop_wrong_n, more_than_a_wave, many_pairs)

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
