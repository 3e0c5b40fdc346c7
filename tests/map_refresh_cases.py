"""The cases of test_map_refresh.py and test_map_refresh_gpu.py: small hand-built maps whose answers the tests work out, and
the generated maps the device is compared with the literal model on.  Each generated case is made once and never modified:
the tests copy what they edit."""
import functools

import numpy as np

from fishbirdeyevisualslam_amd import covis_problem as CP

f32 = np.float32
REFRESH_COUNTS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 130)   # 128 = FB_REFRESH_STAGE: one under, at, one over the LDS staging


def tiny(K, S, observers, kf_order=None, kf_bad=(), centres=None, octave=None, ref=None, xw=None, n_levels=4):
    """A hand-built map: observers[mp] = {kf: idx}; key frame k has the identity rotation and the centre centres[k]."""
    n_mp = len(observers)
    kf_mp = np.full((K, S), -1, np.int32)
    edges = [(mp, kf, idx) for mp, o in enumerate(observers) for kf, idx in o.items()]
    for mp, kf, idx in edges:
        kf_mp[kf, idx] = mp
    centres = np.zeros((K, 3)) if centres is None else np.asarray(centres, np.float64)
    bad = np.zeros(K, np.uint8)
    bad[list(kf_bad)] = 1
    desc = np.zeros((K, S, 32), np.uint8)
    return dict(K=K, S=S, kf_n=np.full(K, S, np.int32), kf_mp=kf_mp, kf_octave=np.zeros((K, S), np.uint8) if octave is None else np.asarray(octave, np.uint8),
                mp_bad=np.zeros(n_mp, np.uint8), obs_mp=np.array([e[0] for e in edges], np.int32), obs_kf=np.array([e[1] for e in edges], np.int32),
                obs_idx=np.array([e[2] for e in edges], np.int32), kf_order=np.arange(1, K + 1, dtype=np.uint64) if kf_order is None else np.asarray(kf_order, np.uint64),
                kf_Tcw=np.stack([CP.pose12(np.eye(3), -centres[k]) for k in range(K)]), kf_bad=bad, kf_desc=desc,
                scale_factors=(f32(1.2) ** np.arange(n_levels, dtype=f32)).astype(f32),
                mp_xw=np.zeros((n_mp, 3), f32) if xw is None else np.asarray(xw, f32), mp_ref_kf=np.zeros(n_mp, np.int32) if ref is None else np.asarray(ref, np.int32),
                mp_normal=np.full((n_mp, 3), 9, f32), mp_min_dist=np.full(n_mp, 9, f32), mp_max_dist=np.full(n_mp, 9, f32),
                mp_desc=np.full((n_mp, 32), 0xAB, np.uint8))


def bits(*set_bits):
    """a descriptor with the given bits set"""
    d = np.zeros(32, np.uint8)
    for b in set_bits:
        d[b // 8] |= 1 << (b % 8)
    return d


@functools.lru_cache(maxsize=None)
def refresh_case():
    """every observer count of the issue around the wave-wide sort (64) and the LDS staging (128), stride 4, descriptors from a
    pool of 8, and 14 more points (bad ones among them)"""
    return CP.make_refresh_problem(seed=31, S=4, counts=REFRESH_COUNTS, n_mp=len(REFRESH_COUNTS) + 14)


@functools.lru_cache(maxsize=None)
def new_keyframe_case(N=70, S=96, K=12, declared=None):
    """A key frame of N features in slot K - 1 of a small map: features that already observe it, NULL entries, bad points, new
    points, one point held at two features and one out-of-range entry.  -> (case, slot, n_features the host passes)"""
    c = dict(CP.make_refresh_problem(seed=47 + N, K=K, S=S, n_mp=150, counts=(), n_recent=5))
    g = np.random.default_rng(900 + N)
    slot = K - 1
    row = np.array(c["kf_mp"][slot])
    has = {int(mp) for mp, kf in zip(c["obs_mp"], c["obs_kf"]) if kf == slot}
    new = [p for p in range(150) if p not in has and not c["mp_bad"][p]]
    badp = [p for p in range(150) if c["mp_bad"][p]]
    twice = new.pop()
    script = []
    for i in range(N):
        if row[i] >= 0:
            continue                                                                                   # already observing the slot
        r = i % 5
        row[i] = -1 if r == 0 else (badp[i % len(badp)] if r == 1 else new.pop())
        script.append(i)
    if N >= 20:
        row[script[3]], row[script[-2]] = twice, twice                                                 # its second feature finds the first's edge
        row[script[6]] = 150 + 5                                                                       # out of range
    row[N:] = -1
    c["kf_mp"] = np.array(c["kf_mp"])
    c["kf_mp"][slot] = row
    c["kf_n"] = np.array(c["kf_n"])
    c["kf_n"][slot] = N
    return c, slot, N if declared is None else declared


CUR_KF_ID = 10


@functools.lru_cache(maxsize=None)
def culling_case(n_list=40):
    """point p has (p % 3) + 1 observers.  n_list == 40: four rounds of ten entries that take every branch at its boundary;
    otherwise random entries on random found / visible / first-id.  -> (case, list)"""
    c = dict(CP.make_refresh_problem(seed=59, K=24, S=32, counts=[1, 2, 3] * 40))
    c["mp_bad"] = np.zeros(120, np.uint8)
    if n_list != 40:
        g = np.random.default_rng(n_list)
        c["mp_bad"][g.choice(120, 10, replace=False)] = 1
        return c, g.integers(0, 120, n_list).astype(np.int32)
    found, vis, first = np.full(120, 4, np.int32), np.full(120, 4, np.int32), np.full(120, CUR_KF_ID - 1, np.int32)
    lst = []
    for r in range(4):
        o1, o2, o3 = 30 * r, 30 * r + 1, 30 * r + 2                                                    # points with 1, 2, 3 observers
        p = [o1, o2 + 3, o3 + 3, o1 + 6, o2 + 6, o3 + 9, o3 + 12, o1 + 12, o2 + 12]
        c["mp_bad"][p[0]] = 1                                                                          # 0: bad -> dropped
        found[p[1]], vis[p[1]] = 1, 5                                                                  # 1: 0.2 < 0.25 -> SetBadFlag
        found[p[2]], vis[p[2]] = 1, 4                                                                  # 2: exactly 0.25, age 1 -> kept
        found[p[3]], vis[p[3]] = 0, 0                                                                  # 3: NaN, age 1 -> kept
        found[p[4]], vis[p[4]], first[p[4]] = 3, 0, CUR_KF_ID - 2                                      # 4: inf, age 2, 2 observers -> SetBadFlag
        first[p[5]] = CUR_KF_ID - 2                                                                    # 5: age 2, 3 observers -> kept
        first[p[6]] = CUR_KF_ID - 3                                                                    # 6: age 3, 3 observers -> dropped
        first[p[7]] = -1 if r == 0 else CUR_KF_ID - 1                                                  # 7: age 1 (or made from a Frame: age 11, 1 observer -> SetBadFlag)
        first[p[8]] = CUR_KF_ID - 3                                                                    # 8: age 3, 2 observers -> SetBadFlag
        lst += p + [p[1]]                                                                              # 9: listed twice -> dropped as bad
    c["mp_found"], c["mp_visible"], c["mp_first_kf_id"] = found, vis, first
    return c, np.array(lst, np.int32)
