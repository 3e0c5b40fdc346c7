"""The FAST score network of csrc/fb_fast_score.h on the CPU: the plain int instantiation and the packed two-pixels-per-
word instantiation (over a bit-level binary16 model of the packed min3 / max3, tests/cpp/fast_score_packed_ref.cpp)
against the oracle's own fast_score (oracle/orb_oracle.cpp), clamped at 0 as the extractor stores it.  Equality is exact."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]  # (dx, dy), cv::FAST's order
RING_IDX = np.array([(3 + dy) * 7 + 3 + dx for dx, dy in RING])
EXTREMES = np.array([0, 1, 127, 128, 254, 255], np.uint8)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(), "libfast_score_packed_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-w",
                               os.path.join(ROOT, "tests", "cpp", "fast_score_packed_ref.cpp"), "-o", so])
        _LIB = C.CDLL(so)
        for f in (_LIB.fsp_score_batch, _LIB.fsp_bad_class_count, _LIB.fsp_check_encoding):
            f.restype = C.c_longlong
    return _LIB


def score(patches):
    """-> (oracle, int network, packed network) for [n, 7, 7] uint8 patches; asserts the two halves of the packed word agree."""
    p = np.ascontiguousarray(patches, np.uint8).reshape(-1, 49)
    out = np.full((len(p), 3), -9, np.int32)
    r = lib().fsp_score_batch(C.c_void_p(p.ctypes.data), C.c_longlong(len(p)), C.c_void_p(out.ctypes.data))
    assert r == 0, "packed network: %d patches score differently in the high half (or -1: stray bytes in the result word)" % r
    return out[:, 0], out[:, 1], out[:, 2]


def check(patches, what):
    ref, si, sp = score(patches)
    assert np.array_equal(si, ref), "%s: int network differs from the oracle at %d patches" % (what, int((si != ref).sum()))
    assert np.array_equal(sp, ref), "%s: packed network differs from the oracle at %d patches" % (what, int((sp != ref).sum()))
    assert lib().fsp_bad_class_count() == 0, "%s: a NaN / infinity / denormal / zero reached the packed min3 / max3" % what
    return ref


def test_encoding_exhaustive():
    """Every (centre, tap) byte pair, the identities and finish() over all (A, Bm): the bias arithmetic is exact."""
    assert lib().fsp_check_encoding() == 0


def test_extreme_rings():
    """Ring values from {0, 1, 127, 128, 254, 255} around every centre of the same set, 3000 random ring assignments per
    centre (the other 32 pixels of the patch random: they must not matter)."""
    rng = np.random.default_rng(41)
    n = 3000
    patches = rng.integers(0, 256, (len(EXTREMES), n, 49), dtype=np.uint8)
    for k, c in enumerate(EXTREMES):
        patches[k, :, 24] = c
        patches[k][:, RING_IDX] = EXTREMES[rng.integers(0, len(EXTREMES), (n, 16))]
    # + the uniform rings: every ring pixel at one value of the set around every centre (score |centre - ring| - 1)
    uni = np.zeros((len(EXTREMES), len(EXTREMES), 49), np.uint8)
    uni[:, :, 24] = EXTREMES[:, None]
    uni[:, :, RING_IDX] = EXTREMES[None, :, None]
    ref = check(np.concatenate([patches.reshape(-1, 7, 7), uni.reshape(-1, 7, 7)]), "extreme rings")
    assert ref[-36:].reshape(6, 6).tolist() == [[max(abs(int(c) - int(r)) - 1, 0) for r in EXTREMES] for c in EXTREMES]
    assert (ref[:-36] > 0).sum() > 1000 and ref[:-36].max() >= 126  # the random assignments do hold corners


def test_uniform_random_patches():
    """10^6 uniformly random 7x7 patches."""
    rng = np.random.default_rng(42)
    check(rng.integers(0, 256, (1000000, 7, 7), dtype=np.uint8), "uniform patches")


def test_synthetic_corners():
    """Arcs of 7..16 ring pixels brighter or darker than the centre by a random margin on a noisy ring: scores of every
    size, both polarities, arcs at every rotation, arcs just too short."""
    rng = np.random.default_rng(43)
    n = 200000
    patches = rng.integers(0, 256, (n, 49), dtype=np.uint8)
    centre = rng.integers(0, 256, n)
    base = centre[:, None] + rng.integers(-6, 7, (n, 16))
    start, length = rng.integers(0, 16, n), rng.integers(7, 17, n)
    margin = rng.integers(1, 256, n) * rng.choice([-1, 1], n)
    inarc = ((np.arange(16)[None, :] - start[:, None]) % 16) < length[:, None]
    ring = np.clip(np.where(inarc, centre[:, None] + margin[:, None] + rng.integers(-3, 4, (n, 16)), base), 0, 255)
    patches[:, 24] = centre
    patches[:, RING_IDX] = ring.astype(np.uint8)
    ref = check(patches.reshape(-1, 7, 7), "synthetic corners")
    assert (ref > 20).sum() > n // 10 and (ref == 0).sum() > n // 20


def test_ring_order_matches_oracle():
    """One bright pixel at ring position k on a dark ring is no corner; nine from position k on are: checks ring_offset()."""
    for k in range(16):
        p = np.zeros((7, 7), np.uint8)
        p[3, 3] = 100
        for j in range(9):
            dx, dy = RING[(k + j) % 16]
            p[3 + dy, 3 + dx] = 100 - 50 - j  # darker arc of 9: score = min(d) - 1 = 49
        q = p.copy()
        for j in range(16):
            dx, dy = RING[j]
            if q[3 + dy, 3 + dx] == 0:
                q[3 + dy, 3 + dx] = 100
        ref = check(np.stack([p, q]), "ring order %d" % k)
        assert ref[1] == 49
