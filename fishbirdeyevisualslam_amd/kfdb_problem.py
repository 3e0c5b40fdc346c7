"""Planted key-frame databases for the KeyFrameDatabase tests (fb_kfdb_*).

K "places", each a pool of words.  A key frame draws most of its words from the pool of its place and a few from a pool
all places share, so key frames of other places are listed by a query (they share a word) but fall below the common-word
threshold.  The key frames of a place form a chain; the covisibility rows link chain neighbours.
"""
import numpy as np


def l1_normalised(ids, weights):
    """BowVector of distinct words: ids ascending, values divided by the L1 norm (added in ascending word order)."""
    ids = np.asarray(ids, np.uint32)
    o = np.argsort(ids, kind="stable")
    ids, w = ids[o], np.asarray(weights, np.float64)[o]
    norm = float(np.add.accumulate(np.abs(w))[-1]) if len(w) else 0.0  # a running sum: ascending word order
    return ids.copy(), (w / norm if norm > 0.0 else w).astype(np.float64)


def _draw(g, pool, n_place, shared, n_shared):
    ids = np.concatenate([g.choice(pool, min(n_place, len(pool)), replace=False), g.choice(shared, min(n_shared, len(shared)), replace=False)])
    ids = np.unique(ids)
    return l1_normalised(ids, g.uniform(0.5, 5.0, len(ids)))


def make_kfdb_problem(seed, n_places=4, per_place=40, pool=420, place_words=(140, 200), n_shared_pool=300, shared_words=25,
                      chain_links=2, vocab=1000000):
    """-> dict: bows [(ids, vals)] per slot, place [n_kf], covis [n_kf][10], queries [(ids, vals, place, connected)].
    Slots are shuffled, so the add order is not the place order."""
    g = np.random.default_rng(seed)
    words = g.choice(vocab, n_places * pool + n_shared_pool, replace=False).astype(np.uint32)
    shared = words[n_places * pool:]
    pools = [words[p * pool:(p + 1) * pool] for p in range(n_places)]
    n_kf = n_places * per_place
    slot_of = g.permutation(n_kf)  # (place, chain position) -> slot
    bows = [None] * n_kf
    place = np.zeros(n_kf, np.int32)
    covis = np.full((n_kf, 10), -1, np.int32)
    for p in range(n_places):
        for c in range(per_place):
            s = int(slot_of[p * per_place + c])
            place[s] = p
            bows[s] = _draw(g, pools[p], int(g.integers(place_words[0], place_words[1] + 1)), shared, shared_words)
            nb = [c + d for k in range(1, chain_links + 1) for d in (k, -k) if 0 <= c + d < per_place]
            covis[s, :len(nb)] = [slot_of[p * per_place + x] for x in nb]
    queries = []
    for p in range(n_places):
        ids, vals = _draw(g, pools[p], place_words[1], shared, shared_words)
        connected = [int(slot_of[p * per_place + c]) for c in (0, 1)]  # the two most recent key frames of the place
        queries.append((ids, vals, p, connected))
    return dict(bows=bows, place=place, covis=covis, queries=queries, n_kf=n_kf)


def make_random_database(seed, n_kf, words=(1, 4096), vocab=20000):
    """Unstructured database: n_kf BowVectors of words[0]..words[1] words over a small vocabulary, random covisibility rows."""
    g = np.random.default_rng(seed)
    bows = []
    for _ in range(n_kf):
        n = int(g.integers(words[0], words[1] + 1))
        ids = g.choice(vocab, min(n, vocab), replace=False).astype(np.uint32)
        bows.append(l1_normalised(ids, g.uniform(0.1, 6.0, len(ids))))
    covis = np.full((max(n_kf, 1), 10), -1, np.int32)
    for s in range(n_kf):
        k = int(g.integers(0, 11))
        if n_kf > 1 and k:
            covis[s, :k] = g.choice(n_kf, k, replace=k > n_kf)
    return dict(bows=bows, covis=covis, n_kf=n_kf)
