"""Generates tests/golden/dbow2_ref.npz and tests/golden/dbow2_ref_pin.npz from the REFERENCE's own DBoW2::FeatureVector /
DBoW2::BowVector, compiled from the reference tree by `make -C oracle ref` (oracle/_ref/libref_dbow2.so).  Run where the
reference is present, after build() (the pin streams go through the oracle as well); the fixtures are data: input id /
weight streams and the containers the reference code produced from them.

    python tests/golden/make_dbow2_ref_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import ref_dbow2  # noqa: E402


def main():
    g = np.random.Generator(np.random.PCG64(8800))
    out = {}
    for c, (n, nnodes, nwords) in enumerate([(2000, 100, 900), (37, 5, 12), (1, 1, 1), (1500, 1000, 100000)]):
        node = g.integers(0, nnodes, n).astype(np.uint32) * 7 + 3
        word = g.integers(0, nwords, n).astype(np.uint32)
        w = g.uniform(0.01, 9.0, n)
        ids, start, items = ref_dbow2.feature_vector(node)
        bid, bval = ref_dbow2.bow_vector(word, w, True)
        bid0, bval0 = ref_dbow2.bow_vector(word, w, False)
        out.update({"c%d_node" % c: node, "c%d_word" % c: word, "c%d_w" % c: w, "c%d_fv_ids" % c: ids, "c%d_fv_start" % c: start,
                    "c%d_fv_items" % c: items, "c%d_bow_ids" % c: bid, "c%d_bow_vals" % c: bval, "c%d_bow_raw" % c: bval0})
    np.savez_compressed(os.path.join(HERE, "dbow2_ref.npz"), **out)
    print("wrote dbow2_ref.npz")

    # every stream the pin tests feed the reference containers, with what the reference build returned for it
    import test_ref_dbow2_pin as T
    fv, bow = [], []

    def rec_fv(node):
        node = np.ascontiguousarray(node, np.uint32)
        r = ref_dbow2.feature_vector(node)
        fv.append((node,) + r)
        return r

    def rec_bow(word, w):
        word, w = np.ascontiguousarray(word, np.uint32), np.ascontiguousarray(w, np.float64)
        r = ref_dbow2.bow_vector(word, w, True)
        bow.append((word, w) + r)
        return r
    T._check_against(rec_fv, rec_bow, "oracle/_ref")
    T._check_synthetic(rec_fv)
    pin = {"n_fv": np.int32(len(fv)), "n_bow": np.int32(len(bow))}
    for i, (node, ids, start, items) in enumerate(fv):
        pin.update({"fv%d_node" % i: node, "fv%d_ids" % i: ids, "fv%d_start" % i: start, "fv%d_items" % i: items})
    for i, (word, w, ids, vals) in enumerate(bow):
        pin.update({"bow%d_word" % i: word, "bow%d_w" % i: w, "bow%d_ids" % i: ids, "bow%d_vals" % i: vals})
    np.savez_compressed(os.path.join(HERE, "dbow2_ref_pin.npz"), **pin)
    print("wrote dbow2_ref_pin.npz (%d FeatureVector, %d BowVector streams)" % (len(fv), len(bow)))


if __name__ == "__main__":
    main()
