"""CreateNewMapPoints (fb_create_new_map_points*): the C-ABI mirror and known answers of the CPU restatement
(tests/new_points_ref.py + tests/cpp/new_points_ref.cpp) that the GPU tests hold the device to."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import new_points_ref as R
from fishbirdeyevisualslam_amd import bow_problem as BP, cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_points_args_layout_matches_the_header():
    src = ('#include <stdio.h>\n#include "fishbird.h"\nint main(void){printf("%zu %d\\n", sizeof(fb_new_points_args), '
           'FB_NEW_POINTS_MAX_NB);return 0;}\n')
    d = tempfile.mkdtemp()
    open(os.path.join(d, "s.c"), "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
    size, maxnb = subprocess.check_output([os.path.join(d, "s")]).decode().split()
    assert int(size) == C.sizeof(cabi.NewPointsArgs)
    assert int(maxnb) == cabi.FB_NEW_POINTS_MAX_NB


def test_jacobi_null_vector_agrees_with_numpy_svd():
    g = np.random.default_rng(5)
    for k in range(200):
        A = g.normal(0, 1, (4, 4)).astype(np.float32)
        if k % 2:  # rank-3 + noise, the triangulation case
            x = g.normal(0, 1, 4)
            A = (A - np.outer(A @ x, x) / (x @ x)).astype(np.float32)
        v = R.null_vector(A)
        ref = np.linalg.svd(A.astype(np.float64))[2][3]
        s = np.sign(v @ ref)
        assert np.abs(v - s * ref).max() < 1e-9 * max(1.0, 1.0 / (np.linalg.svd(A.astype(np.float64))[1][2] - np.linalg.svd(A.astype(np.float64))[1][3]))


@pytest.fixture(scope="module")
def planted():
    p = BP.make_new_points_problem(11, n_nb=6, n1=1500, n2=1500)
    return p, R.create_new_map_points(p)


def test_noiseless_points_are_the_scene():
    p = BP.make_new_points_problem(12, n_nb=5, n1=1200, n2=1200, pixel_noise=0.0, plants=False)
    o = R.create_new_map_points(p)
    assert o["n_new"] > 300
    truth = p["truth"]["xw"][o["idx1"]]
    assert np.isfinite(truth).all()  # only true correspondences triangulate
    T1 = p["truth"]["T1"]
    Ow1 = -T1[:3, :3].T @ T1[:3, 3]
    rel = np.linalg.norm(o["xw"] - truth, axis=1) / np.linalg.norm(truth - Ow1, axis=1)
    assert rel.max() < 1e-4, rel.max()


def test_planted_cases_get_the_expected_decision(planted):
    p, o = planted
    pl, tr = p["truth"]["plants"], p["truth"]
    assert o["nb_skipped"].tolist() == [1 if b == tr["short_nb"] else 0 for b in range(6)]
    assert o["nb_matches"][tr["short_nb"]] == 0 and o["nb_new"][tr["short_nb"]] == 0
    rs = o["reasons"]
    far = [rs[k] for k in rs if k[1] in set(pl["far"].tolist())]
    assert len(far) > 20 and set(far) == {"parallax"}
    behind = [rs[k] for k in rs if k[0] == tr["behind_nb"] and k[1] in set(pl["behind"].tolist())]
    assert len(behind) > 10 and set(behind) == {"behind"}
    chi2 = [rs[k] for k in rs if k[0] == 0 and k[1] in set(pl["chi2"].tolist())]
    assert len(chi2) > 10 and chi2.count("chi2") >= 0.7 * len(chi2) and "ok" not in chi2
    scale = [rs[k] for k in rs if k[0] == 0 and k[1] in set(pl["scale"].tolist())]
    assert len(scale) > 10 and scale.count("scale") >= 0.7 * len(scale) and "ok" not in scale
    # the same features are claimed later by the second neighbour (the serial loop's order)
    won_later = [i for i in np.concatenate([pl["chi2"], pl["scale"]]) if (0, int(i)) in rs and o["kf1_new"][i] >= 0]
    assert won_later and all(o["nb"][o["kf1_new"][i]] == tr["second_nb"] for i in won_later)


def test_many_to_one_keeps_both_points_and_the_later_slot(planted):
    p, o = planted
    seen = 0
    for a, b in p["truth"]["plants"]["dup_pairs"]:
        ra, rb = o["kf1_new"][a], o["kf1_new"][b]
        if ra < 0 or rb < 0 or o["nb"][ra] != o["nb"][rb] or o["idx2"][ra] != o["idx2"][rb]:
            continue
        seen += 1
        assert rb > ra and o["kf2_new"][o["nb"][ra]][o["idx2"][ra]] == rb
    assert seen >= 5


def test_descriptor_follows_the_observation_order(planted):
    p, o = planted
    for r in range(o["n_new"]):
        nb = p["nbs"][o["nb"][r]]
        want = nb["desc"][o["idx2"][r]] if nb["before"] else p["desc1"][o["idx1"][r]]
        assert np.array_equal(o["desc"][r], want)
    assert {int(p["nbs"][b]["before"]) for b in set(o["nb"].tolist())} == {0, 1}
