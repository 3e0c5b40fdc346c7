"""The graphs of tests/ba_cases.py through the CPU oracle alone: proof that each construction does what it claims, before
any kernel is compared on it (tests/test_ba_structure_gpu.py).  No GPU needed.

Per case: the flags known by construction, the one-sided chi2 / depth gate recomputed in numpy float64 from the returned
state, and a condition on the INPUTS: no decision of the oracle's chi2 gate lies within 1e-3 (relative) of 5.991.  HIP and
the oracle differ by about 1e-8 on the poses, so no legitimate rounding difference flips a flag on these graphs; a case that
misses the condition gets another seed, never another bound."""
import numpy as np
import pytest

import ba_cases as BC

MIN_MARGIN = 1e-3
MAX_LEFT_OUT = 0.02


@pytest.mark.parametrize("cid", BC.ALL_IDS, ids=BC.case_name)
def test_case_on_the_oracle(cid, capsys):
    p, ex, out, margin = BC.oracle(cid)
    assert np.isfinite(out["kf_Tcw"]).all() and np.isfinite(out["mp_xw"]).all() and np.isfinite(out["mpb_xw"]).all()
    assert set(np.unique(out["obs_outlier"]).tolist()) <= {0, 1}
    BC.check_flags_by_construction(ex, out)
    bad, left_out = BC.gate_check(p, out, ex["with_odom"])
    with capsys.disabled():
        print("\n[ba structure] %-36s %5d front edges, %3d flagged; oracle margin %.3g; left out of the numpy gate check %.2f %%"
              % (BC.case_name(cid), len(p["obs_kf"]), int(out["obs_outlier"].sum()), margin, 100.0 * left_out), end="")
    assert len(bad) == 0, "edges returned with flag 0 that fail the gate in float64: %s" % bad[:10]
    assert left_out < MAX_LEFT_OUT
    assert margin >= MIN_MARGIN, "change the seed of this case: a chi2 lies within %.3g of the gate" % margin
    fx = p["kf_fixed"] == 1
    np.testing.assert_array_equal(out["kf_Tcw"][fx], p["kf_Tcw"][fx])


@pytest.mark.parametrize("big", [False, True])
def test_behind_camera_is_flagged_by_the_depth_clause_alone(big):
    """Would fail if the oracle lost `|| !depthPositive(e)`: at the returned state the special edge is more than a metre behind
    its camera and fits (chi2 < 3, far below 5.991), yet it is an outlier."""
    p, ex, out, _ = BC.oracle(("structural", "behind_camera", big))
    r = BC.recompute(p, out, 1)
    e = ex["special"]
    assert len(e) >= 3
    assert (r["depth"][e] < -1.0).all(), r["depth"][e]
    assert (r["chi2"][e] < 3.0).all(), r["chi2"][e]
    assert (out["obs_outlier"][e] == 1).all()
    # the point is 3-10 m behind that camera and in front of every other observer
    assert ((r["depth"][e] <= -3.0) & (r["depth"][e] >= -10.0)).all()
    for ed in e:
        others = [x for x in BC.edges_of(p, p["obs_mp"][ed]) if x != ed]
        assert (r["depth"][others] > 0).all()


@pytest.mark.parametrize("big", [False, True])
def test_landmark_fully_gated_construction(big):
    p, ex, out, _ = BC.oracle(("structural", "landmark_fully_gated", big))
    q0 = BC._base(BC.landmark_fully_gated.__defaults__[0], n_mp=300, n_mpb=60, **(BC.BIG if big else BC.SMALL))
    for l in ex["special"]:
        ee = BC.edges_of(p, l)
        assert len(ee) == 2 and (out["obs_outlier"][ee] == 1).all()
        clean = q0["obs_uv"][BC.edges_of(q0, l)[:2]]
        assert (np.linalg.norm(p["obs_uv"][ee].astype(np.float64) - clean, axis=1) >= 50.0).all()


@pytest.mark.parametrize("big", [False, True])
def test_keyframe_fully_gated_construction(big):
    p, ex, out, _ = BC.oracle(("structural", "keyframe_fully_gated", big))
    kf_gated, kf_empty = ex["special"]
    assert ex["with_odom"] == 0 and p["kf_fixed"][kf_gated] == 0 and p["kf_fixed"][kf_empty] == 0
    ee = np.nonzero(p["obs_kf"] == kf_gated)[0]
    assert len(ee) >= 20 and (out["obs_outlier"][ee] == 1).all()
    assert not (p["obs_kf"] == kf_empty).any()
    # the key frame nobody observes never enters the system, and neither does an isolated landmark
    np.testing.assert_allclose(out["kf_Tcw"][kf_empty], p["kf_Tcw"][kf_empty], rtol=0, atol=1e-6)
    lonely = BC.observers(p) == 0
    assert lonely.any()
    np.testing.assert_array_equal(out["mp_xw"][lonely], p["mp_xw"][lonely])


@pytest.mark.parametrize("big", [False, True])
def test_single_observation_and_fixed_only_constructions(big):
    p, ex, out, _ = BC.oracle(("structural", "single_observation_landmark", big))
    assert (BC.observers(p)[ex["special"]] == 1).all()
    assert np.abs(out["mp_xw"][ex["special"]] - p["mp_xw"][ex["special"]]).max() > 0      # they are in the system
    p, ex, out, _ = BC.oracle(("structural", "landmark_seen_only_by_fixed", big))
    for l in ex["special"]:
        assert (p["kf_fixed"][p["obs_kf"][BC.edges_of(p, l)]] == 1).all()
    assert np.abs(out["mp_xw"][ex["special"]] - p["mp_xw"][ex["special"]]).max() > 0      # structure-only, but optimised


def test_counts_are_what_the_cases_say():
    for f in BC.FREE_COUNTS:
        p, ex = BC.free_count(f)
        assert int((p["kf_fixed"] == 0).sum()) == f and int((p["kf_fixed"] == 1).sum()) == 2
    for n in BC.POINT_COUNTS:
        p, ex = BC.point_count(n)
        assert len(p["mp_xw"]) + len(p["mpb_xw"]) == n
    # plan(): up to 4096 points a workgroup takes one chunk of 16; the last one is partial unless 16 divides the count
    assert [n % 16 for n in BC.POINT_COUNTS] == [1, 15, 0, 1, 1, 4]
    n, cap = 100, BC.NWG_CAP_FOR_CHUNKS
    nwg = min(cap, -(-n // 16))
    per = -(-(-(-n // nwg)) // 16) * 16
    assert (per, -(-n // per), n - per) == (64, 2, 36)     # the second workgroup: two full chunks and a tail of four


def test_per_element_norm_is_the_tighter_one():
    """Just under 3 mm on one landmark of a 30 m scene: the old global norm max|d| / max(1, max|y|) passes it, the per-element norm not."""
    ref = np.array([[30.0, 0.0, 0.0], [0.5, 0.2, 0.1]])
    got = ref.copy()
    got[1, 0] += 2.9e-3
    assert np.abs(got - ref).max() / max(1.0, np.abs(ref).max()) <= BC.REL_TOL
    assert BC.worst_point_rel(got, ref) > BC.REL_TOL
    T = np.tile(np.array([1, 0, 0, 30.0, 0, 1, 0, 0, 0, 0, 1, 0]), (2, 1))
    T[1, 3] = 0.2
    G = T.copy()
    G[1, 3] += 2.9e-3
    assert np.abs(G - T).max() / max(1.0, np.abs(T).max()) <= BC.REL_TOL
    assert BC.worst_pose_rel(G, T) > BC.REL_TOL
    G[1, 3] = np.nan
    assert BC.worst_pose_rel(G, T) == float("inf")
