"""CPU: the constructed pose-optimisation cases (tests/pose_cases.py) through the oracle and through the literal model
(tests/pose_ref.py).  For every case: identical masks, inlier count and LM event sequence; poses within POSE_BOUND; the
oracle's gate margin at least MIN_MARGIN; and, from the oracle's trace, the branch the case is about was taken.

Run with -s for one line per case: name, edges, flags per mask, re-admissions, LM events and margin.
"""
import numpy as np
import pytest

import oracle_lib as O
import pose_cases as PC
from fishbirdeyevisualslam_amd import problems as P

MIN_MARGIN = 1e-3          # as tests/test_ba_structure.py: no chi2 within 0.1 % of its gate
# Model and oracle are float64 and both write float32.  The worst relative pose difference measured over all cases is 0:
# the model sums in edge order and factors H + lambda I in the same order as the oracle, which is also what makes the LM
# event sequences comparable at all (the last steps of a round are accepted or rejected on rounding noise).  Ten times the
# measured value is 0, so the float32 poses must be identical.
POSE_BOUND = 0.0
UNREACHED = ("failed_solve",)   # no finite, well-posed frame makes H + lambda I lose positivity

_RESULTS = {}


def _result(case):
    """oracle outputs, oracle trace and model result of a case, computed once"""
    if case["id"] not in _RESULTS:
        out, tr = PC.run_oracle(case, O.lib(), O.call, P.pose_args)
        _RESULTS[case["id"]] = (out, tr, PC.run_model(case))
    return _RESULTS[case["id"]]


def _rel(Ta, Tb):
    Ta, Tb = np.asarray(Ta, np.float64), np.asarray(Tb, np.float64)
    return float(np.abs(Ta - Tb).max() / max(1.0, np.abs(Tb).max()))


CASES = PC.cases()


def test_case_ids_are_unique_and_inputs_are_tame():
    assert len({c["id"] for c in CASES}) == len(CASES)
    for c in CASES:
        p = c["prob"]
        assert c["doc"] and ("Optimizer.cc" in c["doc"] or ".cpp" in c["doc"]), c["id"]
        for k in ("front_xw", "front_obs", "front_inv_sigma2", "bird_xw", "bird_xc", "bird_inv_sigma2", "Tcw0"):
            assert np.isfinite(p[k]).all(), (c["id"], k)
        assert PC.min_abs_depth_at_start(p) >= 0.1, c["id"]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_oracle_equals_model(case):
    out, tr, m = _result(case)
    p, n_f, n_b = case["prob"], len(case["prob"]["front_xw"]), len(case["prob"]["bird_xw"])
    last = max(tr["rounds"] - 1, 0)
    rel = _rel(m["Tcw"], out["Tcw"])
    print("\n%-28s edges %3d+%3d  front flags %s  bird flags %s  re-admitted front %s bird %s  margin %.2e  rel %.1e\n    %s" % (
        case["id"], n_f, n_b, tr["front_flagged"][: last + 1], tr["bird_flagged"][: last + 1], tr["front_readmitted"],
        tr["bird_readmitted"], tr["margin"], rel, tr["events"]))
    if tr["decisions"]:
        assert tr["margin"] >= MIN_MARGIN, "change the seed of this case: a chi2 lies within %.3g of its gate" % tr["margin"]
    np.testing.assert_array_equal(out["front_outlier"][:n_f], m["front_outlier"])
    np.testing.assert_array_equal(out["bird_outlier"][:n_b], m["bird_outlier"])
    assert int(out["ninliers"]) == m["ninliers"]
    assert tr["events"] == m["events"]
    assert rel <= POSE_BOUND, rel
    # the trace's per-round counters tell the same story as the model's rounds
    assert tr["rounds"] == len(m["rounds"])
    for r, rd in enumerate(m["rounds"]):
        for k in PC.ROUND_COUNTERS:
            assert tr[k][r] == rd[k], (k, r)
        if r:
            # the active set of a round is what the round before left at level 0
            assert len(rd["active"]) == (n_f_edges(case) + n_b_edges(case) - m["rounds"][r - 1]["front_flagged"]
                                         - m["rounds"][r - 1]["bird_flagged"])


def n_f_edges(case):
    if case["kw"]["mode"] == PC.BIRD:
        return 0
    v = case["kw"].get("front_valid")
    return len(case["prob"]["front_xw"]) if v is None else int(np.count_nonzero(v[0]))


def n_b_edges(case):
    if case["kw"]["mode"] == PC.FRONT:
        return 0
    v = case["kw"].get("bird_valid")
    return len(case["prob"]["bird_xw"]) if v is None else int(np.count_nonzero(v[0]))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_takes_its_branch(case):
    """so that a later edit to a case cannot make its tests vacuous"""
    out, tr, m = _result(case)
    assert case["expect"], case["id"]
    for name in case["expect"]:
        assert PC.EXPECT[name](case, out, tr, m), "%s: '%s' does not hold; %s" % (case["id"], name, tr)


def test_nine_edges_run_one_round_and_ten_run_four():
    by_id = {c["id"]: c for c in CASES}
    for cid, rounds in (("count_front_9_5", 1), ("count_front_10_5", 4), ("count_bird_20_9", 1), ("count_bird_20_10", 4),
                        ("count_front_bird_3_6", 1), ("count_front_bird_3_7", 4), ("count_front_bird_6_3", 1),
                        ("count_front_bird_6_4", 4), ("count_front_bird_3_0", 1), ("count_front_3_5", 1), ("count_bird_20_3", 1),
                        ("count_front_bird_2_300", 0), ("count_front_2_5", 0), ("count_bird_20_2", 0)):
        assert _result(by_id[cid])[1]["rounds"] == rounds, cid


def test_no_active_edge_leaves_the_start_pose():
    """every edge at level 1 after round 1: optimize() returns at once, the pose set at the head of the round stays"""
    for c in CASES:
        if "no_active" in c["expect"]:
            out, tr, m = _result(c)
            assert tr["events"].endswith("/n/n/n")
            # through a unit quaternion and back: a few float32 steps of the start pose, whose rotation is only
            # orthonormal to float32
            assert _rel(out["Tcw"], c["prob"]["Tcw0"]) <= 1e-6
            assert _rel(m["Tcw"], c["prob"]["Tcw0"]) <= 1e-6


def test_every_counter_is_reached_by_some_case():
    total = {k: 0 for k in PC.COUNTERS + PC.ROUND_COUNTERS}
    for c in CASES:
        tr = _result(c)[1]
        for k in PC.COUNTERS:
            total[k] += tr[k]
        for k in PC.ROUND_COUNTERS:
            total[k] += sum(tr[k])
    for k, v in total.items():
        if k in UNREACHED:
            assert v == 0, "%s is reached now: take it off UNREACHED and DESIGN.md" % k
        else:
            assert v > 0, k
