"""The HIP matchers on the accept/reject boundaries: every constructed case of tests/matcher_edge_cases.py through the
host-pointer entry point and through its `_dev` twin, against the literal model of tests/matcher_ref.py.  Everything compared
is an integer (match arrays over each member's own length, counters; the rotation-dropped set shows as the -1 entries and
in the counters) and must be equal.  For M2 the two entry points are also its two kernels: the host call runs the two-phase
matcher in a workspace of its own, the `_dev` call without a workspace the one-kernel version.

M4, M7 and the M10 entry points (Fuse x2, initialization, Sim3, Proj(KF, Scw)) have no model: their constructed cases
(Hamming thresholds, ties, several queries on one target, the search radius) are compared with the oracle, exactly, again
through both entry points."""
import ctypes as C

import numpy as np
import pytest

import matcher_edge_cases as E
import oracle_lib as O
from device_mirror import Mirror, _lib, _stream, _sync

pytestmark = pytest.mark.gpu

MATCHERS = ("m2", "m3", "m5", "m6", "m8", "m9")


@pytest.mark.parametrize("m", MATCHERS)
def test_hip_equals_model_on_the_cases(m):
    lib, name = _lib(), E.ENTRY[m][1]
    cases = E.modelled(m)
    assert len(cases) > 10
    for c in cases:
        model = E.run_model(c)
        a, out, keep = E.build_args(c, O.grid_build)
        assert getattr(lib, name)(C.byref(a)) == 0, (c["name"], lib.fb_last_error())
        E.compare(c, out, model, name)
        a, out, keep = E.build_args(c, O.grid_build)
        mir = Mirror(out, keep)
        d = mir.struct(a)
        assert getattr(lib, name + "_dev")(C.byref(d), _stream()) == 0, (c["name"], lib.fb_last_error())
        _sync()
        E.compare(c, {k: mir.host(v) for k, v in out.items()}, model, name + "_dev")


@pytest.mark.parametrize("name", sorted(E.ORACLE_ONLY))
def test_hip_equals_oracle_on_the_oracle_only_cases(name):
    lib = _lib()
    orc, hip = E.ORACLE_ONLY[name][:2]
    for cname, p, kw in E.oracle_only_cases(name):
        a, want, keep = E.oracle_only_args(name, p, kw, O.grid_build)
        O.call(orc, a)
        assert any((v >= 0).any() and (v < 0).any() for v in want.values() if v.dtype == np.int32), (name, cname)
        a, out, keep = E.oracle_only_args(name, p, kw, O.grid_build)
        assert getattr(lib, hip)(C.byref(a)) == 0, (name, cname, lib.fb_last_error())
        for k in want:
            np.testing.assert_array_equal(out[k], want[k], err_msg="%s %s %s" % (hip, cname, k))
        a, out, keep = E.oracle_only_args(name, p, kw, O.grid_build)
        mir = Mirror(out, keep)
        d = mir.struct(a)
        assert getattr(lib, hip + "_dev")(C.byref(d), _stream()) == 0, (name, cname, lib.fb_last_error())
        _sync()
        for k in want:
            np.testing.assert_array_equal(mir.host(out[k]), want[k], err_msg="%s_dev %s %s" % (hip, cname, k))
