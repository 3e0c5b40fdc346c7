"""Every argument-array host drop-in (the entry points without `_dev`) against its `_dev` twin: the same inputs, the host
call on numpy arrays and the `_dev` call on device copies, then every output array compared byte for byte over its whole
length.  Entries the kernels do not write (tails past the counts, skipped slots) must keep the caller's sentinel contents
in both.  Also: a call that fails after its inputs were staged leaves the next call on the thread intact, and a null
required input is an argument error on the host."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from device_mirror import Mirror, _lib, _stream, _sync
import test_bird_filter as TBF
import test_bird_guidance as TBG
import test_bow_transform as TBT
from fishbirdeyevisualslam_amd import bow_problem as BP, cabi, kf_problems as KP, more_problems as M, problems as P, synth

pytestmark = pytest.mark.gpu


def _check_outputs(out, mir):
    for k, v in out.items():
        assert v.tobytes() == mir.host(v).tobytes(), k


def _host_vs_dev(name, build, host_fields=(), prep_dev=None, extra=None):
    """build() -> (args, out, keep).  The host drop-in on `args` and `name`_dev on a device mirror of the same inputs."""
    a, out, keep = build()
    mir = Mirror(out, keep, extra)
    d = mir.struct(a, host_fields)
    if prep_dev is not None:
        prep_dev(d)
    lib = _lib()
    assert getattr(lib, name)(C.byref(a)) == 0, lib.fb_last_error()
    assert getattr(lib, name + "_dev")(C.byref(d), _stream()) == 0, lib.fb_last_error()
    _sync()
    _check_outputs(out, mir)
    return out


# ---- front matchers ----------------------------------------------------------------------------------------------------
FRONT = P.grid_geom(synth.front_grid_geom(1280, 720))
BIRD = P.grid_geom(synth.bird_grid_geom(512, 512))


@pytest.mark.parametrize("sizes,stride,retry", [([(1500, 1400), (900, 1200)], None, False), ([(700, 600), (300, 650)], 1000, True)])
def test_match_projection_frame(sizes, stride, retry):
    probs = [synth.make_proj_frame_problem(7100 + i, nc, nl, dup_frac=0.2) for i, (nc, nl) in enumerate(sizes)]
    cs_ = stride or max(n for n, _ in sizes)
    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], FRONT, O.grid_build, cs_)

    def build():
        a, out, keep = P.proj_frame_args(probs, cs, ci, cur_stride=stride)
        if retry:
            out["retried"] = np.full(len(probs), -7, np.int32)
            cabi.fill(a, retried=out["retried"], retry_below=400, retry_th=30.0)
        return a, out, keep
    _host_vs_dev("fb_match_projection_frame", build)


@pytest.mark.parametrize("sizes", [[(1500, 1300), (800, 1400)], [(300, 200), (50, 500), (10, 0)]])
def test_match_projection_keyframe(sizes):
    probs = [M.make_proj_kf_problem(7200 + i, nc, nk) for i, (nc, nk) in enumerate(sizes)]
    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], FRONT, O.grid_build, max(n for n, _ in sizes))
    _host_vs_dev("fb_match_projection_keyframe", lambda: M.proj_kf_args(probs, cs, ci))


@pytest.mark.parametrize("sizes", [[(1500, 2500), (900, 1000)], [(300, 700), (60, 40)]])
def test_match_projection_points(sizes):
    import torch
    probs = [synth.make_proj_points_problem(7300 + i, nc, nm) for i, (nc, nm) in enumerate(sizes)]
    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], FRONT, O.grid_build, max(n for n, _ in sizes))
    lib = _lib()
    lib.fb_match_projection_points_workspace.restype = C.c_size_t
    ws = []

    def prep(d):  # the host drop-in runs the two-phase matcher in a workspace of its own
        nb = lib.fb_match_projection_points_workspace(d.batch, d.mp_stride)
        ws.append(torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda"))
        cabi.fill(d, workspace=ws[0], workspace_bytes=nb)
    _host_vs_dev("fb_match_projection_points", lambda: P.proj_points_args(probs, cs, ci, th=1.0), prep_dev=prep)


@pytest.mark.parametrize("sizes,stride,prefill", [([(1200, 1000), (700, 900)], None, -1), ([(400, 300), (90, 500)], 800, 12345)])
def test_match_bird_mappoints(sizes, stride, prefill):
    probs = [synth.make_bird_mp_problem(7400 + i, nc, nr) for i, (nc, nr) in enumerate(sizes)]
    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], BIRD, O.grid_build, stride or max(n for n, _ in sizes))
    _host_vs_dev("fb_match_bird_mappoints", lambda: P.bird_mp_args(probs, cs, ci, prefill=prefill, cur_stride=stride))


@pytest.mark.parametrize("sizes", [[(1200, 1300), (800, 600)], [(200, 500), (400, 30)]])
def test_match_birdview(sizes):
    probs = [synth.make_birdview_problem(7500 + i, nc, nr) for i, (nc, nr) in enumerate(sizes)]
    cs, ci = P.build_grid_host([p["cur_kps"] for p in probs], BIRD, O.grid_build, max(n for n, _ in sizes))
    _host_vs_dev("fb_match_birdview", lambda: P.birdview_args(probs, cs, ci))


# ---- BoW matchers and new map points -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[(1500, 1400), (900, 1300)], [(200, 300), (40, 10)]])
def test_match_bow(sizes):
    probs = [BP.make_bow_problem(7600 + i, nk, nf) for i, (nk, nf) in enumerate(sizes)]
    _host_vs_dev("fb_match_bow", lambda: BP.bow_args(probs))


@pytest.mark.parametrize("sizes", [[(1500, 1400), (900, 1300)], [(200, 300), (40, 10)]])
def test_match_bow_kf(sizes):
    probs = [M.make_bow_kf_problem(7700 + i, n1, n2) for i, (n1, n2) in enumerate(sizes)]
    _host_vs_dev("fb_match_bow_kf", lambda: M.bow_kf_args(probs))


@pytest.mark.parametrize("sizes", [[(1500, 1400), (900, 1300)], [(200, 300), (40, 10)]])
def test_match_triangulation(sizes):
    probs = [BP.make_triangulation_problem(7800 + i, n1, n2) for i, (n1, n2) in enumerate(sizes)]
    _host_vs_dev("fb_match_triangulation", lambda: BP.triangulation_args(probs))


@pytest.mark.parametrize("n_nb,n1,n2,s1,s2", [(6, 1500, 1400, None, None), (3, 500, 400, 700, 650)])
def test_create_new_map_points(n_nb, n1, n2, s1, s2):
    import torch
    p = BP.make_new_points_problem(7900, n_nb=n_nb, n1=n1, n2=n2)
    lib = _lib()
    lib.fb_create_new_map_points_workspace.restype = C.c_size_t
    ws = []

    def prep(d):
        nb = lib.fb_create_new_map_points_workspace(d.n_nb, d.kf1_stride)
        ws.append(torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda"))
        cabi.fill(d, workspace=ws[0], workspace_bytes=nb)
    _host_vs_dev("fb_create_new_map_points", lambda: BP.new_points_args(p, kf1_stride=s1, kf2_stride=s2),
                 host_fields=("nb_mp_start",), prep_dev=prep)


# ---- frame geometry and pose ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[3000, 2000], [400, 20, 0]])
def test_in_frustum(sizes):
    probs = [M.make_frustum_problem(8000 + i, n) for i, n in enumerate(sizes)]
    _host_vs_dev("fb_in_frustum", lambda: M.frustum_args(probs))


@pytest.mark.parametrize("n1,n2,nm", [(1000, 1000, 800), (300, 200, 50)])
def test_bird_filter_matches(n1, n2, nm):
    _host_vs_dev("fb_bird_filter_matches", lambda: TBF.make(8100, n1, n2, nm))


@pytest.mark.parametrize("mode", [cabi.FB_POSE_FRONT_BIRD, cabi.FB_POSE_FRONT])
def test_pose_opt(mode):
    probs = [synth.make_pose_problem(8200 + i, n_front=700 + 300 * i, n_bird=300 + 100 * i) for i in range(3)]
    a, out, keep = P.pose_args(probs, mode=mode)
    mir = Mirror(out, keep)
    d = mir.struct(a)
    lib = _lib()
    assert lib.fb_pose_opt(C.byref(a)) == 0, lib.fb_last_error()
    assert lib.fb_pose_opt_batch_dev(C.byref(d), _stream()) == 0, lib.fb_last_error()
    _sync()
    _check_outputs(out, mir)


@pytest.mark.parametrize("seed,B,rows,cols,n,with_mask,with_desc,edge_cap", [
    (8300, 2, 384, 384, 900, True, True, 4096), (8301, 3, 300, 420, 700, False, False, 0),
    (8302, 2, 256, 256, 400, True, False, 64), (8303, 2, 384, 384, 600, False, True, 0)])
def test_bird_guidance(seed, B, rows, cols, n, with_mask, with_desc, edge_cap):
    contours, kps, descs, masks = TBG._random_problem(seed, B, rows, cols, n, with_mask, with_desc)
    _host_vs_dev("fb_bird_guidance", lambda: TBG.make_args(contours, kps, descs, masks, edge_cap, stride=n + 50))


@pytest.mark.parametrize("seed,k,L,levelsup,sizes", [(8400, 10, 3, 2, [1500, 900, 33]), (8410, 4, 5, 2, [700, 0, 1])])
def test_bow_transform(seed, k, L, levelsup, sizes):
    v, vk, first_leaf = TBT.make_vocabulary(seed, k=k, L=L)
    descs = TBT._descs(seed + 1, sizes, vk, first_leaf)
    a, out, keep = TBT.make_args(descs, levelsup)
    mir = Mirror(out, keep, vk)
    dv, da = mir.struct(v), mir.struct(a)
    lib = _lib()
    assert lib.fb_bow_transform(C.byref(v), C.byref(a)) == 0, lib.fb_last_error()
    assert lib.fb_bow_transform_dev(C.byref(dv), C.byref(da), _stream()) == 0, lib.fb_last_error()
    _sync()
    _check_outputs(out, mir)


@pytest.mark.parametrize("n", [4, 1000])
def test_undistort_keypoints(n):
    g = synth.rng(8500 + n)
    kps = synth.random_keypoints(g, n, 1280, 720)
    out = np.zeros_like(kps)
    out["x"] = -7.0
    cnt = np.array([n], np.int32)
    mir = Mirror(kps, out, cnt)
    K4, D4 = (np.ascontiguousarray(x, np.float32) for x in (M.FISHEYE_K, M.FISHEYE_D))
    ptr = lambda x: C.c_void_p(x.ctypes.data)
    dptr = lambda x: C.c_void_p(mir.dev(x.ctypes.data))
    lib = _lib()
    assert lib.fb_undistort_keypoints(ptr(kps), C.c_int(n), ptr(K4), ptr(D4), ptr(out)) == 0, lib.fb_last_error()
    assert lib.fb_undistort_keypoints_dev(dptr(kps), dptr(cnt), 1, n, ptr(K4), ptr(D4), dptr(out), _stream()) == 0
    _sync()
    assert out.tobytes() == mir.host(out).tobytes()


@pytest.mark.parametrize("n", [5, 3000])
def test_descriptor_distance(n):
    g = synth.rng(8600 + n)
    a, b = synth.random_descriptors(g, n), synth.random_descriptors(g, n)
    out = np.full(n, -7, np.int32)
    mir = Mirror(a, b, out)
    lib = _lib()
    assert lib.fb_descriptor_distance(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), n, C.c_void_p(out.ctypes.data)) == 0
    assert lib.fb_descriptor_distance_dev(*(C.c_void_p(mir.dev(x.ctypes.data)) for x in (a, b)), n,
                                          C.c_void_p(mir.dev(out.ctypes.data)), _stream()) == 0
    _sync()
    assert out.tobytes() == mir.host(out).tobytes()


# ---- key-frame side matchers (match_kf.inc) ----------------------------------------------------------------------------
def _kf_probs(seed, sizes, sim3):
    probs = [KP.make_kf_points_problem(seed + i, nk, nm, sim3) for i, (nk, nm) in enumerate(sizes)]
    cs, ci = P.build_grid_host([p["kf_kps"] for p in probs], P.grid_geom(synth.front_grid_geom(KP.W, KP.H)), O.grid_build,
                               max(max(n for n, _ in sizes), 1))
    return probs, cs, ci


@pytest.mark.parametrize("name", ["fb_fuse_search", "fb_fuse_sim3_search"])
@pytest.mark.parametrize("sizes", [[(1500, 2500), (900, 1200)], [(300, 200), (50, 500)]])
def test_fuse(name, sizes):
    probs, cs, ci = _kf_probs(8700, sizes, name == "fb_fuse_sim3_search")
    _host_vs_dev(name, lambda: KP.fuse_args(probs, cs, ci))


@pytest.mark.parametrize("sizes", [[(1500, 2500), (900, 1200)], [(300, 200), (50, 500)]])
def test_match_projection_sim3(sizes):
    probs, cs, ci = _kf_probs(8800, sizes, True)
    _host_vs_dev("fb_match_projection_sim3", lambda: KP.proj_sim3_args(probs, cs, ci))


def _sim3_build(seed, sizes):
    probs = [KP.make_sim3_problem(seed + i, n1, n2, ns) for i, (n1, n2, ns) in enumerate(sizes)]
    s1, s2 = max(s[0] for s in sizes), max(s[1] for s in sizes)
    g1 = P.build_grid_host([p["kps1"] for p in probs], FRONT, O.grid_build, s1)
    g2 = P.build_grid_host([p["kps2"] for p in probs], FRONT, O.grid_build, s2)
    return lambda: KP.sim3_args(probs, g1, g2)


@pytest.mark.parametrize("sizes", [[(1500, 1400, 900), (900, 1200, 500)], [(300, 200, 100), (60, 250, 30)]])
def test_match_sim3(sizes):
    _host_vs_dev("fb_match_sim3", _sim3_build(8900, sizes))


def _init_build(seed, sizes):
    probs = [KP.make_init_problem(seed + i, n1, n2) for i, (n1, n2) in enumerate(sizes)]
    cs, ci = P.build_grid_host([p["kps2"] for p in probs], FRONT, O.grid_build, max(s[1] for s in sizes))
    return lambda: KP.init_args(probs, cs, ci)


@pytest.mark.parametrize("sizes", [[(1500, 1400), (900, 1300)], [(200, 300), (40, 10)]])
def test_match_initialization(sizes):
    _host_vs_dev("fb_match_initialization", _init_build(9000, sizes))


@pytest.mark.parametrize("n_mp,max_obs", [(5, 3), (2000, 40)])
def test_distinctive_descriptors(n_mp, max_obs):
    start, desc = KP.make_distinctive_problem(9100 + n_mp, n_mp, max_obs=max_obs, big=2)
    best = np.full(n_mp, -7, np.int32)
    mir = Mirror(start, desc, best)
    dptr = lambda x: C.c_void_p(mir.dev(x.ctypes.data))
    lib = _lib()
    assert lib.fb_distinctive_descriptors(C.c_void_p(start.ctypes.data), C.c_void_p(desc.ctypes.data), n_mp,
                                          C.c_void_p(best.ctypes.data)) == 0, lib.fb_last_error()
    assert lib.fb_distinctive_descriptors_dev(dptr(start), dptr(desc), n_mp, dptr(best), _stream()) == 0
    _sync()
    assert best.tobytes() == mir.host(best).tobytes()


# ---- error paths ---------------------------------------------------------------------------------------------------------
def test_failed_call_after_staging_leaves_the_next_call_intact():
    """mp_stride 50 000 makes fb_match_projection_sim3's LDS plan too large: FB_ERR_CAPACITY after the inputs were staged and
    before any launch.  The next call on the same thread must still see its own inputs.  (This exercises the error path;
    it cannot show that an in-flight copy was waited for.)"""
    lib = _lib()
    probs, cs, ci = _kf_probs(9200, [(900, 1200), (500, 800)], True)
    a0, ref, _k0 = KP.proj_sim3_args(probs, cs, ci)
    assert lib.fb_match_projection_sim3(C.byref(a0)) == 0, lib.fb_last_error()
    big, bcs, bci = _kf_probs(9300, [(600, 50000)], True)
    ab, outb, _kb = KP.proj_sim3_args(big, bcs, bci)
    assert ab.mp.mp_stride == 50000
    assert lib.fb_match_projection_sim3(C.byref(ab)) == cabi.FB_ERR_CAPACITY
    a1, got, _k1 = KP.proj_sim3_args(probs, cs, ci)
    assert lib.fb_match_projection_sim3(C.byref(a1)) == 0, lib.fb_last_error()
    for k in ref:
        assert got[k].tobytes() == ref[k].tobytes(), k


def _null_rejected(name, a, out, field, sub=None):
    lib = _lib()
    before = {k: v.copy() for k, v in out.items()}
    cabi.fill(getattr(a, sub) if sub else a, **{field: None})
    assert getattr(lib, name)(C.byref(a)) == cabi.FB_ERR_ARG
    _sync()
    for k, v in out.items():
        assert v.tobytes() == before[k].tobytes(), k


@pytest.mark.parametrize("name,sub,field", [("fb_fuse_search", "kf", "kf_desc"), ("fb_fuse_sim3_search", None, "pose"),
                                            ("fb_fuse_search", "mp", "mp_xw")])
def test_null_input_fuse(name, sub, field):
    probs, cs, ci = _kf_probs(9400, [(300, 400)], name == "fb_fuse_sim3_search")
    a, out, _keep = KP.fuse_args(probs, cs, ci)
    _null_rejected(name, a, out, field, sub)


@pytest.mark.parametrize("sub,field", [(None, "Scw"), ("mp", "mp_desc")])
def test_null_input_projection_sim3(sub, field):
    probs, cs, ci = _kf_probs(9500, [(300, 400)], True)
    a, out, _keep = KP.proj_sim3_args(probs, cs, ci)
    _null_rejected("fb_match_projection_sim3", a, out, field, sub)


def test_null_input_sim3():
    a, out, _keep = _sim3_build(9600, [(300, 200, 100)])()
    _null_rejected("fb_match_sim3", a, out, "R12")


def test_null_input_initialization():
    a, out, _keep = _init_build(9700, [(300, 250)])()
    _null_rejected("fb_match_initialization", a, out, "desc2")


def test_null_input_bird_guidance():
    contours, kps, descs, masks = TBG._random_problem(9800, 1, 128, 128, 100, False, True)
    for field in ("contour", "kps_in", "edge_sign"):
        a, out, _keep = TBG.make_args(contours, kps, descs, masks, 16)
        _null_rejected("fb_bird_guidance", a, out, field)


def test_null_input_bow_transform():
    v, vk, first_leaf = TBT.make_vocabulary(9900, k=10, L=3)
    a, out, _keep = TBT.make_args(TBT._descs(9901, [100], vk, first_leaf))
    lib = _lib()
    cabi.fill(a, desc=None)
    assert lib.fb_bow_transform(C.byref(v), C.byref(a)) == cabi.FB_ERR_ARG
    v.weights = None
    a2, out2, _keep2 = TBT.make_args(TBT._descs(9901, [100], vk, first_leaf))
    assert lib.fb_bow_transform(C.byref(v), C.byref(a2)) == cabi.FB_ERR_ARG
    assert (out2["n_words"] == -7).all() and (out["n_words"] == -7).all()


def test_null_input_flat_arrays():
    lib = _lib()
    d = np.zeros((8, 32), np.uint8)
    o = np.full(8, -7, np.int32)
    assert lib.fb_descriptor_distance(None, C.c_void_p(d.ctypes.data), 8, C.c_void_p(o.ctypes.data)) == cabi.FB_ERR_ARG
    assert lib.fb_descriptor_distance(C.c_void_p(d.ctypes.data), None, 8, C.c_void_p(o.ctypes.data)) == cabi.FB_ERR_ARG
    kp = np.zeros(8, cabi.KP_DTYPE)
    K4, D4 = (np.ascontiguousarray(x, np.float32) for x in (M.FISHEYE_K, M.FISHEYE_D))
    assert lib.fb_undistort_keypoints(None, 8, C.c_void_p(K4.ctypes.data), C.c_void_p(D4.ctypes.data),
                                      C.c_void_p(kp.ctypes.data)) == cabi.FB_ERR_ARG
    start = np.array([0, 2, 3], np.int32)
    assert lib.fb_distinctive_descriptors(C.c_void_p(start.ctypes.data), None, 2, C.c_void_p(o.ctypes.data)) == cabi.FB_ERR_ARG
    assert (o == -7).all()
