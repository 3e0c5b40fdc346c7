"""Loader for the CPU oracle (oracle/_build/liboracle.so) -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
_LIB = None

from fishbirdeyevisualslam_amd import cabi  # noqa: E402  (ctypes struct mirrors of include/fishbird.h only)


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "liboracle.so")
        if not os.path.exists(so):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
        _LIB = C.CDLL(so)
    return _LIB


def orb_params(**kw):
    from fishbirdeyevisualslam_amd import synth
    d = dict(synth.ORB_DEFAULT)
    d.update(kw)
    return cabi.OrbParams(**d)


def orb_tables(params):
    t = cabi.OrbTables()
    assert lib().orc_orb_tables(C.byref(params), C.byref(t)) == 0
    return t


def orb_extract(params, img):
    img = np.ascontiguousarray(img)
    h, w = img.shape
    cap = params.nfeatures + 8 * params.nlevels
    kps = np.zeros(cap, cabi.KP_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = C.c_int32(0)
    rc = lib().orc_orb_extract(C.byref(params), C.c_void_p(img.ctypes.data), w, h, w, C.c_void_p(kps.ctypes.data),
                               C.c_void_p(desc.ctypes.data), C.byref(n))
    assert rc == 0, rc
    return kps[: n.value].copy(), desc[: n.value].copy()


def orb_level(params, img, level):
    img = np.ascontiguousarray(img)
    h, w = img.shape
    lw, lh = C.c_int(0), C.c_int(0)
    buf = np.zeros(w * h, np.uint8)
    lib().orc_orb_level(C.byref(params), C.c_void_p(img.ctypes.data), w, h, w, level, C.c_void_p(buf.ctypes.data),
                        C.byref(lw), C.byref(lh))
    return buf[: lw.value * lh.value].reshape(lh.value, lw.value).copy()


def orb_candidates(params, img, level, cap=400000):
    img = np.ascontiguousarray(img)
    h, w = img.shape
    xyr = np.zeros((cap, 3), np.int32)
    n = lib().orc_orb_candidates(C.byref(params), C.c_void_p(img.ctypes.data), w, h, w, level,
                                 C.c_void_p(xyr.ctypes.data), cap)
    assert n <= cap
    return xyr[:n].copy()


def grid_build(kps, n, batch, stride, geom, cs, ci):
    rc = lib().orc_grid_build(C.c_void_p(kps.ctypes.data), C.c_void_p(n.ctypes.data), batch, stride, C.byref(geom),
                              C.c_void_p(cs.ctypes.data), C.c_void_p(ci.ctypes.data))
    assert rc == 0


def call(name, args):
    rc = getattr(lib(), name)(C.byref(args))
    assert rc == 0, (name, rc)


def frame_pipeline(params, front, bird, world, fx=500.0, fy=500.0, timings=None):
    """CPU restatement of the per-frame hot path for ONE frame pair, stage by stage, in the order of
    fishbirdeyevisualslam_amd.pipeline.FramePipeline.step().  `world` is one entry of build_world().
    timings (dict): receives the seconds spent inside the oracle's C++ for each stage of BASELINE.md section 3
    (extract_front, extract_bird, match_front, match_bird, pose_opt); the numpy glue between the calls is not counted."""
    import time
    from fishbirdeyevisualslam_amd import synth, problems as P
    from fishbirdeyevisualslam_amd.cabi import fill
    tm = timings if timings is not None else {}
    fh, fw = front.shape
    bh, bw = bird.shape
    cap = params.nfeatures + 8 * params.nlevels
    t = orb_tables(params)
    t0 = time.perf_counter()
    fk, fd = orb_extract(params, front)
    t1 = time.perf_counter()
    bk, bd = orb_extract(params, bird)
    t2 = time.perf_counter()
    tm["extract_front"], tm["extract_bird"] = t1 - t0, t2 - t1
    gf = P.grid_geom(synth.front_grid_geom(fw, fh))
    gb = P.grid_geom(synth.bird_grid_geom(bw, bh))
    fcs, fci = P.build_grid_host([fk], gf, grid_build, cap)
    bcs, bci = P.build_grid_host([bk], gb, grid_build, cap)
    Tbc, Tcb = synth.extrinsics()
    # Frame.cc:365-373 (float result of double arithmetic, then Tcb * p in float)
    base = np.zeros((len(bk), 3), np.float32)
    base[:, 0] = ((bh // 2 - bk["y"].astype(np.float64)) * synth.PIXEL2METER + synth.REAR_AXLE_TO_CENTER).astype(np.float32)
    base[:, 1] = ((bw // 2 - bk["x"].astype(np.float64)) * synth.PIXEL2METER).astype(np.float32)
    Tc = Tcb[:3, :4].astype(np.float32)
    f = np.float32
    bcam = np.zeros((len(bk), 3), np.float32)
    for r in range(3):
        bcam[:, r] = f(f(f(f(Tc[r, 0] * base[:, 0]) + f(Tc[r, 1] * base[:, 1])) + f(Tc[r, 2] * base[:, 2])) + Tc[r, 3])
    nl, nr = world["n_last"], world["n_ref"]
    cx, cy = fw / 2.0, fh / 2.0
    prob = dict(w=fw, h=fh, fx=fx, fy=fy, cx=cx, cy=cy, Tcw=world["Tcw0"], cur_kps=fk, cur_desc=fd,
                cur_blocked=np.zeros(len(fk), np.uint8), last_valid=np.ones(nl, np.uint8), last_obs_pos=np.ones(nl, np.uint8),
                last_xw=world["last_xw"], last_desc=world["last_desc"], last_octave=world["last_octave"],
                last_angle=world["last_angle"])
    a, out3, keep = P.proj_frame_args([prob], fcs, fci, th=15.0, nnratio=0.9, cur_stride=cap,
                                      scale_factors=[t.scale_factor[i] for i in range(params.nlevels)])
    t0 = time.perf_counter()
    call("orc_match_projection_frame", a)
    tm["match_front"] = time.perf_counter() - t0
    m3 = out3["match_cur_to_last"]
    bprob = dict(cols=bw, rows=bh, Tbc=Tbc, Tcb=Tcb, Tcw=world["Tcw0"], cur_kps=bk, cur_desc=bd, cur_cam_xyz=bcam,
                 ref_valid=np.ones(nr, np.uint8), ref_xw=world["ref_xw"], ref_desc=world["ref_desc"])
    a9, out9, keep9 = P.bird_mp_args([bprob], bcs, bci, cur_stride=cap)
    t0 = time.perf_counter()
    call("orc_match_bird_mappoints", a9)
    tm["match_bird"] = time.perf_counter() - t0
    m9 = out9["match_cur_to_ref"]
    # edge construction (Optimizer.cc:525-602)
    inv = np.array([t.inv_level_sigma2[i] for i in range(params.nlevels)], np.float32)
    fv = (m3[0, : len(fk)] >= 0).astype(np.uint8)
    fx_w = np.zeros((len(fk), 3), np.float32)
    fx_w[fv == 1] = world["last_xw"][m3[0, : len(fk)][fv == 1]]
    bv = (m9[0, : len(bk)] >= 0).astype(np.uint8)
    bx_w = np.zeros((len(bk), 3), np.float32)
    bx_w[bv == 1] = world["ref_xw"][m9[0, : len(bk)][bv == 1]]
    pp = dict(fx=fx, fy=fy, cx=cx, cy=cy, front_xw=fx_w, front_obs=np.stack([fk["x"], fk["y"]], 1).astype(np.float32),
              front_inv_sigma2=inv[fk["octave"]], bird_xw=bx_w, bird_xc=bcam, bird_inv_sigma2=inv[bk["octave"]],
              Tcw0=world["Tcw0"])
    ap, outp, keepp = P.pose_args([pp], mode=cabi.FB_POSE_FRONT_BIRD, front_valid=[fv], bird_valid=[bv])
    outp["bird_outlier"][...] = 1  # mvBirdOutlier = vector<bool>(Nbird, true) of a fresh Frame (Frame.cc:356)
    t0 = time.perf_counter()
    call("orc_pose_opt", ap)
    tm["pose_opt"] = time.perf_counter() - t0
    return dict(fk=fk, fd=fd, bk=bk, bd=bd, bcam=bcam, m_front=m3[0], nm_front=int(out3["nmatches"][0]), m_bird=m9[0],
                nm_bird=int(out9["ninliers"][0]), Tcw=outp["Tcw"][0], ninliers=int(outp["ninliers"][0]),
                front_outlier=outp["front_outlier"][0], bird_outlier=outp["bird_outlier"][0], fv=fv, bv=bv)


class OracleChain:
    """CPU counterpart of fishbirdeyevisualslam_amd.track.TrackChain on oracle/track_oracle.cpp (host numpy arrays)."""

    def __init__(self, params, map_cap, bird_cap, use_lists=False):
        self.L = lib()
        self.params = params
        self.B = params.batch
        self.cap = params.orb.nfeatures + 8 * params.orb.nlevels
        self.frames = [C.c_void_p(), C.c_void_p()]
        for f in self.frames:
            assert self.L.orc_frame_create(C.byref(params), C.byref(f)) == 0
        self.k = 0
        self.use_lists = use_lists
        self.map_cap, self.bird_cap = map_cap, bird_cap
        self.targs = cabi.TrackArgs()
        self.keep = {}

    def close(self):
        for f in self.frames:
            if f:
                self.L.orc_frame_destroy(f)
        self.frames = []

    @property
    def cur(self):
        return self.frames[self.k & 1]

    @property
    def last(self):
        return self.frames[(self.k & 1) ^ 1]

    def set_map(self, M, MB, local_mp=None, local_mpb=None):
        self.keep["M"] = {k: np.ascontiguousarray(v).copy() for k, v in M.items()}
        self.keep["MB"] = {k: np.ascontiguousarray(v).copy() for k, v in MB.items()}
        cabi.fill(self.targs.map, stride=self.map_cap, **self.keep["M"])
        cabi.fill(self.targs.mpb, stride=self.bird_cap, **self.keep["MB"])
        cabi.fill(self.targs, wB=1.0, wF=1.0, gate_local_map=1)
        if self.use_lists:
            self.keep["lists"] = [np.ascontiguousarray(x).copy() for x in (local_mp[0], local_mp[1], local_mpb[0], local_mpb[1])]
            l = self.keep["lists"]
            cabi.fill(self.targs, d_local_mp=l[0], d_n_local_mp=l[1], d_local_mpb=l[2], d_n_local_mpb=l[3])

    def extract(self, front, bird, contour=None, mask=None):
        vp = lambda a: C.c_void_p(np.ascontiguousarray(a).ctypes.data) if a is not None else None
        self.keep["img"] = [np.ascontiguousarray(a) if a is not None else None for a in (front, bird, contour, mask)]
        f, b, c, m = self.keep["img"]
        assert self.L.orc_frame_extract(self.cur, vp(f), f.shape[2], vp(b), b.shape[2], vp(c), vp(m)) == 0

    def init_first(self, mp0, mpb0, Tcw0):
        a, b, t = (np.ascontiguousarray(x) for x in (mp0, mpb0, Tcw0))
        assert self.L.orc_frame_set_map_points(self.cur, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data)) == 0
        assert self.L.orc_frame_set_pose(self.cur, C.c_void_p(t.ctypes.data)) == 0
        self.k += 1

    def track(self, front, bird, contour, mask, delta):
        self.extract(front, bird, contour, mask)
        self.keep["delta"] = np.ascontiguousarray(delta, np.float32)
        cabi.fill(self.targs, d_delta=self.keep["delta"])
        assert self.L.orc_frame_track(self.cur, self.last, C.byref(self.targs)) == 0
        self.k += 1

    def track_stage_by_stage(self, front, bird, contour, mask, delta, delta_kf=None, mode="motion"):
        """track_modes(mode = "motion" / "motion+reference") with each "Discard outliers" loop as a call of its own.  Returns
        the frame's views in front of and behind each loop: "motion_pose", "motion_discard" [, "reference_pose",
        "reference_discard"]; the frame after TrackLocalMap is view() as usual."""
        self.extract(front, bird, contour, mask)
        self.keep["delta"] = np.ascontiguousarray(delta, np.float32)
        cabi.fill(self.targs, d_delta=self.keep["delta"])
        out = {}
        assert self.L.orc_frame_track_motion_model_ex(self.cur, self.last, C.byref(self.targs), 0) == 0
        out["motion_pose"] = self.view("cur")
        self.discard_outliers("PROJ_MATCHES", 20)
        out["motion_discard"] = self.view("cur")
        if "reference" in mode:
            self.keep["delta_kf"] = np.ascontiguousarray(delta_kf, np.float32)
            cabi.fill(self.targs, d_delta=self.keep["delta_kf"])
            assert self.L.orc_frame_track_reference_ex(self.cur, self.kf, self.last, C.byref(self.voc), C.byref(self.targs), 0) == 0
            cabi.fill(self.targs, d_delta=self.keep["delta"])
            out["reference_pose"] = self.view("cur")
            self.discard_outliers("BOW_MATCHES", 15)
            out["reference_discard"] = self.view("cur")
        assert self.L.orc_frame_track_local_map(self.cur, self.last, C.byref(self.targs)) == 0
        self.k += 1
        return out

    # ---- reference key frame ----
    def set_vocabulary(self, voc_arrays, L):
        self.keep["voc"] = {k: np.ascontiguousarray(v) for k, v in voc_arrays.items()}
        self.voc = cabi.Vocabulary()
        cabi.fill(self.voc, n_nodes=len(voc_arrays["weights"]), L=L, **self.keep["voc"])
        self.kf = C.c_void_p()
        assert self.L.orc_frame_create(C.byref(self.params), C.byref(self.kf)) == 0
        self.frames.append(self.kf)

    def make_keyframe(self, which="last"):
        f = self.last if which == "last" else self.cur
        assert self.L.orc_frame_copy(self.kf, f) == 0
        assert self.L.orc_frame_compute_bow(self.kf, C.byref(self.voc)) == 0

    def track_modes(self, front, bird, contour, mask, delta, delta_kf=None, mode="motion"):
        self.extract(front, bird, contour, mask)
        self.keep["delta"] = np.ascontiguousarray(delta, np.float32)
        cabi.fill(self.targs, d_delta=self.keep["delta"])
        if mode in ("bird", "bird_kf"):
            if mode == "bird_kf":
                self.keep["delta_kf"] = np.ascontiguousarray(delta_kf, np.float32)
                cabi.fill(self.targs, d_delta=self.keep["delta_kf"])
            src = self.kf if mode == "bird_kf" else self.last
            assert self.L.orc_frame_track_using_bird(self.cur, src, self.last, C.byref(self.targs)) == 0
            cabi.fill(self.targs, d_delta=self.keep["delta"])
            self.k += 1
            return
        if "motion" in mode:
            assert self.L.orc_frame_track_motion_model(self.cur, self.last, C.byref(self.targs)) == 0
        if "reference" in mode:
            self.keep["delta_kf"] = np.ascontiguousarray(delta_kf, np.float32)
            cabi.fill(self.targs, d_delta=self.keep["delta_kf"])
            assert self.L.orc_frame_track_reference(self.cur, self.kf, self.last, C.byref(self.voc), C.byref(self.targs)) == 0
            cabi.fill(self.targs, d_delta=self.keep["delta"])
        assert self.L.orc_frame_track_local_map(self.cur, self.last, C.byref(self.targs)) == 0
        self.k += 1

    # ---- the steps one by one, on the current frame (no k += 1: the caller builds the frame's associations itself) ----
    def set_map_points(self, mp, mpb=None):
        a = np.ascontiguousarray(mp, np.int32)
        b = np.ascontiguousarray(mpb, np.int32) if mpb is not None else None
        assert self.L.orc_frame_set_map_points(self.cur, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data) if b is not None else None) == 0

    def set_pose(self, Tcw):
        t = np.ascontiguousarray(Tcw, np.float32)
        assert self.L.orc_frame_set_pose(self.cur, C.c_void_p(t.ctypes.data)) == 0

    def pose_optimization(self, which=0):
        assert self.L.orc_frame_pose_optimization(self.cur, C.byref(self.targs), which) == 0

    def discard_outliers(self, src="PROJ_MATCHES", gate_min=0):
        assert self.L.orc_frame_discard_outliers(self.cur, C.byref(self.targs), cabi.FB_CNT[src], gate_min) == 0

    def search_local_points(self):
        assert self.L.orc_frame_search_local_points(self.cur, C.byref(self.targs)) == 0

    def drop_outliers(self, which="last"):
        f = self.last if which == "last" else self.cur
        assert self.L.orc_frame_drop_outliers(f) == 0

    def view(self, which="last"):
        f = self.last if which == "last" else (self.kf if which == "kf" else self.cur)
        v = cabi.FrameView()
        assert self.L.orc_frame_view(f, C.byref(v)) == 0
        B, cap = self.B, self.cap
        from fishbirdeyevisualslam_amd.track import VIEW_FIELDS
        out = {}
        for name, dt, shp in VIEW_FIELDS:
            shape = (B,) + tuple(cap if s == "cap" else s for s in shp)
            nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
            buf = (C.c_char * nbytes).from_address(getattr(v, name))
            out[name] = np.frombuffer(buf, dtype=dt).reshape(shape).copy()
        buf = (C.c_char * (cabi.FB_CNT_COUNT * B * 4)).from_address(v.counts)
        out["counts"] = np.frombuffer(buf, dtype=np.int32).reshape(cabi.FB_CNT_COUNT, B).copy()
        return out

    def stage_seconds(self, which="last"):
        f = self.last if which == "last" else self.cur
        s = (C.c_double * 8)()
        self.L.orc_frame_stage_seconds(f, s)
        return list(s)

    def bird_table_host(self):
        return self.keep["MB"]
