"""Device-resident per-frame hot path: extract(front) + extract(bird) + grids + front match (M3)
+ bird match (M9) + edge gather + PoseOptimizationWithBird, batched over B independent frame
pairs (one tracked sequence each), every stage through the C-ABI (*_dev entry points).

This is the order Tracking::GrabImageMonocularWithOdom -> TrackWithMotionModel runs them
(Tracking.cc:292-339, 1312-1385).  torch is used only for device memory and the stream.

Everything behind the extraction of a camera -- grid, matcher, edge gather, the counts and the predicted pose -- is ONE
launch (fb_frame_tail_front_dev / fb_frame_tail_bird_dev).  step() runs both on the pose stream, ahead of the pose
kernel, so that the extraction streams carry nothing but extraction; for that every buffer between extraction and pose
optimisation exists twice (set k & 1 belongs to step k).
"""
import ctypes as C

import numpy as np
import torch

from . import cabi, lib, check, synth
from .cabi import fill


def _vp(t):
    return C.c_void_p(t.data_ptr())


class FramePipeline:
    _streams = {}  # device -> (front, bird, pose) streams

    def __init__(self, batch, front_wh=(1280, 720), bird_wh=(512, 512), n_last=2000, n_ref=1000, device="cuda:0",
                 fx=500.0, fy=500.0, orb=None):
        self.L = lib()
        self.B = batch
        self.dev = torch.device(device)
        self.fw, self.fh = front_wh
        self.bw, self.bh = bird_wh
        self.fx, self.fy, self.cx, self.cy = fx, fy, self.fw / 2.0, self.fh / 2.0
        self.params = cabi.OrbParams(**(orb or synth.ORB_DEFAULT))
        self.L.fb_orb_capacity.restype = C.c_int
        self.cap = self.L.fb_orb_capacity(C.byref(self.params))
        self.orb_f, self.orb_b = C.c_void_p(), C.c_void_p()
        check(self.L.fb_orb_create(C.byref(self.params), C.byref(self.orb_f)), "fb_orb_create")
        check(self.L.fb_orb_create(C.byref(self.params), C.byref(self.orb_b)), "fb_orb_create")
        self.tables = cabi.OrbTables()
        check(self.L.fb_orb_get_tables(self.orb_f, C.byref(self.tables)), "fb_orb_get_tables")
        self.Tbc, self.Tcb = synth.extrinsics()
        B, cap, d = batch, self.cap, self.dev
        z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt, device=d)
        self.f_img, self.b_img = z(B, self.fh, self.fw), z(B, self.bh, self.bw)
        self.geom_f = fill(cabi.GridGeom(), **synth.front_grid_geom(self.fw, self.fh))
        self.geom_b = fill(cabi.GridGeom(), **synth.bird_grid_geom(self.bw, self.bh))
        # last frame / reference bird map points (filled by set_map)
        self.nl, self.nr = n_last, n_ref
        self.last = dict(valid=z(B, n_last), obs=z(B, n_last), xw=z(B, n_last, 3, dt=torch.float32), desc=z(B, n_last, 32),
                         octave=z(B, n_last, dt=torch.int32), angle=z(B, n_last, dt=torch.float32), n=z(B, dt=torch.int32))
        self.ref = dict(valid=z(B, n_ref), xw=z(B, n_ref, 3, dt=torch.float32), desc=z(B, n_ref, 32), n=z(B, dt=torch.int32))
        self.Tcw0 = z(B, 12, dt=torch.float32)
        # Everything a step writes exists TWICE (set k & 1 belongs to step k): what extraction writes and the tail reads
        # (key points, descriptors, counts), the tail's own outputs (cell lists, bird camera positions, matches) and the
        # pose stage (edge arrays, pose, outlier flags, counts).  The extraction of step k + 1 therefore never waits for
        # the tail or the pose kernel of step k; a set is reused two steps later, behind its evP.
        ncf, ncb = self.geom_f.cols * self.geom_f.rows + 1, self.geom_b.cols * self.geom_b.rows + 1
        self._sets = []
        for _ in range(2):
            self._sets.append(dict(
                f_kps=z(B, cap * 24), b_kps=z(B, cap * 24), f_desc=z(B, cap, 32), b_desc=z(B, cap, 32),
                f_n=z(B, dt=torch.int32), b_n=z(B, dt=torch.int32), f_cs=z(B, ncf, dt=torch.int32), b_cs=z(B, ncb, dt=torch.int32),
                f_ci=z(B, cap, dt=torch.int32), b_ci=z(B, cap, dt=torch.int32), b_cam=z(B, cap, 3, dt=torch.float32),
                m_front=z(B, cap, dt=torch.int32), nm_front=z(B, dt=torch.int32), m_bird=z(B, cap, dt=torch.int32), nm_bird=z(B, dt=torch.int32),
                Tcw=z(B, 12, dt=torch.float32), e_fxw=z(B, cap, 3, dt=torch.float32), e_fobs=z(B, cap, 2, dt=torch.float32),
                e_finf=z(B, cap, dt=torch.float32), e_fvalid=z(B, cap), e_fout=z(B, cap), e_bxw=z(B, cap, 3, dt=torch.float32),
                e_bxc=z(B, cap, 3, dt=torch.float32), e_binf=z(B, cap, dt=torch.float32), e_bvalid=z(B, cap), e_bout=z(B, cap),
                ninl=z(B, dt=torch.int32), e_nf=z(B, dt=torch.int32), e_nb=z(B, dt=torch.int32), evP=torch.cuda.Event(), pending=False))
        self._last = self._sets[0]  # the set of the last step (of build_world's extraction before the first one)
        self._k = 0  # step counter; results_host() reads the set of the last step
        # three streams: front extraction, bird extraction, tails + pose optimisation (latency-bound, overlap the next extraction)
        # (the three streams are shared by every pipeline of a device: the HIP runtime folds streams onto a few hardware queues,
        # and streams that land on one queue serialise -- a second pipeline with streams of its own measured 0.72 instead of
        # 0.47 ms per step at B = 8)
        key = str(d)
        if key not in FramePipeline._streams:
            FramePipeline._streams[key] = tuple(torch.cuda.Stream(device=d) for _ in range(3))
        self.sF, self.sB, self.sP = FramePipeline._streams[key]
        self.evF, self.evB = (torch.cuda.Event() for _ in range(2))
        self._inv_sigma2 = (C.c_float * cabi.FB_MAX_LEVELS)(*self.tables.inv_level_sigma2)
        self._Tcb12 = (C.c_float * 12)(*[float(x) for x in self.Tcb[:3, :4].reshape(12)])
        self._build_args()

    def close(self):
        for h in (self.orb_f, self.orb_b):
            if h:
                self.L.fb_orb_destroy(h)
        self.orb_f = self.orb_b = C.c_void_p()

    # the buffers of the last step's set under their plain names (pipe.f_kps, pipe.m_front, ...)
    def __getattr__(self, name):
        sets = self.__dict__.get("_last")
        if sets is not None and name in sets:
            return sets[name]
        raise AttributeError(name)

    # ---- argument structs (pointers are fixed for the lifetime of the pipeline), one of each per set ----
    def _build_args(self):
        B, cap, nl = self.B, self.cap, self.params.nlevels
        for S in self._sets:
            tf = cabi.FrameTailFrontArgs()
            a = tf.m3
            fill(a, batch=B, cur_stride=cap, last_stride=self.nl, n_cur=S["f_n"], cur_kps=S["f_kps"], cur_desc=S["f_desc"],
                 cur_cell_start=S["f_cs"], cur_cell_items=S["f_ci"], cur_blocked=None, cur_Tcw=self.Tcw0,
                 n_last=self.last["n"], last_valid=self.last["valid"], last_obs_pos=self.last["obs"], last_xw=self.last["xw"],
                 last_desc=self.last["desc"], last_octave=self.last["octave"], last_angle=self.last["angle"], th=15.0,
                 match_cur_to_last=S["m_front"], nmatches=S["nm_front"],
                 scale_factors=[self.tables.scale_factor[i] for i in range(cabi.FB_MAX_LEVELS)])
            fill(a.cam, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy, min_x=0.0, min_y=0.0, max_x=float(self.fw), max_y=float(self.fh))
            a.grid = self.geom_f
            fill(a.matcher, nnratio=0.9, check_orientation=1)  # ORBmatcher matcher(0.9,true), Tracking.cc:1339
            fill(tf.edge, inv_sigma2=[self.tables.inv_level_sigma2[i] for i in range(nl)], nlevels=nl)
            fill(tf, front_xw=S["e_fxw"], front_obs=S["e_fobs"], front_inv_sigma2=S["e_finf"], front_valid=S["e_fvalid"],
                 n_front=S["e_nf"], Tcw=S["Tcw"])   # Tcw = Tcw0: SetPose(prediction), Tracking.cc:1314-1320
            S["a_tail_front"] = tf
            tb = cabi.FrameTailBirdArgs()
            m = tb.m9
            fill(m, batch=B, cur_stride=cap, ref_stride=self.nr, n_cur=S["b_n"], cur_kps=S["b_kps"], cur_desc=S["b_desc"],
                 cur_cam_xyz=S["b_cam"], cur_cell_start=S["b_cs"], cur_cell_items=S["b_ci"], cur_Tcw=self.Tcw0,
                 n_ref=self.ref["n"], ref_valid=self.ref["valid"], ref_xw=self.ref["xw"], ref_desc=self.ref["desc"],
                 Tbc=[float(x) for x in self.Tbc[:3, :4].reshape(12)], bird_cols=self.bw, bird_rows=self.bh,
                 meter2pixel=synth.METER2PIXEL, rear_axle_to_center=synth.REAR_AXLE_TO_CENTER, window_size=10,
                 filter_size=0.05, match_cur_to_ref=S["m_bird"], ninliers=S["nm_bird"])
            m.grid = self.geom_b
            fill(m.matcher, nnratio=0.9, check_orientation=1)  # Tracking.cc:2008
            fill(tb.edge, inv_sigma2=[self.tables.inv_level_sigma2[i] for i in range(nl)], nlevels=nl)
            # m_bird starts at -1 (mvpMapPointsBird of a new frame) and e_bout at 1 (mvBirdOutlier of a fresh Frame,
            # Frame.cc:356): the tail kernel writes both over the whole stride
            fill(tb, pixel2meter=synth.PIXEL2METER, Tcb=list(self._Tcb12), bird_xw=S["e_bxw"], bird_xc=S["e_bxc"],
                 bird_inv_sigma2=S["e_binf"], bird_valid=S["e_bvalid"], bird_outlier=S["e_bout"], n_bird=S["e_nb"])
            S["a_tail_bird"] = tb
            p = cabi.PoseOptArgs()
            fill(p, batch=B, mode=cabi.FB_POSE_FRONT_BIRD, front_stride=cap, bird_stride=cap, fx=self.fx, fy=self.fy,
                 cx=self.cx, cy=self.cy, wF=1.0, wB=1.0, n_front=S["e_nf"], front_xw=S["e_fxw"], front_obs=S["e_fobs"],
                 front_inv_sigma2=S["e_finf"], front_valid=S["e_fvalid"], n_bird=S["e_nb"], bird_xw=S["e_bxw"],
                 bird_xc=S["e_bxc"], bird_inv_sigma2=S["e_binf"], bird_valid=S["e_bvalid"], bird_outlier=S["e_bout"],
                 Tcw=S["Tcw"], front_outlier=S["e_fout"], ninliers=S["ninl"])
            S["a_pose"] = p

    # ---- stages (S = the set they work on; by default the last step's) ----
    def extract(self, s, which="both", S=None):
        L, B, S = self.L, self.B, S or self._last
        if which in ("both", "front"):
            check(L.fb_orb_extract_batch_dev(self.orb_f, _vp(self.f_img), B, self.fw, self.fh, self.fw, C.c_size_t(self.fw * self.fh),
                                             _vp(S["f_kps"]), _vp(S["f_desc"]), _vp(S["f_n"]), s), "extract front")
        if which in ("both", "bird"):
            check(L.fb_orb_extract_batch_dev(self.orb_b, _vp(self.b_img), B, self.bw, self.bh, self.bw, C.c_size_t(self.bw * self.bh),
                                             _vp(S["b_kps"]), _vp(S["b_desc"]), _vp(S["b_n"]), s), "extract bird")

    def grids(self, s, which="both", S=None):
        """The cell lists and the bird camera positions alone (build_world; a step gets them from its tail launches)."""
        L, B, cap, S = self.L, self.B, self.cap, S or self._last
        if which in ("both", "front"):
            check(L.fb_grid_build_batch_dev(_vp(S["f_kps"]), _vp(S["f_n"]), B, cap, C.byref(self.geom_f), _vp(S["f_cs"]), _vp(S["f_ci"]), s), "grid front")
        if which in ("both", "bird"):
            check(L.fb_grid_build_batch_dev(_vp(S["b_kps"]), _vp(S["b_n"]), B, cap, C.byref(self.geom_b), _vp(S["b_cs"]), _vp(S["b_ci"]), s), "grid bird")
            check(L.fb_bird_keys_to_cam_dev(_vp(S["b_kps"]), _vp(S["b_n"]), B, cap, self.bw, self.bh, C.c_double(synth.PIXEL2METER),
                                            C.c_double(synth.REAR_AXLE_TO_CENTER), self._Tcb12, _vp(S["b_cam"]), s), "bird cam")

    def tail_front(self, s, S):
        """grid -> M3 -> front edges, e_nf, Tcw = Tcw0, in one launch"""
        check(self.L.fb_frame_tail_front_dev(C.byref(S["a_tail_front"]), s), "tail front")

    def tail_bird(self, s, S):
        """grid -> bird camera positions -> M9 on a fresh match array -> bird edges, e_nb, fresh outlier flags, in one launch"""
        check(self.L.fb_frame_tail_bird_dev(C.byref(S["a_tail_bird"]), s), "tail bird")

    def pose(self, s, S):
        check(self.L.fb_pose_opt_batch_dev(C.byref(S["a_pose"]), s), "pose opt")

    def step(self):
        """One pass of the hot path over the batch.  The front and the bird extraction run on their own streams; the two
        tail launches and the pose optimisation (one workgroup per frame, latency bound) run on a third one, where they
        overlap the next step's extraction.  Callers synchronise with torch.cuda.synchronize() / results_host()."""
        cur = torch.cuda.current_stream(self.dev)
        S = self._sets[self._k & 1]
        self.sF.wait_stream(cur)
        self.sB.wait_stream(cur)
        if S["pending"]:  # the tails and the pose kernel of two steps ago read this set (long done in steady state)
            self.sF.wait_event(S["evP"])
            self.sB.wait_event(S["evP"])
        with torch.cuda.stream(self.sF):
            self.extract(C.c_void_p(self.sF.cuda_stream), "front", S)
            self.evF.record(self.sF)  # extraction has finished reading the images
        with torch.cuda.stream(self.sB):
            self.extract(C.c_void_p(self.sB.cuda_stream), "bird", S)
            self.evB.record(self.sB)
        with torch.cuda.stream(self.sP):
            s = C.c_void_p(self.sP.cuda_stream)
            self.sP.wait_event(self.evF)
            self.tail_front(s, S)
            self.sP.wait_event(self.evB)
            self.tail_bird(s, S)
            self.pose(s, S)
            S["evP"].record(self.sP)
            S["pending"] = True
        self._last = S
        self._k += 1

    def step_serial(self):
        """The same pass on torch's current stream only (used by tests and for single-stream timing)."""
        cur = torch.cuda.current_stream(self.dev)
        s = C.c_void_p(cur.cuda_stream)
        S = self._sets[self._k & 1]
        if S["pending"]:  # a tail or pose kernel of an overlapped step() may still read this set on the pose stream
            cur.wait_event(S["evP"])
            S["pending"] = False
        self.extract(s, "both", S)
        self.tail_front(s, S)
        self.tail_bird(s, S)
        self.pose(s, S)
        self._last = S
        self._k += 1

    # ---- synthetic world (untimed setup) ----
    def set_images(self, front, bird):
        self.f_img.copy_(torch.from_numpy(np.ascontiguousarray(front)).to(self.dev))
        self.b_img.copy_(torch.from_numpy(np.ascontiguousarray(bird)).to(self.dev))

    def keypoints_host(self, which="front"):
        S = self._last
        kps, desc, n = (S["f_kps"], S["f_desc"], S["f_n"]) if which == "front" else (S["b_kps"], S["b_desc"], S["b_n"])
        n = n.cpu().numpy()
        k = kps.cpu().numpy().view(cabi.KP_DTYPE).reshape(self.B, self.cap)
        return [k[b, : n[b]].copy() for b in range(self.B)], [desc[b, : n[b]].cpu().numpy() for b in range(self.B)]

    def build_world(self, seed=5000, rot_sigma=0.002, t_sigma=0.01, outlier_frac=0.1):
        """From one extraction of the current images, synthesise the previous frame's map points and the
        reference bird map points so that matching and pose optimisation have real work."""
        torch.cuda.synchronize()
        s = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        self.extract(s)
        self.grids(s)
        torch.cuda.synchronize()
        fk, fd = self.keypoints_host("front")
        bk, bd = self.keypoints_host("bird")
        bcam = self._last["b_cam"].cpu().numpy()
        B, nl, nr = self.B, self.nl, self.nr
        world = []
        for b in range(B):
            g = synth.rng(seed + b)
            T = synth.random_pose(g)
            R, t = T[:3, :3], T[:3, 3]
            k, dsc = fk[b], fd[b]
            m = min(nl, len(k))
            sel = g.permutation(len(k))[:m]
            z = g.uniform(2.0, 30.0, m)
            u = k["x"][sel].astype(np.float64) + g.normal(0, 0.5, m)
            v = k["y"][sel].astype(np.float64) + g.normal(0, 0.5, m)
            bad = g.random(m) < outlier_frac
            u[bad] += g.uniform(-20, 20, int(bad.sum()))
            v[bad] += g.uniform(-20, 20, int(bad.sum()))
            Xc = np.stack([(u - self.cx) / self.fx * z, (v - self.cy) / self.fy * z, z], 1)
            Xw = (R.T @ (Xc - t).T).T
            w = dict(T_true=T, Tcw0=synth.to12(synth.perturb_pose(g, T, rot_sigma, t_sigma)), n_last=m,
                     last_xw=Xw.astype(np.float32), last_desc=synth.flip_bits(g, dsc[sel]),
                     last_octave=k["octave"][sel].astype(np.int32),
                     last_angle=np.mod(k["angle"][sel] + 7.0 + g.normal(0, 3.0, m), 360.0).astype(np.float32))
            kb, db = bk[b], bd[b]
            mb = min(nr, len(kb))
            selb = g.permutation(len(kb))[:mb]
            pc = bcam[b, selb].astype(np.float64) + g.normal(0, 0.005, (mb, 3))
            w.update(n_ref=mb, ref_xw=((R.T @ (pc - t).T).T).astype(np.float32), ref_desc=synth.flip_bits(g, db[selb], p=0.05))
            world.append(w)
        self.set_world(world)
        return world

    def set_world(self, world):
        B = self.B
        up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(self.dev)

        def stack(key, n, shape, dt):
            out = np.zeros((B, n) + shape, dt)
            for b, w in enumerate(world):
                out[b, : len(w[key])] = w[key]
            return out
        self.last["n"].copy_(up(np.array([w["n_last"] for w in world], np.int32)))
        self.last["xw"].copy_(up(stack("last_xw", self.nl, (3,), np.float32)))
        self.last["desc"].copy_(up(stack("last_desc", self.nl, (32,), np.uint8)))
        self.last["octave"].copy_(up(stack("last_octave", self.nl, (), np.int32)))
        self.last["angle"].copy_(up(stack("last_angle", self.nl, (), np.float32)))
        self.last["valid"].fill_(1)
        self.last["obs"].fill_(1)
        self.ref["n"].copy_(up(np.array([w["n_ref"] for w in world], np.int32)))
        self.ref["xw"].copy_(up(stack("ref_xw", self.nr, (3,), np.float32)))
        self.ref["desc"].copy_(up(stack("ref_desc", self.nr, (32,), np.uint8)))
        self.ref["valid"].fill_(1)
        self.Tcw0.copy_(up(np.stack([w["Tcw0"] for w in world])))
        torch.cuda.synchronize()

    def results_host(self):
        torch.cuda.synchronize()
        S = self._last
        return dict(n_front=S["f_n"].cpu().numpy(), n_bird=S["b_n"].cpu().numpy(), nm_front=S["nm_front"].cpu().numpy(),
                    nm_bird=S["nm_bird"].cpu().numpy(), ninliers=S["ninl"].cpu().numpy(), Tcw=S["Tcw"].cpu().numpy(),
                    front_outlier=S["e_fout"].cpu().numpy(), bird_outlier=S["e_bout"].cpu().numpy(),
                    m_front=S["m_front"].cpu().numpy(), m_bird=S["m_bird"].cpu().numpy())
