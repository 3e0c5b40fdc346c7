"""The covisibility graph on the device (fb_covis_* in include/fishbird.h) over torch tensors.

A key frame is a slot in [0, max_keyframes).  Nothing here synchronises except error_count(): results are device tensors
on the current stream.
"""
import ctypes as C

import numpy as np
import torch

from . import cabi, check, lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(cabi.ptr(t))


class DeviceMap:
    """fb_covis_map over device tensors.  Built from the dict of covis_problem.make_covis_problem or from keyword arrays."""
    FIELDS = (("kf_n", np.int32), ("kf_mp", np.int32), ("kf_octave", np.uint8), ("mp_bad", np.uint8), ("obs_mp", np.int32),
              ("obs_kf", np.int32), ("obs_idx", np.int32), ("kf_order", np.uint64))

    def __init__(self, arrays, device="cuda:0", obs_spare=0):
        """obs_spare: entries the three edge arrays hold beyond n_obs (tombstones), for process_new_keyframe to append to."""
        self.device = torch.device(device)
        self.K, self.S = np.asarray(arrays["kf_mp"]).shape
        self.n_mp, self.n_obs = len(arrays["mp_bad"]), len(arrays["obs_kf"])
        self.obs_cap = self.n_obs + int(obs_spare)
        self.t = {}
        for name, dt in self.FIELDS:
            a = np.ascontiguousarray(arrays[name], dt)
            if name.startswith("obs_") and obs_spare:
                a = np.concatenate([a, np.full(int(obs_spare), -1, dt)])
            if a.size == 0:
                a = np.zeros(1, dt)
            if dt == np.uint64:
                a = a.view(np.int64)
            self.t[name] = torch.from_numpy(a.copy()).to(self.device)
        self.c = cabi.CovisMap()
        cabi.fill(self.c, max_keyframes=self.K, kp_stride=self.S, n_mp=self.n_mp, n_obs=self.n_obs, **self.t)

    def grow(self, n):
        """The edge list is n entries longer (the block a process_new_keyframe wrote)."""
        assert self.n_obs + int(n) <= self.obs_cap
        self.n_obs += int(n)
        self.c.n_obs = self.n_obs

    def bytes(self):
        return b"".join(self.t[name].cpu().numpy().tobytes() for name, _ in self.FIELDS)


class DeviceTables:
    """fb_covis_kf_tables over device tensors, from the dict of covis_problem.make_window_problem.  The bird side is there when
    the dict has bobs_kf."""
    FRONT = (("kf_Tcw", np.float32), ("kf_bad", np.uint8), ("kf_init", np.uint8), ("kf_keys_un", None), ("inv_level_sigma2", np.float32),
             ("mp_xw", np.float32))
    BIRD = (("kf_nb", np.int32), ("kf_mpb", np.int32), ("kf_bird_octave", np.uint8), ("kf_bird_xc", np.float32), ("mpb_bad", np.uint8),
            ("mpb_xw", np.float32), ("bobs_mpb", np.int32), ("bobs_kf", np.int32), ("bobs_idx", np.int32))

    def __init__(self, arrays, device="cuda:0"):
        self.device = torch.device(device)
        self.bird = "bobs_kf" in arrays
        self.t = {}
        for name, dt in self.FRONT + (self.BIRD if self.bird else ()):
            a = np.ascontiguousarray(arrays[name]) if dt is None else np.ascontiguousarray(arrays[name], dt)
            if dt is None:
                a = a.view(np.uint8).reshape(-1)
            if a.size == 0:
                a = np.zeros(4, a.dtype)
            self.t[name] = torch.from_numpy(a.copy()).to(self.device)
        self.n_mpb = len(arrays["mpb_bad"]) if self.bird else 0
        self.n_bobs = len(arrays["bobs_kf"]) if self.bird else 0
        self.c = cabi.CovisKfTables()
        cabi.fill(self.c, n_levels=len(arrays["inv_level_sigma2"]), bird_stride=np.asarray(arrays["kf_mpb"]).shape[1] if self.bird else 0,
                  n_mpb=self.n_mpb, n_bobs=self.n_bobs, **self.t)


class DeviceBirdTables:
    """What the bird calls (update_bird_connections, local_bird_map) read, over device tensors: a fb_covis_map that carries
    max_keyframes and kf_order only, and a fb_covis_kf_tables with kf_nb, kf_mpb, mpb_bad, the bird edge list and, when given,
    kf_Tcw.  `arrays` holds kf_order, kf_nb, kf_mpb [K][bird_stride], mpb_bad, bobs_mpb, bobs_kf, bobs_idx (+ kf_Tcw)."""
    FIELDS = (("kf_nb", np.int32), ("kf_mpb", np.int32), ("mpb_bad", np.uint8), ("bobs_mpb", np.int32), ("bobs_kf", np.int32),
              ("bobs_idx", np.int32))

    def __init__(self, arrays, device="cuda:0"):
        self.device = torch.device(device)
        self.K, self.BS = np.asarray(arrays["kf_mpb"]).shape
        self.n_mpb, self.n_bobs = len(arrays["mpb_bad"]), len(arrays["bobs_kf"])
        self.t = {}
        for name, dt in self.FIELDS + ((("kf_Tcw", np.float32),) if "kf_Tcw" in arrays else ()):
            a = np.ascontiguousarray(arrays[name], dt)
            if a.size == 0:
                a = np.zeros(1, dt)
            self.t[name] = torch.from_numpy(a.copy()).to(self.device)
        self.order = torch.from_numpy(np.ascontiguousarray(arrays["kf_order"], np.uint64).view(np.int64).copy()).to(self.device)
        self.c = cabi.CovisKfTables()
        cabi.fill(self.c, bird_stride=self.BS, n_mpb=self.n_mpb, n_bobs=self.n_bobs, **self.t)
        self.map = cabi.CovisMap()
        cabi.fill(self.map, max_keyframes=self.K, kp_stride=1, kf_order=self.order)


WINDOW_ARRAYS = (("kf_slot", "cap_kf", 1, torch.int32), ("kf_fixed", "cap_kf", 1, torch.uint8), ("kf_Tcw", "cap_kf", 12, torch.float32),
                 ("mp_index", "cap_mp", 1, torch.int32), ("mp_xw", "cap_mp", 3, torch.float32), ("obs_kf", "cap_obs", 1, torch.int32),
                 ("obs_mp", "cap_obs", 1, torch.int32), ("obs_src", "cap_obs", 1, torch.int32), ("obs_uv", "cap_obs", 2, torch.float32),
                 ("obs_inv_sigma2", "cap_obs", 1, torch.float32), ("mpb_index", "cap_mpb", 1, torch.int32),
                 ("mpb_xw", "cap_mpb", 3, torch.float32), ("bobs_kf", "cap_bobs", 1, torch.int32), ("bobs_mpb", "cap_bobs", 1, torch.int32),
                 ("bobs_src", "cap_bobs", 1, torch.int32), ("bobs_xc", "cap_bobs", 3, torch.float32),
                 ("bobs_inv_sigma2", "cap_bobs", 1, torch.float32))


class CovisibilityGraph:
    def __init__(self, max_keyframes, device="cuda:0"):
        self.K = int(max_keyframes)
        self.device = torch.device(device)
        self.h = C.c_void_p()
        check(lib().fb_covis_create(self.K, C.byref(self.h)), "fb_covis_create")

    def close(self):
        if self.h:
            lib().fb_covis_destroy(self.h)
            self.h = C.c_void_p()

    def _i32(self, n, fill=0):
        return torch.full((max(int(n), 1),), fill, dtype=torch.int32, device=self.device)

    def _dev(self, x, dtype=torch.int32):
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x), dtype=dtype)
        return x.to(device=self.device, dtype=dtype).contiguous()

    def clear(self):
        check(lib().fb_covis_clear(self.h, _stream()), "fb_covis_clear")

    def reserve(self, n_mp, n_obs, n_q):
        check(lib().fb_covis_reserve(self.h, int(n_mp), int(n_obs), int(n_q)), "fb_covis_reserve")

    def set_order(self, kf_order):
        t = kf_order if torch.is_tensor(kf_order) else torch.from_numpy(np.ascontiguousarray(kf_order, np.uint64).view(np.int64).copy())
        t = t.to(self.device)
        check(lib().fb_covis_set_order_dev(self.h, _p(t), _stream()), "fb_covis_set_order_dev")
        self._keep = t

    def error_count(self):
        n = C.c_int32(0)
        check(lib().fb_covis_error_count(self.h, C.byref(n), _stream()), "fb_covis_error_count")
        return n.value

    def update_connections(self, m, slots):
        """KeyFrame::UpdateConnections of the listed slots, one after the other -> (n_counter, front) device int32 tensors."""
        slots = self._dev(slots).reshape(-1)
        n = slots.numel()
        n_counter, front = self._i32(n), self._i32(n, -1)
        check(lib().fb_covis_update_connections_dev(self.h, C.byref(m.c), n, _p(slots), _p(n_counter), _p(front), _stream()),
              "fb_covis_update_connections_dev")
        self._keep = (m, slots)
        return n_counter[:n], front[:n]

    def add_connection(self, slot, other, weight):
        check(lib().fb_covis_add_connection_dev(self.h, int(slot), int(other), int(weight), _stream()), "fb_covis_add_connection_dev")

    def erase_connection(self, slot, other):
        check(lib().fb_covis_erase_connection_dev(self.h, int(slot), int(other), _stream()), "fb_covis_erase_connection_dev")

    def erase_keyframe(self, slot):
        check(lib().fb_covis_erase_keyframe_dev(self.h, int(slot), _stream()), "fb_covis_erase_keyframe_dev")

    def ordered(self, slot):
        """GetVectorCovisibleKeyFrames + mvOrderedWeights -> (n[1], slots[K], weights[K])"""
        n, s, w = self._i32(1), self._i32(self.K, -1), self._i32(self.K, -1)
        check(lib().fb_covis_ordered_dev(self.h, int(slot), _p(n), _p(s), _p(w), _stream()), "fb_covis_ordered_dev")
        return n, s, w

    def by_weight(self, slot, w):
        n, s = self._i32(1), self._i32(self.K, -1)
        check(lib().fb_covis_by_weight_dev(self.h, int(slot), int(w), _p(n), _p(s), _stream()), "fb_covis_by_weight_dev")
        return n, s

    def connected(self, slot):
        n, s = self._i32(1), self._i32(self.K, -1)
        check(lib().fb_covis_connected_dev(self.h, int(slot), _p(n), _p(s), _stream()), "fb_covis_connected_dev")
        return n, s

    def weight(self, slot, other):
        w = self._i32(1)
        check(lib().fb_covis_weight_dev(self.h, int(slot), int(other), _p(w), _stream()), "fb_covis_weight_dev")
        return w

    def kfdb_rows(self, slots=None, out=None):
        """[K][FB_KFDB_COVIS] rows for fb_kfdb_query_args.covis (slots=None: every row)"""
        if out is None:
            out = torch.full((self.K, cabi.FB_KFDB_COVIS), -1, dtype=torch.int32, device=self.device)
        s = None if slots is None else self._dev(slots).reshape(-1)
        check(lib().fb_covis_kfdb_rows_dev(self.h, 0 if s is None else s.numel(), _p(s), _p(out), _stream()), "fb_covis_kfdb_rows_dev")
        self._keep = s
        return out

    def keyframe_culling(self, m, cur_slot, id0_slot=-1, not_erase=None):
        """LocalMapping::KeyFrameCulling -> dict of device tensors: n[1], slots, n_redundant, n_mps, culled [K], mp_bad_after [n_mp]"""
        ne = None if not_erase is None else self._dev(not_erase, torch.uint8)
        out = dict(n=self._i32(1), slots=self._i32(self.K, -1), n_redundant=self._i32(self.K), n_mps=self._i32(self.K),
                   culled=torch.zeros(self.K, dtype=torch.uint8, device=self.device),
                   mp_bad_after=torch.zeros(max(m.n_mp, 1), dtype=torch.uint8, device=self.device))
        check(lib().fb_covis_keyframe_culling_dev(self.h, C.byref(m.c), int(cur_slot), int(id0_slot), _p(ne), _p(out["n"]),
                                                  _p(out["slots"]), _p(out["n_redundant"]), _p(out["n_mps"]), _p(out["culled"]),
                                                  _p(out["mp_bad_after"]), _stream()), "fb_covis_keyframe_culling_dev")
        self._keep = (m, ne)
        return out

    # ---- the local-BA window -------------------------------------------------------------------------------------------------
    def reserve_window(self, n_mp, n_obs, n_mpb=0, n_bobs=0):
        check(lib().fb_covis_reserve_window(self.h, int(n_mp), int(n_obs), int(n_mpb), int(n_bobs)), "fb_covis_reserve_window")

    def window_arrays(self, caps, guard=0, fill=-1):
        """Device arrays of a fb_covis_window with the given capacities (cap_kf, cap_mp, cap_obs, cap_mpb, cap_bobs), each followed
        by `guard` extra elements the library never sees -> (dict of tensors, cabi.CovisWindow)."""
        w = {}
        for name, cap, width, dt in WINDOW_ARRAYS:
            w[name] = torch.full(((int(caps[cap]) + guard) * width + (0 if guard else 1),), fill if dt != torch.uint8 else 0xEE, dtype=dt,
                                 device=self.device)
        w["header"] = torch.full((8,), -1, dtype=torch.int32, device=self.device)
        c = cabi.CovisWindow()
        cabi.fill(c, **{k: int(v) for k, v in caps.items()}, **w)
        return w, c

    def local_window(self, m, t, cur_slot, with_bird=True, caps=None, guard=0):
        """The window of cur_slot -> dict of device tensors (the fb_covis_window arrays at their capacities, "header" int32[7])
        with the struct under "c".  Default capacities hold any window of the map.  Nothing synchronises."""
        bird = bool(with_bird) and t.bird
        if caps is None:
            caps = dict(cap_kf=self.K, cap_mp=m.n_mp, cap_obs=m.n_obs, cap_mpb=t.n_mpb if bird else 0, cap_bobs=t.n_bobs if bird else 0)
        w, c = self.window_arrays(caps, guard)
        check(lib().fb_covis_local_window_dev(self.h, C.byref(m.c), C.byref(t.c), int(cur_slot), 1 if with_bird else 0, C.byref(c), _stream()),
              "fb_covis_local_window_dev")
        w["c"], w["caps"] = c, dict(caps)
        self._win_cap_kf = int(caps["cap_kf"])
        self._keep = (m, t, w)
        return w

    def window_header(self):
        """The one synchronisation, for the last local_window -> (rc, header fields as a dict, kf_slot, kf_fixed as numpy arrays of
        n_local + n_fixed entries, or of cap_kf if that is less)"""
        n = min(self._win_cap_kf, self.K)
        h = cabi.CovisWindowHeader()
        slots, fixed = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), 7, np.uint8)
        rc = lib().fb_covis_local_window_header(self.h, C.byref(h), C.c_void_p(slots.ctypes.data), C.c_void_p(fixed.ctypes.data), _stream())
        hd = {k: getattr(h, k) for k, _ in cabi.CovisWindowHeader._fields_}
        n_kf = min(hd["n_local"] + hd["n_fixed"], n)
        return rc, hd, slots[:n_kf], fixed[:n_kf]

    def window_scatter(self, m, t, w, obs_outlier=None, bobs_outlier=None):
        """Optimised poses / points back into the tables of t; -> (n_erase int32[2], erase [cap_obs][4], berase [cap_bobs][4])"""
        n = torch.zeros(2, dtype=torch.int32, device=self.device)
        er = torch.full((max(w["caps"]["cap_obs"], 1), 4), -1, dtype=torch.int32, device=self.device)
        ber = torch.full((max(w["caps"]["cap_bobs"], 1), 4), -1, dtype=torch.int32, device=self.device)
        check(lib().fb_covis_window_scatter_dev(self.h, C.byref(m.c), C.byref(t.c), C.byref(w["c"]), _p(obs_outlier), _p(bobs_outlier),
                                                _p(n), _p(er), _p(ber), _stream()), "fb_covis_window_scatter_dev")
        self._keep = (m, t, w, obs_outlier, bobs_outlier)
        return n, er, ber

    # ---- the spanning tree -------------------------------------------------------------------------------------------------------
    def tree_set(self, parent=None, linked=None, first=None):
        p = None if parent is None else self._dev(parent)
        l = None if linked is None else self._dev(linked, torch.uint8)
        f = None if first is None else self._dev(first, torch.uint8)
        check(lib().fb_covis_tree_set_dev(self.h, _p(p), _p(l), _p(f), _stream()), "fb_covis_tree_set_dev")
        self._keep = (p, l, f)

    def tree_get(self):
        """(parent int32[K], linked uint8[K], first uint8[K]) device tensors"""
        p, l, f = self._i32(self.K, -7), torch.zeros(self.K, dtype=torch.uint8, device=self.device), torch.zeros(self.K, dtype=torch.uint8, device=self.device)
        check(lib().fb_covis_tree_get_dev(self.h, _p(p), _p(l), _p(f), _stream()), "fb_covis_tree_get_dev")
        return p, l, f

    def change_parent(self, slot, parent):
        check(lib().fb_covis_change_parent_dev(self.h, int(slot), int(parent), _stream()), "fb_covis_change_parent_dev")

    def erase_child(self, parent, slot):
        check(lib().fb_covis_erase_child_dev(self.h, int(parent), int(slot), _stream()), "fb_covis_erase_child_dev")

    def children(self, slot):
        n, s = self._i32(1), self._i32(self.K, -1)
        check(lib().fb_covis_children_dev(self.h, int(slot), _p(n), _p(s), _stream()), "fb_covis_children_dev")
        return n, s

    def parent(self, slot):
        p = self._i32(1, -7)
        check(lib().fb_covis_parent_dev(self.h, int(slot), _p(p), _stream()), "fb_covis_parent_dev")
        return p

    def first_connection(self, slots, n_counter, front, id0_slot=-1, now_state4=False, kf_frame_id=None, kf_in_map=None):
        """KeyFrame.cc:665-690 on the outputs of update_connections(m, slots)"""
        slots = self._dev(slots).reshape(-1)
        fid = None if kf_frame_id is None else self._dev(kf_frame_id)
        inm = None if kf_in_map is None else self._dev(kf_in_map, torch.uint8)
        check(lib().fb_covis_first_connection_dev(self.h, slots.numel(), _p(slots), _p(n_counter), _p(front), int(id0_slot),
                                                  1 if now_state4 else 0, _p(fid), _p(inm), _stream()), "fb_covis_first_connection_dev")
        self._keep = (slots, n_counter, front, fid, inm)

    def tree_erase_keyframe(self, slot, kf_bad):
        b = self._dev(kf_bad, torch.uint8)
        check(lib().fb_covis_tree_erase_keyframe_dev(self.h, int(slot), _p(b), _stream()), "fb_covis_tree_erase_keyframe_dev")
        self._keep = b

    # ---- Tracking::UpdateLocalMap --------------------------------------------------------------------------------------------------
    def reserve_local_map(self, n_mp, n_obs, n_q=0, batch=1, with_window=False):
        check(lib().fb_covis_reserve_local_map(self.h, int(n_mp), int(n_obs), int(n_q), int(batch), 1 if with_window else 0),
              "fb_covis_reserve_local_map")

    def local_map_arrays(self, n, map_point, kf_bad, cap_kf, cap_mp, local_kf=None, ref_kf=None, gate_row=None, gate_min=0, guard=0):
        """Device arrays of a fb_local_map_args for frames n [B], map_point [B][S]; local_kf: per sequence the list that comes in.
        Each output array is followed by `guard` elements the library never sees.  -> (dict of tensors, cabi.LocalMapArgs)"""
        mp = self._dev(map_point)
        B, S = mp.shape
        t = dict(d_n=self._dev(n).reshape(-1), d_map_point=mp.clone(), d_kf_bad=self._dev(kf_bad, torch.uint8))
        t["d_local_kf"] = torch.full((B * cap_kf + guard + 1,), -5, dtype=torch.int32, device=self.device)
        t["d_n_local_kf"] = self._i32(B)
        for b, l in enumerate(local_kf or ()):
            t["d_local_kf"][b * cap_kf:b * cap_kf + min(len(l), cap_kf)] = self._dev(list(l)[:cap_kf]) if len(l) and cap_kf else self._i32(0)[:0]
            t["d_n_local_kf"][b] = len(l)
        t["d_local_mp"] = torch.full((B * cap_mp + guard + 1,), -5, dtype=torch.int32, device=self.device)
        t["d_n_local_mp"] = self._i32(B, -5)
        t["d_ref_kf"] = self._i32(B, -1) if ref_kf is None else self._dev(ref_kf).reshape(-1).clone()
        t["d_n_voters"], t["d_overflow"] = self._i32(B, -5), self._i32(B, -5)
        if gate_row is not None:
            t["d_gate_row"] = self._dev(gate_row).reshape(-1)
        a = cabi.LocalMapArgs()
        cabi.fill(a, batch=B, kp_stride=S, cap_kf=int(cap_kf), cap_mp=int(cap_mp), gate_min=int(gate_min), reuse_index=0, **t)
        return t, a

    def local_map(self, m, a, reuse_index=False):
        """Tracking::UpdateLocalMap for the arrays of local_map_arrays; enqueues only"""
        a.reuse_index = 1 if reuse_index else 0
        check(lib().fb_covis_local_map_dev(self.h, C.byref(m.c), C.byref(a), _stream()), "fb_covis_local_map_dev")
        self._keep = (m, a)

    # ---- map correction: CorrectLoop and the tail of RunGlobalBundleAdjustment -------------------------------------------------
    def reserve_correct_loop(self, n_mp, n_obs, n_q=0, n_mpb=0, bird_stride=0):
        check(lib().fb_covis_reserve_correct_loop(self.h, int(n_mp), int(n_obs), int(n_q), int(n_mpb), int(bird_stride)),
              "fb_covis_reserve_correct_loop")

    def _filled(self, x, dtype, n, fill=0):
        """x (n elements) as a flat device tensor of at least one element"""
        out = torch.full((max(n, 1),), fill, dtype=dtype, device=self.device)
        if x is not None and n:
            out[:n] = self._dev(x, dtype).reshape(-1)
        return out

    def correct_loop_arrays(self, m, scale_factors, mp_ref_kf, mp_normal, mp_min_dist, mp_max_dist, with_set_scw=False, guard=0):
        """Device arrays of a fb_correct_loop_args for the map m: the in/out MapPoint members and the outputs; with_set_scw:
        also d_set_Scw [K][12] (the corrected Sim3 of every set member for SearchAndFuse), followed by `guard` floats.
        -> (dict of tensors, cabi.CorrectLoopArgs)"""
        n = m.n_mp
        t = dict(scale_factors=self._dev(scale_factors, torch.float32).reshape(-1), mp_ref_kf=self._filled(mp_ref_kf, torch.int32, n, -1),
                 mp_normal=self._filled(mp_normal, torch.float32, 3 * n), mp_min_dist=self._filled(mp_min_dist, torch.float32, n),
                 mp_max_dist=self._filled(mp_max_dist, torch.float32, n), d_mp_corrected_ref=self._i32(n, -1), d_n_set=self._i32(1),
                 d_set_slots=self._i32(self.K, -1))
        if with_set_scw:
            t["d_set_Scw"] = torch.full((12 * self.K + guard,), 7.0, dtype=torch.float32, device=self.device)
        a = cabi.CorrectLoopArgs()
        cabi.fill(a, reuse_index=0, **t)
        return t, a

    def correct_loop(self, m, t, a, cur_slot, q, tr, s, reuse_index=False):
        """LoopClosing::CorrectLoop (:438-541) with mg2oScw = (q xyzw, tr, s) on the tables t and the arrays of
        correct_loop_arrays; the graph row of cur_slot must be current.  Enqueues only."""
        cabi.fill(a, q=[float(x) for x in q], t=[float(x) for x in tr], s=float(s), cur_slot=int(cur_slot), reuse_index=1 if reuse_index else 0)
        check(lib().fb_covis_correct_loop_dev(self.h, C.byref(m.c), C.byref(t.c), C.byref(a), _stream()), "fb_covis_correct_loop_dev")
        self._keep = (m, t, a)

    def propagate_gba_arrays(self, m, t, origins, kf_gba, kf_Tcw_gba, kf_Tcw_bef, mp_gba, mp_pos_gba, mp_ref_kf, mpb_gba=None,
                             mpb_pos_gba=None, mpb_ref_kf=None):
        """Device arrays of a fb_propagate_gba_args -> (dict of tensors, cabi.PropagateGbaArgs)"""
        K, n, nb = self.K, m.n_mp, t.n_mpb
        origins = self._dev(origins).reshape(-1)
        d = dict(origins=origins if origins.numel() else self._i32(1), kf_gba=self._filled(kf_gba, torch.uint8, K),
                 kf_Tcw_gba=self._filled(kf_Tcw_gba, torch.float32, 12 * K), kf_Tcw_bef=self._filled(kf_Tcw_bef, torch.float32, 12 * K),
                 mp_gba=self._filled(mp_gba, torch.uint8, n), mp_pos_gba=self._filled(mp_pos_gba, torch.float32, 3 * n),
                 mp_ref_kf=self._filled(mp_ref_kf, torch.int32, n, -1), d_reached=self._filled(None, torch.uint8, K))
        if t.bird:
            d.update(mpb_gba=self._filled(mpb_gba, torch.uint8, nb), mpb_pos_gba=self._filled(mpb_pos_gba, torch.float32, 3 * nb),
                     mpb_ref_kf=self._filled(mpb_ref_kf, torch.int32, nb, -1))
        a = cabi.PropagateGbaArgs()
        cabi.fill(a, n_origins=int(origins.numel()), **d)
        return d, a

    def propagate_gba(self, m, t, a):
        """The map update that ends RunGlobalBundleAdjustment (:714-825) over the handle's spanning tree.  Enqueues only."""
        check(lib().fb_covis_propagate_gba_dev(self.h, C.byref(m.c), C.byref(t.c), C.byref(a), _stream()), "fb_covis_propagate_gba_dev")
        self._keep = (m, t, a)

    # ---- the per-point side of LocalMapping: refresh, ProcessNewKeyFrame, MapPointCulling ----------------------------------------
    def reserve_refresh_points(self, n_mp, n_obs, n_q=0):
        check(lib().fb_covis_reserve_refresh_points(self.h, int(n_mp), int(n_obs), int(n_q)), "fb_covis_reserve_refresh_points")

    def refresh_arrays(self, m, kf_Tcw, kf_bad, kf_desc, scale_factors, mp_xw, mp_ref_kf, mp_normal, mp_min_dist, mp_max_dist, mp_desc,
                       guard=0):
        """Device arrays of a fb_point_refresh_args for the map m; the four in/out arrays are followed by `guard` rows the
        library never sees -> (dict of tensors, cabi.PointRefreshArgs)"""
        n, K, S = m.n_mp, self.K, m.S

        def padded(x, dtype, width, fill):
            out = torch.full(((max(n, 1) + guard) * width,), fill, dtype=dtype, device=self.device)
            if n:
                out[:n * width] = self._dev(x, dtype).reshape(-1)
            return out
        t = dict(kf_Tcw=self._filled(kf_Tcw, torch.float32, 12 * K), kf_bad=self._filled(kf_bad, torch.uint8, K),
                 kf_desc=self._filled(kf_desc, torch.uint8, 32 * K * S), scale_factors=self._dev(scale_factors, torch.float32).reshape(-1),
                 mp_xw=self._filled(mp_xw, torch.float32, 3 * n), mp_ref_kf=self._filled(mp_ref_kf, torch.int32, n, -1),
                 mp_normal=padded(mp_normal, torch.float32, 3, 7.0), mp_min_dist=padded(mp_min_dist, torch.float32, 1, 7.0),
                 mp_max_dist=padded(mp_max_dist, torch.float32, 1, 7.0), mp_desc=padded(mp_desc, torch.uint8, 32, 0xEE))
        a = cabi.PointRefreshArgs()
        cabi.fill(a, n_levels=int(t["scale_factors"].numel()), what=cabi.FB_REFRESH_NORMAL_DEPTH | cabi.FB_REFRESH_DESCRIPTOR, **t)
        return t, a

    def refresh_points(self, m, a, points=None, n_points=None, what=None, reuse_index=False):
        """UpdateNormalAndDepth and / or ComputeDistinctiveDescriptors for the listed points (None: every point; n_points: a
        device int32[1] that holds the list's length) on the arrays of refresh_arrays.  Enqueues only."""
        lst = None if points is None else self._dev(points).reshape(-1)
        keep = lst
        if lst is not None and lst.numel() == 0:
            lst = self._i32(1)
        cabi.fill(a, d_list=lst, d_n_list=n_points, n_list=0 if keep is None else int(keep.numel()),
                  reuse_index=1 if reuse_index else 0)
        if what is not None:
            a.what = int(what)
        check(lib().fb_covis_refresh_points_dev(self.h, C.byref(m.c), C.byref(a), _stream()), "fb_covis_refresh_points_dev")
        self._keep = (m, a, lst, n_points)

    def recent_list(self, cap, points=()):
        """mlpRecentAddedMapPoints as device arrays -> (d_recent int32[cap], d_n_recent int32[1])"""
        r, n = self._i32(cap, -1), self._i32(1)
        pts = list(points)
        if pts:
            r[:len(pts)] = self._dev(pts)
            n[0] = len(pts)
        return r, n

    def process_new_keyframe(self, m, refresh, slot, n_features, recent, n_recent):
        """The point loop of LocalMapping::ProcessNewKeyFrame for the key frame in `slot` of m (a DeviceMap with obs_spare) on
        the arrays of refresh_arrays and recent_list -> d_n_added int32[1].  The edge list of m is n_features longer
        afterwards (m.grow); UpdateConnections and the first connection are the caller's next calls.  Enqueues only."""
        a = cabi.NewKeyframeArgs()
        n_added = self._i32(1, -1)
        cabi.fill(a, slot=int(slot), n_features=int(n_features), obs_cap=int(m.obs_cap), obs_mp=m.t["obs_mp"], obs_kf=m.t["obs_kf"],
                  obs_idx=m.t["obs_idx"], d_n_added=n_added, recent_cap=int(recent.numel()), d_recent=recent, d_n_recent=n_recent)
        a.refresh = refresh
        check(lib().fb_covis_process_new_keyframe_dev(self.h, C.byref(m.c), C.byref(a), _stream()), "fb_covis_process_new_keyframe_dev")
        m.grow(n_features)
        self._keep = (m, a, refresh, recent, n_recent, n_added)
        return n_added

    def map_point_culling(self, m, cur_kf_id, mp_first_kf_id, mp_found, mp_visible, recent, n_recent, n_th_obs=2, erased_cap=None):
        """LocalMapping::MapPointCulling over the recent list, editing kf_mp, mp_bad and obs_kf of m -> dict of device tensors:
        n_culled[1], culled[cap], n_erased[1], erased[erased_cap][4] rows (kf slot, point, feature, edge).  Enqueues only."""
        cap = int(recent.numel())
        ecap = m.n_obs if erased_cap is None else int(erased_cap)
        out = dict(n_culled=self._i32(1, -1), culled=self._i32(cap, -1), n_erased=self._i32(1, -1),
                   erased=torch.full((max(ecap, 1), 4), -1, dtype=torch.int32, device=self.device))
        t = (self._dev(mp_first_kf_id), self._dev(mp_found), self._dev(mp_visible))
        a = cabi.MapPointCullingArgs()
        cabi.fill(a, cur_kf_id=int(cur_kf_id), n_th_obs=int(n_th_obs), mp_first_kf_id=t[0], mp_found=t[1], mp_visible=t[2],
                  recent_cap=cap, d_recent=recent, d_n_recent=n_recent, kf_mp=m.t["kf_mp"], mp_bad=m.t["mp_bad"], obs_kf=m.t["obs_kf"],
                  d_n_culled=out["n_culled"], d_culled=out["culled"], d_n_erased=out["n_erased"], erased_cap=ecap, d_erased=out["erased"])
        check(lib().fb_covis_map_point_culling_dev(self.h, C.byref(m.c), C.byref(a), _stream()), "fb_covis_map_point_culling_dev")
        self._keep = (m, a, t, recent, n_recent, out)
        return out

    # ---- MapPoint::Replace and the loop fusion of CorrectLoop ---------------------------------------------------------------------
    def reserve_replace_points(self, n_mp, n_obs, n_q=0):
        check(lib().fb_covis_reserve_replace_points(self.h, int(n_mp), int(n_obs), int(n_q)), "fb_covis_reserve_replace_points")

    def reserve_loop_fuse(self, n_mp, n_obs, n_features, n_q=0):
        check(lib().fb_covis_reserve_loop_fuse(self.h, int(n_mp), int(n_obs), int(n_q), int(n_features)), "fb_covis_reserve_loop_fuse")

    def point_fuse_arrays(self, m, kf_bad, kf_desc, mp_desc, mp_found, mp_visible, mp_replaced=None, replaced_cap=0, guard=0):
        """Device arrays of a fb_point_fuse_arrays for the map m (kf_mp, mp_bad, obs_mp and obs_kf are m's own tensors); the
        per-point in/out arrays and d_replaced are followed by `guard` rows the library never sees
        -> (dict of tensors, cabi.PointFuseArrays)"""
        n, K, S = m.n_mp, self.K, m.S

        def padded(x, dtype, rows, width, fill):
            out = torch.full(((max(rows, 1) + guard) * width,), fill, dtype=dtype, device=self.device)
            if x is not None and rows:
                out[:rows * width] = self._dev(x, dtype).reshape(-1)
            return out
        t = dict(kf_bad=self._filled(kf_bad, torch.uint8, K), kf_desc=self._filled(kf_desc, torch.uint8, 32 * K * S),
                 mp_desc=padded(mp_desc, torch.uint8, n, 32, 0xEE), mp_found=padded(mp_found, torch.int32, n, 1, -5),
                 mp_visible=padded(mp_visible, torch.int32, n, 1, -5),
                 mp_replaced=padded(np.full(n, -1, np.int32) if mp_replaced is None else mp_replaced, torch.int32, n, 1, -5),
                 d_n_replaced=self._i32(1, -1), d_replaced=padded(None, torch.int32, int(replaced_cap), 2, -5))
        a = cabi.PointFuseArrays()
        cabi.fill(a, kf_mp=m.t["kf_mp"], mp_bad=m.t["mp_bad"], obs_mp=m.t["obs_mp"], obs_kf=m.t["obs_kf"], replaced_cap=int(replaced_cap), **t)
        return t, a

    def replace_points(self, m, fuse, pairs_from, pairs_to, n_pairs=None):
        """from[i]->Replace(to[i]) (MapPoint.cc:177-215) for the listed pairs, one after another, on m and the arrays of
        point_fuse_arrays; from[i] < 0 is skipped; n_pairs: a device int32[1] that holds the list's length.  The rows that
        took effect land in fuse's d_replaced / d_n_replaced.  Enqueues only."""
        f, t = self._dev(pairs_from).reshape(-1), self._dev(pairs_to).reshape(-1)
        assert f.numel() == t.numel()
        n = int(f.numel())
        if n == 0:
            f, t = self._i32(1, -1), self._i32(1, -1)
        a = cabi.ReplacePointsArgs()
        cabi.fill(a, n_pairs=n, d_n_pairs=n_pairs, d_from=f, d_to=t)
        a.map = fuse
        check(lib().fb_covis_replace_points_dev(self.h, C.byref(m.c), C.byref(a), _stream()), "fb_covis_replace_points_dev")
        self._keep = (m, a, fuse, f, t, n_pairs)

    def loop_fuse(self, m, fuse, cur_slot, matched, added_cap=None, guard=0):
        """The loop fusion of LoopClosing::CorrectLoop (:545-560) for the key frame in cur_slot of m (a DeviceMap with obs_spare)
        and mvpCurrentMatchedPoints as point indices (-1 = NULL) -> (d_n_added int32[1], d_added [added_cap][4] rows of
        key frame slot, point, feature, edge).  The edge list of m is len(matched) longer afterwards (m.grow).  Enqueues only."""
        mt = self._dev(matched).reshape(-1)
        nf = int(mt.numel())
        cap = nf if added_cap is None else int(added_cap)
        n_added = self._i32(1, -1)
        added = torch.full(((max(cap, 1) + guard) * 4,), -5, dtype=torch.int32, device=self.device)
        a = cabi.LoopFuseArgs()
        cabi.fill(a, cur_slot=int(cur_slot), n_features=nf, d_matched=mt if nf else self._i32(1, -1), obs_cap=int(m.obs_cap),
                  obs_idx=m.t["obs_idx"], d_n_added=n_added, added_cap=cap, d_added=added)
        a.map = fuse
        check(lib().fb_covis_loop_fuse_dev(self.h, C.byref(m.c), C.byref(a), _stream()), "fb_covis_loop_fuse_dev")
        m.grow(nf)
        self._keep = (m, a, fuse, mt, n_added, added)
        return n_added, added

    def search_and_fuse(self, m, fuse, target, set_slots, set_scw, loop_mp, kf_keys_un, mp_xw, mp_normal, mp_min_dist, mp_max_dist, th=4.0,
                        added_cap=None, guard=0):
        """LoopClosing::SearchAndFuse (:616-642) for the key frames set_slots (a list or a device tensor, in the order given)
        with their Scw rows set_scw [n_set][12] and mvpLoopMapPoints loop_mp as point indices; target: a cabi.KfTarget whose
        cam, grid, scale tables and n_levels are read.  -> (d_n_fused [n_set], d_n_added [1], d_added rows).  The edge list
        of m is n_set * kp_stride longer afterwards (m.grow).  Enqueues only."""
        slots = self._dev(set_slots).reshape(-1)
        n_set, n = int(slots.numel()), m.n_mp
        lp = self._dev(loop_mp).reshape(-1)
        n_loop = int(lp.numel())
        kp = kf_keys_un if torch.is_tensor(kf_keys_un) else torch.from_numpy(np.ascontiguousarray(kf_keys_un).view(np.uint8).reshape(-1).copy()).to(self.device)
        cap = n_set * m.S if added_cap is None else int(added_cap)
        t = dict(d_set_slots=slots if n_set else self._i32(1), d_set_Scw=self._filled(set_scw, torch.float32, 12 * n_set),
                 d_loop_mp=lp if n_loop else self._i32(1), kf_keys_un=kp, mp_xw=self._filled(mp_xw, torch.float32, 3 * n),
                 mp_normal=self._filled(mp_normal, torch.float32, 3 * n), mp_min_dist=self._filled(mp_min_dist, torch.float32, n),
                 mp_max_dist=self._filled(mp_max_dist, torch.float32, n), d_n_fused=self._i32(n_set + guard, -5), d_n_added=self._i32(1, -1),
                 d_added=torch.full(((max(cap, 1) + guard) * 4,), -5, dtype=torch.int32, device=self.device))
        a = cabi.SearchAndFuseArgs()
        cabi.fill(a, n_set=n_set, n_loop=n_loop, th=float(th), log_scale_factor=target.log_scale_factor, n_levels=target.n_levels,
                  obs_cap=int(m.obs_cap), obs_idx=m.t["obs_idx"], added_cap=cap, **t)
        a.cam, a.grid, a.scale_factors, a.inv_level_sigma2, a.map = target.cam, target.grid, target.scale_factors, target.inv_level_sigma2, fuse
        check(lib().fb_covis_search_and_fuse_dev(self.h, C.byref(m.c), C.byref(a), _stream()), "fb_covis_search_and_fuse_dev")
        m.grow(n_set * m.S)
        self._keep = (m, a, fuse, t)
        return t["d_n_fused"], t["d_n_added"], t["d_added"]

    # ---- LocalMapping::SearchInNeighbors ---------------------------------------------------------------------------------------------
    def fuse_targets(self, cur_slot, kf_bad, nn=20, nn2=5, target_cap=None, guard=0):
        """vpTargetKFs of LocalMapping::SearchInNeighbors (:481-503) from the handle's graph, duplicates included
        -> (d_n_targets int32[1], the uncut length; d_targets int32[target_cap]).  Enqueues only."""
        cap = int(nn) * (1 + int(nn2)) if target_cap is None else int(target_cap)
        bad = self._filled(kf_bad, torch.uint8, self.K)
        n, t = self._i32(1, -1), self._i32(cap + guard, -5)
        check(lib().fb_covis_fuse_targets_dev(self.h, int(cur_slot), int(nn), int(nn2), _p(bad), cap, _p(n), _p(t), _stream()),
              "fb_covis_fuse_targets_dev")
        self._keep = (bad, n, t)
        return n, t

    def reserve_search_in_neighbors(self, n_mp, n_obs, new_edge_cap, kp_stride, n_targets, cand_cap, grid_cells):
        check(lib().fb_covis_reserve_search_in_neighbors(self.h, int(n_mp), int(n_obs), int(new_edge_cap), int(kp_stride), int(n_targets),
                                                         int(cand_cap), int(grid_cells)), "fb_covis_reserve_search_in_neighbors")

    def search_in_neighbors(self, m, fuse, refresh, target, cur_slot, n_features, n_targets, d_n_targets, d_targets, kf_keys_un, new_edge_cap,
                            cand_cap, th=3.0, added_cap=None, guard=0):
        """LocalMapping::SearchInNeighbors (:506-557) for the key frame in cur_slot of m (a DeviceMap with obs_spare) and the
        target list fuse_targets left on the device; n_targets: the launch bound (the exact count or the cap).  fuse: the
        struct of point_fuse_arrays; refresh: the struct of refresh_arrays on the same map (kf_Tcw, mp_xw, mp_ref_kf and the
        three arrays step 5 writes are read from it; its mp_desc is not used, fuse's is); target: a cabi.KfTarget whose cam,
        grid, scale tables and n_levels are read.  -> dict of device tensors: n_fused [n_targets + 1], n_candidates [1],
        candidates [cand_cap], n_added [1], added rows, n_counter [1], front [1].  The edge list of m is new_edge_cap
        longer afterwards (m.grow).  Enqueues only."""
        kp = kf_keys_un if torch.is_tensor(kf_keys_un) else torch.from_numpy(np.ascontiguousarray(kf_keys_un).view(np.uint8).reshape(-1).copy()).to(self.device)
        n_targets, cand_cap, new_edge_cap = int(n_targets), int(cand_cap), int(new_edge_cap)
        cap = new_edge_cap if added_cap is None else int(added_cap)
        t = dict(d_n_fused=self._i32(n_targets + 1 + guard, -5), d_n_candidates=self._i32(1, -1), d_candidates=self._i32(cand_cap + guard, -5),
                 d_n_added=self._i32(1, -1), d_added=torch.full(((max(cap, 1) + guard) * 4,), -5, dtype=torch.int32, device=self.device),
                 d_n_counter=self._i32(1, -1), d_front=self._i32(1, -7))
        a = cabi.SearchInNeighborsArgs()
        cabi.fill(a, cur_slot=int(cur_slot), n_features=int(n_features), n_targets=n_targets, d_n_targets=d_n_targets, d_targets=d_targets,
                  th=float(th), log_scale_factor=target.log_scale_factor, n_levels=target.n_levels, kf_keys_un=kp, obs_cap=int(m.obs_cap),
                  obs_idx=m.t["obs_idx"], new_edge_cap=new_edge_cap, cand_cap=cand_cap, added_cap=cap, **t)
        for k in ("kf_Tcw", "mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_ref_kf"):
            setattr(a, k, getattr(refresh, k))
        a.cam, a.grid, a.scale_factors, a.inv_level_sigma2, a.map = target.cam, target.grid, target.scale_factors, target.inv_level_sigma2, fuse
        check(lib().fb_covis_search_in_neighbors_dev(self.h, C.byref(m.c), C.byref(a), _stream()), "fb_covis_search_in_neighbors_dev")
        m.grow(new_edge_cap)
        self._keep = (m, a, fuse, refresh, t, kp, d_n_targets, d_targets)
        return {k[2:]: v for k, v in t.items()}

    # ---- the bird side: UpdateBirdConnections and the local bird map ------------------------------------------------------------
    def reserve_local_bird_map(self, n_mpb, n_bobs):
        check(lib().fb_covis_reserve_local_bird_map(self.h, int(n_mpb), int(n_bobs)), "fb_covis_reserve_local_bird_map")

    def update_bird_connections(self, m, t, slots, n_counter=None, now_state=0, id0_slot=-1, kf_frame_id=None, kf_in_map=None):
        """KeyFrame::UpdateBirdConnections(now_state) of the listed slots -> (n_bird_counter, bird_front) device int32 tensors.
        m: a cabi.CovisMap or an object with one under .c (only max_keyframes and kf_order are read); t: DeviceTables with
        the bird side or DeviceBirdTables; n_counter: the front update_connections' output for the same slots, None = all act."""
        slots = self._dev(slots).reshape(-1)
        n = slots.numel()
        fid = None if kf_frame_id is None else self._dev(kf_frame_id)
        inm = None if kf_in_map is None else self._dev(kf_in_map, torch.uint8)
        nbc, bf = self._i32(n, -7), self._i32(n, -7)
        mc = m if isinstance(m, cabi.CovisMap) else m.c
        check(lib().fb_covis_update_bird_connections_dev(self.h, C.byref(mc), C.byref(t.c), n, _p(slots), _p(n_counter), int(now_state),
                                                         int(id0_slot), _p(fid), _p(inm), _p(nbc), _p(bf), _stream()),
              "fb_covis_update_bird_connections_dev")
        self._keep = (m, t, slots, n_counter, fid, inm)
        return nbc[:n], bf[:n]

    def bird_connected(self, slot):
        """GetBirdConnectedBirdKeyFrames + the bird weights -> (n[1], slots[K], weights[K])"""
        n, s, w = self._i32(1), self._i32(self.K, -1), self._i32(self.K, -1)
        check(lib().fb_covis_bird_connected_dev(self.h, int(slot), _p(n), _p(s), _p(w), _stream()), "fb_covis_bird_connected_dev")
        return n, s, w

    def local_bird_map_arrays(self, cap_kf, cap_mpb, kf_ow=None, mpb_order=None, guard=0):
        """Device arrays of a fb_local_bird_map_args with an empty localKFbird; each list is followed by `guard` elements the
        library never sees -> (dict of tensors, cabi.LocalBirdMapArgs)"""
        t = dict(d_local_kf_bird=torch.full((int(cap_kf) + guard + 1,), -5, dtype=torch.int32, device=self.device), d_n_local_kf_bird=self._i32(1),
                 d_local_mpb=torch.full((int(cap_mpb) + guard + 1,), -5, dtype=torch.int32, device=self.device), d_n_local_mpb=self._i32(1, -5),
                 d_overflow=self._i32(1, -5))
        if kf_ow is not None:
            t["d_kf_ow"] = self._dev(kf_ow, torch.float32).reshape(-1)
        if mpb_order is not None:
            t["d_mpb_order"] = torch.from_numpy(np.ascontiguousarray(mpb_order, np.uint64).view(np.int64).copy()).to(self.device)
        a = cabi.LocalBirdMapArgs()
        cabi.fill(a, new_slot=0, cap_kf=int(cap_kf), cap_mpb=int(cap_mpb), **t)
        return t, a

    def local_bird_map(self, m, t, a, new_slot):
        """The bird block of Map::AddKeyFrame(new_slot) + Map::UpdateLocalBirdMap on the arrays of local_bird_map_arrays.
        Enqueues only."""
        a.new_slot = int(new_slot)
        mc = m if isinstance(m, cabi.CovisMap) else m.c
        check(lib().fb_covis_local_bird_map_dev(self.h, C.byref(mc), C.byref(t.c), C.byref(a), _stream()), "fb_covis_local_bird_map_dev")
        self._keep = (m, t, a)

    # ---- loop closing: consistency groups, mvpLoopMapPoints, LoopConnections ------------------------------------------------------
    def reserve_loop_groups(self, cap_groups):
        check(lib().fb_covis_reserve_loop_groups(self.h, int(cap_groups)), "fb_covis_reserve_loop_groups")
        self._loop_cap = int(cap_groups)

    def detect_loop(self, n_candidates, candidates, consistency_th=3, guard=0):
        """The consistency check of LoopClosing::DetectLoop on the candidate list of fb_kfdb_query_dev (device int32[1] and
        int32[K]) -> (n_enough int32[1], enough int32[K + guard], header int32[2 + guard] = n_groups, overflow).  Enqueues only."""
        n_enough = self._i32(1, -5)
        enough = torch.full((self.K + guard,), -5, dtype=torch.int32, device=self.device)
        header = torch.full((2 + guard,), -5, dtype=torch.int32, device=self.device)
        check(lib().fb_covis_detect_loop_dev(self.h, _p(n_candidates), _p(candidates), int(consistency_th), _p(n_enough), _p(enough),
                                             _p(header), _stream()), "fb_covis_detect_loop_dev")
        self._keep = (n_candidates, candidates, n_enough, enough, header)
        return n_enough, enough, header

    def loop_groups(self):
        """mvConsistentGroups as it stands -> list of (sorted slots, consistency counter); synchronises"""
        cap, nw = getattr(self, "_loop_cap", self.K), (self.K + 31) // 32
        n = C.c_int32(0)
        cons, bits = np.zeros(cap, np.int32), np.zeros((cap, nw), np.uint32)
        check(lib().fb_covis_loop_groups(self.h, C.byref(n), C.c_void_p(cons.ctypes.data), C.c_void_p(bits.ctypes.data), _stream()),
              "fb_covis_loop_groups")
        out = []
        for k in range(n.value):
            slots = [s for s in range(self.K) if (int(bits[k, s >> 5]) >> (s & 31)) & 1]
            out.append((slots, int(cons[k])))
        return out

    def reserve_loop_map_points(self, n_mp):
        check(lib().fb_covis_reserve_loop_map_points(self.h, int(n_mp)), "fb_covis_reserve_loop_map_points")

    def loop_map_points(self, m, matched_slot, cap=None, guard=0):
        """mvpLoopMapPoints of the matched key frame -> (n_loop int32[1], loop_mp int32[cap + guard], overflow int32[1]).
        Enqueues only."""
        cap = m.n_mp if cap is None else int(cap)
        n_loop, overflow = self._i32(1, -5), self._i32(1, -5)
        loop_mp = torch.full((cap + guard + 1,), -5, dtype=torch.int32, device=self.device)
        check(lib().fb_covis_loop_map_points_dev(self.h, C.byref(m.c), int(matched_slot), cap, _p(n_loop), _p(loop_mp), _p(overflow),
                                                 _stream()), "fb_covis_loop_map_points_dev")
        self._keep = (m, n_loop, loop_mp, overflow)
        return n_loop, loop_mp, overflow

    def reserve_loop_connections(self, n_mp, n_obs, set_cap):
        check(lib().fb_covis_reserve_loop_connections(self.h, int(n_mp), int(n_obs), int(set_cap)), "fb_covis_reserve_loop_connections")

    def loop_connections(self, m, set_slots, n_set=None, lc_cap=None, guard=0):
        """The LoopConnections pass that ends CorrectLoop over mvpCurrentConnectedKFs = set_slots (a list or a device tensor;
        n_set: a device int32[1] that holds its length, None = all of it) -> dict of device tensors: n_counter, front
        [set_cap + guard], lc_off [set_cap + 1 + guard], lc_slots [lc_cap + guard], header int32[2] = total, overflow.
        Enqueues only."""
        slots = self._dev(set_slots).reshape(-1)
        cap = int(slots.numel())
        if n_set is None:
            n_set = self._i32(1, cap)
        lc_cap = cap * self.K if lc_cap is None else int(lc_cap)
        out = dict(n_counter=self._i32(cap + guard, -5), front=self._i32(cap + guard, -5), lc_off=self._i32(cap + 1 + guard, -5),
                   lc_slots=self._i32(lc_cap + guard, -5), header=self._i32(2 + guard, -5))
        a = cabi.LoopConnectionsArgs()
        cabi.fill(a, set_cap=cap, d_n_set=n_set, d_set=slots if cap else self._i32(1), d_n_counter=out["n_counter"], d_front=out["front"],
                  lc_cap=lc_cap, d_lc_off=out["lc_off"], d_lc_slots=out["lc_slots"], d_header=out["header"])
        check(lib().fb_covis_loop_connections_dev(self.h, C.byref(m.c), C.byref(a), _stream()), "fb_covis_loop_connections_dev")
        self._keep = (m, a, slots, n_set, out)
        return out
