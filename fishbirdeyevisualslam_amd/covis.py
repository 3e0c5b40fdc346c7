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

    def __init__(self, arrays, device="cuda:0"):
        self.device = torch.device(device)
        self.K, self.S = np.asarray(arrays["kf_mp"]).shape
        self.n_mp, self.n_obs = len(arrays["mp_bad"]), len(arrays["obs_kf"])
        self.t = {}
        for name, dt in self.FIELDS:
            a = np.ascontiguousarray(arrays[name], dt)
            if a.size == 0:
                a = np.zeros(1, dt)
            if dt == np.uint64:
                a = a.view(np.int64)
            self.t[name] = torch.from_numpy(a.copy()).to(self.device)
        self.c = cabi.CovisMap()
        cabi.fill(self.c, max_keyframes=self.K, kp_stride=self.S, n_mp=self.n_mp, n_obs=self.n_obs, **self.t)

    def bytes(self):
        return b"".join(self.t[name].cpu().numpy().tobytes() for name, _ in self.FIELDS)


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
