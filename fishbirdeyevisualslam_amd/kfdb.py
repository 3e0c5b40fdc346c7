"""KeyFrameDatabase on the device (fb_kfdb_* in include/fishbird.h) over torch tensors.

A key frame is a slot in [0, max_keyframes).  Nothing here synchronises: results are device tensors on the current stream.
"""
import ctypes as C

import torch

from . import cabi, check, lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(cabi.ptr(t))


class KeyFrameDatabase:
    def __init__(self, max_keyframes, word_stride, device="cuda:0"):
        self.K, self.S = int(max_keyframes), int(word_stride)
        self.device = torch.device(device)
        self.h = C.c_void_p()
        p = cabi.KfdbParams(self.K, self.S)
        check(lib().fb_kfdb_create(C.byref(p), C.byref(self.h)), "fb_kfdb_create")
        self.covis = torch.full((self.K, cabi.FB_KFDB_COVIS), -1, dtype=torch.int32, device=self.device)

    def close(self):
        if self.h:
            lib().fb_kfdb_destroy(self.h)
            self.h = C.c_void_p()

    def _dev(self, x, dtype):
        if not torch.is_tensor(x):
            x = torch.as_tensor(x, dtype=dtype)
        return x.to(device=self.device, dtype=dtype).contiguous()

    def _bow(self, n_words, ids, vals):
        """-> device (n_words[1] int32, ids uint32 as int32 bits, vals float64), at least one entry each"""
        ids = self._dev(ids, torch.int32) if torch.is_tensor(ids) else torch.from_numpy(_u32_bits(ids)).to(self.device)
        vals = self._dev(vals, torch.float64)
        if n_words is None:
            n_words = [ids.numel()]
        n = self._dev(n_words, torch.int32).reshape(-1)
        if ids.numel() == 0:
            ids, vals = torch.zeros(1, dtype=torch.int32, device=self.device), torch.zeros(1, dtype=torch.float64, device=self.device)
        return n, ids, vals

    def add(self, slot, ids, vals, n_words=None):
        """KeyFrameDatabase::add.  ids / vals: the BowVector (device tensors or arrays); n_words: device int32[1] (default: len)."""
        n, ids, vals = self._bow(n_words, ids, vals)
        check(lib().fb_kfdb_add_dev(self.h, int(slot), _p(n), _p(ids), _p(vals), _stream()), "fb_kfdb_add_dev")
        self._keep = (n, ids, vals)

    def add_frame(self, slot, frame):
        """add() of a frame handle (ctypes pointer of fb_frame_create) whose BoW is computed."""
        check(lib().fb_kfdb_add_frame_dev(self.h, int(slot), frame, _stream()), "fb_kfdb_add_frame_dev")

    def erase(self, slot):
        check(lib().fb_kfdb_erase(self.h, int(slot), _stream()), "fb_kfdb_erase")

    def clear(self):
        check(lib().fb_kfdb_clear(self.h, _stream()), "fb_kfdb_clear")

    def set_covisibility(self, covis):
        """[max_keyframes][10] slots of GetBestCovisibilityKeyFrames(10) per key frame, -1 padded."""
        self.covis = self._dev(covis, torch.int32).reshape(self.K, cabi.FB_KFDB_COVIS)

    def _query(self, mode, query_id, ids, vals, n_words, min_score, connected, extras):
        n, ids, vals = self._bow(n_words, ids, vals)
        out = {"n_candidates": torch.zeros(1, dtype=torch.int32, device=self.device),
               "candidates": torch.full((self.K,), -1, dtype=torch.int32, device=self.device)}
        a = cabi.KfdbQueryArgs()
        conn = None
        if connected is not None and len(connected):
            conn = self._dev(connected, torch.int32)
        cabi.fill(a, mode=mode, query_id=int(query_id), n_words=n, bow_ids=ids, bow_vals=vals, min_score=float(min_score),
                  n_connected=0 if conn is None else conn.numel(), connected=conn, covis=self.covis, **out)
        if extras:
            ex = {k: torch.zeros(1, dtype=torch.int32, device=self.device) for k in ("n_sharing", "max_common_words", "n_scored")}
            ex["common_words"] = torch.zeros(self.K, dtype=torch.int32, device=self.device)
            ex["scores"] = torch.zeros(self.K, dtype=torch.float32, device=self.device)
            cabi.fill(a, **ex)
            out.update(ex)
        check(lib().fb_kfdb_query_dev(self.h, C.byref(a), _stream()), "fb_kfdb_query_dev")
        out["_keep"] = (n, ids, vals, conn, self.covis)
        return out

    def detect_relocalization_candidates(self, query_id, ids, vals, n_words=None, extras=False):
        return self._query(cabi.FB_KFDB_RELOC, query_id, ids, vals, n_words, 0.0, None, extras)

    def detect_loop_candidates(self, query_id, ids, vals, min_score, connected=None, n_words=None, extras=False):
        return self._query(cabi.FB_KFDB_LOOP, query_id, ids, vals, n_words, min_score, connected, extras)

    def min_score(self, ids, vals, slots, skip=None, n_words=None):
        """-> (scores float32[len(slots)], min_score float32[1]) device tensors (LoopClosing.cc:127-141)."""
        n, ids, vals = self._bow(n_words, ids, vals)
        slots = self._dev(slots, torch.int32)
        skip_t = None if skip is None else self._dev(skip, torch.uint8)
        scores = torch.zeros(max(slots.numel(), 1), dtype=torch.float32, device=self.device)
        mn = torch.zeros(1, dtype=torch.float32, device=self.device)
        check(lib().fb_kfdb_min_score_dev(self.h, _p(n), _p(ids), _p(vals), slots.numel(), _p(slots), _p(skip_t), _p(scores), _p(mn),
                                          _stream()), "fb_kfdb_min_score_dev")
        self._keep = (n, ids, vals, slots, skip_t)
        return scores[: slots.numel()], mn


def _u32_bits(ids):
    import numpy as np
    return np.ascontiguousarray(ids, np.uint32).view(np.int32).copy()


def bow_score(a_ids, a_vals, na, b_ids, b_vals, nb, device="cuda:0"):
    """TemplatedVocabulary::score (L1) of [batch] pairs: ids uint32 [batch][stride] arrays, vals float64 -> float64[batch] tensor."""
    import numpy as np
    dev = torch.device(device)
    batch, stride = np.asarray(a_ids).shape
    t = [torch.from_numpy(_u32_bits(a_ids)).to(dev), torch.from_numpy(np.ascontiguousarray(a_vals, np.float64)).to(dev),
         torch.from_numpy(np.ascontiguousarray(na, np.int32)).to(dev), torch.from_numpy(_u32_bits(b_ids)).to(dev),
         torch.from_numpy(np.ascontiguousarray(b_vals, np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(nb, np.int32)).to(dev)]
    out = torch.zeros(batch, dtype=torch.float64, device=dev)
    check(lib().fb_bow_score_dev(batch, stride, _p(t[2]), _p(t[0]), _p(t[1]), _p(t[5]), _p(t[3]), _p(t[4]), _p(out), _stream()),
          "fb_bow_score_dev")
    torch.cuda.current_stream().synchronize()
    return out
