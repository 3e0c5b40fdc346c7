"""Step 0 of the tail fusion: how much does the step gain when the per-frame tail (grid, matcher, gather, fills and copies)
leaves the extraction streams, before any kernel is fused?  Runs bench.py (arguments passed through) with a FramePipeline
whose tail launches are the SEPARATE entry points and torch fills / copies, enqueued on the pose stream on alternating buffer
sets exactly as the fused launches are.  Compare its ms_per_step with the parent's and with the fused pipeline's.

    python profiles/probes/tail_offstream.py [bench.py arguments]
"""
import ctypes as C
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from fishbirdeyevisualslam_amd import pipeline as P  # noqa: E402

_vp = P._vp


def tail_front(self, s, S):
    L, B, cap, nl = self.L, self.B, self.cap, self.params.nlevels
    self.grids(s, "front", S)
    P.check(L.fb_match_projection_frame_dev(C.byref(S["a_tail_front"].m3), s), "M3")
    S["e_nf"].copy_(S["f_n"])
    S["Tcw"].copy_(self.Tcw0)
    P.check(L.fb_pose_gather_front_dev(B, cap, self.nl, _vp(S["f_n"]), _vp(S["f_kps"]), _vp(S["m_front"]), _vp(self.last["xw"]),
                                       self._inv_sigma2, nl, _vp(S["e_fxw"]), _vp(S["e_fobs"]), _vp(S["e_finf"]), _vp(S["e_fvalid"]), s), "gather front")


def tail_bird(self, s, S):
    L, B, cap, nl = self.L, self.B, self.cap, self.params.nlevels
    self.grids(s, "bird", S)
    S["m_bird"].fill_(-1)
    P.check(L.fb_match_bird_mappoints_dev(C.byref(S["a_tail_bird"].m9), s), "M9")
    S["e_nb"].copy_(S["b_n"])
    S["e_bout"].fill_(1)
    P.check(L.fb_pose_gather_bird_dev(B, cap, self.nr, _vp(S["b_n"]), _vp(S["b_kps"]), _vp(S["b_cam"]), _vp(S["m_bird"]), _vp(self.ref["xw"]),
                                      self._inv_sigma2, nl, _vp(S["e_bxw"]), _vp(S["e_bxc"]), _vp(S["e_binf"]), _vp(S["e_bvalid"]), s), "gather bird")


P.FramePipeline.tail_front = tail_front
P.FramePipeline.tail_bird = tail_bird
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
