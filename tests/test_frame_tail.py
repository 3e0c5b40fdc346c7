"""The fused per-frame tail launches (fb_frame_tail_front_dev / fb_frame_tail_bird_dev) against the separate entry points
they stand for (grid build -> [bird camera positions] -> M3 / M9 -> edge gather, plus the fills and copies between them), on
the same inputs.  The separate entry points are pinned to the oracle elsewhere; here every output array is compared byte
for byte over its full stride, padding included: both sides start from the same 0x5A fill, so a store that one side makes
and the other does not shows.  Inputs are real extractions of synth.synth_image at 160x120 / 96x96 with build_world, then
edited per case."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from fishbirdeyevisualslam_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT_WH, BIRD_WH = (160, 120), (96, 96)
INPUTS = ("f_kps", "f_desc", "f_n", "b_kps", "b_desc", "b_n")
OUTPUTS = ("f_cs", "f_ci", "b_cs", "b_ci", "b_cam", "m_front", "nm_front", "m_bird", "nm_bird", "Tcw", "e_fxw", "e_fobs", "e_finf",
           "e_fvalid", "e_bxw", "e_bxc", "e_binf", "e_bvalid", "e_bout", "e_nf", "e_nb")
WORLD = ("last", "ref")


def test_tail_arg_structs_match_the_header_layout():
    names = {"fb_pose_gather_levels": C.sizeof(cabi.PoseGatherLevels), "fb_frame_tail_front_args": C.sizeof(cabi.FrameTailFrontArgs),
             "fb_frame_tail_bird_args": C.sizeof(cabi.FrameTailBirdArgs)}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "fishbird.h"\nint main(void){\n' + "".join(
        'printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names) + \
        'printf("front_tcw %zu\\n", offsetof(fb_frame_tail_front_args, Tcw));\n' \
        'printf("bird_n %zu\\n", offsetof(fb_frame_tail_bird_args, n_bird));\nreturn 0;}\n'
    d = tempfile.mkdtemp()
    open(os.path.join(d, "s.c"), "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
    got = dict(l.split() for l in subprocess.check_output([os.path.join(d, "s")]).decode().splitlines())
    for n, sz in names.items():
        assert int(got[n]) == sz, (n, got[n], sz)
    assert int(got["front_tcw"]) == cabi.FrameTailFrontArgs.Tcw.offset
    assert int(got["bird_n"]) == cabi.FrameTailBirdArgs.n_bird.offset


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _make_pipe(B, seed=0, **kw):
    import torch  # noqa: F401
    from fishbirdeyevisualslam_amd import synth
    from fishbirdeyevisualslam_amd.pipeline import FramePipeline
    front = np.stack([synth.synth_image(3100 + seed + i, *FRONT_WH) for i in range(B)])
    bird = np.stack([synth.synth_image(3600 + seed + i, *BIRD_WH) for i in range(B)])
    pipe = FramePipeline(B, FRONT_WH, BIRD_WH, device="cuda:0", fx=120.0, fy=120.0, **kw)
    pipe.set_images(front, bird)
    pipe.build_world(seed=7300 + seed)
    return pipe


class _Bed:
    """One pipeline and a pristine copy of its extraction and world: set 0 runs the separate entry points, set 1 the fused ones."""

    def __init__(self, B, **kw):
        import torch
        self.torch = torch
        self.pipe = _make_pipe(B, **kw)
        p = self.pipe
        torch.cuda.synchronize()
        self.pristine = {k: p._sets[0][k].clone() for k in INPUTS}
        self.pristine.update({("last", k): v.clone() for k, v in p.last.items()})
        self.pristine.update({("ref", k): v.clone() for k, v in p.ref.items()})
        self.pristine["Tcw0"] = p.Tcw0.clone()

    def reset(self):
        p = self.pipe
        for k in INPUTS:
            p._sets[0][k].copy_(self.pristine[k])
        for k in p.last:
            p.last[k].copy_(self.pristine[("last", k)])
        for k in p.ref:
            p.ref[k].copy_(self.pristine[("ref", k)])
        p.Tcw0.copy_(self.pristine["Tcw0"])

    def reference(self, S):
        """what FramePipeline ran per step before the fused launches existed"""
        p, L = self.pipe, self.pipe.L
        B, cap, nl = p.B, p.cap, p.params.nlevels
        s = C.c_void_p(self.torch.cuda.current_stream(p.dev).cuda_stream)
        p.grids(s, "both", S)
        assert L.fb_match_projection_frame_dev(C.byref(S["a_tail_front"].m3), s) == 0
        S["m_bird"].fill_(-1)
        assert L.fb_match_bird_mappoints_dev(C.byref(S["a_tail_bird"].m9), s) == 0
        S["e_nf"].copy_(S["f_n"])
        S["Tcw"].copy_(p.Tcw0)
        assert L.fb_pose_gather_front_dev(B, cap, p.nl, _vp(S["f_n"]), _vp(S["f_kps"]), _vp(S["m_front"]), _vp(p.last["xw"]), p._inv_sigma2, nl,
                                          _vp(S["e_fxw"]), _vp(S["e_fobs"]), _vp(S["e_finf"]), _vp(S["e_fvalid"]), s) == 0
        S["e_nb"].copy_(S["b_n"])
        S["e_bout"].fill_(1)
        assert L.fb_pose_gather_bird_dev(B, cap, p.nr, _vp(S["b_n"]), _vp(S["b_kps"]), _vp(S["b_cam"]), _vp(S["m_bird"]), _vp(p.ref["xw"]),
                                         p._inv_sigma2, nl, _vp(S["e_bxw"]), _vp(S["e_bxc"]), _vp(S["e_binf"]), _vp(S["e_bvalid"]), s) == 0

    def run(self):
        """both paths on the inputs now in set 0 -> (separate, fused) output dicts as host bytes"""
        p, torch = self.pipe, self.torch
        S0, S1 = p._sets
        for k in INPUTS:
            S1[k].copy_(S0[k])
        for S in (S0, S1):
            for k in OUTPUTS:
                S[k].view(-1).view(torch.uint8).fill_(0x5A)
        self.reference(S0)
        s = C.c_void_p(torch.cuda.current_stream(p.dev).cuda_stream)
        p.tail_front(s, S1)
        p.tail_bird(s, S1)
        torch.cuda.synchronize()
        return tuple({k: S[k].cpu().numpy() for k in OUTPUTS} for S in (S0, S1))

    def check(self):
        sep, fused = self.run()
        for k in OUTPUTS:
            assert sep[k].tobytes() == fused[k].tobytes(), "%s differs" % k
        return sep


@pytest.fixture(scope="module")
def bed3():
    b = _Bed(3)
    yield b
    b.pipe.close()


@pytest.fixture(scope="module")
def bed1():
    b = _Bed(1)
    yield b
    b.pipe.close()


def _crafted_kps(g, n, wh, cell=None, nlevels=8):
    """n key points spread over the image, or all inside one grid cell (cell = its centre, +-0.2 px)"""
    k = np.zeros(n, cabi.KP_DTYPE)
    if cell is None:
        k["x"], k["y"] = g.uniform(1, wh[0] - 2, n), g.uniform(1, wh[1] - 2, n)
    else:
        k["x"], k["y"] = cell[0] + g.uniform(-0.2, 0.2, n), cell[1] + g.uniform(-0.2, 0.2, n)
    k["size"], k["angle"], k["response"] = 31.0, g.uniform(0, 360, n), g.uniform(1, 100, n)
    k["octave"] = g.integers(0, nlevels, n)
    return k


def _put_frame(bed, b, side, kps, desc):
    """replace frame b's key points / descriptors / count of one camera in set 0"""
    torch, S = bed.torch, bed.pipe._sets[0]
    n = len(kps)
    raw = torch.from_numpy(np.ascontiguousarray(kps).view(np.uint8).reshape(-1)).to(bed.pipe.dev)
    S[side + "_kps"][b, : n * 24] = raw
    S[side + "_desc"][b, :n] = torch.from_numpy(np.ascontiguousarray(desc)).to(bed.pipe.dev)
    S[side + "_n"][b] = n


@pytest.mark.gpu
def test_real_extraction_b3(bed3):
    bed3.reset()
    sep = bed3.check()
    assert (sep["e_nf"] > 0).all() and (sep["nm_front"] > 0).all(), "the case must have front matches to compare"
    assert (sep["e_nb"] > 0).all()


@pytest.mark.gpu
def test_real_extraction_b1(bed1):
    bed1.reset()
    sep = bed1.check()
    assert sep["nm_front"][0] > 0


@pytest.mark.gpu
def test_frame_without_key_points(bed3):
    bed3.reset()
    S = bed3.pipe._sets[0]
    S["f_n"][1] = 0
    S["b_n"][1] = 0
    sep = bed3.check()
    assert sep["nm_front"][1] == 0 and sep["nm_bird"][1] == 0 and not sep["e_fvalid"][1].any()


@pytest.mark.gpu
def test_frame_without_queries(bed3):
    bed3.reset()
    bed3.pipe.last["n"][2] = 0
    bed3.pipe.ref["n"][2] = 0
    sep = bed3.check()
    assert sep["nm_front"][2] == 0 and sep["nm_bird"][2] == 0 and (sep["m_front"][2, : sep["e_nf"][2]] == -1).all()


@pytest.mark.gpu
def test_all_key_points_in_one_cell(bed3):
    bed3.reset()
    g = np.random.default_rng(11)
    nl = bed3.pipe.params.nlevels
    for side, wh, n, geom in (("f", FRONT_WH, 300, bed3.pipe.geom_f), ("b", BIRD_WH, 200, bed3.pipe.geom_b)):
        centre = (geom.min_x + (geom.cols // 2) / geom.inv_w, geom.min_y + (geom.rows // 2) / geom.inv_h)  # PosInGrid rounds
        k = _crafted_kps(g, n, wh, cell=centre, nlevels=nl)
        _put_frame(bed3, 0, side, k, g.integers(0, 256, (n, 32), dtype=np.uint8))
    sep = bed3.check()
    for cs, n in ((sep["f_cs"][0], 300), (sep["b_cs"][0], 200)):
        assert cs[-1] == n and np.count_nonzero(np.diff(cs)) == 1, "one long cell, all others empty"


@pytest.mark.gpu
def test_frame_at_capacity(bed3):
    bed3.reset()
    g = np.random.default_rng(12)
    cap, nl = bed3.pipe.cap, bed3.pipe.params.nlevels
    for side, wh in (("f", FRONT_WH), ("b", BIRD_WH)):
        _put_frame(bed3, 1, side, _crafted_kps(g, cap, wh, nlevels=nl), g.integers(0, 256, (cap, 32), dtype=np.uint8))
    sep = bed3.check()
    assert sep["e_nf"][1] == cap and sep["e_nb"][1] == cap


def _large_stride_bed(nfeatures, side, **kw):
    """Batch 2 at a key-point stride of nfeatures + 64, where the 160 KiB of LDS decide the variant (the stride decides, not
    the count).  Frame 0 is the real extraction; frame 1 of `side` is filled to the stride behind its real key points, so
    that every array of the launch is used to its end while the matches of the real key points stay."""
    from fishbirdeyevisualslam_amd import synth
    bed = _Bed(2, orb=dict(synth.ORB_DEFAULT, nfeatures=nfeatures), **kw)
    p = bed.pipe
    assert p.cap == nfeatures + 64
    S = p._sets[0]
    n = int(S[side + "_n"][1])
    k = S[side + "_kps"][1].cpu().numpy().view(cabi.KP_DTYPE)[:n]
    d = S[side + "_desc"][1, :n].cpu().numpy()
    g = np.random.default_rng(13)
    fill = _crafted_kps(g, p.cap - n, FRONT_WH if side == "f" else BIRD_WH, nlevels=p.params.nlevels)
    _put_frame(bed, 1, side, np.concatenate([k, fill]), np.concatenate([d, g.integers(0, 256, (p.cap - n, 32), dtype=np.uint8)]))
    return bed


@pytest.mark.gpu
def test_front_tail_with_the_grid_items_outside_lds():
    """cur 2800 / last 1400 on the 64 x 48 grid: the staged frame and the grid's counters fit the LDS, the 2800 items of the
    build do not (itemsInLds = 0; tests/cpp/match_plan_test.cpp pins the shape), so they are sorted in the caller's array
    and staged from there."""
    bed = _large_stride_bed(2736, "f", n_last=1400)
    try:
        sep = bed.check()
        assert sep["e_nf"].tolist()[1] == 2800 and (sep["nm_front"] > 0).all(), sep["nm_front"]
    finally:
        bed.pipe.close()


@pytest.mark.gpu
def test_bird_tail_with_items_and_camera_copy_outside_lds():
    """Stride 3200 on the 32 x 32 bird grid: descriptors in LDS, but neither the grid items nor the LDS copy of the camera
    positions fit beside them (itemsInLds = 0, camInLds = 0; pinned in tests/cpp/match_plan_test.cpp)."""
    bed = _large_stride_bed(3136, "b")
    try:
        sep = bed.check()
        assert sep["e_nb"].tolist()[1] == 3200 and (sep["nm_bird"] > 0).all(), sep["nm_bird"]
    finally:
        bed.pipe.close()


@pytest.mark.gpu
def test_claim_chain_runs_more_than_one_round(bed3):
    """Four targets, four queries that all project between them.  Query 0 and query 1 both want target 0; query q > 0 wants
    target q - 1 first and target q second, so the serial rule moves query 1, then 2, then 3 one target on: a chain three
    deep, which the fixed point resolves one link per round."""
    bed3.reset()
    p, torch = bed3.pipe, bed3.torch

    def bits(*ranges):
        v = np.zeros(256, np.uint8)
        for a, b in ranges:
            v[a:b] = 1
        return np.packbits(v)
    tdesc = np.stack([bits((20 * i, 20 * i + 20)) for i in range(4)])
    qdesc = np.stack([tdesc[0]] + [bits((20 * (q - 1), 20 * q), (20 * q, 20 * q + 5)) for q in (1, 2, 3)])
    dist = np.unpackbits(qdesc[:, None, :] ^ tdesc[None, :, :], axis=2).sum(2)
    for q in (1, 2, 3):
        order = np.argsort(dist[q], kind="stable")
        assert order[0] == q - 1 and order[1] == q and dist[q].max() <= 100
    assert dist[0].argmin() == 0
    k = np.zeros(4, cabi.KP_DTYPE)
    k["x"], k["y"], k["size"], k["response"] = 80.0 + 3.0 * np.arange(4), 60.0, 31.0, 10.0
    _put_frame(bed3, 0, "f", k, tdesc)
    z = 5.0
    xw = np.tile(np.array([(84.5 - p.cx) / p.fx * z, (60.0 - p.cy) / p.fy * z, z], np.float32), (4, 1))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(p.dev)
    p.last["n"][0] = 4
    p.last["xw"][0, :4] = up(xw)
    p.last["desc"][0, :4] = up(qdesc)
    p.last["octave"][0, :4] = 0
    p.last["angle"][0, :4] = 0.0
    p.Tcw0[0] = up(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32))
    sep = bed3.check()
    assert sep["m_front"][0, :4].tolist() == [0, 1, 2, 3] and sep["nm_front"][0] == 4


@pytest.mark.gpu
def test_two_overlapped_steps_equal_two_serial_steps():
    """step() alternates between two buffer sets and runs the tails beside the next extraction; with other images in the
    second step, results_host() / keypoints_host() must be those of the second step alone."""
    import torch
    from fishbirdeyevisualslam_amd import synth
    B = 2
    imgs = [(np.stack([synth.synth_image(4100 + 10 * k + i, *FRONT_WH) for i in range(B)]),
             np.stack([synth.synth_image(4600 + 10 * k + i, *BIRD_WH) for i in range(B)])) for k in range(2)]
    got = []
    for overlapped in (True, False):
        pipe = _make_pipe(B, seed=50)
        cur = torch.cuda.current_stream(pipe.dev)
        for k in range(2):
            if k:  # the previous step's extraction must be done with the images before they change
                cur.wait_event(pipe.evF)
                cur.wait_event(pipe.evB)
            pipe.set_images(*imgs[k])
            pipe.step() if overlapped else pipe.step_serial()
        res = pipe.results_host()
        for side in ("front", "bird"):
            kps, desc = pipe.keypoints_host(side)
            res[side + "_kps"] = np.concatenate(kps)
            res[side + "_desc"] = np.concatenate(desc)
        got.append(res)
        pipe.close()
    assert sorted(got[0]) == sorted(got[1])
    for k in got[0]:
        assert got[0][k].tobytes() == got[1][k].tobytes(), k
    assert (got[0]["nm_front"] > 0).all()
