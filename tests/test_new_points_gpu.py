"""fb_create_new_map_points_dev / fb_create_new_map_points on the device against the CPU restatement of the reference's
serial loop (tests/new_points_ref.py), and the LocalMapping chain M7 -> new points -> Fuse -> local BA without a host copy."""
import ctypes as C

import numpy as np
import pytest

import new_points_ref as R
from fishbirdeyevisualslam_amd import bow_problem as BP, cabi, synth

pytestmark = pytest.mark.gpu
OUT_FIELDS = ("has_mp1", "has_mp2", "n_new", "xw", "normal", "max_dist", "min_dist", "desc", "idx1", "nb", "idx2", "kf1_new",
              "kf2_new", "nb_matches", "nb_new", "nb_skipped")


def _run_dev(prob, n_nb=None, has_mp1=None, check_orientation=0, empty_nb=None, keep_on_device=False):
    """-> (rc, host copies of the outputs, device tensors)"""
    import torch
    import fishbirdeyevisualslam_amd as fb
    dev = torch.device("cuda:0")
    a, out, (keep, k1, k2) = BP.new_points_args(prob, n_nb=n_nb)
    if has_mp1 is not None:
        out["has_mp1"][: len(has_mp1)] = has_mp1
    if empty_nb is not None:
        st = keep["nb_mp_start"]
        st[empty_nb + 1:] -= st[empty_nb + 1] - st[empty_nb]
        keep["nb_mp_start"] = st
        cabi.fill(a, nb_mp_start=st)
    d = {}
    for k, v in list(keep.items()) + list(out.items()):
        if k == "nb_mp_start":
            continue
        arr = np.ascontiguousarray(v.view(np.uint8) if v.dtype == cabi.KP_DTYPE else v)
        d[k] = torch.from_numpy(arr.copy()).to(dev)
        cabi.fill(a, **{k: d[k]})
    for fv, kk in ((a.fv1, k1), (a.fv2, k2)):
        for name, arr in zip(("n_nodes", "node_ids", "node_start", "items"), kk):
            t = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
            d[id(fv), name] = t
            cabi.fill(fv, **{name: t})
    a.matcher.check_orientation = check_orientation
    lib = fb.lib()
    lib.fb_create_new_map_points_workspace.restype = C.c_size_t
    wsb = lib.fb_create_new_map_points_workspace(a.n_nb, a.kf1_stride)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    cabi.fill(a, workspace=ws, workspace_bytes=wsb)
    s = torch.cuda.current_stream()
    rc = lib.fb_create_new_map_points_dev(C.byref(a), C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    host = {k: d[k].cpu().numpy() for k in OUT_FIELDS}
    return rc, host, (d, a, ws, keep)


def _check(prob, got, ref, n_nb=None):
    B = len(prob["nbs"]) if n_nb is None else n_nb
    n = ref["n_new"]
    n1 = len(prob["kps1"])
    assert int(got["n_new"][0]) == n
    for k in ("idx1", "nb", "idx2"):
        np.testing.assert_array_equal(got[k][:n], ref[k], err_msg=k)
    np.testing.assert_array_equal(got["desc"][:n], ref["desc"])
    np.testing.assert_array_equal(got["has_mp1"][:n1], ref["has_mp1"])
    np.testing.assert_array_equal(got["kf1_new"][:n1], ref["kf1_new"])
    for b in range(B):
        m = len(prob["nbs"][b]["kps"])
        np.testing.assert_array_equal(got["has_mp2"][b, :m], ref["has_mp2"][b], err_msg="has_mp2 %d" % b)
        np.testing.assert_array_equal(got["kf2_new"][b, :m], ref["kf2_new"][b], err_msg="kf2_new %d" % b)
    for k in ("nb_matches", "nb_new", "nb_skipped"):
        np.testing.assert_array_equal(got[k][:B], ref[k], err_msg=k)
    for k in ("xw", "normal", "max_dist", "min_dist"):
        g, r = got[k][:n].astype(np.float64), ref[k].astype(np.float64)
        scale = np.maximum(np.abs(r), 1.0)
        assert (np.abs(g - r) / scale).max(initial=0.0) <= 1e-4, k
        # the device repeats the restatement's arithmetic: equality is expected
        assert np.array_equal(got[k][:n], ref[k]), "%s differs in %d rows" % (k, int((got[k][:n] != ref[k]).reshape(n, -1).any(1).sum()))


@pytest.mark.parametrize("seed,n_nb,n1,n2,full1", [(21, 20, 2000, 2000, False), (22, 7, 777, 1001, False), (23, 1, 1500, 1500, False),
                                                  (24, 7, 2000, 1999, True), (25, 20, 1201, 640, False)])
def test_parity_with_the_serial_loop(seed, n_nb, n1, n2, full1):
    p = BP.make_new_points_problem(seed, n_nb=n_nb, n1=n1, n2=n2)
    if full1:
        p["has_mp1"][:] = 1
    ref = R.create_new_map_points(p)
    rc, got, _ = _run_dev(p)
    assert rc == 0
    _check(p, got, ref)
    if not full1:
        assert ref["n_new"] > 50
    else:
        assert ref["n_new"] == 0 and int(got["n_new"][0]) == 0


def test_serial_claim_order():
    p = BP.make_new_points_problem(31, n_nb=6, n1=2000, n2=2000)
    ref = R.create_new_map_points(p)
    rc, got, _ = _run_dev(p)
    assert rc == 0
    _check(p, got, ref)
    # a feature that neighbours 0 and 3 both triangulate goes to 0
    only3 = dict(p, nbs=[p["nbs"][3]])
    tri3 = set(R.create_new_map_points(only3)["idx1"].tolist())
    both = [i for i in tri3 if got["kf1_new"][i] >= 0 and got["nb"][got["kf1_new"][i]] == 0]
    assert len(both) >= 10
    # a feature that neighbour 0 matches but fails to triangulate goes to 3 and counts for both neighbours' nb_matches
    failed0 = [i for (b, i), r in ref["reasons"].items() if b == 0 and r != "ok"]
    to3 = [i for i in failed0 if got["kf1_new"][i] >= 0 and got["nb"][got["kf1_new"][i]] == 3]
    assert len(to3) >= 5
    for i in to3:
        assert (3, i) in ref["reasons"] and ref["reasons"][(3, i)] == "ok"
    np.testing.assert_array_equal(got["nb_matches"][:6], ref["nb_matches"])


def test_many_to_one_slot_holds_the_later_point():
    p = BP.make_new_points_problem(32, n_nb=4, n1=1500, n2=1500)
    rc, got, _ = _run_dev(p)
    assert rc == 0
    n = int(got["n_new"][0])
    key = got["nb"][:n].astype(np.int64) * 100000 + got["idx2"][:n]
    u, cnt = np.unique(key, return_counts=True)
    shared = u[cnt > 1]
    assert len(shared) >= 5
    for k in shared:
        rows = np.nonzero(key == k)[0]
        b, i2 = divmod(int(k), 100000)
        assert got["kf2_new"][b, i2] == rows.max() and got["has_mp2"][b, i2] == 1
        assert all(got["kf1_new"][got["idx1"][r]] == r for r in rows)


def test_first_k_neighbours_give_the_prefix():
    p = BP.make_new_points_problem(33, n_nb=12, n1=2000, n2=2000)
    rc, full, _ = _run_dev(p)
    assert rc == 0
    for k in (1, 5, 9):
        rc, part, _ = _run_dev(p, n_nb=k)
        assert rc == 0
        n = int(part["n_new"][0])
        assert n == int(full["nb_new"][:k].sum())
        for f in ("xw", "normal", "max_dist", "min_dist", "desc", "idx1", "nb", "idx2"):
            assert np.array_equal(part[f][:n], full[f][:n]), f
        for f in ("nb_matches", "nb_new", "nb_skipped"):
            assert np.array_equal(part[f][:k], full[f][:k]), f


def test_host_drop_in_is_byte_equal_to_dev():
    import fishbirdeyevisualslam_amd as fb
    p = BP.make_new_points_problem(34, n_nb=7, n1=1800, n2=1700)
    rc, got, _ = _run_dev(p)
    assert rc == 0
    a, out, keep = BP.new_points_args(p)
    assert fb.lib().fb_create_new_map_points(C.byref(a)) == 0
    n = int(got["n_new"][0])
    assert int(out["n_new"][0]) == n
    for k in OUT_FIELDS:
        if k in ("xw", "normal", "max_dist", "min_dist", "desc", "idx1", "nb", "idx2"):
            assert out[k][:n].tobytes() == got[k][:n].tobytes(), k
        else:
            assert out[k].tobytes() == got[k].tobytes(), k


def test_bad_arguments_and_empty_call():
    import fishbirdeyevisualslam_amd as fb
    p = BP.make_new_points_problem(35, n_nb=4, n1=600, n2=600)
    rc, _, _ = _run_dev(p, check_orientation=1)
    assert rc == cabi.FB_ERR_ARG and b"check_orientation" in fb.lib().fb_last_error()
    rc, _, _ = _run_dev(p, empty_nb=2)
    assert rc == cabi.FB_ERR_ARG and b"no map point" in fb.lib().fb_last_error()
    rc, got, _ = _run_dev(p, n_nb=0)
    assert rc == 0 and int(got["n_new"][0]) == 0 and (got["kf1_new"] == -1).all()
    assert np.array_equal(got["has_mp1"][:600], p["has_mp1"])
    ref = R.create_new_map_points(p)  # and the library works afterwards
    rc, got, _ = _run_dev(p)
    assert rc == 0
    _check(p, got, ref)


def test_new_points_feed_fuse_and_local_ba_on_the_device():
    """LocalMapping's hand-over (LocalMapping.cc:71-96): the new points go from fb_create_new_map_points_dev into
    fb_fuse_search_dev (as the fb_mp_list, n_mp = the device count) and fb_local_ba_dev (points + their two observations)
    on one stream, reading the arrays where they lie on the device (the test downloads copies only for the oracle, and the
    point count to size the BA graph)."""
    import torch
    import fishbirdeyevisualslam_amd as fb
    import oracle_lib as O
    from fishbirdeyevisualslam_amd import ba_problem, problems as P
    dev = torch.device("cuda:0")
    p = BP.make_new_points_problem(36, n_nb=5, n1=2000, n2=2000)
    rc, got, (d, a, ws, keep) = _run_dev(p)
    assert rc == 0
    s = torch.cuda.current_stream()
    lib = fb.lib()
    W, H = 640, 480
    # ---- Fuse(pKF = neighbour 0, new points) search half, fed with the device arrays as they lie
    nb0 = p["nbs"][0]
    geom = P.grid_geom(synth.front_grid_geom(W, H))
    cs, ci = P.build_grid_host([nb0["kps"]], geom, O.grid_build, len(nb0["kps"]))
    kt = cabi.KfTarget()
    sf, _, _, inv_sig2 = synth.scale_tables()
    kkeep = dict(n_kf=np.array([len(nb0["kps"])], np.int32), kf_kps=np.ascontiguousarray(nb0["kps"]), kf_desc=np.ascontiguousarray(nb0["desc"]),
                 kf_cell_start=np.ascontiguousarray(cs), kf_cell_items=np.ascontiguousarray(ci))
    kdev = {k: torch.from_numpy(v.view(np.uint8) if v.dtype == cabi.KP_DTYPE else v).to(dev) for k, v in kkeep.items()}
    cabi.fill(kt, kf_stride=len(nb0["kps"]), n_levels=8, log_scale_factor=float(np.log(np.float32(1.2))), **kdev)
    cabi.fill(kt.cam, fx=p["fx"], fy=p["fy"], cx=p["cx"], cy=p["cy"], min_x=0.0, min_y=0.0, max_x=float(W), max_y=float(H))
    cabi.fill(kt.grid, **synth.front_grid_geom(W, H))
    cabi.fill(kt, scale_factors=[float(x) for x in sf], inv_level_sigma2=[float(x) for x in inv_sig2])
    T2 = synth.to12(nb0["T"])
    ow = np.array([np.float32(-sum(float(T2[k * 4 + r]) * float(T2[k * 4 + 3]) for k in range(3))) for r in range(3)], np.float32)
    s1 = a.kf1_stride
    mvalid = torch.ones(s1, dtype=torch.uint8, device=dev)
    mp = cabi.MpList()
    cabi.fill(mp, mp_stride=s1, n_mp=d["n_new"], mp_valid=mvalid, mp_xw=d["xw"], mp_normal=d["normal"], mp_max_dist=d["max_dist"],
              mp_min_dist=d["min_dist"], mp_desc=d["desc"])
    fa = cabi.FuseArgs()
    pose_d, ow_d = torch.from_numpy(T2.copy()).to(dev), torch.from_numpy(ow).to(dev)
    best = torch.full((s1,), -7, dtype=torch.int32, device=dev)
    cabi.fill(fa, batch=1, th=3.0, pose=pose_d, Ow=ow_d, best_idx=best)
    fa.kf, fa.mp = kt, mp
    assert lib.fb_fuse_search_dev(C.byref(fa), C.c_void_p(s.cuda_stream)) == 0, lib.fb_last_error()
    # ---- local BA over KF1 (fixed) + the neighbours, the new points and their two observations, built on the device
    n = int(got["n_new"][0])
    assert n > 200
    kps1 = d["kps1"].view(torch.float32).view(-1, 6)
    kps2 = d["kps2"].view(torch.float32).view(a.n_nb, a.kf2_stride, 6)
    i1, nb, i2 = d["idx1"][:n].long(), d["nb"][:n].long(), d["idx2"][:n].long()
    uv1, uv2 = kps1[i1, :2], kps2[nb, i2, :2]
    o1 = d["kps1"].view(torch.int32).view(-1, 6)[i1, 5].long()
    o2 = d["kps2"].view(torch.int32).view(a.n_nb, a.kf2_stride, 6)[nb, i2, 5].long()
    inv_s2 = torch.from_numpy(inv_sig2).to(dev)
    ar = torch.arange(n, device=dev, dtype=torch.int32)
    dv = dict(kf_Tcw=torch.cat([d["Tcw1"].view(1, 12), d["Tcw2"]]).contiguous(), mp_xw=d["xw"][:n].contiguous(),
              obs_kf=torch.stack([torch.zeros_like(ar), (nb + 1).int()], 1).reshape(-1).contiguous(),
              obs_mp=torch.stack([ar, ar], 1).reshape(-1).contiguous(),
              obs_uv=torch.stack([uv1, uv2], 1).reshape(-1, 2).contiguous(),
              obs_inv_sigma2=torch.stack([inv_s2[o1], inv_s2[o2]], 1).reshape(-1).contiguous(),
              obs_outlier=torch.full((2 * n,), 9, dtype=torch.uint8, device=dev), bobs_outlier=torch.zeros(1, dtype=torch.uint8, device=dev))
    graph = {k: v.cpu().numpy().copy() for k, v in dv.items()}  # (downloaded for the oracle only; the device path does not wait on it)
    fuse_in = dict(xw=got["xw"], normal=got["normal"], max_dist=got["max_dist"], min_dist=got["min_dist"], desc=got["desc"])
    kf_fixed = np.array([1] + [0] * a.n_nb, np.uint8)
    ba = cabi.LocalBAArgs()
    cabi.fill(ba, with_odom=0, fx=p["fx"], fy=p["fy"], cx=p["cx"], cy=p["cy"], wF=1.0, wB=1.0, wP=3.0, n_kf=a.n_nb + 1, n_mp=n, n_mpb=0,
              n_obs=2 * n, n_bobs=0, n_odom=0, kf_fixed=kf_fixed, **dv)
    assert lib.fb_local_ba_dev(C.byref(ba), C.c_void_p(s.cuda_stream)) == 0, lib.fb_last_error()
    torch.cuda.synchronize()
    # ---- the oracle on the downloaded inputs
    fo = cabi.FuseArgs()
    okt = cabi.KfTarget()
    cabi.fill(okt, kf_stride=len(nb0["kps"]), n_levels=8, log_scale_factor=float(np.log(np.float32(1.2))), **kkeep)
    okt.cam, okt.grid = kt.cam, kt.grid
    cabi.fill(okt, scale_factors=[float(x) for x in sf], inv_level_sigma2=[float(x) for x in inv_sig2])
    omp = cabi.MpList()
    mkeep = dict(n_mp=np.array([n], np.int32), mp_valid=np.ones(s1, np.uint8), mp_xw=np.ascontiguousarray(fuse_in["xw"]),
                 mp_normal=np.ascontiguousarray(fuse_in["normal"]), mp_max_dist=np.ascontiguousarray(fuse_in["max_dist"]),
                 mp_min_dist=np.ascontiguousarray(fuse_in["min_dist"]), mp_desc=np.ascontiguousarray(fuse_in["desc"]))
    cabi.fill(omp, mp_stride=s1, **mkeep)
    obest = np.full(s1, -7, np.int32)
    cabi.fill(fo, batch=1, th=3.0, pose=T2, Ow=ow, best_idx=obest)
    fo.kf, fo.mp = okt, omp
    O.call("orc_fuse_search", fo)
    np.testing.assert_array_equal(best.cpu().numpy()[:n], obest[:n])
    assert (obest[:n] >= 0).sum() > 20
    bp = dict(fx=p["fx"], fy=p["fy"], cx=p["cx"], cy=p["cy"], wP=3.0, kf_Tcw=graph["kf_Tcw"], kf_fixed=kf_fixed, mp_xw=graph["mp_xw"],
              mpb_xw=np.zeros((0, 3), np.float32), obs_kf=graph["obs_kf"], obs_mp=graph["obs_mp"], obs_uv=graph["obs_uv"],
              obs_inv_sigma2=graph["obs_inv_sigma2"], bobs_kf=np.zeros(0, np.int32), bobs_mpb=np.zeros(0, np.int32),
              bobs_xc=np.zeros((0, 3), np.float32), bobs_inv_sigma2=np.zeros(0, np.float32), odom_kf_i=np.zeros(0, np.int32),
              odom_kf_j=np.zeros(0, np.int32), odom_Tij=np.zeros((0, 12), np.float32), odom_info=np.zeros(0, np.float64))
    a1, out_o, _ = ba_problem.local_ba_args(bp, with_odom=0)
    O.call("orc_local_ba", a1)
    rel = lambda x, y: float(np.abs(x - y).max() / max(1.0, np.abs(y).max()))
    assert rel(dv["kf_Tcw"].cpu().numpy(), out_o["kf_Tcw"]) <= 1e-4
    assert rel(dv["mp_xw"].cpu().numpy(), out_o["mp_xw"]) <= 1e-4
