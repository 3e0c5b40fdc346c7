"""fb_covis_local_window* / fb_covis_window_scatter_dev on the GPU against tests/local_window_ref.py: integer lists and
copied floats, so every comparison is for equality."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import covis_ref as R
import local_window_ref as LW
from fishbirdeyevisualslam_amd import cabi, covis_problem as P
from test_covis import MAP_FIELDS, _host_map, ref_map

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTS = (("kf_slot", "n_kf", 1), ("kf_fixed", "n_kf", 1), ("kf_Tcw", "n_kf", 12), ("mp_index", "n_mp", 1), ("mp_xw", "n_mp", 3),
         ("obs_kf", "n_obs", 1), ("obs_mp", "n_obs", 1), ("obs_src", "n_obs", 1), ("obs_uv", "n_obs", 2), ("obs_inv_sigma2", "n_obs", 1),
         ("mpb_index", "n_mpb", 1), ("mpb_xw", "n_mpb", 3), ("bobs_kf", "n_bobs", 1), ("bobs_mpb", "n_bobs", 1), ("bobs_src", "n_bobs", 1),
         ("bobs_xc", "n_bobs", 3), ("bobs_inv_sigma2", "n_bobs", 1))
HEADER = ("n_local", "n_fixed", "n_mp", "n_obs", "n_mpb", "n_bobs", "overflow")


def _graphs(p, slots, extra=None):
    """the model graph and the device graph after the same UpdateConnections (+ extra(graph) on both)"""
    from fishbirdeyevisualslam_amd.covis import CovisibilityGraph, DeviceMap, DeviceTables
    g = R.Graph(p["K"], p["kf_order"])
    m = ref_map(p)
    for a in slots:
        g.update_connections(m, a)
    dm, dt = DeviceMap(p), DeviceTables(p)
    G = CovisibilityGraph(p["K"])
    G.update_connections(dm, slots)
    if extra:
        extra(g)
        extra(G)
    return g, G, dm, dt


def _counts(hd):
    n = dict(zip(HEADER, hd))
    n["n_kf"] = n["n_local"] + n["n_fixed"]
    return n


def _assert_window(w, ref, caps=None):
    """every list of the device window w (tensors or numpy arrays) equals the model's; with caps: the prefix that fits"""
    hd = np.asarray(w["header"].cpu() if hasattr(w["header"], "cpu") else w["header"]).reshape(-1)[:7].tolist()
    assert hd[:6] == ref["header"][:6], (hd, ref["header"])
    n = _counts(ref["header"])
    for name, cnt, width in LISTS:
        k = n[cnt] if caps is None else min(n[cnt], caps["cap_" + cnt[2:]])
        got = w[name].cpu().numpy() if hasattr(w[name], "cpu") else np.asarray(w[name])
        np.testing.assert_array_equal(got.reshape(-1)[:k * width], np.asarray(ref[name]).reshape(-1)[:k * width], err_msg=name)
    return hd


def test_window_equals_the_model_with_and_without_bird():
    p = P.make_window_problem(K=70, S=96)
    g, G, dm, dt = _graphs(p, p["used"])
    cur = p["cur"]
    ref = LW.local_window(g, p, cur, True)
    # the case is not degenerate, judged on the model alone
    neigh = g.get_vector_covisible_keyframes(cur)
    local = ref["kf_slot"][:ref["n_local"]].tolist()
    obs = R.Map(*[p[k] for k in MAP_FIELDS]).observations()
    assert sum(int(p["kf_bad"][k]) for k in neigh) >= 1
    feats = [int(p["kf_mp"][k, i]) for k in local for i in range(int(p["kf_n"][k])) if p["kf_mp"][k, i] >= 0]
    assert sum(int(p["mp_bad"][mp]) for mp in feats) >= 1
    assert len([mp for mp in feats if not p["mp_bad"][mp]]) > len(ref["mp_index"])                    # duplicates
    assert any(p["kf_bad"][k] and k not in neigh and k != cur for mp in ref["mp_index"] for k in obs[mp])  # a bad fixed observer
    assert ref["n_fixed"] >= 2 and 5 <= ref["n_local"] <= 23
    local_pts = set(ref["mp_index"].tolist())
    assert sum(1 for mp, kf in zip(p["obs_mp"], p["obs_kf"]) if kf < 0 and int(mp) in local_pts) >= 1   # tombstoned edges
    assert any(np.diff([int(p["kf_order"][k]) for k in sorted(local)]) < 0)                           # kf_order is not the slot order
    ref0 = LW.local_window(g, p, cur, False)
    assert ref["n_fixed"] > ref0["n_fixed"] and len(ref["bobs_kf"]) > 0                                # the bird walk adds cameras
    _assert_window(G.local_window(dm, dt, cur, True), ref)
    rc, hd, slots, fixed = G.window_header()
    assert rc == 0 and [hd[k] for k in HEADER] == ref["header"]
    np.testing.assert_array_equal(slots, ref["kf_slot"])
    np.testing.assert_array_equal(fixed, ref["kf_fixed"])
    _assert_window(G.local_window(dm, dt, cur, False), ref0)
    assert G.error_count() == 0
    G.close()


def _hub():
    p = P.make_hub_problem(K=1300, S=1280, n_spokes=1250)
    outside = list(range(1251, 1300))
    hub = P.add_point(p, list(range(1, 252)) + outside, octave=2)           # 300 observers
    for k in range(6):                                                      # local points seen from outside: the fixed order
        P.add_point(p, [3 + k, outside[-1 - k], outside[k]], octave=1)
    p["kf_order"] = np.asarray(p["kf_order"]).copy()
    p["kf_order"][outside] = 0x7F3900000000 + np.random.default_rng(9).permutation(len(outside)).astype(np.uint64) * np.uint64(0x2D0)
    p.update(P.window_tables(p, 11, kf_bad=[7, 200, 1260], kf_init=[1]))
    return p, hub


def test_hub_point_and_a_row_above_a_workgroup():
    """One point with 300 observers (above a wave, above 256) and slot 0 with 1250 features at stride 1280: the edge order inside
    the point and the order of the fixed cameras."""
    p, hub = _hub()
    g, G, dm, dt = _graphs(p, [0], extra=lambda x: x.add_connection(0, 1, 2))   # the row changed: every entry joins the ordered list
    ref = LW.local_window(g, p, 0, False)
    assert ref["n_local"] > 1024 and ref["n_fixed"] >= 40
    j = ref["mp_index"].tolist().index(hub)
    assert (ref["obs_mp"] == j).sum() > 256
    w = G.local_window(dm, dt, 0, False)
    _assert_window(w, ref)
    assert G.error_count() == 0
    G.close()


@pytest.mark.parametrize("cur", [0, 4095])
def test_full_slot_range(cur):
    p = P.make_sparse_problem(K=4096, S=32)
    p.update(P.window_tables(p, 12, kf_bad=[2]))
    g, G, dm, dt = _graphs(p, p["used"])
    ref = LW.local_window(g, p, cur, False)
    assert ref["n_fixed"] >= 1 and max(ref["kf_slot"][ref["n_local"]:]) >= 2048
    _assert_window(G.local_window(dm, dt, cur, False), ref)
    G.close()


def _dirty(p):
    """out-of-range front and bird edges and kf_mp entries planted; the cleaned map has them erased instead"""
    d = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    K, S, BS, cur = p["K"], p["S"], p["BS"], p["cur"]
    live = np.flatnonzero((d["obs_kf"] >= 0) & np.isin(d["obs_kf"], [9, 10, 30]))[:3]
    d["obs_kf"][live[0]] = K + 5; d["obs_mp"][live[1]] = len(p["mp_bad"]) + 3; d["obs_idx"][live[2]] = S
    blive = np.flatnonzero(d["bobs_kf"] >= 0)[:3]
    d["bobs_kf"][blive[0]] = 1 << 20; d["bobs_mpb"][blive[1]] = len(p["mpb_bad"]); d["bobs_idx"][blive[2]] = BS + 1
    i, ib = int(d["kf_n"][cur]), int(d["kf_nb"][cur])
    d["kf_mp"][cur, i] = len(p["mp_bad"]) + 100; d["kf_n"][cur] += 1
    d["kf_mpb"][cur, ib] = len(p["mpb_bad"]) + 100; d["kf_nb"][cur] += 1
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    c["obs_kf"][live] = -1; c["bobs_kf"][blive] = -1
    c["kf_mp"][cur, i] = -1; c["kf_mpb"][cur, ib] = -1
    return d, c


def test_out_of_range_entries_and_small_capacities():
    p = P.make_window_problem(K=70, S=96)
    d, c = _dirty(p)
    g, G, dm, dt = _graphs(d, d["used"])
    gc = R.Graph(c["K"], c["kf_order"])
    for a in c["used"]:
        gc.update_connections(ref_map(c), a)
    ref = LW.local_window(gc, c, c["cur"], True)
    e0 = G.error_count()
    _assert_window(G.local_window(dm, dt, d["cur"], True), ref)
    assert G.error_count() - e0 == 8      # 3 front edges + 3 bird edges (the two indexes) + one kf_mp entry of each side
    # capacities one short of every list: overflow is flagged, what fits is written, the guard words stay
    n = _counts(ref["header"])
    caps = dict(cap_kf=n["n_kf"] - 1, cap_mp=n["n_mp"] - 1, cap_obs=n["n_obs"] - 1, cap_mpb=n["n_mpb"] - 1, cap_bobs=n["n_bobs"] - 1)
    guard = 16
    w = G.local_window(dm, dt, d["cur"], True, caps=caps, guard=guard)
    hd = _assert_window(w, ref, caps)
    assert hd[6] != 0
    rc, h, slots, _ = G.window_header()
    assert rc == cabi.FB_ERR_CAPACITY and h["overflow"] != 0 and len(slots) == caps["cap_kf"]
    for name, cnt, width in LISTS:
        cap = caps["cap_" + cnt[2:]]
        tail = w[name].cpu().numpy()[cap * width:]
        assert len(tail) == guard * width and (tail == tail[0]).all() and tail[0] in (-1, 0xEE), name
    for one in caps:                      # each capacity alone
        big = dict(cap_kf=n["n_kf"], cap_mp=n["n_mp"], cap_obs=n["n_obs"], cap_mpb=n["n_mpb"], cap_bobs=n["n_bobs"])
        big[one] -= 1
        w1 = G.local_window(dm, dt, d["cur"], True, caps=big, guard=1)
        assert int(w1["header"][6]) != 0, one
    w2 = G.local_window(dm, dt, d["cur"], True, caps=dict(cap_kf=n["n_kf"], cap_mp=n["n_mp"], cap_obs=n["n_obs"], cap_mpb=n["n_mpb"],
                                                         cap_bobs=n["n_bobs"]), guard=1)
    assert _assert_window(w2, ref)[6] == 0   # exactly enough
    G.close()


TABLE_FIELDS = ("kf_Tcw", "kf_bad", "kf_init", "kf_keys_un", "inv_level_sigma2", "mp_xw", "kf_nb", "kf_mpb", "kf_bird_octave", "kf_bird_xc",
                "mpb_bad", "mpb_xw", "bobs_mpb", "bobs_kf", "bobs_idx")


def test_host_pointer_variant_equals_the_device_variant():
    import fishbirdeyevisualslam_amd as fb
    p = P.make_window_problem(K=70, S=96)
    g, G, dm, dt = _graphs(p, p["used"])
    ref = LW.local_window(g, p, p["cur"], True)
    wd = G.local_window(dm, dt, p["cur"], True)
    m, keep = _host_map(p)
    tk = {k: np.ascontiguousarray(p[k]) for k in TABLE_FIELDS}
    t = cabi.CovisKfTables()
    cabi.fill(t, n_levels=len(tk["inv_level_sigma2"]), bird_stride=p["BS"], n_mpb=len(tk["mpb_bad"]), n_bobs=len(tk["bobs_kf"]), **tk)
    n = _counts(ref["header"])
    out = {}
    for name, cnt, width in LISTS:
        dtp = wd[name].cpu().numpy().dtype
        out[name] = np.full((n[cnt] + 4) * width, 77, dtp)
    out["header"] = np.zeros(8, np.int32)
    w = cabi.CovisWindow()
    cabi.fill(w, cap_kf=n["n_kf"] + 4, cap_mp=n["n_mp"] + 4, cap_obs=n["n_obs"] + 4, cap_mpb=n["n_mpb"] + 4, cap_bobs=n["n_bobs"] + 4, **out)
    rc = fb.lib().fb_covis_local_window(G.h, C.byref(m), C.byref(t), int(p["cur"]), 1, C.byref(w))
    assert rc == 0, fb.lib().fb_last_error()
    _assert_window(out, ref)
    for name, cnt, width in LISTS:
        np.testing.assert_array_equal(out[name][:n[cnt] * width], wd[name].cpu().numpy()[:n[cnt] * width], err_msg=name)
        assert (out[name][n[cnt] * width:] == 77).all(), name      # entries past the counts keep the caller's contents
    w.cap_obs = 3
    assert fb.lib().fb_covis_local_window(G.h, C.byref(m), C.byref(t), int(p["cur"]), 1, C.byref(w)) == cabi.FB_ERR_CAPACITY
    G.close()


def _odometry(q, slot, kf_slot, n_local):
    """the BA problem's odometry edges between local key frames, as indices into the window's key frame list"""
    widx = {int(s): w for w, s in enumerate(kf_slot[:n_local])}
    keep = [e for e in range(len(q["odom_kf_i"])) if int(slot[q["odom_kf_i"][e]]) in widx and int(slot[q["odom_kf_j"][e]]) in widx]
    return dict(odom_kf_i=np.array([widx[int(slot[q["odom_kf_i"][e]])] for e in keep], np.int32),
                odom_kf_j=np.array([widx[int(slot[q["odom_kf_j"][e]])] for e in keep], np.int32),
                odom_Tij=np.ascontiguousarray(q["odom_Tij"][keep], np.float32), odom_info=np.ascontiguousarray(q["odom_info"][keep]))


def test_window_feeds_the_ba_on_the_device_and_scatters_back():
    """window -> host odometry edges -> fb_local_ba_dev on the window's device arrays -> scatter, against fb_local_ba on the
    model's lists (the two BA entry points agree bit for bit, tests/test_ba_gpu.py) and the model's write-back."""
    import torch
    import fishbirdeyevisualslam_amd as fb
    from fishbirdeyevisualslam_amd import ba_problem
    p, q, slot = P.make_window_ba_problem()
    g, G, dm, dt = _graphs(p, p["used"])
    cur = p["cur"]
    ref = LW.local_window(g, p, cur, True)
    n = _counts(ref["header"])
    assert 2 <= n["n_local"] - int(ref["kf_fixed"][:n["n_local"]].sum()) <= 23 and n["n_fixed"] >= 1 and 100 <= n["n_mp"] <= 999
    before = {k: dt.t[k].clone() for k in ("kf_Tcw", "mp_xw", "mpb_xw")}
    w = G.local_window(dm, dt, cur, True)
    rc, hd, kf_slot, kf_fixed = G.window_header()
    assert rc == 0 and [hd[k] for k in HEADER] == ref["header"]
    odom = _odometry(q, slot, kf_slot, hd["n_local"])
    assert len(odom["odom_kf_i"]) >= 1
    outl = torch.full((max(hd["n_obs"], 1),), 9, dtype=torch.uint8, device="cuda:0")
    boutl = torch.full((max(hd["n_bobs"], 1),), 9, dtype=torch.uint8, device="cuda:0")
    a = cabi.LocalBAArgs()
    keep = dict(kf_fixed=np.ascontiguousarray(kf_fixed), **odom)
    cabi.fill(a, with_odom=1, fx=q["fx"], fy=q["fy"], cx=q["cx"], cy=q["cy"], wF=1.0, wB=1.0, wP=q["wP"], n_kf=len(kf_slot), n_mp=hd["n_mp"],
              n_mpb=hd["n_mpb"], n_obs=hd["n_obs"], n_bobs=hd["n_bobs"], n_odom=len(odom["odom_kf_i"]), obs_outlier=outl, bobs_outlier=boutl,
              **{k: w[k] for k in ("kf_Tcw", "mp_xw", "mpb_xw", "obs_kf", "obs_mp", "obs_uv", "obs_inv_sigma2", "bobs_kf", "bobs_mpb", "bobs_xc",
                                   "bobs_inv_sigma2")}, **keep)
    rc = fb.lib().fb_local_ba_dev(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, fb.lib().fb_last_error()
    # the same graph from the model's lists through the host entry point
    hp = dict(fx=q["fx"], fy=q["fy"], cx=q["cx"], cy=q["cy"], wP=q["wP"], **{k: ref[k] for k in (
        "kf_Tcw", "kf_fixed", "mp_xw", "mpb_xw", "obs_kf", "obs_mp", "obs_uv", "obs_inv_sigma2", "bobs_kf", "bobs_mpb", "bobs_xc",
        "bobs_inv_sigma2")}, **_odometry(q, slot, ref["kf_slot"], ref["n_local"]))
    ah, out_h, keep_h = ba_problem.local_ba_args(hp, with_odom=1)
    assert fb.lib().fb_local_ba(C.byref(ah)) == 0
    got = {k: w[k].cpu().numpy() for k in ("kf_Tcw", "mp_xw", "mpb_xw")}
    np.testing.assert_array_equal(got["kf_Tcw"][:n["n_kf"] * 12], out_h["kf_Tcw"].reshape(-1))
    np.testing.assert_array_equal(got["mp_xw"][:n["n_mp"] * 3], out_h["mp_xw"].reshape(-1))
    np.testing.assert_array_equal(got["mpb_xw"][:n["n_mpb"] * 3], out_h["mpb_xw"].reshape(-1))
    o, bo = outl.cpu().numpy()[:n["n_obs"]], boutl.cpu().numpy()[:n["n_bobs"]]
    np.testing.assert_array_equal(o, out_h["obs_outlier"][:n["n_obs"]])
    np.testing.assert_array_equal(bo, out_h["bobs_outlier"][:n["n_bobs"]])
    assert o.sum() >= 1 and np.abs(out_h["kf_Tcw"] - ref["kf_Tcw"]).max() > 0                          # the BA did something
    n_er, er, ber = G.window_scatter(dm, dt, w, outl, boutl)
    wb = LW.write_back(ref, p, out_h["kf_Tcw"], out_h["mp_xw"], out_h["mpb_xw"], o, bo)
    n_er = n_er.cpu().numpy().tolist()
    assert n_er == [len(wb["erase"]), len(wb["berase"])]
    np.testing.assert_array_equal(er.cpu().numpy()[:n_er[0]], wb["erase"])
    np.testing.assert_array_equal(ber.cpu().numpy()[:n_er[1]], wb["berase"])
    # slots and points outside the window, and the fixed cameras, bit-identical to before (the model's write-back leaves them)
    for k in ("kf_Tcw", "mp_xw", "mpb_xw"):
        np.testing.assert_array_equal(dt.t[k].cpu().numpy().reshape(-1), wb[k].reshape(-1), err_msg=k)
    fixed_slots = ref["kf_slot"][ref["n_local"]:]
    np.testing.assert_array_equal(dt.t["kf_Tcw"].cpu().numpy().reshape(-1, 12)[fixed_slots], before["kf_Tcw"].cpu().numpy().reshape(-1, 12)[fixed_slots])
    outside = np.setdiff1d(np.arange(len(p["mp_bad"])), ref["mp_index"])
    np.testing.assert_array_equal(dt.t["mp_xw"].cpu().numpy().reshape(-1, 3)[outside], before["mp_xw"].cpu().numpy().reshape(-1, 3)[outside])
    G.close()


def test_host_header_window_builds_and_runs():
    """tests/cpp/window_host_test.cpp drives fishbird::LocalWindow (host/fishbird_host.hpp) in a fresh child process."""
    import fishbirdeyevisualslam_amd as fb
    pkg = os.path.dirname(fb.LIB_PATH)
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "window_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"),
                           os.path.join(ROOT, "tests", "cpp", "window_host_test.cpp"), "-o", exe, "-L", pkg, "-lfishbird_hip",
                           "-Wl,-rpath," + pkg])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"window_host_test ok" in r.stdout
