"""A literal Python restatement of the window of Optimizer::LocalBundleAdjustmentWithOdom, written from the reference (not
from the kernels) as the model the device is compared with.  Test infrastructure: the package never imports it.

    the local key frames, local points, fixed cameras (+ bird)     src/Optimizer.cc:2139-2227  (:838-889 without bird)
    the vertices and the edge loops                                 :2245-2284, :2312-2417
    the erase lists and the write-back                              :2574-2669

The walks mark what they have seen (mnBALocalForKF / mnBAFixedForKF) exactly as the C++ does, and a point's observations
iterate like std::map<KeyFrame*, size_t>: ascending kf_order.  The marks start "unset", which is the reference's state
for every current key frame except mnId == 0 (the documented precondition).
"""
import numpy as np

import covis_ref as R


def _observations(n_pt, K, S, e_pt, e_kf, e_idx):
    """mObservations of every point with the edge's index in the list: pt -> {kf: (idx, e)}"""
    obs = [dict() for _ in range(n_pt)]
    for e, (pt, kf, idx) in enumerate(zip(np.asarray(e_pt).tolist(), np.asarray(e_kf).tolist(), np.asarray(e_idx).tolist())):
        if kf < 0 or kf >= K or pt < 0 or pt >= n_pt or idx < 0 or idx >= S:
            continue
        obs[pt][kf] = (idx, e)
    return obs


def front_side(p):
    return dict(S=p["kf_mp"].shape[1], kf_n=p["kf_n"], kf_mp=p["kf_mp"], bad=p["mp_bad"], e_pt=p["obs_mp"], e_kf=p["obs_kf"],
                e_idx=p["obs_idx"], xw=p["mp_xw"])


def bird_side(p):
    return dict(S=p["kf_mpb"].shape[1], kf_n=p["kf_nb"], kf_mp=p["kf_mpb"], bad=p["mpb_bad"], e_pt=p["bobs_mpb"], e_kf=p["bobs_kf"],
                e_idx=p["bobs_idx"], xw=p["mpb_xw"])


def local_window(g, p, cur, with_bird):
    """g: covis_ref.Graph (the ordered lists); p: the map and the tables as numpy arrays (covis_problem.make_window_problem)."""
    K = len(p["kf_bad"])
    key = lambda kf: (int(p["kf_order"][kf]), kf)
    mnBALocalForKF, mnBAFixedForKF = [False] * K, [False] * K
    lLocalKeyFrames = [cur]                                                                            # :2142-2143
    mnBALocalForKF[cur] = True
    for pKFi in g.get_vector_covisible_keyframes(cur):                                                 # :2145-2152
        mnBALocalForKF[pKFi] = True
        if not p["kf_bad"][pKFi]:
            lLocalKeyFrames.append(pKFi)
    lFixedCameras = []
    sides = [front_side(p)] + ([bird_side(p)] if with_bird else [])
    lists = []
    for sd in sides:
        n_pt, S = len(sd["bad"]), sd["S"]
        obs = _observations(n_pt, K, S, sd["e_pt"], sd["e_kf"], sd["e_idx"])
        mark = [False] * n_pt
        lLocal = []
        for pKF in lLocalKeyFrames:                                                                    # :2156-2170, :2193-2211
            for i in range(min(max(int(sd["kf_n"][pKF]), 0), S)):
                pMP = int(sd["kf_mp"][pKF, i])
                if pMP < 0 or pMP >= n_pt:
                    continue
                if not sd["bad"][pMP] and not mark[pMP]:
                    lLocal.append(pMP)
                    mark[pMP] = True
        for pMP in lLocal:                                                                             # :2174-2188, :2213-2226
            for pKFi in sorted(obs[pMP], key=key):
                if not mnBALocalForKF[pKFi] and not mnBAFixedForKF[pKFi]:
                    mnBAFixedForKF[pKFi] = True
                    if not p["kf_bad"][pKFi]:
                        lFixedCameras.append(pKFi)
        lists.append((lLocal, obs))
    kf_slot = lLocalKeyFrames + lFixedCameras                                                          # :2246-2284
    vertex = {kf: w for w, kf in enumerate(kf_slot)}
    out = dict(kf_slot=np.array(kf_slot, np.int32),
               kf_fixed=np.array([int(p["kf_init"][kf]) for kf in lLocalKeyFrames] + [1] * len(lFixedCameras), np.uint8),
               kf_Tcw=np.asarray(p["kf_Tcw"], np.float32).reshape(K, 12)[kf_slot])
    for sd, (lLocal, obs), pre in zip(sides, lists, ("", "b")):
        e_kf, e_pt, e_src, e_idx, meas, inv = [], [], [], [], [], []
        for j, pMP in enumerate(lLocal):                                                               # :2312-2375, :2378-2417
            for pKFi in sorted(obs[pMP], key=key):
                if p["kf_bad"][pKFi]:
                    continue
                idx, e = obs[pMP][pKFi]
                e_kf.append(vertex[pKFi]); e_pt.append(j); e_src.append(e); e_idx.append(idx)
                if pre == "":
                    kp = p["kf_keys_un"][pKFi, idx]
                    meas.append((kp["x"], kp["y"]))
                    inv.append(p["inv_level_sigma2"][int(kp["octave"])])
                else:
                    meas.append(tuple(p["kf_bird_xc"][pKFi, idx]))
                    inv.append(p["inv_level_sigma2"][int(p["kf_bird_octave"][pKFi, idx])])
        names = ("mp_index", "mp_xw", "obs_kf", "obs_mp", "obs_src", "obs_idx", "obs_uv", "obs_inv_sigma2") if pre == "" else \
                ("mpb_index", "mpb_xw", "bobs_kf", "bobs_mpb", "bobs_src", "bobs_idx", "bobs_xc", "bobs_inv_sigma2")
        vals = (np.array(lLocal, np.int32), np.asarray(sd["xw"], np.float32).reshape(-1, 3)[lLocal],
                np.array(e_kf, np.int32), np.array(e_pt, np.int32), np.array(e_src, np.int32), np.array(e_idx, np.int32),
                np.array(meas, np.float32).reshape(-1, 2 if pre == "" else 3), np.array(inv, np.float32))
        out.update(zip(names, vals))
    if not with_bird:
        out.update(mpb_index=np.zeros(0, np.int32), mpb_xw=np.zeros((0, 3), np.float32), bobs_kf=np.zeros(0, np.int32),
                   bobs_mpb=np.zeros(0, np.int32), bobs_src=np.zeros(0, np.int32), bobs_idx=np.zeros(0, np.int32),
                   bobs_xc=np.zeros((0, 3), np.float32), bobs_inv_sigma2=np.zeros(0, np.float32))
    out["n_local"], out["n_fixed"] = len(lLocalKeyFrames), len(lFixedCameras)
    out["header"] = [out["n_local"], out["n_fixed"], len(out["mp_index"]), len(out["obs_kf"]), len(out["mpb_index"]),
                     len(out["bobs_kf"]), 0]
    return out


def write_back(w, p, kf_Tcw, mp_xw, mpb_xw, obs_outlier, bobs_outlier):
    """:2574-2669 on the model's window w: the optimised values go back into copies of the tables; the erase lists are rows
    (key frame slot, point index, feature index, edge index) in edge order."""
    out = dict(kf_Tcw=np.array(p["kf_Tcw"], np.float32).reshape(-1, 12).copy(), mp_xw=np.array(p["mp_xw"], np.float32).copy(),
               mpb_xw=np.array(p["mpb_xw"], np.float32).copy() if "mpb_xw" in p else None)
    erase = [(int(w["kf_slot"][w["obs_kf"][i]]), int(w["mp_index"][w["obs_mp"][i]]), int(w["obs_idx"][i]), int(w["obs_src"][i]))
             for i in range(len(w["obs_kf"])) if obs_outlier[i]]                                        # :2579-2596
    berase = [(int(w["kf_slot"][w["bobs_kf"][i]]), int(w["mpb_index"][w["bobs_mpb"][i]]), int(w["bobs_idx"][i]), int(w["bobs_src"][i]))
              for i in range(len(w["bobs_kf"])) if bobs_outlier[i]]                                     # :2600-2610
    for k in range(w["n_local"]):                                                                      # :2640-2653
        out["kf_Tcw"][w["kf_slot"][k]] = np.asarray(kf_Tcw).reshape(-1, 12)[k]
    for j, mp in enumerate(w["mp_index"]):                                                             # :2656-2662
        out["mp_xw"][mp] = np.asarray(mp_xw).reshape(-1, 3)[j]
    for j, mp in enumerate(w["mpb_index"]):                                                            # :2664-2669
        out["mpb_xw"][mp] = np.asarray(mpb_xw).reshape(-1, 3)[j]
    out["erase"] = np.array(erase, np.int32).reshape(-1, 4)
    out["berase"] = np.array(berase, np.int32).reshape(-1, 4)
    return out
