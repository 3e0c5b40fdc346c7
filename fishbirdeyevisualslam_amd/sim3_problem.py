"""Synthetic problems + C-ABI argument builder for the Sim3Solver entry points (fb_sim3_solver*).

One key frame KF1 and C loop candidates observe one scene.  Each candidate's map is a similarity-transformed copy of KF1's
(the drift a loop closure corrects), so the camera-frame points obey X3Dc1 = s12 R12 X3Dc2 + t12 with a known (s12, R12, t12).
The solver never sees key points, only map points: "pixel noise" is 3-D noise on the candidate's points sized to move their
projection by that many pixels.  A chosen share of the matches points at a wrong map point.  Planted cases: matches whose
KF1 point is NULL / bad, whose KF2 point is bad, whose GetIndexInKeyFrame is -1 on either side; mixed octaves; exact
correspondence counts per candidate (below, at and above min_inliers)."""
import numpy as np

from . import cabi, synth
from .cabi import fill

W, H = 1280, 720
FX, FY = 500.0, 500.0
RAND_MAX = 2147483647


def random_int_table(g, n_corr, n_hyp=cabi.FB_SIM3_MAX_HYP):
    """[n_hyp][3] values of DUtils::Random::RandomInt(0, size-1) = int((rand()/(RAND_MAX+1.0))*d)+min for the three draws of
    an iteration (size = N, N-1, N-2), rand() taken from the seeded generator g."""
    out = np.zeros((n_hyp, 3), np.int32)
    if n_corr < 3:
        return out
    r = g.integers(0, RAND_MAX + 1, (n_hyp, 3)).astype(np.float64)
    for j in range(3):
        d = n_corr - j
        out[:, j] = (r[:, j] / (RAND_MAX + 1.0) * d).astype(np.int32) + 0
    return out


def _sim3_between(T1, T2, Sg):
    """X3Dc1 = s R X3Dc2 + t for Xw2 = Sg(Xw1) = sg Rg Xw1 + tg, all in double."""
    sg, Rg, tg = Sg
    R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
    # Xw1 = Rg^T (Xw2 - tg) / sg ; Xw2 = R2^T (Xc2 - t2)
    A = R1 @ Rg.T @ R2.T / sg
    b = t1 - R1 @ Rg.T @ (R2.T @ t2 + tg) / sg
    s = 1.0 / sg
    return s, A / s, b


def make_problem(seed, n_corr, n1=1000, n2=1000, outlier_share=0.2, pixel_noise=0.5, fix_scale=0, scale=1.08, plants=True,
                 min_inliers=20, max_iterations=cabi.FB_SIM3_MAX_HYP, n_outliers=None):
    """n_corr: correspondences the constructor keeps, one entry per candidate.  n_outliers: exact number of wrong matches per
    candidate (a list), in place of the random outlier_share."""
    g = synth.rng(seed)
    C = len(n_corr)
    cx, cy = W / 2.0, H / 2.0
    T1 = synth.random_pose(g)
    u = g.uniform(40, W - 40, n1)
    v = g.uniform(40, H - 40, n1)
    z = g.uniform(3.0, 25.0, n1)
    Xc1 = np.stack([(u - cx) / FX * z, (v - cy) / FY * z, z], 1)
    Xw1 = (T1[:3, :3].T @ (Xc1 - T1[:3, 3]).T).T
    kps1 = synth.random_keypoints(g, n1, W, H)
    kps1["octave"] = g.integers(0, 8, n1)
    valid1 = np.ones(n1, np.uint8)
    index1 = np.arange(n1, dtype=np.int32)
    n_plant = 6 if plants else 0
    # KF1-side plants are shared by every candidate (KF1 is): NULL / bad points and GetIndexInKeyFrame = -1
    perm0 = g.permutation(n1)
    null1, noindex1, rest1 = perm0[:n_plant], perm0[n_plant:2 * n_plant], perm0[2 * n_plant:]
    valid1[null1] = 0
    index1[noindex1] = -1
    cands, truth = [], []
    for c in range(C):
        nc = int(n_corr[c])
        assert nc + 4 * n_plant <= min(len(rest1), n2)
        T2 = synth.perturb_pose(g, T1, rot_sigma=0.03, t_sigma=0.3)
        sg = 1.0 / scale
        Rg = synth.perturb_pose(g, np.eye(4), rot_sigma=0.02, t_sigma=0.0)[:3, :3]
        tg = g.normal(0, 0.2, 3)
        s12, R12, t12 = _sim3_between(T1, T2, (sg, Rg, tg))
        perm1 = rest1[g.permutation(len(rest1))]
        slot2 = g.permutation(n2)
        i1s, j2s = perm1[:nc], slot2[:nc]
        # the candidate's other points: anywhere in front of its camera
        zz = g.uniform(3.0, 25.0, n2)
        Xc2r = np.stack([(g.uniform(40, W - 40, n2) - cx) / FX * zz, (g.uniform(40, H - 40, n2) - cy) / FY * zz, zz], 1)
        xw2 = (T2[:3, :3].T @ (Xc2r - T2[:3, 3]).T).T
        true2 = sg * (Xw1[i1s] @ Rg.T) + tg
        zc2 = (true2 @ T2[:3, :3].T + T2[:3, 3])[:, 2]
        xw2[j2s] = true2 + g.normal(0, 1.0, (nc, 3)) * (pixel_noise * np.abs(zc2) / FX)[:, None]
        is_out = g.random(nc) < outlier_share
        if n_outliers is not None:
            is_out = np.arange(nc) < int(n_outliers[c])
        m12 = np.full(n1, -1, np.int32)
        wrong = slot2[nc + 4 * n_plant:]
        is_out &= len(wrong) > 0
        for k in range(nc):
            m12[i1s[k]] = wrong[g.integers(0, len(wrong))] if is_out[k] else j2s[k]
        kps2 = synth.random_keypoints(g, n2, W, H)
        kps2["octave"] = g.integers(0, 8, n2)
        valid2 = np.ones(n2, np.uint8)
        index2 = np.arange(n2, dtype=np.int32)
        plant = {}
        if plants:  # matched features the constructor must skip (never among the nc kept ones); their geometry is true
            e1 = np.concatenate([null1, noindex1, perm1[nc:nc + 2 * n_plant]])
            e2 = slot2[nc:nc + 4 * n_plant]
            m12[e1] = e2
            xw2[e2] = sg * (Xw1[e1] @ Rg.T) + tg
            plant = dict(null1=null1, index1=noindex1, bad2=e2[2 * n_plant:3 * n_plant], index2=e2[3 * n_plant:], i1=e1)
            valid2[plant["bad2"]] = 0
            index2[plant["index2"]] = -1
        cands.append(dict(kps2=kps2, valid2=valid2, index2=index2, xw2=xw2.astype(np.float32), T2=synth.to12(T2), matches12=m12))
        truth.append(dict(s=s12, R=R12, t=t12, i1=i1s, j2=j2s, outlier=is_out, plant=plant))
    sf, _, sig2, _ = synth.scale_tables()
    p = dict(C=C, n1=n1, n2=n2, kps1=kps1, valid1=valid1, index1=index1, xw1=Xw1.astype(np.float32), T1=synth.to12(T1), cands=cands,
             truth=truth, level_sigma2=np.asarray(sig2, np.float32), fix_scale=int(fix_scale), fx=FX, fy=FY, cx=cx, cy=cy,
             ransac_prob=0.99, min_inliers=min_inliers, max_iterations=max_iterations)
    kept = [count_kept(p, c) for c in range(C)]
    gr = synth.rng(seed + 9001)
    p["rand_idx"] = np.stack([random_int_table(gr, kept[c]) for c in range(C)])
    p["n_kept"] = kept
    return p


def count_kept(p, c):
    """The constructor's N for candidate c, counted from the problem's own flags (the draws need it)."""
    cd = p["cands"][c]
    m = cd["matches12"]
    i1 = np.nonzero(m >= 0)[0]
    j = m[i1]
    ok = (p["valid1"][i1] != 0) & (cd["valid2"][j] != 0) & (p["index1"][i1] >= 0) & (cd["index2"][j] >= 0)
    return int(ok.sum())


def solver_args(p, accept_above=None, with_index=True):
    """-> (cabi.Sim3SolverArgs on host arrays, outputs dict, keepalive dict)"""
    C, n1, n2 = p["C"], p["n1"], p["n2"]
    mw = (n1 + 31) // 32
    MAXH = cabi.FB_SIM3_MAX_HYP
    keep = dict(n_kf1=np.array([n1], np.int32), kps1=np.ascontiguousarray(p["kps1"]),
                kps2=np.ascontiguousarray(np.stack([c["kps2"] for c in p["cands"]])),
                valid1=np.ascontiguousarray(p["valid1"]), xw1=np.ascontiguousarray(p["xw1"]),
                valid2=np.ascontiguousarray(np.stack([c["valid2"] for c in p["cands"]])),
                xw2=np.ascontiguousarray(np.stack([c["xw2"] for c in p["cands"]])),
                T1w=np.ascontiguousarray(p["T1"], np.float32), T2w=np.ascontiguousarray(np.stack([c["T2"] for c in p["cands"]]), np.float32),
                kf1_index=np.ascontiguousarray(p["index1"]), kf2_index=np.ascontiguousarray(np.stack([c["index2"] for c in p["cands"]])),
                matches12=np.ascontiguousarray(np.stack([c["matches12"] for c in p["cands"]])),
                rand_idx=np.ascontiguousarray(p["rand_idx"], np.int32))
    if accept_above is not None:
        keep["accept_above"] = np.ascontiguousarray(accept_above, np.int32)
    out = dict(N=np.full(C, -7, np.int32), indices1=np.full((C, n1), -7, np.int32), corr=np.zeros((C, n1), cabi.SIM3_CORR_DTYPE),
               max_its=np.full(C, -7, np.int32), n_hyp_done=np.full(C, -7, np.int32), first_accept=np.full(C, -7, np.int32),
               no_more=np.full(C, -7, np.int32), s=np.full((C, MAXH), -7.0, np.float32), R=np.full((C, MAXH, 9), -7.0, np.float32),
               t=np.full((C, MAXH, 3), -7.0, np.float32), n_inliers=np.full((C, MAXH), -7, np.int32),
               accept=np.full((C, MAXH), 9, np.uint8), inlier_mask=np.zeros((C, MAXH, mw), np.uint32))
    a = cabi.Sim3SolverArgs()
    fill(a, n_cand=C, T1w=keep["T1w"], T2w=keep["T2w"], matches12=keep["matches12"], rand_idx=keep["rand_idx"],
         level_sigma2=[float(x) for x in p["level_sigma2"]], fix_scale=p["fix_scale"], ransac_prob=p["ransac_prob"],
         min_inliers=p["min_inliers"], max_iterations=p["max_iterations"], **out)
    if with_index:
        fill(a, kf1_index=keep["kf1_index"], kf2_index=keep["kf2_index"])
    if accept_above is not None:
        fill(a, accept_above=keep["accept_above"])
    fill(a.kf1, kf_stride=n1, n_kf=keep["n_kf1"], kf_kps=keep["kps1"])
    fill(a.kf2, kf_stride=n2, kf_kps=keep["kps2"])
    for k in (a.kf1, a.kf2):
        fill(k.cam, fx=p["fx"], fy=p["fy"], cx=p["cx"], cy=p["cy"], min_x=0.0, min_y=0.0, max_x=float(W), max_y=float(H))
    fill(a.mp1, mp_stride=n1, mp_valid=keep["valid1"], mp_xw=keep["xw1"])
    fill(a.mp2, mp_stride=n2, mp_valid=keep["valid2"], mp_xw=keep["xw2"])
    return a, out, keep


# the pointer fields of Sim3SolverArgs by (sub-struct, field, key in `keep`), for callers that move the arrays to the device
INPUT_FIELDS = [("kf1", "n_kf", "n_kf1"), ("kf1", "kf_kps", "kps1"), ("kf2", "kf_kps", "kps2"), ("mp1", "mp_valid", "valid1"),
                ("mp1", "mp_xw", "xw1"), ("mp2", "mp_valid", "valid2"), ("mp2", "mp_xw", "xw2"), (None, "T1w", "T1w"), (None, "T2w", "T2w"),
                (None, "kf1_index", "kf1_index"), (None, "kf2_index", "kf2_index"), (None, "matches12", "matches12"),
                (None, "rand_idx", "rand_idx"), (None, "accept_above", "accept_above")]
OUTPUT_FIELDS = ["N", "indices1", "corr", "max_its", "n_hyp_done", "first_accept", "no_more", "s", "R", "t", "n_inliers", "accept",
                 "inlier_mask"]
