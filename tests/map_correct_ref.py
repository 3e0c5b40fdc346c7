"""A literal Python restatement of the two places where the loop closer rewrites the map, written from the reference (not
from the kernels) on top of covis_ref.Graph and local_map_ref.Tree.  Test infrastructure: the package never imports it.

    LoopClosing::CorrectLoop, Sim3 propagation and pose write       src/LoopClosing.cc:438-541
    MapPoint::UpdateNormalAndDepth                                   src/MapPoint.cc:330-371
    KeyFrame::SetPose                                                src/KeyFrame.cc:104-118
    LoopClosing::RunGlobalBundleAdjustment, the map update           src/LoopClosing.cc:714-825
    g2o::Sim3                                                        Thirdparty/g2o/g2o/types/sim3.h:64, :144, :233, :266

Seams: a cv::Mat (CV_32F) product accumulates in double and rounds once; CV_32F additions and subtractions are float;
cv::norm is double; Mat / scalar multiplies by the float reciprocal; the Sim3 algebra is double, with Eigen's
Quaterniond(R), toRotationMatrix, q * v and q * q restated from their published algorithms.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64


# ---- Eigen quaternions (x, y, z, w) in double ----------------------------------------------------------------------------
def quat_from_R(R):
    R = np.asarray(R, f64)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = [0.0] * 4
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return np.array(q, f64)


def quat_to_R(q):
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]], f64)


def quat_rotate(q, v):
    qv = np.asarray(q[:3], f64)
    uv = np.cross(qv, v)
    uv = uv + uv
    return v + q[3] * uv + np.cross(qv, uv)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], f64)


class Sim3:
    def __init__(self, r, t, s):
        self.r, self.t, self.s = np.asarray(r, f64), np.asarray(t, f64), float(s)

    @staticmethod
    def from_Rt(R, t, s):                                                                              # sim3.h:64: Quaterniond(R), not normalised
        return Sim3(quat_from_R(np.asarray(R, f64)), np.asarray(t, f64), s)

    def map(self, xyz):                                                                                # :144
        return self.s * quat_rotate(self.r, np.asarray(xyz, f64)) + self.t

    def inverse(self):                                                                                 # :233
        c = np.array([-self.r[0], -self.r[1], -self.r[2], self.r[3]], f64)
        return Sim3(c, quat_rotate(c, (-1. / self.s) * self.t), 1. / self.s)

    def __mul__(self, o):                                                                              # :266
        return Sim3(quat_mul(self.r, o.r), self.s * quat_rotate(self.r, o.t) + self.t, self.s * o.s)


# ---- cv::Mat seams ---------------------------------------------------------------------------------------------------------
def cv_mul(A, B):
    """CV_32F product: double accumulation, one term after the other, rounded once"""
    A, B = np.asarray(A, f32).astype(f64), np.asarray(B, f32).astype(f64)
    acc = np.zeros((A.shape[0], B.shape[1]), f64)
    for k in range(A.shape[1]):
        acc = acc + A[:, k:k + 1] * B[k:k + 1, :]
    return acc.astype(f32)


def T44(T12):
    return np.vstack([np.asarray(T12, f32).reshape(3, 4), np.array([[0, 0, 0, 1]], f32)])


def set_pose(T12):
    """KeyFrame::SetPose (KeyFrame.cc:104-118) -> (Twc 4x4, Ow 3)"""
    T = T44(T12)
    Rwc = T[:3, :3].T.copy()
    Ow = -cv_mul(Rwc, T[:3, 3:4])
    Twc = np.eye(4, dtype=f32)
    Twc[:3, :3] = Rwc
    Twc[:3, 3] = Ow[:, 0]
    return Twc, Ow[:, 0].copy()


def cv_norm(v):
    v = np.asarray(v, f32).astype(f64)
    return math.sqrt(float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))


def edge_errors(m):
    """the edges the point -> edge index skips and counts when it is built"""
    n = 0
    for mp, kf, idx in zip(m.obs_mp.tolist(), m.obs_kf.tolist(), m.obs_idx.tolist()):
        if kf >= 0 and (kf >= m.K or mp < 0 or mp >= m.n_mp or idx < 0 or idx >= m.S):
            n += 1
    return n


# ---- LoopClosing::CorrectLoop ----------------------------------------------------------------------------------------------------
def correct_loop(g, m, c, cur, q, t, s):
    """:438-541 on copies of the arrays of the case c (kf_Tcw, mp_xw, mp_ref_kf, mp_normal, mp_min_dist, mp_max_dist,
    scale_factors and, with "kf_mpb", kf_nb, mpb_bad, mpb_xw) -> dict of the arrays after, the integer outputs and the
    entries skipped as out of range (without the edges, see edge_errors)."""
    K = g.K
    kf_Tcw = np.array(c["kf_Tcw"], f32).reshape(-1, 12)
    mp_xw = np.array(c["mp_xw"], f32).reshape(-1, 3)
    normal = np.array(c["mp_normal"], f32).reshape(-1, 3)
    mind, maxd = np.array(c["mp_min_dist"], f32), np.array(c["mp_max_dist"], f32)
    scale = np.asarray(c["scale_factors"], f32)
    bird = "kf_mpb" in c
    mpb_xw = np.array(c["mpb_xw"], f32).reshape(-1, 3) if bird else None
    obs = m.observations()
    errors = 0
    corrected_ref = np.full(m.n_mp, -1, np.int32)
    corrected_by = [False] * m.n_mp                                                                    # mnCorrectedByKF == mpCurrentKF->mnId
    Scw = Sim3(q, t, s)

    def centre(kf):                                                                                    # GetCameraCenter() right now
        return set_pose(kf_Tcw[kf])[1]

    def update_normal_and_depth(mp):                                                                   # MapPoint.cc:330-371
        nonlocal errors
        observations = dict(obs[mp])
        if not observations:                                                                           # :345
            return
        pRefKF = int(c["mp_ref_kf"][mp])
        if pRefKF < 0 or pRefKF >= K:
            errors += 1
            return
        Pos = mp_xw[mp].copy()
        nrm, n = np.zeros(3, f32), 0
        for pKF in sorted(observations, key=g.key):                                                    # :350
            normali = (Pos - centre(pKF)).astype(f32)
            nrm = (nrm + normali * f32(1.0 / cv_norm(normali))).astype(f32)
            n += 1
        PC = (Pos - centre(pRefKF)).astype(f32)
        dist = f32(cv_norm(PC))
        level = int(m.kf_octave[pRefKF, observations.get(pRefKF, 0)])                                  # :361: operator[] inserts 0
        if level >= len(scale):
            errors += 1
            return
        maxd[mp] = f32(dist * scale[level])                                                            # :367-369
        mind[mp] = f32(maxd[mp] / scale[len(scale) - 1])
        normal[mp] = (nrm * f32(1.0 / n)).astype(f32)

    conn = g.get_vector_covisible_keyframes(cur) + [cur]                                               # :438-439
    Corrected, NonCorrected = {cur: Scw}, {}
    Twc = set_pose(kf_Tcw[cur])[0]                                                                     # :443
    for pKFi in conn:                                                                                  # :450
        Tiw = T44(kf_Tcw[pKFi])
        if pKFi != cur:
            Tic = cv_mul(Tiw, Twc)
            Corrected[pKFi] = Sim3.from_Rt(Tic[:3, :3], Tic[:3, 3], 1.0) * Scw
        NonCorrected[pKFi] = Sim3.from_Rt(Tiw[:3, :3], Tiw[:3, 3], 1.0)
    order = sorted(Corrected, key=g.key)                                                               # a std::map<KeyFrame*, Sim3>
    for pKFi in order:                                                                                 # :475
        Siw_c = Corrected[pKFi]
        Swi_c, Siw = Siw_c.inverse(), NonCorrected[pKFi]
        for i in range(min(max(int(m.kf_n[pKFi]), 0), m.S)):                                           # :484
            mp = int(m.kf_mp[pKFi, i])
            if mp < 0:
                continue
            if mp >= m.n_mp:
                errors += 1
                continue
            if m.mp_bad[mp] or corrected_by[mp]:
                continue
            mp_xw[mp] = Swi_c.map(Siw.map(mp_xw[mp].astype(f64))).astype(f32)                          # :495-500
            corrected_by[mp] = True
            corrected_ref[mp] = pKFi
            update_normal_and_depth(mp)                                                                # :503
        if bird:
            BS = c["kf_mpb"].shape[1]
            for i in range(min(max(int(c["kf_nb"][pKFi]), 0), BS)):                                    # :507
                mpb = int(c["kf_mpb"][pKFi, i])
                if mpb < 0:
                    continue
                if mpb >= len(c["mpb_bad"]):
                    errors += 1
                    continue
                if c["mpb_bad"][mpb]:
                    continue
                mpb_xw[mpb] = Swi_c.map(Siw.map(mpb_xw[mpb].astype(f64))).astype(f32)                  # :517-523: the == marks nothing
        R = quat_to_R(Siw_c.r)                                                                         # :529-537
        eigt = Siw_c.t * (1. / Siw_c.s)
        kf_Tcw[pKFi] = np.hstack([R.astype(f32), eigt.astype(f32)[:, None]]).reshape(12)
    return dict(kf_Tcw=kf_Tcw, mp_xw=mp_xw, mpb_xw=mpb_xw, mp_normal=normal, mp_min_dist=mind, mp_max_dist=maxd,
                mp_corrected_ref=corrected_ref, set_slots=np.array(order, np.int32), n_set=len(order), errors=errors)


# ---- RunGlobalBundleAdjustment, the map update ---------------------------------------------------------------------------------------
def propagate_gba(tree, m, c):
    """:714-825 on copies of the arrays of the case c (kf_Tcw, mp_xw, origins, kf_gba, kf_Tcw_gba, kf_Tcw_bef, mp_gba, mp_pos_gba,
    mp_ref_kf and, with "mpb_xw", mpb_bad, mpb_gba, mpb_pos_gba, mpb_ref_kf)."""
    K = tree.g.K
    kf_Tcw = np.array(c["kf_Tcw"], f32).reshape(-1, 12)
    gba, Tgba, Tbef = np.array(c["kf_gba"], np.uint8), np.array(c["kf_Tcw_gba"], f32).reshape(-1, 12), np.array(c["kf_Tcw_bef"], f32).reshape(-1, 12)
    mp_xw = np.array(c["mp_xw"], f32).reshape(-1, 3)
    errors = 0
    reached = np.zeros(K, np.uint8)
    lpKFtoCheck, seen = [], set()
    for o in [int(x) for x in c["origins"]]:                                                           # the precondition, checked
        if o < 0 or o >= K or tree.parent[o] != -1 or o in seen:
            errors += 1
            continue
        seen.add(o)
        lpKFtoCheck.append(o)
    while lpKFtoCheck:                                                                                 # :717
        pKF = lpKFtoCheck[0]
        Twc = set_pose(kf_Tcw[pKF])[0]                                                                 # :721
        for pChild in tree.get_childs(pKF):
            if not gba[pChild]:                                                                        # :726
                Tchildc = cv_mul(T44(kf_Tcw[pChild]), Twc)
                Tgba[pChild] = cv_mul(Tchildc, T44(Tgba[pKF]))[:3].reshape(12)
                gba[pChild] = 1
            lpKFtoCheck.append(pChild)
        Tbef[pKF] = kf_Tcw[pKF]                                                                        # :736-737
        kf_Tcw[pKF] = Tgba[pKF]
        reached[pKF] = 1
        lpKFtoCheck.pop(0)

    def points(xw, bad, flag, pos, ref_kf, is_bird):
        nonlocal errors
        for i in range(len(bad)):
            if bad[i]:
                continue
            if flag[i]:
                xw[i] = np.asarray(pos, f32).reshape(-1, 3)[i]
                continue
            pRefKF = int(ref_kf[i])
            if is_bird and pRefKF == -1:                                                               # :799-803
                continue
            if pRefKF < 0 or pRefKF >= K:
                errors += 1
                continue
            if not gba[pRefKF]:
                continue
            Tb = T44(Tbef[pRefKF])
            Xc = (cv_mul(Tb[:3, :3], xw[i][:, None])[:, 0] + Tb[:3, 3]).astype(f32)                    # :768-770
            Twc = set_pose(kf_Tcw[pRefKF])[0]
            xw[i] = (cv_mul(Twc[:3, :3], Xc[:, None])[:, 0] + Twc[:3, 3]).astype(f32)                  # :773-777

    points(mp_xw, m.mp_bad, c["mp_gba"], c["mp_pos_gba"], c["mp_ref_kf"], False)
    mpb_xw = None
    if "mpb_xw" in c and c.get("mpb_gba") is not None:
        mpb_xw = np.array(c["mpb_xw"], f32).reshape(-1, 3)
        points(mpb_xw, c["mpb_bad"], c["mpb_gba"], c["mpb_pos_gba"], c["mpb_ref_kf"], True)
    return dict(kf_Tcw=kf_Tcw, kf_gba=gba, kf_Tcw_gba=Tgba, kf_Tcw_bef=Tbef, reached=reached, mp_xw=mp_xw, mpb_xw=mpb_xw, errors=errors)
