// match_kf.inc -- the remaining ORBmatcher entry points (SURVEY M10) + MapPoint::ComputeDistinctiveDescriptors.
// Included at the end of match.hip (shares its LDS staging, grid walk and histogram helpers).
//
// Replaces (reference file:line):
//   ORBmatcher::Fuse(pKF, vpMapPoints, th)                        src/ORBmatcher.cc:826-976    (search half)
//   ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)      src/ORBmatcher.cc:978-1101   (search half)
//   ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched) src/ORBmatcher.cc:291-404
//   ORBmatcher::SearchBySim3                                      src/ORBmatcher.cc:1103-1327
//   ORBmatcher::SearchForInitialization                           src/ORBmatcher.cc:406-521
//   MapPoint::ComputeDistinctiveDescriptors                       src/MapPoint.cc:242-307
//
// Layout as in match.hip: one workgroup per problem, the searched key frame staged once in LDS, one lane per query.

namespace {

enum { MODE_FUSE = 0, MODE_FUSE_SIM3 = 1, MODE_PROJ_SIM3 = 2 };

struct KfTargetLds {
  TargetLds T;
  int n;
};

__device__ __forceinline__ Carve kf_carve(const fb_kf_target &K, bool withDesc) {
  return Carve(K.kf_stride, K.grid.cols * K.grid.rows, withDesc);
}
__device__ __forceinline__ KfTargetLds stage_kf(uint8_t *smem, const Carve &cv, const fb_kf_target &K, int b, bool withDesc) {
  const int ncell = K.grid.cols * K.grid.rows;
  const size_t o = (size_t)b * K.kf_stride;
  KfTargetLds r;
  r.n = K.n_kf[b];
  r.T = stage_target(smem, cv, r.n, ncell, K.kf_kps + o, K.kf_desc + o * 32, K.kf_cell_start + (size_t)b * (ncell + 1),
                     K.kf_cell_items + o, withDesc);
  return r;
}

// Scw -> Rcw | tcw, Ow (ORBmatcher.cc:300-304, :987-991)
__device__ __forceinline__ void decompose_sim3(const float *S, float *T, float *Ow) {
  double dot = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) dot += (double)S[k] * (double)S[k];
  const float scw = (float)sqrt(dot);
  const float inv = (float)(1.0 / (double)scw);
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = S[i] * inv;
  fb::camera_centre(T, Ow);
}

__device__ __forceinline__ bool is_in_image(const fb_camera &c, float x, float y) {  // KeyFrame.cc:942-945
  return x >= c.min_x && x < c.max_x && y >= c.min_y && y < c.max_y;
}

// geometric gates of :843-889 / :1007-1047 / :317-357 for one map point; level < 0 = rejected
template <int MODE>
__device__ __forceinline__ int gate_point(const fb_kf_target &K, const float *T, const float *Ow, const fb_mp_list &M,
                                          size_t e, float &u, float &v) {
  const float X[3] = {M.mp_xw[e * 3], M.mp_xw[e * 3 + 1], M.mp_xw[e * 3 + 2]};
  float pc[3];
  xform(T, X, pc);
  if (pc[2] < 0.0f) return -1;
  const float invz = MODE == MODE_FUSE_SIM3 ? (float)(1.0 / pc[2]) : 1.0f / pc[2];
  const float x = pc[0] * invz, y = pc[1] * invz;
  u = K.cam.fx * x + K.cam.cx;
  v = K.cam.fy * y + K.cam.cy;
  if (!is_in_image(K.cam, u, v)) return -1;
  const float maxD = M.mp_max_dist[e];
  const float PO0 = X[0] - Ow[0], PO1 = X[1] - Ow[1], PO2 = X[2] - Ow[2];
  const float dist3D = fb::norm3(PO0, PO1, PO2);
  if (dist3D < 0.8f * M.mp_min_dist[e] || dist3D > 1.2f * maxD) return -1;
  double dot = 0.0;
  dot += (double)PO0 * (double)M.mp_normal[e * 3];
  dot += (double)PO1 * (double)M.mp_normal[e * 3 + 1];
  dot += (double)PO2 * (double)M.mp_normal[e * 3 + 2];
  if (dot < 0.5 * dist3D) return -1;
  return fb::predict_scale(maxD, dist3D, K.log_scale_factor, K.n_levels);
}

// best key point for one gated map point
template <int MODE, typename Blocked>
__device__ __forceinline__ int search_point(const fb_kf_target &K, const TargetLds &T, const uint8_t *mp_desc, float u, float v,
                                            int lvl, float th, Blocked blocked) {
  const float radius = th * K.scale_factors[lvl];
  uint32_t d[8];
  fb::load_desc(mp_desc, d);
  int bestDist = MODE == MODE_FUSE_SIM3 ? INT_MAX : 256, best = NONE;
  for_area<false>(K.grid, T, u, v, radius, -1, -1, [&](int idx) {
    if (blocked(idx)) return;
    const int kpLevel = T.oct[idx];
    if (kpLevel < lvl - 1 || kpLevel > lvl) return;
    if (MODE == MODE_FUSE) {  // mono reprojection gate, :917-926
      const float2 p = T.xy[idx];
      const float ex = u - p.x, ey = v - p.y;
      const float e2 = ex * ex + ey * ey;
      if ((double)(e2 * K.inv_level_sigma2[kpLevel]) > 5.99) return;
    }
    const int dist = target_hamming(T, d, idx);
    if (dist < bestDist) { bestDist = dist; best = idx; }
  });
  if (bestDist > TH_LOW) best = NONE;
  return best;
}

template <int MODE>
__global__ __launch_bounds__(MATCH_THREADS) void k_fuse_search(fb_fuse_args A, int descInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const KfTargetLds KT = stage_kf(smem, kf_carve(A.kf, descInLds != 0), A.kf, b, descInLds != 0);
  struct Shared { float T[12], Ow[3]; };
  __shared__ Shared s_;
  static_assert(up16(sizeof(Shared)) == STATIC_FUSE, "match_plan.h");
  auto &s_T = s_.T; auto &s_Ow = s_.Ow;
  if (tid == 0) {
    if (MODE == MODE_FUSE) {
      for (int i = 0; i < 12; i++) s_T[i] = A.pose[(size_t)b * 12 + i];
      for (int i = 0; i < 3; i++) s_Ow[i] = A.Ow[(size_t)b * 3 + i];
    } else {
      decompose_sim3(A.pose + (size_t)b * 12, s_T, s_Ow);
    }
  }
  __syncthreads();
  const size_t mo = (size_t)b * A.mp.mp_stride;
  const int nmp = A.mp.n_mp[b];
  for (int q = tid; q < nmp; q += nt) {
    int best = NONE;
    if (A.mp.mp_valid[mo + q]) {
      float u, v;
      const int lvl = gate_point<MODE>(A.kf, s_T, s_Ow, A.mp, mo + q, u, v);
      if (lvl >= 0) best = search_point<MODE>(A.kf, KT.T, A.mp.mp_desc + (mo + q) * 32, u, v, lvl, A.th, [](int) { return false; });
    }
    A.best_idx[mo + q] = best == NONE ? -1 : best;
  }
}

// SearchByProjection(pKF, Scw, ...): greedy in point order (a slot written to vpMatched blocks later points, :372),
// resolved with the fixed-point iteration of fb_claims.h
__global__ __launch_bounds__(MATCH_THREADS) void k_proj_sim3(fb_proj_sim3_args A, int descInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const Carve cv = kf_carve(A.kf, descInLds != 0);
  const KfTargetLds KT = stage_kf(smem, cv, A.kf, b, descInLds != 0);
  const int nkf = KT.n, ms = A.mp.mp_stride, ks = A.kf.kf_stride;
  struct Shared { float T[12], Ow[3]; fb::ClaimFlags cf; };
  __shared__ Shared s_;
  static_assert(up16(sizeof(Shared)) == STATIC_PROJ_SIM3, "match_plan.h");
  auto &s_T = s_.T; auto &s_Ow = s_.Ow; auto &s_cf = s_.cf;
  if (tid == 0) decompose_sim3(A.Scw + (size_t)b * 12, s_T, s_Ow);
  const size_t mo = (size_t)b * ms, ko = (size_t)b * ks;
  const int nmp = A.mp.n_mp[b];
  // per-point state is one u16 pair (vpPoints of a loop closure can be several thousand); the cheap geometric gates are
  // re-evaluated every round instead of being stored
  ClaimsLds L;
  claims_layout(L, cv.end, ks, ms, 2, CLAIMS_U16_SLACK);
  fb::Claims<uint16_t> C(s_cf, lds_at<int>(smem, L.owners), ks, lds_at<uint16_t>(smem, L.assigns), ms,
                         A.kf_matched ? A.kf_matched + ko : nullptr, nkf, nmp);
  C.start();
  const float th = (float)A.th;
  for (int round = 0; C.more(round); round++) {
    C.begin_round();
    for (int q = tid; q < nmp; q += nt) {
      int best = NONE;
      if (A.mp.mp_valid[mo + q]) {
        float u, v;
        const int lvl = gate_point<MODE_PROJ_SIM3>(A.kf, s_T, s_Ow, A.mp, mo + q, u, v);
        if (lvl >= 0)
          best = search_point<MODE_PROJ_SIM3>(A.kf, KT.T, A.mp.mp_desc + (mo + q) * 32, u, v, lvl, th,
                                              [&](int idx) { return C.taken(idx, q); });
      }
      C.submit(q, best);
    }
    if (C.end_round()) break;
  }
  const int *matchL = fb::commit_matches<false>(C, fb::QueryIndex());  // one claimer per slot
  for (int i = tid; i < nkf; i += nt) A.match_kf_to_mp[ko + i] = matchL[i];
  if (tid == 0) A.nmatches[b] = s_cf.n;
}

// one direction of SearchBySim3 for the points of the query key frame (:1151-1223 / :1226-1298)
__device__ __forceinline__ void sim3_direction(const fb_kf_target &Kt, const TargetLds &T, const fb_mp_list &M, size_t mo, int nq,
                                               const float *Tqw, const float *sR, const float *tt, float th, int *vnMatch) {
  for (int q = threadIdx.x; q < nq; q += blockDim.x) {
    int best = -1;
    if (M.mp_valid[mo + q]) {
      const float X[3] = {M.mp_xw[(mo + q) * 3], M.mp_xw[(mo + q) * 3 + 1], M.mp_xw[(mo + q) * 3 + 2]};
      float pq[3], pt[3];
      xform(Tqw, X, pq);
#pragma unroll
      for (int r = 0; r < 3; r++) pt[r] = ((sR[r * 3] * pq[0] + sR[r * 3 + 1] * pq[1]) + sR[r * 3 + 2] * pq[2]) + tt[r];
      if (!(pt[2] < 0.0f)) {
        const float invz = (float)(1.0 / pt[2]);
        const float x = pt[0] * invz, y = pt[1] * invz;
        const float u = Kt.cam.fx * x + Kt.cam.cx, v = Kt.cam.fy * y + Kt.cam.cy;
        if (is_in_image(Kt.cam, u, v)) {
          const float maxD = M.mp_max_dist[mo + q];
          const float dist3D = fb::norm3(pt[0], pt[1], pt[2]);
          if (!(dist3D < 0.8f * M.mp_min_dist[mo + q] || dist3D > 1.2f * maxD)) {
            const int lvl = fb::predict_scale(maxD, dist3D, Kt.log_scale_factor, Kt.n_levels);
            const float radius = th * Kt.scale_factors[lvl];
            uint32_t d[8];
            fb::load_desc(M.mp_desc + (mo + q) * 32, d);
            int bestDist = INT_MAX;
            for_area<false>(Kt.grid, T, u, v, radius, -1, -1, [&](int idx) {
              const int oct = T.oct[idx];
              if (oct < lvl - 1 || oct > lvl) return;
              const int dist = target_hamming(T, d, idx);
              if (dist < bestDist) { bestDist = dist; best = idx; }
            });
            if (bestDist > TH_HIGH) best = -1;
          }
        }
      }
    }
    vnMatch[q] = best;
  }
}

__global__ __launch_bounds__(MATCH_THREADS) void k_sim3(fb_sim3_args A, int carveStride, int carveCells, int descInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  Sim3Lds L;  // behind the carve of the larger key frame
  sim3_layout(L, Carve(carveStride, carveCells, descInLds != 0).end, A.mp1.mp_stride, A.mp2.mp_stride);
  int *vnMatch1 = lds_at<int>(smem, L.match1), *vnMatch2 = lds_at<int>(smem, L.match2);
  struct Shared { float sR12[9], sR21[9], t21[3], t12[3], T1[12], T2[12]; int n; };
  __shared__ Shared s_;
  static_assert(up16(sizeof(Shared)) == STATIC_SIM3, "match_plan.h");
  auto &s_sR12 = s_.sR12; auto &s_sR21 = s_.sR21; auto &s_t21 = s_.t21; auto &s_t12 = s_.t12; auto &s_T1 = s_.T1; auto &s_T2 = s_.T2;
  auto &s_n = s_.n;
  if (tid == 0) {
    const float s12 = A.s12[b], *R12 = A.R12 + (size_t)b * 9, *t12 = A.t12 + (size_t)b * 3;
    const float inv = (float)(1.0 / (double)s12);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        s_sR12[r * 3 + c] = R12[r * 3 + c] * s12;  // :1120
        s_sR21[r * 3 + c] = R12[c * 3 + r] * inv;  // :1121
      }
    for (int r = 0; r < 3; r++) {
      s_t21[r] = -((s_sR21[r * 3] * t12[0] + s_sR21[r * 3 + 1] * t12[1]) + s_sR21[r * 3 + 2] * t12[2]);  // :1122
      s_t12[r] = t12[r];
    }
    for (int i = 0; i < 12; i++) { s_T1[i] = A.T1w[(size_t)b * 12 + i]; s_T2[i] = A.T2w[(size_t)b * 12 + i]; }
    s_n = 0;
  }
  const int N1 = A.mp1.n_mp[b], N2 = A.mp2.n_mp[b];
  const size_t o1 = (size_t)b * A.mp1.mp_stride, o2 = (size_t)b * A.mp2.mp_stride;
  {  // KF1 points into KF2
    const KfTargetLds KT = stage_kf(smem, kf_carve(A.kf2, descInLds != 0), A.kf2, b, descInLds != 0);
    __syncthreads();
    sim3_direction(A.kf2, KT.T, A.mp1, o1, N1, s_T1, s_sR21, s_t21, A.th, vnMatch1);
  }
  __syncthreads();
  {  // KF2 points into KF1
    const KfTargetLds KT = stage_kf(smem, kf_carve(A.kf1, descInLds != 0), A.kf1, b, descInLds != 0);
    __syncthreads();
    sim3_direction(A.kf1, KT.T, A.mp2, o2, N2, s_T2, s_sR12, s_t12, A.th, vnMatch2);
  }
  __syncthreads();
  for (int i1 = tid; i1 < N1; i1 += nt) {  // agreement, :1301-1317
    const int idx2 = vnMatch1[i1];
    int m = -1;
    if (idx2 >= 0 && idx2 < N2 && vnMatch2[idx2] == i1) { m = idx2; atomicAdd(&s_n, 1); }
    A.matches12[o1 + i1] = m;
  }
  __syncthreads();
  if (tid == 0) A.nfound[b] = s_n;
}

// SearchForInitialization.  Serial dependence (:445-446): candidate i2 is skipped when an EARLIER query was accepted on it
// with a distance <= ours.  Fixed point as in M2/M3, but the claim on a target is the list of (query, distance) pairs
// of the previous round (LDS linked list: head[i2], next[q]); query q honours only claims of q' < q.
__global__ __launch_bounds__(MATCH_THREADS) void k_init_match(fb_init_match_args A, int descInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int ncell = A.grid.cols * A.grid.rows;
  const size_t o1 = (size_t)b * A.f1_stride, o2 = (size_t)b * A.f2_stride;
  const int n1 = A.n1[b], n2 = A.n2[b];
  const Carve cv(A.f2_stride, ncell, descInLds != 0);
  const TargetLds T = stage_target(smem, cv, n2, ncell, A.kps2 + o2, A.desc2 + o2 * 32,
                                   A.f2_cell_start + (size_t)b * (ncell + 1), A.f2_cell_items + o2, descInLds != 0);
  // per-query state in 16 bits (indices < 65536, distances <= 256) so that 2 x 4000 key points fit
  typedef unsigned short u16;
  constexpr int NONE16 = 0xFFFF;
  InitLds L;
  init_layout(L, cv.end, A.f1_stride, A.f2_stride);
  int *headA = lds_at<int>(smem, L.headA), *headB = lds_at<int>(smem, L.headB);      // first claimer of a target, -1 = none
  u16 *nextA = lds_at<u16>(smem, L.nextA), *nextB = lds_at<u16>(smem, L.nextB);      // next claimer, NONE16 = end
  u16 *assignA = lds_at<u16>(smem, L.assignA), *assignB = lds_at<u16>(smem, L.assignB);  // target or NONE16
  u16 *distA = lds_at<u16>(smem, L.distA), *distB = lds_at<u16>(smem, L.distB);      // accepted distance
  struct Shared { int changed, n; fb::RotHist rot; };
  __shared__ Shared s_;
  static_assert(up16(sizeof(Shared)) == STATIC_INIT, "match_plan.h");
  auto &s_changed = s_.changed; auto &s_n = s_.n; auto &s_rot = s_.rot;
  for (int i = tid; i < n2; i += nt) headA[i] = -1;
  for (int q = tid; q < n1; q += nt) { assignA[q] = NONE16; distA[q] = 0; nextA[q] = NONE16; }
  __syncthreads();
  const float *prev = A.prev_matched + o1 * 2;
  for (int round = 0; round <= n1 + 1; round++) {
    for (int i = tid; i < n2; i += nt) headB[i] = -1;
    if (tid == 0) s_changed = 0;
    __syncthreads();
    for (int q = tid; q < n1; q += nt) {
      int best = NONE, bestDist = INT_MAX, bestDist2 = INT_MAX;
      const fb_keypoint kp1 = A.kps1[o1 + q];
      if (!(kp1.octave > 0)) {
        uint32_t d[8];
        fb::load_desc(A.desc1 + (o1 + q) * 32, d);
        for_area<false>(A.grid, T, prev[q * 2], prev[q * 2 + 1], (float)A.window_size, kp1.octave, kp1.octave, [&](int i2) {
          const int dist = target_hamming(T, d, i2);
          // vMatchedDistance[i2] just before q = min accepted distance of earlier queries on i2
          for (int c = headA[i2]; c >= 0 && c != NONE16; c = nextA[c])
            if (c < q && distA[c] <= dist) return;
          if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; best = i2; }
          else if (dist < bestDist2) bestDist2 = dist;
        });
        if (!(bestDist <= TH_LOW && bestDist < (float)bestDist2 * A.matcher.nnratio)) best = NONE;
      }
      const int best16 = best == NONE ? NONE16 : best;
      const int dist16 = best == NONE ? 0 : bestDist;
      assignB[q] = (u16)best16;
      distB[q] = (u16)dist16;
      if (best16 != assignA[q] || dist16 != distA[q]) s_changed = 1;
      if (best != NONE) nextB[q] = (u16)atomicExch(&headB[best], q);  // previous head, -1 -> NONE16
    }
    __syncthreads();
    const int changed = s_changed;
    int *t = headA; headA = headB; headB = t;
    u16 *t16 = nextA; nextA = nextB; nextB = t16;
    t16 = assignA; assignA = assignB; assignB = t16;
    t16 = distA; distA = distB; distB = t16;
    __syncthreads();
    if (!changed) break;
  }
  // commit: the LAST accepted query on a target keeps it (:457-463); every acceptance is pushed to the histogram (:465-475)
  int *last = headB;  // [n2] largest accepted query
  u16 *bins = nextB;  // [n1] histogram bin, NONE16 = not pushed
  for (int i = tid; i < n2; i += nt) last[i] = -1;
  s_rot.clear();
  if (tid == 0) s_n = 0;
  __syncthreads();
  const bool ori = A.matcher.check_orientation != 0;
  for (int q = tid; q < n1; q += nt) {
    const int c = assignA[q];
    bins[q] = NONE16;
    if (c == NONE16) continue;
    atomicMax(&last[c], q);
    if (ori) {
      const int bin = rot_bin(A.kps1[o1 + q].angle - A.kps2[o2 + c].angle);
      s_rot.add(bin);
      bins[q] = (u16)bin;
    }
  }
  __syncthreads();
  if (ori) s_rot.pick(); else __syncthreads();
  float *prevw = A.prev_matched + o1 * 2;
  for (int q = tid; q < n1; q += nt) {
    const int c = assignA[q];
    int m = -1;
    if (c != NONE16 && last[c] == q) {
      m = c;
      if (ori) {
        const int bin = bins[q];
        if (!s_rot.keeps(bin)) m = -1;
      }
    }
    A.matches12[o1 + q] = m;
    if (m >= 0) {
      atomicAdd(&s_n, 1);
      const float2 p = T.xy[m];
      prevw[q * 2] = p.x;  // :514-516
      prevw[q * 2 + 1] = p.y;
    }
  }
  __syncthreads();
  if (tid == 0) A.nmatches[b] = s_n;
}

// ComputeDistinctiveDescriptors: one wave per map point; lane i owns observation i (i, i+64, ...).  The median of row i
// is found by bisection on the distance value (0..256), recomputing the row's distances from LDS each step
// (fb::distinctive_pick, shared with k_pt_refresh).
constexpr int DISTINCT_MAX_OBS = 1024;
__global__ __launch_bounds__(64) void k_distinctive(const int32_t *__restrict__ obs_start, const uint8_t *__restrict__ obs_desc,
                                                    int n_mp, int32_t *__restrict__ best_obs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint4 *D = reinterpret_cast<uint4 *>(smem);
  const int p = blockIdx.x, lane = threadIdx.x;
  const int s0 = obs_start[p], N = obs_start[p + 1] - s0;
  if (N <= 0 || N > DISTINCT_MAX_OBS) { if (lane == 0) best_obs[p] = N <= 0 ? -1 : -2; return; }  // -2: over the LDS capacity
  const uint4 *src = reinterpret_cast<const uint4 *>(obs_desc + (size_t)s0 * 32);
  for (int i = lane; i < N * 2; i += 64) D[i] = src[i];
  __syncthreads();
  const int bestIdx = fb::distinctive_pick(lane, N, [&](int j) { return D + j * 2; });
  if (lane == 0) best_obs[p] = bestIdx;
}

int kf_target_ok(const fb_kf_target &K) {
  return K.kf_stride > 0 && K.kf_stride < 65536 && K.n_levels > 0 && K.n_levels <= FB_MAX_LEVELS && K.grid.cols > 0 && K.grid.rows > 0;
}

// host-pointer drop-ins: a key-frame target / a map-point list (B problems) join the call's staged upload
int stage(fb::Stager &st, fb_kf_target &d, size_t B) {
  const size_t ks = d.kf_stride, ncell = (size_t)d.grid.cols * d.grid.rows;
  FB_ARG(d.n_kf && d.kf_kps && d.kf_desc && d.kf_cell_start && d.kf_cell_items);
  st.in(d.n_kf, B * 4); st.in(d.kf_kps, B * ks * sizeof(fb_keypoint)); st.in(d.kf_desc, B * ks * 32);
  st.in(d.kf_cell_start, B * (ncell + 1) * 4); st.in(d.kf_cell_items, B * ks * 4);
  return FB_OK;
}
int stage(fb::Stager &st, fb_mp_list &d, size_t B) {
  const size_t ms = d.mp_stride;
  FB_ARG(d.n_mp && (ms == 0 || (d.mp_valid && d.mp_xw && d.mp_max_dist && d.mp_min_dist && d.mp_desc)));
  st.in(d.n_mp, B * 4); st.in(d.mp_valid, B * ms); st.in(d.mp_xw, B * ms * 12); st.in(d.mp_normal, B * ms * 12);
  st.in(d.mp_max_dist, B * ms * 4); st.in(d.mp_min_dist, B * ms * 4); st.in(d.mp_desc, B * ms * 32);
  return FB_OK;
}

template <int MODE>
int fuse_dev(const fb_fuse_args *A, void *stream, const char *what) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && kf_target_ok(A->kf) && A->mp.mp_stride >= 0 && A->pose && A->best_idx);
  FB_ARG(MODE != MODE_FUSE || A->Ow);
  if (A->batch == 0 || A->mp.mp_stride == 0) return FB_OK;
  const int ncell = A->kf.grid.cols * A->kf.grid.rows;
  DescPlan lp;
  FB_TRY(plan_staged(A->kf.kf_stride, ncell, [](size_t at) { return at; }, STATIC_FUSE, what, &lp));
  const size_t lds = lp.bytes;
  FB_TRY(set_max_lds(k_fuse_search<MODE>, lds));
  fb::ProfScope prof_(fb::P_FUSE, fb::as_stream(stream));
  k_fuse_search<MODE><<<A->batch, MATCH_THREADS, lds, fb::as_stream(stream)>>>(*A, lp.descInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

template <int MODE>
int fuse_host(const fb_fuse_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0);
  fb_fuse_args D = *H;
  const size_t B = H->batch, ms = H->mp.mp_stride;
  if (B == 0 || ms == 0) return FB_OK;
  FB_ARG(H->pose && H->best_idx);
  fb::Stager st;
  FB_TRY(stage(st, D.kf, B));
  FB_TRY(stage(st, D.mp, B));
  st.in(D.pose, B * 48); st.in(D.Ow, B * 12);
  st.out(D.best_idx, B * ms * 4, true);  // copy-in: entries past n keep the caller's contents
  FB_TRY(st.commit(nullptr));
  FB_TRY((fuse_dev<MODE>(&D, nullptr, "fb_fuse_search")));
  return st.fetch(nullptr);
}

}  // namespace

extern "C" {

int fb_fuse_search_dev(const fb_fuse_args *A, void *stream) { return fuse_dev<MODE_FUSE>(A, stream, "fb_fuse_search"); }
int fb_fuse_sim3_search_dev(const fb_fuse_args *A, void *stream) { return fuse_dev<MODE_FUSE_SIM3>(A, stream, "fb_fuse_sim3_search"); }
int fb_fuse_search(const fb_fuse_args *H) { return fuse_host<MODE_FUSE>(H); }
int fb_fuse_sim3_search(const fb_fuse_args *H) { return fuse_host<MODE_FUSE_SIM3>(H); }

int fb_match_projection_sim3_dev(const fb_proj_sim3_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && kf_target_ok(A->kf) && A->mp.mp_stride >= 0 && A->Scw && A->match_kf_to_mp && A->nmatches);
  if (A->batch == 0) return FB_OK;
  const int ncell = A->kf.grid.cols * A->kf.grid.rows;
  DescPlan lp;
  ClaimsLds L;
  FB_TRY(plan_staged(A->kf.kf_stride, ncell, [&](size_t at) { return claims_layout(L, at, A->kf.kf_stride, A->mp.mp_stride, 2, CLAIMS_U16_SLACK); },
                     STATIC_PROJ_SIM3, "fb_match_projection_sim3", &lp));
  const size_t lds = lp.bytes;
  FB_TRY(set_max_lds(k_proj_sim3, lds));
  fb::ProfScope prof_(fb::P_FUSE, fb::as_stream(stream));
  k_proj_sim3<<<A->batch, MATCH_THREADS, lds, fb::as_stream(stream)>>>(*A, lp.descInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_match_projection_sim3(const fb_proj_sim3_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0);
  fb_proj_sim3_args D = *H;
  const size_t B = H->batch, ks = H->kf.kf_stride;
  if (B == 0) return FB_OK;
  FB_ARG(H->Scw && H->match_kf_to_mp && H->nmatches);
  fb::Stager st;
  FB_TRY(stage(st, D.kf, B));
  FB_TRY(stage(st, D.mp, B));
  st.in(D.Scw, B * 48); st.in(D.kf_matched, B * ks);
  st.out(D.match_kf_to_mp, B * ks * 4, true);
  st.out(D.nmatches, B * 4, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_match_projection_sim3_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_match_sim3_dev(const fb_sim3_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && kf_target_ok(A->kf1) && kf_target_ok(A->kf2) && A->mp1.mp_stride >= 0 && A->mp2.mp_stride >= 0);
  FB_ARG(A->T1w && A->T2w && A->s12 && A->R12 && A->t12 && A->matches12 && A->nfound);
  if (A->batch == 0) return FB_OK;
  const int nc1 = A->kf1.grid.cols * A->kf1.grid.rows, nc2 = A->kf2.grid.cols * A->kf2.grid.rows;
  const int cs = A->kf1.kf_stride > A->kf2.kf_stride ? A->kf1.kf_stride : A->kf2.kf_stride, cc = nc1 > nc2 ? nc1 : nc2;
  DescPlan lp;
  Sim3Lds L;
  FB_TRY(plan_staged(cs, cc, [&](size_t at) { return sim3_layout(L, at, A->mp1.mp_stride, A->mp2.mp_stride); }, STATIC_SIM3, "fb_match_sim3", &lp));
  const size_t lds = lp.bytes;
  FB_TRY(set_max_lds(k_sim3, lds));
  fb::ProfScope prof_(fb::P_FUSE, fb::as_stream(stream));
  k_sim3<<<A->batch, MATCH_THREADS, lds, fb::as_stream(stream)>>>(*A, cs, cc, lp.descInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_match_sim3(const fb_sim3_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0);
  fb_sim3_args D = *H;
  const size_t B = H->batch, s1 = H->mp1.mp_stride;
  if (B == 0) return FB_OK;
  FB_ARG(H->T1w && H->T2w && H->s12 && H->R12 && H->t12 && H->matches12 && H->nfound);
  fb::Stager st;
  FB_TRY(stage(st, D.kf1, B));
  FB_TRY(stage(st, D.kf2, B));
  FB_TRY(stage(st, D.mp1, B));
  FB_TRY(stage(st, D.mp2, B));
  st.in(D.T1w, B * 48); st.in(D.T2w, B * 48); st.in(D.s12, B * 4); st.in(D.R12, B * 36); st.in(D.t12, B * 12);
  st.out(D.matches12, B * s1 * 4, true);
  st.out(D.nfound, B * 4, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_match_sim3_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_match_initialization_dev(const fb_init_match_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && A->f1_stride > 0 && A->f2_stride > 0 && A->f2_stride < 65536 && A->prev_matched && A->matches12 && A->nmatches);
  if (A->batch == 0) return FB_OK;
  const int ncell = A->grid.cols * A->grid.rows;
  FB_ARG(A->f1_stride < 65535);
  DescPlan lp;  // 2 x 4000 key points of the initialisation extractor do not fit with descriptors
  InitLds L;
  FB_TRY(plan_staged(A->f2_stride, ncell, [&](size_t at) { return init_layout(L, at, A->f1_stride, A->f2_stride); }, STATIC_INIT,
                     "fb_match_initialization", &lp));
  const size_t lds = lp.bytes;
  const int descInLds = lp.descInLds;
  FB_TRY(set_max_lds(k_init_match, lds));
  fb::ProfScope prof_(fb::P_FUSE, fb::as_stream(stream));
  k_init_match<<<A->batch, MATCH_THREADS, lds, fb::as_stream(stream)>>>(*A, descInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_match_initialization(const fb_init_match_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0);
  fb_init_match_args D = *H;
  const size_t B = H->batch, s1 = H->f1_stride, s2 = H->f2_stride, ncell = (size_t)H->grid.cols * H->grid.rows;
  if (B == 0) return FB_OK;
  FB_ARG(H->n1 && H->kps1 && H->desc1 && H->n2 && H->kps2 && H->desc2 && H->f2_cell_start && H->f2_cell_items);
  FB_ARG(H->prev_matched && H->matches12 && H->nmatches);
  fb::Stager st;
  st.in(D.n1, B * 4); st.in(D.kps1, B * s1 * sizeof(fb_keypoint)); st.in(D.desc1, B * s1 * 32);
  st.in(D.n2, B * 4); st.in(D.kps2, B * s2 * sizeof(fb_keypoint)); st.in(D.desc2, B * s2 * 32);
  st.in(D.f2_cell_start, B * (ncell + 1) * 4); st.in(D.f2_cell_items, B * s2 * 4);
  st.out(D.prev_matched, B * s1 * 8, true);
  st.out(D.matches12, B * s1 * 4, true);
  st.out(D.nmatches, B * 4, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_match_initialization_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_distinctive_descriptors_dev(const int32_t *d_obs_start, const uint8_t *d_obs_desc, int n_mp, int32_t *d_best_obs,
                                   void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(n_mp >= 0);
  if (n_mp == 0) return FB_OK;
  FB_ARG(d_obs_start && d_obs_desc && d_best_obs);
  const size_t lds = (size_t)DISTINCT_MAX_OBS * 32;
  FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_distinctive), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  fb::ProfScope prof_(fb::P_DISTINCT, fb::as_stream(stream));
  k_distinctive<<<n_mp, 64, lds, fb::as_stream(stream)>>>(d_obs_start, d_obs_desc, n_mp, d_best_obs);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_distinctive_descriptors(const int32_t *obs_start, const uint8_t *obs_desc, int n_mp, int32_t *best_obs) {
  FB_TRY(fb::check_device());
  FB_ARG(n_mp >= 0);
  if (n_mp == 0) return FB_OK;
  FB_ARG(obs_start && obs_desc && best_obs);
  const size_t total = (size_t)obs_start[n_mp];
  for (int p = 0; p < n_mp; p++)
    if (obs_start[p + 1] - obs_start[p] > DISTINCT_MAX_OBS) {
      fb::set_error("fb_distinctive_descriptors: map point %d has more than %d observations", p, DISTINCT_MAX_OBS);
      return FB_ERR_CAPACITY;
    }
  if (total == 0) { for (int p = 0; p < n_mp; p++) best_obs[p] = -1; return FB_OK; }
  fb::Stager st;
  st.in(obs_start, (size_t)(n_mp + 1) * 4); st.in(obs_desc, total * 32);
  st.out(best_obs, (size_t)n_mp * 4, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_distinctive_descriptors_dev(obs_start, obs_desc, n_mp, best_obs, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
