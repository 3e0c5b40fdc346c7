// track_kernels.inc -- the glue kernels of the tracking chain and the pointer blocks they take by value (part of track.hip;
// the handle that owns the memory and the stages that launch these are there and in track_stages.inc).
namespace {

constexpr int TT = 256;     // lane-per-slot kernels
constexpr int WG = 1024;    // workgroup-per-sequence kernels

struct FrameDev {  // device pointers of one frame, passed to kernels by value
  int cap;
  int map_cap; uint8_t *seen_mark;  // [batch][map_cap] pMP->mnLastFrameSeen == this frame's mnId, written by k_discard
  int32_t *n; fb_keypoint *kps, *kps_un; uint8_t *desc; int32_t *mp; uint8_t *outlier;
  int32_t *nb; fb_keypoint *bkps; uint8_t *bdesc; float *bcam; int32_t *mpb; uint8_t *boutlier;
  float *Tcw;
};

// mvpMapPoints = NULL, mvbOutlier = false (Frame.cc:327-328); mvpMapPointsBird = NULL, mvBirdOutlier = TRUE (:355-356).
// A new Frame has a new mnId (Frame.cc:265): no map point carries it in mnLastFrameSeen yet, so the marks are cleared.
__global__ __launch_bounds__(TT) void k_frame_reset(FrameDev F, int32_t *counts, int B) {
  const int b = blockIdx.y, i = blockIdx.x * TT + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < FB_CNT_COUNT) counts[threadIdx.x * B + b] = 0;
  for (int j = i; j < F.map_cap; j += gridDim.x * TT) F.seen_mark[(size_t)b * F.map_cap + j] = 0;
  if (i >= F.cap) return;
  const size_t o = (size_t)b * F.cap + i;
  F.mp[o] = -1; F.outlier[o] = 0; F.mpb[o] = -1; F.boutlier[o] = 1;
}

// mCurrentFrame.SetPose(detlaT * mLastFrame.mTcw) (Tracking.cc:1320): cv::Mat 4x4 * 4x4 CV_32F = gemm's small-matrix
// path, every element ((a0*b0 + a1*b1) + a2*b2) + a3*b3 in float; the last row of both is (0 0 0 1)
__global__ void k_predict_pose(const float *delta, const float *Tlast, float *Tcur, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float *D = delta + (size_t)b * 12, *L = Tlast + (size_t)b * 12;
  float *C = Tcur + (size_t)b * 12;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) {
      float s = (D[r * 4 + 0] * L[0 * 4 + c] + D[r * 4 + 1] * L[1 * 4 + c]) + D[r * 4 + 2] * L[2 * 4 + c];
      s = s + D[r * 4 + 3] * (c == 3 ? 1.0f : 0.0f);
      C[r * 4 + c] = s;
    }
}

struct MapDev { int stride; const int32_t *n; const uint8_t *bad, *obs_pos; const float *xw, *normal, *max_dist, *min_dist; const uint8_t *desc; };
struct BirdMapDev { int stride; int32_t *n; float *xw; uint8_t *desc; };

struct M3Scratch { uint8_t *valid, *obs; float *xw; uint8_t *desc; int32_t *oct; float *ang; };

// SearchByProjection(cur, last): the per-slot view of the last frame the matcher reads (ORBmatcher.cc:1355-1392:
// pMP = LastFrame.mvpMapPoints[i], !LastFrame.mvbOutlier[i], GetWorldPos, GetDescriptor, mvKeys[i].octave,
// mvKeysUn[i].angle, Observations() > 0) + the fill(mvpMapPoints, NULL) both call sites do first (Tracking.cc:1330,1344)
__global__ __launch_bounds__(TT) void k_m3_prepare(FrameDev cur, FrameDev last, MapDev map, M3Scratch S) {
  const int b = blockIdx.y, i = blockIdx.x * TT + threadIdx.x;
  if (i >= cur.cap) return;
  const size_t o = (size_t)b * cur.cap + i;
  cur.mp[o] = -1;
  uint8_t v = 0;
  if (i < last.n[b]) {
    const int id = last.mp[o];
    if (id >= 0 && !last.outlier[o]) {
      v = 1;
      const size_t m = (size_t)b * map.stride + id;
      S.obs[o] = map.obs_pos[m];
      S.xw[o * 3] = map.xw[m * 3]; S.xw[o * 3 + 1] = map.xw[m * 3 + 1]; S.xw[o * 3 + 2] = map.xw[m * 3 + 2];
      const uint4 *src = reinterpret_cast<const uint4 *>(map.desc + m * 32);
      uint4 *dst = reinterpret_cast<uint4 *>(S.desc + o * 32);
      dst[0] = src[0]; dst[1] = src[1];
      S.oct[o] = last.kps[o].octave;
      S.ang[o] = last.kps_un[o].angle;
    }
  }
  S.valid[o] = v;
}

// SearchByBoW(pKF, F, ...): vpMapPointsKF[i] && !isBad() per key-frame slot (ORBmatcher.cc:196-203)
__global__ __launch_bounds__(TT) void k_bow_prepare(FrameDev kf, MapDev map, uint8_t *has_mp) {
  const int b = blockIdx.y, i = blockIdx.x * TT + threadIdx.x;
  if (i >= kf.cap) return;
  const size_t o = (size_t)b * kf.cap + i;
  uint8_t v = 0;
  if (i < kf.n[b]) {
    const int id = kf.mp[o];
    v = id >= 0 && !map.bad[(size_t)b * map.stride + id];
  }
  has_mp[o] = v;
}

// dense view of a vlocalMPB list for BirdMapPointMatch (ref_valid / ref_xw / ref_desc by list position)
__global__ __launch_bounds__(TT) void k_m9_prepare(BirdMapDev mpb, const int32_t *local, const int32_t *n_local, int lcap,
                                                   uint8_t *valid, float *xw, uint8_t *desc, int32_t *n_eff, int32_t *match, int cap) {
  const int b = blockIdx.y, j = blockIdx.x * TT + threadIdx.x;
  if (j < cap) match[(size_t)b * cap + j] = -1;
  const int nl = min(max(n_local[b], 0), lcap);
  if (j == 0) n_eff[b] = nl > 10 ? nl : 0;  // Tracking.cc:2004: if (vlocalMPB.size() > 10)
  if (j >= nl) return;
  const size_t o = (size_t)b * lcap + j;
  const int id = local[o];
  const bool ok = id >= 0 && id < mpb.n[b];
  valid[o] = ok ? 1 : 0;
  if (!ok) return;
  const size_t m = (size_t)b * mpb.stride + id;
  xw[o * 3] = mpb.xw[m * 3]; xw[o * 3 + 1] = mpb.xw[m * 3 + 1]; xw[o * 3 + 2] = mpb.xw[m * 3 + 2];
  const uint4 *src = reinterpret_cast<const uint4 *>(mpb.desc + m * 32);
  uint4 *dst = reinterpret_cast<uint4 *>(desc + o * 32);
  dst[0] = src[0]; dst[1] = src[1];
}
// whole table as the list: only the count rule and the match pre-fill
__global__ __launch_bounds__(TT) void k_m9_prepare_all(BirdMapDev mpb, int32_t *n_eff, int32_t *match, int cap) {
  const int b = blockIdx.y, j = blockIdx.x * TT + threadIdx.x;
  if (j < cap) match[(size_t)b * cap + j] = -1;
  if (j == 0) { const int nl = min(max(mpb.n[b], 0), mpb.stride); n_eff[b] = nl > 10 ? nl : 0; }
}

struct EdgeOut { float *fxw, *fobs, *finf; uint8_t *fvalid; float *bxw, *bxc, *binf; uint8_t *bvalid; };
struct SigmaTab { float inv_sigma2[FB_MAX_LEVELS]; };

// Edge construction loops of PoseOptimizationWithBird (Optimizer.cc:525-571 front, :575-602 bird) straight from the
// frame's members, after committing the matcher result that precedes the optimisation:
//   commit 1 (after M3): mvpMapPoints[i] = LastFrame.mvpMapPoints[match[i]]           (ORBmatcher.cc:1430)
//                        mvpMapPointsBird[i] = vlocalMPB[match_bird[i]]                (ORBmatcher.cc:1891)
//   commit 2 (after M2): mvpMapPoints[i] = mvpLocalMapPoints[match[i]] where matched  (ORBmatcher.cc:124)
struct Commit {  // the matcher result a frame has not folded into mvpMapPoints / mvpMapPointsBird yet
  int kind;                 // 0 none, 1 after M3 (+ M9), 2 after M2, 3 after SearchByBoW (replace every slot, gated)
  const int32_t *match;     // kind 1: slot of the last frame; kind 2: position in mvpLocalMapPoints
  const int32_t *src_mp;    // kind 1: LastFrame.mvpMapPoints; kind 2: the local list (NULL = the table itself)
  int src_stride;
  const int32_t *match_bird;  // kind 1: position in vlocalMPB, or NULL
  const int32_t *local_mpb;   // the vlocalMPB list (NULL = the table itself)
  int lcap_mpb;
  const int32_t *gate;        // kind 3: the matcher's count row; a sequence below gate_min "returned false" (Tracking.cc:1212):
  int gate_min;               //         no commit, no edges (the optimiser then leaves pose and flags alone)
  int no_front;               // BirdOptimization (Optimizer.cc:708-835) builds bird edges only
};
__device__ __forceinline__ bool commit_gate_open(const Commit &C, int b) { return !C.gate || C.gate[b] >= C.gate_min; }
__device__ __forceinline__ void commit_slot(const FrameDev &F, const Commit &C, int b, int i, size_t o, int &id, int &idb) {
  id = -1; idb = -1;
  if (i < F.n[b]) {
    id = F.mp[o];
    if (C.kind == 1 && C.match) {
      const int m = C.match[o];
      id = m >= 0 ? C.src_mp[(size_t)b * C.src_stride + m] : -1;
      F.mp[o] = id;
    } else if (C.kind == 2) {
      const int m = C.match[o];
      if (m >= 0) { id = C.src_mp ? C.src_mp[(size_t)b * C.src_stride + m] : m; F.mp[o] = id; }
    } else if (C.kind == 3 && commit_gate_open(C, b)) {  // mCurrentFrame.mvpMapPoints = vpMapPointMatches (Tracking.cc:1215)
      const int m = C.match[o];
      id = m >= 0 ? C.src_mp[(size_t)b * C.src_stride + m] : -1;
      F.mp[o] = id;
    }
  } else if (C.kind == 3 && commit_gate_open(C, b)) {
    F.mp[o] = -1;
  }
  if (i < F.nb[b]) {
    idb = F.mpb[o];
    if (C.kind == 1 && C.match_bird) {
      const int m = C.match_bird[o];
      if (m >= 0) { idb = C.local_mpb ? C.local_mpb[(size_t)b * C.lcap_mpb + m] : m; F.mpb[o] = idb; }
    }
  }
}

__global__ __launch_bounds__(TT) void k_commit(FrameDev F, Commit C) {
  const int b = blockIdx.y, i = blockIdx.x * TT + threadIdx.x;
  if (i >= F.cap) return;
  int id, idb;
  commit_slot(F, C, b, i, (size_t)b * F.cap + i, id, idb);
}

__global__ __launch_bounds__(TT) void k_edges(FrameDev F, MapDev map, BirdMapDev mpb, SigmaTab G, EdgeOut E, Commit C) {
  const int b = blockIdx.y, i = blockIdx.x * TT + threadIdx.x;
  if (i >= F.cap) return;
  const size_t o = (size_t)b * F.cap + i;
  int id, idb;
  commit_slot(F, C, b, i, o, id, idb);
  if (!commit_gate_open(C, b)) { id = -1; idb = -1; }
  if (C.no_front) id = -1;
  if (id >= 0) {
    const fb_keypoint kp = F.kps_un[o];
    const float *X = map.xw + ((size_t)b * map.stride + id) * 3;
    E.fxw[o * 3] = X[0]; E.fxw[o * 3 + 1] = X[1]; E.fxw[o * 3 + 2] = X[2];
    E.fobs[o * 2] = kp.x; E.fobs[o * 2 + 1] = kp.y;
    E.finf[o] = G.inv_sigma2[kp.octave];
    E.fvalid[o] = 1;
  } else {
    E.fvalid[o] = 0;
  }
  if (idb >= 0) {
    const float *X = mpb.xw + ((size_t)b * mpb.stride + idb) * 3;
    E.bxw[o * 3] = X[0]; E.bxw[o * 3 + 1] = X[1]; E.bxw[o * 3 + 2] = X[2];
    E.bxc[o * 3] = F.bcam[o * 3]; E.bxc[o * 3 + 1] = F.bcam[o * 3 + 1]; E.bxc[o * 3 + 2] = F.bcam[o * 3 + 2];
    E.binf[o] = G.inv_sigma2[F.bkps[o].octave];
    E.bvalid[o] = 1;
  } else {
    E.bvalid[o] = 0;
  }
}


// "Discard outliers" of TrackWithMotionModel (Tracking.cc:1358-1376): one workgroup per sequence
// and of TrackReferenceKeyFrame (:1222-1241); src_slot = the matcher count nmatches starts from; gate_min > 0: a sequence
// whose src_slot count is below it returned before the loop (:1212-1213).
// pMP->mnLastFrameSeen = mCurrentFrame.mnId of a dropped point (:1370 / :1235) is a byte per map point on the frame handle
// (the caller's map arrays stay read-only).  It lives as long as the frame id: a second discard in the same frame (the
// fall-back from the motion model to the reference key frame) adds its marks, only Frame construction clears them.
// pMP->mbTrackInView = false (:1369 / :1234) needs no state: k_local_points rebuilds the track members.
__global__ __launch_bounds__(WG) void k_discard(FrameDev F, MapDev map, int32_t *counts, int B, int src_slot, int gate_min) {
  __shared__ int s_w[WG / 64];
  const int b = blockIdx.x, n = min(F.n[b], F.cap);
  if (gate_min > 0 && counts[src_slot * B + b] < gate_min) return;
  int dropped = 0, inmap = 0;
  for (int i = threadIdx.x; i < n; i += WG) {
    const size_t o = (size_t)b * F.cap + i;
    const int id = F.mp[o];
    if (id < 0) continue;
    if (F.outlier[o]) {
      if (id < F.map_cap) F.seen_mark[(size_t)b * F.map_cap + id] = 1;   // (always: map_ok() holds map.stride <= map_cap; kept as the store's own bound)
      F.mp[o] = -1; F.outlier[o] = 0; dropped++;
    }
    else if (map.obs_pos[(size_t)b * map.stride + id]) inmap++;
  }
  dropped = fb::block_sum<WG>(dropped, s_w);
  inmap = fb::block_sum<WG>(inmap, s_w);
  if (threadIdx.x == 0) {
    counts[FB_CNT_MATCHES * B + b] = counts[src_slot * B + b] - dropped;
    counts[FB_CNT_MATCHES_MAP * B + b] = inmap;
  }
}

// FilterBirdOutlierInFront (Tracking.cc:1825-1914) on the result of BirdviewMatch, one workgroup per sequence.
// vDMatches12 = (i1, vnMatches12[i1]) for ascending i1 with vnMatches12[i1] > 0 (sic, ORBmatcher.cc:1755).  Walking it in
// order: skip when the train slot holds a point (on entry or through an earlier PASSING match), test, on a pass take the
// slot.  => kept(i1) = passes(i1) && i1 is the smallest passing query of its train slot && the slot was free on entry.
// New MapPointBirds get ids in list order (mnId = nNextId++, here: the next table row).
// only_below > 0 (TrackReferenceKeyFrame, Tracking.cc:1196-1200): numPt = GetBirdMapPointsNum() (Frame.cc:1081-1092) is
// counted first and a sequence holding that many bird points or more skips the step (its BirdviewMatch count reads 0).
__global__ __launch_bounds__(WG) void k_bird_commit(FrameDev cur, FrameDev ref, BirdMapDev mpb, const int32_t *m12,
                                                    float window, int32_t *counts, int B, int only_below, const int32_t *gate_row,
                                                    int gate_min, const int32_t *m8_count) {
  extern __shared__ int s_first[];  // [cap] smallest passing query per train slot
  __shared__ int s_w[WG / 64];
  __shared__ float s_Twc1[12], s_T2[12];
  const int b = blockIdx.x, tid = threadIdx.x, cap = cur.cap;
  const size_t fo = (size_t)b * cap;
  const int nref = min(ref.nb[b], cap);
  if (gate_row && gate_row[b] < gate_min) return;  // TrackLocalMap does not run for this sequence (Tracking.cc:642: if (bOK))
  if (tid == 0) counts[FB_CNT_BIRDVIEW_MATCHES * B + b] = m8_count[b];  // (the matcher counted into scratch: a gated sequence keeps its counter)
  if (only_below > 0) {
    int have = 0;
    const int ncur = min(cur.nb[b], cap);
    for (int i = tid; i < ncur; i += WG) have += cur.mpb[fo + i] >= 0;
    have = fb::block_sum<WG>(have, s_w);
    if (tid == 0) counts[FB_CNT_BIRD_POINTS * B + b] = have;
    if (have >= only_below) {
      if (tid == 0) counts[FB_CNT_BIRDVIEW_MATCHES * B + b] = 0;
      return;
    }
    __syncthreads();
  }
  if (tid == 0) {
    fb::inv_T(ref.Tcw + (size_t)b * 12, s_Twc1);
    for (int i = 0; i < 12; i++) s_T2[i] = cur.Tcw[(size_t)b * 12 + i];
  }
  for (int i = tid; i < cap; i += WG) s_first[i] = 0x7fffffff;
  __syncthreads();
  const int per = (nref + WG - 1) / WG;   // a thread owns a contiguous run of queries: ids in list order from one scan
  const int i0 = min(nref, tid * per), i1e = min(nref, i0 + per);
  for (int i1 = i0; i1 < i1e; i1++) {
    const int t = m12[fo + i1];
    if (!(t > 0)) continue;
    if (cur.mpb[fo + t] >= 0) continue;
    float ptw[3];
    if (fb::bird_filter_test(s_Twc1, s_T2, ref.bcam + (fo + i1) * 3, cur.bcam + (fo + t) * 3, window, ptw)) atomicMin(&s_first[t], i1);
  }
  __syncthreads();
  int nkept = 0, nnew = 0;
  for (int i1 = i0; i1 < i1e; i1++) {
    const int t = m12[fo + i1];
    if (!(t > 0) || s_first[t] != i1) continue;
    nkept++;
    if (ref.mpb[fo + i1] < 0) nnew++;
  }
  int totalNew;
  int idBase = fb::block_excl_scan<WG>(nnew, s_w, &totalNew);
  const int totalKept = fb::block_sum<WG>(nkept, s_w);
  const int n0 = min(max(mpb.n[b], 0), mpb.stride);
  for (int i1 = i0; i1 < i1e; i1++) {
    const int t = m12[fo + i1];
    if (!(t > 0) || s_first[t] != i1) continue;
    cur.boutlier[fo + t] = 0;
    int id = ref.mpb[fo + i1];
    if (id < 0) {
      id = n0 + idBase++;
      if (id < mpb.stride) {  // new MapPointBird(ptwC, MatchedFrame2, mpMap, trainIdx) (Tracking.cc:1897, MapPointBird.cc:18-28)
        float ptw[3];
        fb::bird_filter_test(s_Twc1, s_T2, ref.bcam + (fo + i1) * 3, cur.bcam + (fo + t) * 3, window, ptw);
        const size_t m = (size_t)b * mpb.stride + id;
        mpb.xw[m * 3] = ptw[0]; mpb.xw[m * 3 + 1] = ptw[1]; mpb.xw[m * 3 + 2] = ptw[2];
        const uint4 *src = reinterpret_cast<const uint4 *>(cur.bdesc + (fo + t) * 32);
        uint4 *dst = reinterpret_cast<uint4 *>(mpb.desc + m * 32);
        dst[0] = src[0]; dst[1] = src[1];
        ref.mpb[fo + i1] = id;
      } else {
        id = -1;  // table full: the point is not created (documented capacity)
      }
    }
    cur.mpb[fo + t] = id;
  }
  if (tid == 0) {
    mpb.n[b] = min(n0 + totalNew, mpb.stride);
    counts[FB_CNT_BIRD_INLIERS * B + b] = totalKept;
    counts[FB_CNT_BIRD_NEW * B + b] = totalNew;
  }
  __syncthreads();  // (this workgroup's own writes to cur.mpb)
  {
    int have = 0;
    const int ncur = min(cur.nb[b], cap);
    for (int i = tid; i < ncur; i += WG) have += cur.mpb[fo + i] >= 0;
    have = fb::block_sum<WG>(have, s_w);
    if (tid == 0) counts[FB_CNT_BIRD_POINTS_FINAL * B + b] = have;
  }
}

struct LocalScratch { uint8_t *seen, *blocked, *inview, *obs; float *proj; int32_t *level; float *cosv; uint8_t *desc; int32_t *n_eff; };
struct FrustumK { fb_camera cam; float log_scale_factor; int n_levels; };

// SearchLocalPoints (Tracking.cc:1947-1984), one workgroup per sequence:
//   0. "seen" starts from the marks the discard loops of this frame left (k_discard): mnLastFrameSeen == mnId already
//   1. points the frame holds: bad ones are dropped from the frame, the others are marked seen (mnLastFrameSeen = mnId)
//   2. every other good point of mvpLocalMapPoints (:1974-1977): isInFrustum(pMP, 0.5) -> the dense track members M2 reads
__global__ __launch_bounds__(WG) void k_local_points(FrameDev F, MapDev map, const int32_t *local, const int32_t *n_local, int lcap,
                                                     FrustumK K, LocalScratch S, int32_t *counts, int B, const int32_t *gate_row, int gate_min) {
  __shared__ int s_w[WG / 64];
  __shared__ float s_T[12], s_Ow[3];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (gate_row && gate_row[b] < gate_min) {  // no TrackLocalMap for this sequence: M2 gets an empty list
    if (tid == 0) S.n_eff[b] = 0;
    return;
  }
  const size_t fo = (size_t)b * F.cap, mo = (size_t)b * map.stride, lo = (size_t)b * lcap;
  const int nmap = min(max(map.n[b], 0), map.stride);
  if (tid < 12) s_T[tid] = F.Tcw[(size_t)b * 12 + tid];
  if (tid == 64) fb::camera_centre(F.Tcw + (size_t)b * 12, s_Ow);
  // (nmap <= map.stride <= map_cap by map_ok(); the test only bounds the load on its own array)
  for (int i = tid; i < nmap; i += WG) S.seen[mo + i] = i < F.map_cap ? F.seen_mark[(size_t)b * F.map_cap + i] : 0;
  __syncthreads();
  const int n = min(F.n[b], F.cap);
  for (int i = tid; i < n; i += WG) {
    const int id = F.mp[fo + i];
    uint8_t blk = 0;
    if (id >= 0) {
      if (map.bad[mo + id]) F.mp[fo + i] = -1;
      else { S.seen[mo + id] = 1; blk = map.obs_pos[mo + id]; }
    }
    S.blocked[fo + i] = blk;  // M2 skips a slot whose point has observations (ORBmatcher.cc:88-90)
  }
  __syncthreads();
  const int nl = local ? min(max(n_local[b], 0), lcap) : min(nmap, lcap);
  int toMatch = 0;
  for (int j = tid; j < nl; j += WG) {
    const int id = local ? local[lo + j] : j;
    uint8_t v = 0;
    if (id >= 0 && id < nmap && !S.seen[mo + id] && !map.bad[mo + id]) {
      const size_t m = mo + id;
      fb::FrustumOut o;
      if (fb::in_frustum(s_T, s_Ow, K.cam, map.xw[m * 3], map.xw[m * 3 + 1], map.xw[m * 3 + 2], map.normal[m * 3], map.normal[m * 3 + 1],
                         map.normal[m * 3 + 2], map.max_dist[m], map.min_dist[m], 0.5f, K.log_scale_factor, K.n_levels, o)) {
        v = 1;
        toMatch++;
        S.proj[(lo + j) * 2] = o.u; S.proj[(lo + j) * 2 + 1] = o.v;
        S.level[lo + j] = o.level;
        S.cosv[lo + j] = o.view_cos;
        S.obs[lo + j] = map.obs_pos[m];
        const uint4 *src = reinterpret_cast<const uint4 *>(map.desc + m * 32);
        uint4 *dst = reinterpret_cast<uint4 *>(S.desc + (lo + j) * 32);
        dst[0] = src[0]; dst[1] = src[1];
      }
    }
    S.inview[lo + j] = v;
  }
  toMatch = fb::block_sum<WG>(toMatch, s_w);
  if (tid == 0) { S.n_eff[b] = nl; counts[FB_CNT_TO_MATCH * B + b] = toMatch; }
}

// End of a tracked frame: mnMatchesInliers (Tracking.cc:1411-1424), clean VO matches (:690-701), drop outliers (:721-725)
// gate_row / gate_min: sequences whose first stage failed did not run TrackLocalMap (nothing to count, nothing to clean);
// min_inliers: TrackLocalMap returns mnMatchesInliers >= 30 (Tracking.cc:1438) and the clean-up sits inside if (bOK) (:681);
// keep_outliers: the final "mvpMapPoints[i] = NULL for outliers" (:721-725) is left to fb_frame_drop_outliers_dev, for a host
// that creates its key frame in between (:716-718: the outliers pass to the new key frame)
__global__ __launch_bounds__(WG) void k_finish(FrameDev F, MapDev map, int32_t *counts, int B, const int32_t *gate_row, int gate_min,
                                               int min_inliers, int keep_outliers) {
  __shared__ int s_w[WG / 64];
  const int b = blockIdx.x, n = min(F.n[b], F.cap);
  if (gate_row && gate_row[b] < gate_min) return;
  int inl = 0;
  for (int i = threadIdx.x; i < n; i += WG) {
    const size_t o = (size_t)b * F.cap + i;
    const int id = F.mp[o];
    if (id < 0) continue;
    if (!F.outlier[o] && map.obs_pos[(size_t)b * map.stride + id] != 0) inl++;
  }
  inl = fb::block_sum<WG>(inl, s_w);
  if (threadIdx.x == 0) counts[FB_CNT_MATCHES_INLIERS * B + b] = inl;
  if (inl < min_inliers) return;   // bOK = false: mState = LOST, the frame keeps its members (Tracking.cc:668-675)
  for (int i = threadIdx.x; i < n; i += WG) {
    const size_t o = (size_t)b * F.cap + i;
    const int id = F.mp[o];
    if (id < 0) continue;
    const bool obs = map.obs_pos[(size_t)b * map.stride + id] != 0;
    if (!obs) { F.outlier[o] = 0; F.mp[o] = -1; }                     // Observations() < 1
    else if (F.outlier[o] && !keep_outliers) F.mp[o] = -1;            // mvbOutlier stays set, as in the reference
  }
}
// Tracking.cc:721-725 on its own (after a key-frame decision), for the sequences whose clean-up ran
__global__ __launch_bounds__(WG) void k_drop_outliers(FrameDev F, const int32_t *counts, int B, int min_inliers) {
  const int b = blockIdx.x, n = min(F.n[b], F.cap);
  if (counts[FB_CNT_MATCHES_INLIERS * B + b] < min_inliers) return;
  for (int i = threadIdx.x; i < n; i += WG) {
    const size_t o = (size_t)b * F.cap + i;
    if (F.mp[o] >= 0 && F.outlier[o]) F.mp[o] = -1;
  }
}

__global__ __launch_bounds__(TT) void k_set_map_points(FrameDev F, const int32_t *mp, const int32_t *mpb) {
  const int b = blockIdx.y, i = blockIdx.x * TT + threadIdx.x;
  if (i >= F.cap) return;
  const size_t o = (size_t)b * F.cap + i;
  if (mp) { F.mp[o] = i < F.n[b] ? mp[o] : -1; F.outlier[o] = 0; }
  if (mpb) F.mpb[o] = i < F.nb[b] ? mpb[o] : -1;
}

__global__ __launch_bounds__(TT) void k_clear_mp(FrameDev F) {
  const int b = blockIdx.y, i = blockIdx.x * TT + threadIdx.x;
  if (i < F.cap) F.mp[(size_t)b * F.cap + i] = -1;
}

}  // namespace
