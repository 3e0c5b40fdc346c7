// fishbird_host.hpp -- C++ host side above the C-ABI (include/fishbird.h), mirroring the reference's
// operator interface for the hot path: same class names, argument meaning and return values as
//   ORBextractor  (include/ORBextractor.h:51-85)
//   ORBmatcher    (include/ORBmatcher.h:41-88)      SearchByProjection x2, SearchByBoW(KF, F), SearchForInitialization,
//                                                   BirdMapPointMatch, BirdviewMatch
//   Optimizer     (include/Optimizer.h:40-68)       PoseOptimization, PoseOptimizationWithBird, BirdOptimization,
//                                                   LocalBundleAdjustment[WithOdom] on a flattened graph
// on plain-old-data frames.  The key-frame / map side entry points (Fuse, SearchBySim3, ... and the graph collection of
// the BA functions) walk KeyFrame / MapPoint / Map objects, which are out of scope: INTEGRATION.md shows
// the gather -> C-ABI call -> scatter shim a maintainer adds inside the reference's own classes (the reference's Frame/KeyFrame/MapPoint own OpenCV and graph state that stays in the
// host application).  Header only; link with -lfishbird_hip.  Errors throw std::runtime_error(fb_last_error()).
#ifndef FISHBIRD_HOST_HPP_
#define FISHBIRD_HOST_HPP_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <vector>

#include "../../include/fishbird.h"

namespace fishbird {

// DBoW2::BowVector / FeatureVector (Thirdparty/DBoW2/DBoW2/BowVector.h:54, FeatureVector.h:22): ordered maps
typedef std::map<unsigned, double> BowVector;
typedef std::map<unsigned, std::vector<unsigned>> FeatureVector;

inline void check(int rc) {
  if (rc != FB_OK) throw std::runtime_error(fb_last_error());
}

// ---- the part of Frame (include/Frame.h) the hot path reads and writes -------------------------------------------
struct MapPointRef {            // what the path needs from a MapPoint / MapPointBird
  bool valid = false;           // pointer != NULL (&& !isBad())
  bool hasObservations = true;  // Observations() > 0
  float Xw[3] = {0, 0, 0};      // GetWorldPos()
  uint8_t descriptor[32] = {0}; // GetDescriptor()
};

struct LocalMapPoint {          // a MapPoint of the local map: what isInFrustum reads and the track members it writes
  MapPointRef ref;
  float normal[3] = {0, 0, 0};  // GetNormal()
  float mfMaxDistance = 0, mfMinDistance = 0;
  bool mbTrackInView = false;   // MapPoint.h track members (written by Frame::isInFrustum)
  float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0, mTrackViewCos = 0;
  int mnTrackScaleLevel = 0;
};

struct Frame {
  // intrinsics and static grid data (Frame.h statics)
  float fx = 0, fy = 0, cx = 0, cy = 0;
  float mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
  int birdviewCols = 0, birdviewRows = 0;
  std::vector<float> mvScaleFactors, mvInvLevelSigma2;
  float mTcw[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // rows 0..2 of the 4x4
  // front
  std::vector<fb_keypoint> mvKeysUn;
  std::vector<uint8_t> mDescriptors;          // N x 32
  BowVector mBowVec;                          // Frame::ComputeBoW (ORBVocabulary::ComputeBoW below)
  FeatureVector mFeatVec;
  std::vector<int32_t> mvpMapPoints;          // index into the caller's map-point table, -1 = NULL
  std::vector<uint8_t> mvpMapPointHasObs;     // Observations()>0 of the point currently in slot i
  std::vector<uint8_t> mvbOutlier;
  // bird
  std::vector<fb_keypoint> mvKeysBird;
  std::vector<uint8_t> mDescriptorsBird;
  std::vector<float> mvKeysBirdCamXYZ;        // NB x 3
  std::vector<int32_t> mvpMapPointsBird;
  std::vector<uint8_t> mvBirdOutlier;
  // grids (Frame::AssignFeaturesToGrid), CSR with cell id = ix*rows+iy
  std::vector<int32_t> gridStart, gridItems, gridBirdStart, gridBirdItems;

  int N() const { return (int)mvKeysUn.size(); }
  int Nbird() const { return (int)mvKeysBird.size(); }
  fb_grid_geom frontGrid() const { return {mnMinX, mnMinY, 64.f / (mnMaxX - mnMinX), 48.f / (mnMaxY - mnMinY), 64, 48}; }
  fb_grid_geom birdGrid() const { return {0.f, 0.f, 32.f / (float)birdviewCols, 32.f / (float)birdviewRows, 32, 32}; }

  // Frame::AssignFeaturesToGrid (Frame.cc:381-411) on the host (tiny); PosInGrid rounding as Frame.cc:548-570
  static void assignToGrid(const std::vector<fb_keypoint> &k, const fb_grid_geom &g, std::vector<int32_t> &start,
                           std::vector<int32_t> &items) {
    const int ncell = g.cols * g.rows;
    std::vector<std::vector<int32_t>> cells(ncell);
    for (size_t i = 0; i < k.size(); i++) {
      const int px = (int)std::round((k[i].x - g.min_x) * g.inv_w), py = (int)std::round((k[i].y - g.min_y) * g.inv_h);
      if (px < 0 || px >= g.cols || py < 0 || py >= g.rows) continue;
      cells[px * g.rows + py].push_back((int32_t)i);
    }
    start.assign(ncell + 1, 0);
    items.assign(k.size() ? k.size() : 1, 0);
    int off = 0;
    for (int c = 0; c < ncell; c++) { start[c] = off; for (int32_t i : cells[c]) items[off++] = i; }
    start[ncell] = off;
  }
  void AssignFeaturesToGrid() {
    assignToGrid(mvKeysUn, frontGrid(), gridStart, gridItems);
    if (birdviewCols > 0) assignToGrid(mvKeysBird, birdGrid(), gridBirdStart, gridBirdItems);
  }

  // Frame::UndistortKeyPoints (Frame.cc:636-669): mvKeys -> mvKeysUn through cv::fisheye::undistortPoints(K, D, R=I, P=K);
  // DistCoef[0] == 0 copies.  K4 = fx, fy, cx, cy; D4 = k1..k4.
  void UndistortKeyPoints(const std::vector<fb_keypoint> &mvKeys, const float D4[4]) {
    mvKeysUn.resize(mvKeys.size());
    if (mvKeys.empty()) return;
    const float K4[4] = {fx, fy, cx, cy};
    check(fb_undistort_keypoints(mvKeys.data(), (int)mvKeys.size(), K4, D4, mvKeysUn.data()));
  }
  // Frame::ComputeImageBounds (Frame.cc:741-795), including its numeric_limits<float>::min() quirk: sets mnMinX..mnMaxY
  void ComputeImageBounds(int cols, int rows, const float D4[4]) {
    const float K4[4] = {fx, fy, cx, cy};
    float bnd[4];
    check(fb_image_bounds(cols, rows, K4, D4, bnd));
    mnMinX = bnd[0]; mnMaxX = bnd[1]; mnMinY = bnd[2]; mnMaxY = bnd[3];
  }

  // Frame::isInFrustum(pMP, viewingCosLimit) (Frame.cc:435-491) over the whole local map in one call, the loop of
  // Tracking::SearchLocalPoints (Tracking.cc:1071-1091).  Writes the track members of every point; returns how many
  // are in view.  mOw = -Rcw^T tcw as Frame::UpdatePoseMatrices computes it (float Mat product, double accumulation).
  int isInFrustum(std::vector<LocalMapPoint> &points, float viewingCosLimit, float mbf = 0.f) const {
    const int32_t n = (int32_t)points.size();
    if (n == 0) return 0;
    std::vector<uint8_t> valid(n), inView(n, 0);
    std::vector<float> xw((size_t)n * 3), nrm((size_t)n * 3), mx(n), mn(n), proj((size_t)n * 2, 0.f), xr(n, 0.f), vc(n, 0.f);
    std::vector<int32_t> lvl(n, 0);
    for (int i = 0; i < n; i++) {
      valid[i] = points[i].ref.valid;
      std::memcpy(&xw[3 * (size_t)i], points[i].ref.Xw, 12);
      std::memcpy(&nrm[3 * (size_t)i], points[i].normal, 12);
      mx[i] = points[i].mfMaxDistance; mn[i] = points[i].mfMinDistance;
    }
    float Ow[3];
    for (int r = 0; r < 3; r++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += (double)mTcw[k * 4 + r] * (double)mTcw[k * 4 + 3];
      Ow[r] = (float)(-s);
    }
    fb_frustum_args a{};
    a.batch = 1; a.mp_stride = n; a.Tcw = mTcw; a.Ow = Ow; a.n_mp = &n; a.mp_valid = valid.data(); a.mp_xw = xw.data();
    a.mp_normal = nrm.data(); a.mp_max_dist = mx.data(); a.mp_min_dist = mn.data();
    a.cam = {fx, fy, cx, cy, mnMinX, mnMinY, mnMaxX, mnMaxY};
    a.mbf = mbf; a.viewing_cos_limit = viewingCosLimit;
    a.log_scale_factor = mvScaleFactors.size() > 1 ? std::log(mvScaleFactors[1]) : 1.f;
    a.n_levels = (int32_t)mvScaleFactors.size();
    a.in_view = inView.data(); a.proj = proj.data(); a.proj_xr = xr.data(); a.level = lvl.data(); a.view_cos = vc.data();
    check(fb_in_frustum(&a));
    int cnt = 0;
    for (int i = 0; i < n; i++) {
      points[i].mbTrackInView = inView[i] != 0;
      if (!inView[i]) continue;
      cnt++;
      points[i].mTrackProjX = proj[2 * (size_t)i]; points[i].mTrackProjY = proj[2 * (size_t)i + 1];
      points[i].mTrackProjXR = xr[i]; points[i].mnTrackScaleLevel = lvl[i]; points[i].mTrackViewCos = vc[i];
    }
    return cnt;
  }
};

// ---- ORBextractor ------------------------------------------------------------------------------------------------
class ORBextractor {
 public:
  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
      : p_{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST} {
    check(fb_orb_create(&p_, &h_));
    check(fb_orb_get_tables(h_, &t_));
  }
  ~ORBextractor() { fb_orb_destroy(h_); }
  ORBextractor(const ORBextractor &) = delete;
  ORBextractor &operator=(const ORBextractor &) = delete;

  // operator()(image, mask, keypoints, descriptors); the mask is ignored like in the reference (ORBextractor.h:58)
  void operator()(const uint8_t *image, int width, int height, int stride, std::vector<fb_keypoint> &keypoints,
                  std::vector<uint8_t> &descriptors) {
    keypoints.clear();
    descriptors.clear();
    if (!image || width <= 0 || height <= 0) return;  // _image.empty()
    const int cap = fb_orb_capacity(&p_);
    keypoints.resize(cap);
    descriptors.resize((size_t)cap * 32);
    int32_t n = 0;
    check(fb_orb_extract(h_, image, width, height, stride, keypoints.data(), descriptors.data(), &n));
    keypoints.resize(n);
    descriptors.resize((size_t)n * 32);
  }
  // detect(image, keypoints, mask) of cv::ORB (Frame.cc:337: cv::ORB::create(nfeatures)->detect(bird, mask)): FAST at one
  // threshold over every level, Harris responses, the best nfeatures split over the levels, IC_Angle; no descriptors (follow
  // it with compute()).  The rules are at fb_orb_detect_args.  Ties at a cut all stay: a result above the capacity is fetched
  // whole by a second call.
  void detect(const uint8_t *image, int width, int height, int stride, std::vector<fb_keypoint> &keypoints,
              const uint8_t *mask = nullptr, int maskStride = 0, int fastThreshold = 20) {
    keypoints.clear();
    if (!image || width <= 0 || height <= 0) return;
    int32_t n = 0, nTrue = 0;
    fb_orb_detect_args a{};
    a.batch = 1; a.width = width; a.height = height; a.stride = stride; a.images = image;
    a.mask = mask; a.mask_stride = maskStride; a.fast_threshold = fastThreshold;
    a.n = &n; a.n_true = &nTrue;
    for (int cap = fb_orb_capacity(&p_);; cap = nTrue) {
      keypoints.resize(cap);
      a.kp_stride = cap; a.kps = keypoints.data();
      check(fb_orb_detect(h_, &a));
      if (nTrue <= cap) break;
    }
    keypoints.resize(n);
  }
  // compute(image, keypoints, descriptors) of cv::ORB on key points the caller supplies (Frame.cc:352-355 after cornerSubPix):
  // descriptors of `keys` on the pyramid of the LAST operator() call, keys[i].octave selecting the level.  The angles are
  // kept as given (OpenCV 3); with icAngle they are recomputed on `image`, which must be the image of that call.  Nothing
  // is erased: status[i] (FB_DESCRIBE_*) tells which rows were written (fb_orb_describe_args).
  void compute(std::vector<fb_keypoint> &keys, std::vector<uint8_t> &descriptors, std::vector<uint8_t> *status = nullptr,
               bool icAngle = false, const uint8_t *image = nullptr, int stride = 0) {
    descriptors.resize(keys.size() * 32);
    if (status) status->assign(keys.size(), FB_DESCRIBE_OK);
    if (keys.empty()) return;
    const int32_t n = (int32_t)keys.size();
    fb_orb_describe_args a{};
    a.batch = 1; a.kp_stride = n; a.n = &n; a.kps = keys.data(); a.desc = descriptors.data();
    a.status = status ? status->data() : nullptr;
    a.angle_mode = icAngle ? FB_DESCRIBE_IC_ANGLE : FB_DESCRIBE_KEEP_ANGLE;
    a.images = image; a.stride = stride;
    check(fb_orb_describe(h_, &a));
  }
  int GetLevels() const { return p_.nlevels; }
  float GetScaleFactor() const { return p_.scale_factor; }
  std::vector<float> GetScaleFactors() const { return {t_.scale_factor, t_.scale_factor + p_.nlevels}; }
  std::vector<float> GetInverseScaleFactors() const { return {t_.inv_scale_factor, t_.inv_scale_factor + p_.nlevels}; }
  std::vector<float> GetScaleSigmaSquares() const { return {t_.level_sigma2, t_.level_sigma2 + p_.nlevels}; }
  std::vector<float> GetInverseScaleSigmaSquares() const { return {t_.inv_level_sigma2, t_.inv_level_sigma2 + p_.nlevels}; }
  fb_orb *handle() const { return h_; }              // for the device-resident Frame (DeviceFrame below)
  const fb_orb_params &params() const { return p_; }

 private:
  fb_orb_params p_;
  fb_orb *h_ = nullptr;
  fb_orb_tables t_;
};

// ---- ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>, TemplatedVocabulary.h) ------------------
// The tree as flat arrays (fb_vocabulary).  transform() is Frame::ComputeBoW / KeyFrame::ComputeBoW (Frame.cc:628-635):
// mBowVec as word id -> value, mFeatVec as NodeId -> feature indices.
class ORBVocabulary {
 public:
  int L = 0;
  std::vector<int32_t> child_start{0}, children, word_ids;
  std::vector<uint8_t> descriptors;
  std::vector<double> weights;

  void transform(const std::vector<uint8_t> &features, BowVector &v, FeatureVector &fv, int levelsup) const {
    v.clear();
    fv.clear();
    const int32_t n = (int32_t)(features.size() / 32);
    if (n == 0) return;
    fb_vocabulary V{};
    V.n_nodes = (int32_t)word_ids.size(); V.L = L; V.child_start = child_start.data(); V.children = children.data();
    V.descriptors = descriptors.data(); V.weights = weights.data(); V.word_ids = word_ids.data();
    std::vector<uint32_t> bid(n), nid(n);
    std::vector<double> bval(n);
    std::vector<int32_t> nstart(n + 1), items(n);
    int32_t nw = 0, nn = 0;
    fb_bow_transform_args a{};
    a.batch = 1; a.f_stride = n; a.n_f = &n; a.desc = features.data(); a.levelsup = levelsup;
    a.n_words = &nw; a.bow_ids = bid.data(); a.bow_vals = bval.data();
    a.fv_n_nodes = &nn; a.fv_node_ids = nid.data(); a.fv_node_start = nstart.data(); a.fv_items = items.data();
    check(fb_bow_transform(&V, &a));
    for (int i = 0; i < nw; i++) v[bid[i]] = bval[i];
    for (int k = 0; k < nn; k++) {
      std::vector<unsigned> &dst = fv[nid[k]];
      for (int j = nstart[k]; j < nstart[k + 1]; j++) dst.push_back((unsigned)items[j]);
    }
  }
  // Frame::ComputeBoW (Frame.cc:628-635): only when mBowVec is still empty
  void ComputeBoW(Frame &F) const { if (F.mBowVec.empty()) transform(F.mDescriptors, F.mBowVec, F.mFeatVec, 4); }
};

// ---- ORBmatcher --------------------------------------------------------------------------------------------------
class ORBmatcher {
 public:
  explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : m_{nnratio, checkOri ? 1 : 0} {}

  static int DescriptorDistance(const uint8_t *a, const uint8_t *b) {
    int32_t d = 0;
    check(fb_descriptor_distance(a, b, 1, &d));
    return d;
  }

  // SearchByProjection(CurrentFrame, LastFrame, th, bMono=true), ORBmatcher.cc:1329-1471.
  // lastPoints[i] describes LastFrame.mvpMapPoints[i] (valid = pointer && !mvbOutlier[i]).
  int SearchByProjection(Frame &cur, const Frame &last, const std::vector<MapPointRef> &lastPoints, float th) const {
    const int32_t N = cur.N(), NL = last.N();
    std::vector<uint8_t> valid(NL), obs(NL), desc((size_t)NL * 32), blocked(N, 0);
    std::vector<float> xw((size_t)NL * 3), angle(NL);
    std::vector<int32_t> oct(NL), match(N > 0 ? N : 1);
    for (int i = 0; i < NL; i++) {
      valid[i] = lastPoints[i].valid && !(i < (int)last.mvbOutlier.size() && last.mvbOutlier[i]);
      obs[i] = lastPoints[i].hasObservations;
      std::memcpy(&xw[3 * i], lastPoints[i].Xw, 12);
      std::memcpy(&desc[32 * (size_t)i], lastPoints[i].descriptor, 32);
      oct[i] = last.mvKeysUn[i].octave;
      angle[i] = last.mvKeysUn[i].angle;
    }
    for (int i = 0; i < N; i++) blocked[i] = cur.mvpMapPoints[i] >= 0 && cur.mvpMapPointHasObs[i];
    fb_proj_frame_args a{};
    a.batch = 1; a.cur_stride = N; a.last_stride = NL;
    a.n_cur = &N; a.cur_kps = cur.mvKeysUn.data(); a.cur_desc = cur.mDescriptors.data();
    a.cur_cell_start = cur.gridStart.data(); a.cur_cell_items = cur.gridItems.data(); a.cur_blocked = blocked.data();
    a.cur_Tcw = cur.mTcw; a.n_last = &NL; a.last_valid = valid.data(); a.last_obs_pos = obs.data(); a.last_xw = xw.data();
    a.last_desc = desc.data(); a.last_octave = oct.data(); a.last_angle = angle.data();
    a.cam = {cur.fx, cur.fy, cur.cx, cur.cy, cur.mnMinX, cur.mnMinY, cur.mnMaxX, cur.mnMaxY};
    a.grid = cur.frontGrid();
    for (size_t i = 0; i < cur.mvScaleFactors.size() && i < FB_MAX_LEVELS; i++) a.scale_factors[i] = cur.mvScaleFactors[i];
    a.th = th; a.matcher = m_;
    int32_t nmatches = 0;
    a.match_cur_to_last = match.data(); a.nmatches = &nmatches;
    check(fb_match_projection_frame(&a));
    for (int i = 0; i < N; i++)
      if (match[i] >= 0) { cur.mvpMapPoints[i] = last.mvpMapPoints[match[i]]; cur.mvpMapPointHasObs[i] = obs[match[i]]; }
    // culled assignments (rotation histogram) are already -1 in match[]; reproduce the NULL writes
    return nmatches;
  }

  // SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th), ORBmatcher.cc:46-130 (TrackLocalMap).
  // points[i] carries the MapPoint's track members as Frame::isInFrustum left them (below); returns nmatches and
  // writes F.mvpMapPoints[idx] = index of the matched point.
  int SearchByProjection(Frame &F, const std::vector<LocalMapPoint> &points, float th = 1.f) const {
    const int32_t N = F.N(), NM = (int32_t)points.size();
    std::vector<uint8_t> track(NM > 0 ? NM : 1), obs(NM > 0 ? NM : 1), desc((size_t)(NM > 0 ? NM : 1) * 32), blocked(N > 0 ? N : 1, 0);
    std::vector<float> proj((size_t)(NM > 0 ? NM : 1) * 2), vcos(NM > 0 ? NM : 1);
    std::vector<int32_t> level(NM > 0 ? NM : 1), match(N > 0 ? N : 1);
    for (int i = 0; i < NM; i++) {
      track[i] = points[i].mbTrackInView && points[i].ref.valid;
      obs[i] = points[i].ref.hasObservations;
      proj[2 * i] = points[i].mTrackProjX; proj[2 * i + 1] = points[i].mTrackProjY;
      level[i] = points[i].mnTrackScaleLevel; vcos[i] = points[i].mTrackViewCos;
      std::memcpy(&desc[32 * (size_t)i], points[i].ref.descriptor, 32);
    }
    for (int i = 0; i < N; i++) blocked[i] = F.mvpMapPoints[i] >= 0 && F.mvpMapPointHasObs[i];
    fb_proj_points_args a{};
    a.batch = 1; a.cur_stride = N; a.mp_stride = NM > 0 ? NM : 1;
    a.n_cur = &N; a.cur_kps = F.mvKeysUn.data(); a.cur_desc = F.mDescriptors.data();
    a.cur_cell_start = F.gridStart.data(); a.cur_cell_items = F.gridItems.data(); a.cur_blocked = blocked.data();
    a.n_mp = &NM; a.mp_track = track.data(); a.mp_obs_pos = obs.data(); a.mp_proj = proj.data(); a.mp_level = level.data();
    a.mp_view_cos = vcos.data(); a.mp_desc = desc.data();
    a.grid = F.frontGrid();
    for (size_t i = 0; i < F.mvScaleFactors.size() && i < FB_MAX_LEVELS; i++) a.scale_factors[i] = F.mvScaleFactors[i];
    a.th = th; a.matcher = m_;
    int32_t nmatches = 0;
    a.match_cur_to_mp = match.data(); a.nmatches = &nmatches;
    check(fb_match_projection_points(&a));
    for (int i = 0; i < N; i++)
      if (match[i] >= 0) { F.mvpMapPoints[i] = match[i]; F.mvpMapPointHasObs[i] = obs[match[i]]; }
    return nmatches;
  }

  // BirdMapPointMatch(CurF, vRefMapPointsBird, windowSize, filterSize), ORBmatcher.cc:1763-1902
  int BirdMapPointMatch(Frame &cur, const std::vector<MapPointRef> &ref, const float Tbc[12], int windowSize,
                        float filterSize, double meter2pixel = 25.1, double rearAxleToCenter = 1.393) const {
    const int32_t NB = cur.Nbird(), NR = (int32_t)ref.size();
    std::vector<uint8_t> valid(NR), desc((size_t)NR * 32);
    std::vector<float> xw((size_t)NR * 3);
    for (int i = 0; i < NR; i++) {
      valid[i] = ref[i].valid;
      std::memcpy(&xw[3 * i], ref[i].Xw, 12);
      std::memcpy(&desc[32 * (size_t)i], ref[i].descriptor, 32);
    }
    fb_bird_mp_args a{};
    a.batch = 1; a.cur_stride = NB; a.ref_stride = NR;
    a.n_cur = &NB; a.cur_kps = cur.mvKeysBird.data(); a.cur_desc = cur.mDescriptorsBird.data();
    a.cur_cam_xyz = cur.mvKeysBirdCamXYZ.data(); a.cur_cell_start = cur.gridBirdStart.data();
    a.cur_cell_items = cur.gridBirdItems.data(); a.cur_Tcw = cur.mTcw;
    a.n_ref = &NR; a.ref_valid = valid.data(); a.ref_xw = xw.data(); a.ref_desc = desc.data();
    std::memcpy(a.Tbc, Tbc, sizeof(a.Tbc));
    a.bird_cols = cur.birdviewCols; a.bird_rows = cur.birdviewRows; a.meter2pixel = meter2pixel;
    a.rear_axle_to_center = rearAxleToCenter; a.grid = cur.birdGrid(); a.window_size = windowSize;
    a.filter_size = filterSize; a.matcher = m_;
    int32_t ninl = 0;
    a.match_cur_to_ref = cur.mvpMapPointsBird.data(); a.ninliers = &ninl;
    check(fb_match_bird_mappoints(&a));
    return ninl;
  }

  // SearchByBoW(pKF, F, vpMapPointMatches), ORBmatcher.cc:160-289, on POD frames: KF plays the key frame (its mFeatVec and
  // key points), kfHasMapPoint[i] = vpMapPointsKF[i] && !isBad().  matchFtoKF[iF] = key-frame feature whose MapPoint lands
  // in vpMapPointMatches[iF] (-1 = NULL); returns nmatches.
  int SearchByBoW(const Frame &KF, const std::vector<uint8_t> &kfHasMapPoint, Frame &F, std::vector<int32_t> &matchFtoKF) const {
    const int32_t NK = KF.N(), NF = F.N();
    matchFtoKF.assign(NF, -1);
    if (NK == 0 || NF == 0) return 0;
    FvFlat fk(KF.mFeatVec), ff(F.mFeatVec);
    int32_t n = 0;
    fb_bow_args a{};
    a.batch = 1; a.kf_stride = NK; a.f_stride = NF;
    a.n_kf = &NK; a.kf_kps = KF.mvKeysUn.data(); a.kf_desc = KF.mDescriptors.data(); a.kf_has_mp = kfHasMapPoint.data(); a.kf_fv = fk.view();
    a.n_f = &NF; a.f_kps = F.mvKeysUn.data(); a.f_desc = F.mDescriptors.data(); a.f_fv = ff.view();
    a.matcher = m_; a.match_f_to_kf = matchFtoKF.data(); a.nmatches = &n;
    check(fb_match_bow(&a));
    return n;
  }

  // SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize), ORBmatcher.cc:406-521.
  // vbPrevMatched: N1 x (x, y), updated in place with the matched F2 positions (:514-517).
  int SearchForInitialization(Frame &F1, Frame &F2, std::vector<float> &vbPrevMatched, std::vector<int> &vnMatches12,
                              int windowSize = 10) const {
    const int32_t N1 = F1.N(), N2 = F2.N();
    vnMatches12.assign(N1, -1);
    if (N1 == 0 || N2 == 0) return 0;
    std::vector<int32_t> m12(N1, -1);
    int32_t n = 0;
    fb_init_match_args a{};
    a.batch = 1; a.f1_stride = N1; a.f2_stride = N2;
    a.n1 = &N1; a.kps1 = F1.mvKeysUn.data(); a.desc1 = F1.mDescriptors.data();
    a.n2 = &N2; a.kps2 = F2.mvKeysUn.data(); a.desc2 = F2.mDescriptors.data();
    a.f2_cell_start = F2.gridStart.data(); a.f2_cell_items = F2.gridItems.data(); a.grid = F2.frontGrid();
    a.window_size = windowSize; a.matcher = m_;
    a.prev_matched = vbPrevMatched.data(); a.matches12 = m12.data(); a.nmatches = &n;
    check(fb_match_initialization(&a));
    for (int i = 0; i < N1; i++) vnMatches12[i] = m12[i];
    return n;
  }

  // BirdviewMatch(CurF, vRefKeysBird, DescriptorsBird, vRefMapPointsBird, vDMatches12, isProject = 0, windowSize),
  // ORBmatcher.cc:1602-1760 (the live form, Tracking.cc:2728).  DMatch = {queryIdx, trainIdx, distance}.
  struct DMatch { int queryIdx, trainIdx; float distance; };
  int BirdviewMatch(Frame &CurF, const std::vector<fb_keypoint> &vRefKeysBird, const std::vector<uint8_t> &DescriptorsBird,
                    std::vector<DMatch> &vDMatches12, int windowSize = 10) const {
    vDMatches12.clear();
    const int32_t NC = CurF.Nbird(), NR = (int32_t)vRefKeysBird.size();
    if (NC == 0 || NR == 0) return 0;
    std::vector<int32_t> m(NR, -1), dist(NR, 0);
    int32_t n = 0, nd = 0;
    fb_birdview_args a{};
    a.batch = 1; a.cur_stride = NC; a.ref_stride = NR;
    a.n_cur = &NC; a.cur_kps = CurF.mvKeysBird.data(); a.cur_desc = CurF.mDescriptorsBird.data();
    a.cur_cell_start = CurF.gridBirdStart.data(); a.cur_cell_items = CurF.gridBirdItems.data();
    a.n_ref = &NR; a.ref_kps = vRefKeysBird.data(); a.ref_desc = DescriptorsBird.data();
    a.grid = CurF.birdGrid(); a.window_size = windowSize; a.matcher = m_;
    a.match_ref_to_cur = m.data(); a.match_dist = dist.data(); a.nmatches = &n; a.n_dmatches = &nd;
    check(fb_match_birdview(&a));
    for (int i = 0; i < NR; i++) if (m[i] > 0) vDMatches12.push_back({i, m[i], (float)dist[i]});  // sic: index 0 is dropped (:1755)
    return n;
  }

 private:
  // flat views of the host containers for the C-ABI
  struct FvFlat {
    std::vector<uint32_t> ids;
    std::vector<int32_t> start, items;
    int32_t n = 0;
    explicit FvFlat(const FeatureVector &fv) {
      start.push_back(0);
      for (FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        ids.push_back(it->first);
        for (size_t k = 0; k < it->second.size(); k++) items.push_back((int32_t)it->second[k]);
        start.push_back((int32_t)items.size());
      }
      n = (int32_t)ids.size();
      if (ids.empty()) { ids.push_back(0); start.push_back(0); }
      if (items.empty()) items.push_back(0);
    }
    fb_feature_vector view() const { return {(int32_t)ids.size(), (int32_t)items.size(), &n, ids.data(), start.data(), items.data()}; }
  };

  fb_matcher_params m_;
};

// ---- Optimizer ---------------------------------------------------------------------------------------------------
struct Sim3KeyFrame;               // (below, with Sim3Solver)
struct Sim3 {                      // g2o::Sim3's own members
  double q[4] = {0, 0, 0, 1};      // r (x, y, z, w), not normalised
  double t[3] = {0, 0, 0};
  double s = 1;
};

class Optimizer {
 public:
  // Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (Optimizer.cc:1560-1775) as LoopClosing.cc:341-368
  // calls it: R12 / t12 / s12 are pSolver->GetEstimated*() and gScm = Sim3(R, t, s) is built from them as at :357.
  // vnMatches1[i1] = feature of pKF2 whose MapPoint is vpMatches1[i1], or -1 (fb_match_sim3's matches12); entries the
  // reference nulls become -1.  g2oS12 receives the optimised Sim3 (the input one when 0 is returned); mg2oScw = gScm * gSmw
  // (:364-366) and Scw (rows 0..2 of Converter::toCvMat(mg2oScw), 12 floats) are filled when given.  Returns nInliers.
  static int OptimizeSim3(const Sim3KeyFrame &kf1, const Sim3KeyFrame &kf2, std::vector<int32_t> &vnMatches1, const float *R12,
                          const float *t12, float s12, Sim3 &g2oS12, float th2, bool bFixScale, const float *mvInvLevelSigma2,
                          int nLevels, Sim3 *mg2oScw = nullptr, float *Scw = nullptr);
  // points[i] / birdPoints[i] describe pFrame->mvpMapPoints[i] / mvpMapPointsBird[i]
  static int PoseOptimization(Frame *f, const std::vector<MapPointRef> &points) {
    return run(f, FB_POSE_FRONT, points, {}, 1.f, 1.f);
  }
  static int PoseOptimizationWithBird(Frame *f, const std::vector<MapPointRef> &points,
                                      const std::vector<MapPointRef> &birdPoints, float wB = 1.f, float wF = 1.f) {
    return run(f, FB_POSE_FRONT_BIRD, points, birdPoints, wB, wF);
  }
  static int BirdOptimization(Frame *f, const std::vector<MapPointRef> &birdPoints, float wB = 1.f) {
    return run(f, FB_POSE_BIRD, {}, birdPoints, wB, 1.f);
  }
  // LocalBundleAdjustment / LocalBundleAdjustmentWithOdom on an already flattened graph
  static void LocalBundleAdjustment(fb_local_ba_args &graph, bool *pbStopFlag) {
    graph.with_odom = 0;
    graph.stop_flag = reinterpret_cast<volatile uint8_t *>(pbStopFlag);
    check(fb_local_ba(&graph));
  }
  static void LocalBundleAdjustmentWithOdom(fb_local_ba_args &graph, bool *pbStopFlag, float wF = 1.f, float wB = 1.f,
                                            float wP = 3.f) {
    graph.with_odom = 1;
    graph.wF = wF; graph.wB = wB; graph.wP = wP;
    graph.stop_flag = reinterpret_cast<volatile uint8_t *>(pbStopFlag);
    check(fb_local_ba(&graph));
  }

 private:
  static int run(Frame *f, int mode, const std::vector<MapPointRef> &points, const std::vector<MapPointRef> &birdPoints,
                 float wB, float wF) {
    const int32_t N = mode == FB_POSE_BIRD ? 0 : f->N(), NB = mode == FB_POSE_FRONT ? 0 : f->Nbird();
    std::vector<float> fxw((size_t)N * 3 + 3), fobs((size_t)N * 2 + 2), finf(N + 1), bxw((size_t)NB * 3 + 3), binf(NB + 1);
    std::vector<uint8_t> fvalid(N + 1), bvalid(NB + 1);
    for (int i = 0; i < N; i++) {
      fvalid[i] = points[i].valid;
      std::memcpy(&fxw[3 * i], points[i].Xw, 12);
      fobs[2 * i] = f->mvKeysUn[i].x; fobs[2 * i + 1] = f->mvKeysUn[i].y;
      finf[i] = f->mvInvLevelSigma2[f->mvKeysUn[i].octave];
    }
    for (int i = 0; i < NB; i++) {
      bvalid[i] = birdPoints[i].valid;
      std::memcpy(&bxw[3 * i], birdPoints[i].Xw, 12);
      binf[i] = f->mvInvLevelSigma2[f->mvKeysBird[i].octave];
    }
    // only the edge family the mode optimises is (re)sized: BirdOptimization (Optimizer.cc:708-835) never touches
    // mvbOutlier, PoseOptimization (:246-475) never touches mvBirdOutlier, and Tracking indexes both right after
    if (mode != FB_POSE_BIRD) f->mvbOutlier.resize(N, 0);
    if (mode != FB_POSE_FRONT) f->mvBirdOutlier.resize(NB, 0);
    uint8_t unusedFamily[4] = {0, 0, 0, 0};
    fb_pose_opt_args a{};
    a.batch = 1; a.mode = mode; a.front_stride = N; a.bird_stride = NB;
    a.fx = f->fx; a.fy = f->fy; a.cx = f->cx; a.cy = f->cy; a.wF = wF; a.wB = wB;
    a.n_front = &N; a.front_xw = fxw.data(); a.front_obs = fobs.data(); a.front_inv_sigma2 = finf.data();
    a.front_valid = fvalid.data();
    a.n_bird = &NB; a.bird_xw = bxw.data(); a.bird_xc = f->mvKeysBirdCamXYZ.empty() ? bxw.data() : f->mvKeysBirdCamXYZ.data();
    a.bird_inv_sigma2 = binf.data(); a.bird_valid = bvalid.data();
    a.bird_outlier = (mode == FB_POSE_FRONT || NB == 0) ? unusedFamily : f->mvBirdOutlier.data();
    a.Tcw = f->mTcw; a.front_outlier = (mode == FB_POSE_BIRD || N == 0) ? unusedFamily : f->mvbOutlier.data();
    int32_t ninl = 0;
    a.ninliers = &ninl;
    check(fb_pose_opt(&a));
    return ninl;
  }
};

// cv::cornerSubPix(image, corners, winSize, Size(-1,-1), {EPS + MAX_ITER, maxCount, epsilon}) on a u8 image (Frame.cc:345-352
// calls it on mBirdviewImg with winSize (5,5), 40, 0.001): corners = [n][2] floats (cv::Point2f), refined in place.
inline void cornerSubPix(const uint8_t *image, int cols, int rows, int step, float *corners, int n, int winW = 5, int winH = 5,
                         int maxCount = 40, double epsilon = 0.001) {
  std::vector<fb_keypoint> k((size_t)n);
  for (int i = 0; i < n; i++) { k[i] = fb_keypoint{}; k[i].x = corners[2 * i]; k[i].y = corners[2 * i + 1]; }
  const int32_t cnt = n;
  fb_corner_subpix_args a{};
  a.batch = 1; a.kp_stride = n; a.cols = cols; a.rows = rows; a.pitch = step; a.image_stride = (size_t)rows * step;
  a.image = image; a.n = &cnt; a.kps = k.data();
  a.half_win_x = winW; a.half_win_y = winH; a.max_iter = maxCount; a.eps = epsilon;
  check(fb_corner_subpix(&a));
  for (int i = 0; i < n; i++) { corners[2 * i] = k[i].x; corners[2 * i + 1] = k[i].y; }
}

// ---- the device-resident Frame and the per-frame chain ------------------------------------------------------------
// DeviceFrame = the reference's Frame with its per-key-point members in HBM (fb_frame, include/fishbird.h); the methods
// below carry the names of the reference functions they stand for and only ENQUEUE on `stream`.  TrackedFrame() is what
// Tracking::Track runs for a frame in state OK (TrackWithMotionModel + TrackLocalMap, Tracking.cc:1312-1441) followed by the
// one read-back the state machine needs; retries / LOST handling stay with the caller.
struct DeviceMap {                 // the caller's MapPoint / MapPointBird tables on the device + the local-map index lists
  fb_map_points points{};
  fb_map_points_bird birdPoints{};
  const int32_t *localPoints = nullptr, *nLocalPoints = nullptr;      // mvpLocalMapPoints (nullptr = the whole table)
  const int32_t *localBirdPoints = nullptr, *nLocalBirdPoints = nullptr;  // Map::GetLocalMapPointsBird()
};

class DeviceFrame {
 public:
  explicit DeviceFrame(const fb_frame_params &p) : p_(p) { check(fb_frame_create(&p_, &h_)); }
  ~DeviceFrame() { fb_frame_destroy(h_); }
  DeviceFrame(const DeviceFrame &) = delete;
  DeviceFrame &operator=(const DeviceFrame &) = delete;
  fb_frame *handle() const { return h_; }
  int batch() const { return p_.batch; }

  // Frame::Frame(imGray, BirdGray, ..., birdviewmask, ..., birdviewContourICP, ..., extractor, ...) from host images
  void Construct(ORBextractor &front, ORBextractor &bird, const uint8_t *imGray, int stride, const uint8_t *birdGray, int birdStride,
                 const uint8_t *contourICP, const uint8_t *mask, void *stream = nullptr) {
    check(fb_frame_extract(h_, front.handle(), bird.handle(), imGray, stride, birdGray, birdStride, contourICP, mask, stream));
  }
  // cv::cornerSubPix on the bird key points inside every later Construct (Frame.cc:345-352); halfWin = 0: off (the default)
  void SetBirdSubPix(int halfWin = 5, int maxCount = 40, double epsilon = 0.001) { check(fb_frame_set_bird_subpix(h_, halfWin, maxCount, epsilon)); }
  // extractorBird->compute at the refined positions (Frame.cc:352-355): runs inside Construct while SetBirdSubPix is on
  void SetBirdRedescribe(bool on = true) { check(fb_frame_set_bird_redescribe(h_, on ? 1 : 0)); }
  // cv::ORB's detector instead of ORBextractor on the bird image inside every later Construct (Frame.cc:337-355)
  void SetBirdDetector(bool cvOrb = true, int fastThreshold = 20) {
    check(fb_frame_set_bird_detector(h_, cvOrb ? FB_BIRD_DETECT_CVORB : FB_BIRD_DETECT_ORBEXTRACTOR, fastThreshold));
  }
  void SetPose(const float *d_Tcw, void *stream = nullptr) { check(fb_frame_set_pose_dev(h_, d_Tcw, stream)); }

  struct TrackResult {             // what Tracking reads after a frame (one synchronisation)
    std::vector<int32_t> counts;   // [FB_CNT_COUNT][batch]
    std::vector<float> Tcw;        // [batch][12]
    int count(int slot, int b = 0) const { return counts[(size_t)slot * (counts.size() / FB_CNT_COUNT) + b]; }
    bool trackedWithMotionModel(int b = 0) const { return count(FB_CNT_PROJ_MATCHES, b) >= 20 && count(FB_CNT_MATCHES_MAP, b) >= 10; }  // Tracking.cc:1351,1384
    bool trackedLocalMap(int b = 0) const { return count(FB_CNT_MATCHES_INLIERS, b) >= 30; }                                              // :1438
    // Tracking::BirdNeedKF (Tracking.cc:2063-2083) on the counters of a frame tracked with TrackUsingBird
    bool birdNeedKF(int b = 0) const {
      const int kf = count(FB_CNT_BIRD_KF_MATCHES, b), numPt = count(FB_CNT_BIRD_POINTS_FINAL, b);
      return kf < 0.7 * numPt || (kf < 10 && numPt > 10);
    }
    bool trackedReferenceKeyFrame(int b = 0) const { return count(FB_CNT_BOW_MATCHES, b) >= 15 && count(FB_CNT_MATCHES_MAP, b) >= 10; }   // :1212,1243
  };
  // Tracking::Track, state OK: this frame against `last`; d_deltaT = rows 0..2 of detlaT (Tracking.cc:1316) on the device
  TrackResult TrackedFrame(DeviceFrame &last, const DeviceMap &map, const float *d_deltaT, float wB = 1.f, float wF = 1.f, void *stream = nullptr) {
    const fb_track_args T = Args(map, d_deltaT, wB, wF);
    check(fb_frame_track_dev(h_, last.h_, &T, stream));
    return Result(stream);
  }

  // the pieces of Tracking::Track a state machine chooses between (Tracking.cc:529-540, 640-643), each one enqueue + one read-back:
  //   bOK = TrackWithMotionModel(); if (!bOK) bOK = TrackReferenceKeyFrame(); if (bOK) bOK = TrackLocalMap();
  TrackResult TrackWithMotionModel(DeviceFrame &last, const DeviceMap &map, const float *d_deltaT, float wB = 1.f, float wF = 1.f, void *stream = nullptr) {
    const fb_track_args T = Args(map, d_deltaT, wB, wF);
    check(fb_frame_track_motion_model_dev(h_, last.h_, &T, stream));
    return Result(stream);
  }
  // mpReferenceKF = the frame handle the key frame was made from (CopyFrom + ComputeBoW); d_deltaT = detlaT of Tracking.cc:1185
  TrackResult TrackReferenceKeyFrame(DeviceFrame &referenceKF, DeviceFrame &tmpRefFrame, const fb_vocabulary &d_voc, const DeviceMap &map,
                                     const float *d_deltaT, float wB = 1.f, float wF = 1.f, void *stream = nullptr) {
    const fb_track_args T = Args(map, d_deltaT, wB, wF);
    check(fb_frame_track_reference_dev(h_, referenceKF.h_, tmpRefFrame.h_, &d_voc, &T, stream));
    return Result(stream);
  }
  // Tracking::TrackUsingBird (Tracking.cc:2014-2061): poseSource = mpReferenceKF's handle (IsbirdWithRefKF == 1) or tmpRefFrame
  TrackResult TrackUsingBird(DeviceFrame &poseSource, DeviceFrame &tmpRefFrame, const DeviceMap &map, const float *d_deltaT, void *stream = nullptr) {
    const fb_track_args T = Args(map, d_deltaT, 1.f, 1.f);
    check(fb_frame_track_using_bird_dev(h_, poseSource.h_, tmpRefFrame.h_, &T, stream));
    return Result(stream);
  }
  TrackResult TrackLocalMap(DeviceFrame &tmpRefFrame, const DeviceMap &map, float wB = 1.f, float wF = 1.f, void *stream = nullptr) {
    const fb_track_args T = Args(map, nullptr, wB, wF);
    check(fb_frame_track_local_map_dev(h_, tmpRefFrame.h_, &T, stream));
    return Result(stream);
  }
  void DropOutliers(void *stream = nullptr) { check(fb_frame_drop_outliers_dev(h_, stream)); }  // Tracking.cc:721-725, after the key-frame decision
  void ComputeBoW(const fb_vocabulary &d_voc, void *stream = nullptr) { check(fb_frame_compute_bow_dev(h_, &d_voc, stream)); }  // Frame.cc:628-635
  void CopyFrom(const DeviceFrame &f, void *stream = nullptr) { check(fb_frame_copy_dev(h_, f.h_, stream)); }  // Frame(const Frame&), KeyFrame(Frame&, ...)

  TrackResult Result(void *stream = nullptr) {
    TrackResult r;
    r.counts.resize((size_t)FB_CNT_COUNT * p_.batch);
    r.Tcw.resize((size_t)12 * p_.batch);
    check(fb_frame_counts(h_, r.counts.data(), r.Tcw.data(), stream));
    return r;
  }

 private:
  static fb_track_args Args(const DeviceMap &map, const float *d_deltaT, float wB, float wF) {
    fb_track_args T{};
    T.map = map.points; T.mpb = map.birdPoints; T.d_delta = d_deltaT;
    T.d_local_mp = map.localPoints; T.d_n_local_mp = map.nLocalPoints; T.d_local_mpb = map.localBirdPoints; T.d_n_local_mpb = map.nLocalBirdPoints;
    T.wB = wB; T.wF = wF;
    T.gate_local_map = 1;       // every step follows its sequence's own bOK
    T.defer_outlier_drop = 0;   // set to 1 by a caller that copies its key frame before DropOutliers()
    return T;
  }
  fb_frame_params p_;
  fb_frame *h_ = nullptr;
};

// the one-call-per-reference-function forms on device frames (results stay in the frames; counts via fb_frame_counts)
inline void SearchByProjection(const ORBmatcher &, DeviceFrame &cur, const DeviceFrame &last, const DeviceMap &map, float th, float nnratio = 0.9f,
                               bool checkOri = true, void *stream = nullptr) {  // ORBmatcher::SearchByProjection(Frame&, const Frame&, th, mono)
  const fb_matcher_params m{nnratio, checkOri ? 1 : 0};
  check(fb_frame_search_by_projection_dev(cur.handle(), last.handle(), &map.points, th, &m, stream));
}
inline void SearchByBoW(const ORBmatcher &, const DeviceFrame &kf, DeviceFrame &cur, const DeviceMap &map, float nnratio = 0.7f, bool checkOri = true,
                        int minMatches = 15, void *stream = nullptr) {  // ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) + Tracking.cc:1212-1215
  const fb_matcher_params m{nnratio, checkOri ? 1 : 0};
  check(fb_frame_search_by_bow_dev(cur.handle(), kf.handle(), &map.points, &m, minMatches, stream));
}
inline void PoseOptimizationWithBird(DeviceFrame &f, const DeviceMap &map, float wB = 1.f, float wF = 1.f, int which = 0, void *stream = nullptr) {
  check(fb_frame_pose_optimization_dev(f.handle(), &map.points, &map.birdPoints, FB_POSE_FRONT_BIRD, wB, wF, which, stream));
}

// ---- KeyFrameDatabase (include/KeyFrameDatabase.h:44-73) on slots ------------------------------------------------
// A key frame is the host's index for pKF (its slot, as the map tables are indexed).  The BowVectors live on the device;
// the covisibility rows (GetBestCovisibilityKeyFrames(10) per slot) are kept here and refreshed by the caller where the
// reference runs UpdateConnections.  Single-threaded, like the reference under KeyFrameDatabase::mMutex.
class KeyFrameDatabase {
 public:
  KeyFrameDatabase(int max_keyframes, int word_stride) : K_(max_keyframes), covis_((size_t)max_keyframes * FB_KFDB_COVIS, -1) {
    fb_kfdb_params p = {max_keyframes, word_stride};
    check(fb_kfdb_create(&p, &db_));
  }
  ~KeyFrameDatabase() { fb_kfdb_destroy(db_); }
  KeyFrameDatabase(const KeyFrameDatabase &) = delete;
  KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;

  void add(int slot, const BowVector &bow) {
    std::vector<uint32_t> ids; std::vector<double> vals;
    flatten(bow, ids, vals);
    check(fb_kfdb_add(db_, slot, (int32_t)ids.size(), ids.data(), vals.data()));
  }
  void erase(int slot) { check(fb_kfdb_erase(db_, slot, nullptr)); }
  void clear() { check(fb_kfdb_clear(db_, nullptr)); }
  // vpNeighs = pKF->GetBestCovisibilityKeyFrames(10) as slots
  void SetBestCovisibilityKeyFrames(int slot, const std::vector<int> &neighs) {
    for (int c = 0; c < FB_KFDB_COVIS; c++) covis_[(size_t)slot * FB_KFDB_COVIS + c] = c < (int)neighs.size() ? neighs[c] : -1;
  }
  std::vector<int> DetectLoopCandidates(uint64_t mnId, const BowVector &bow, const std::vector<int> &connected, float minScore) {
    return query(FB_KFDB_LOOP, mnId, bow, connected, minScore);
  }
  std::vector<int> DetectRelocalizationCandidates(uint64_t mnId, const BowVector &bow) {
    return query(FB_KFDB_RELOC, mnId, bow, std::vector<int>(), 0.0f);
  }
  // LoopClosing::DetectLoop, LoopClosing.cc:127-141: the lowest score to a connected key frame that is not bad
  float MinScore(const BowVector &bow, const std::vector<int> &connected, const std::vector<uint8_t> &isBad) {
    std::vector<uint32_t> ids; std::vector<double> vals;
    flatten(bow, ids, vals);
    float m = 1.0f;
    check(fb_kfdb_min_score(db_, (int32_t)ids.size(), ids.data(), vals.data(), (int32_t)connected.size(), connected.data(),
                            isBad.empty() ? nullptr : isBad.data(), nullptr, &m));
    return m;
  }
  // ORBVocabulary::score
  static double score(const BowVector &a, const BowVector &b) {
    std::vector<uint32_t> ai, bi; std::vector<double> av, bv;
    flatten(a, ai, av); flatten(b, bi, bv);
    const int32_t na = (int32_t)ai.size(), nb = (int32_t)bi.size();
    const size_t stride = std::max<size_t>(1, std::max(ai.size(), bi.size()));
    ai.resize(stride); av.resize(stride); bi.resize(stride); bv.resize(stride);
    double s = 0;
    check(fb_bow_score(1, (int32_t)stride, &na, ai.data(), av.data(), &nb, bi.data(), bv.data(), &s));
    return s;
  }

 private:
  static void flatten(const BowVector &bow, std::vector<uint32_t> &ids, std::vector<double> &vals) {
    for (const auto &kv : bow) { ids.push_back(kv.first); vals.push_back(kv.second); }
  }
  std::vector<int> query(int mode, uint64_t id, const BowVector &bow, const std::vector<int> &connected, float minScore) {
    std::vector<uint32_t> ids; std::vector<double> vals;
    flatten(bow, ids, vals);
    const int32_t nw = (int32_t)ids.size();
    int32_t n = 0;
    std::vector<int32_t> cand(K_, -1);
    fb_kfdb_query_args a;
    memset(&a, 0, sizeof(a));
    a.mode = mode; a.query_id = id; a.n_words = &nw; a.bow_ids = ids.data(); a.bow_vals = vals.data(); a.min_score = minScore;
    a.n_connected = (int32_t)connected.size(); a.connected = connected.data(); a.covis = covis_.data();
    a.n_candidates = &n; a.candidates = cand.data();
    check(fb_kfdb_query(db_, &a));
    return std::vector<int>(cand.begin(), cand.begin() + n);
  }
  fb_kfdb *db_ = nullptr;
  int K_;
  std::vector<int32_t> covis_;
};

// ---- the covisibility graph of KeyFrame (KeyFrame.cc:179-270, 564-663, 797-808, 885-899) on slots ----------------------
// CovisibilityMap is what the graph reads of the caller's Map: per key frame N, mvpMapPoints and mvKeysUn[i].octave, per
// map point isBad(), and every MapPoint::mObservations entry as one edge list (erase = obs_kf < 0).  The methods carry
// the reference's names with the key frame's slot as first argument; each one is one call of fb_covis_* with host
// pointers.  UpdateConnections returns front() for the spanning tree's first connection; UpdateBirdConnections sets its
// parents in the handle.
struct CovisibilityMap {
  int maxKeyFrames, kpStride;
  std::vector<int32_t> kfN, kfMapPoints;            // [K], [K][kpStride] (-1 = NULL)
  std::vector<uint8_t> kfOctave, mpBad;             // [K][kpStride], [points]
  std::vector<int32_t> obsMp, obsKf, obsIdx;
  std::vector<uint64_t> kfOrder;                    // (uintptr_t)pKF
  CovisibilityMap(int K, int stride)
      : maxKeyFrames(K), kpStride(stride), kfN(K, 0), kfMapPoints((size_t)K * stride, -1), kfOctave((size_t)K * stride, 0), kfOrder(K, 0) {}
  int NewMapPoint() { mpBad.push_back(0); return (int)mpBad.size() - 1; }
  // pKF->AddMapPoint(pMP, idx); pMP->AddObservation(pKF, idx)
  void AddObservation(int mp, int kf, int idx, int octave) {
    kfMapPoints[(size_t)kf * kpStride + idx] = mp; kfOctave[(size_t)kf * kpStride + idx] = (uint8_t)octave;
    kfN[kf] = std::max(kfN[kf], idx + 1);
    obsMp.push_back(mp); obsKf.push_back(kf); obsIdx.push_back(idx);
  }
  fb_covis_map view() const {
    fb_covis_map m;
    memset(&m, 0, sizeof(m));
    m.max_keyframes = maxKeyFrames; m.kp_stride = kpStride; m.kf_n = kfN.data(); m.kf_mp = kfMapPoints.data(); m.kf_octave = kfOctave.data();
    m.n_mp = (int32_t)mpBad.size(); m.mp_bad = mpBad.data(); m.n_obs = (int32_t)obsKf.size();
    m.obs_mp = obsMp.data(); m.obs_kf = obsKf.data(); m.obs_idx = obsIdx.data(); m.kf_order = kfOrder.data();
    return m;
  }

  // ---- the per-point side of LocalMapping (MapPoint.cc:151-168, :242-307, :330-371; LocalMapping.cc:158-179, :207-228) ----
  // PointTables is what these calls read and write next to the map: per key frame pose, isBad() and mDescriptors, per point
  // position, mpRefKF as a slot, normal, the two distances, the descriptor, and mnFound / mnVisible / (int)mnFirstKFid.
  struct PointTables {
    std::vector<float> kfTcw, scaleFactors, mpXw, mpNormal, mpMinDist, mpMaxDist;   // [K][12], [levels], [points][3], [points][3], [points] x 2
    std::vector<uint8_t> kfBad, kfDesc, mpDesc;                                     // [K], [K][kpStride][32], [points][32]
    std::vector<int32_t> mpRefKF, mpFound, mpVisible, mpFirstKFid;                  // [points]
    std::vector<int32_t> mpReplaced;                                                // [points] mpReplaced as a point index, -1 = NULL
    PointTables(const CovisibilityMap &m, int nLevels)
        : kfTcw((size_t)m.maxKeyFrames * 12, 0.f), scaleFactors(nLevels, 1.f), kfBad(m.maxKeyFrames, 0),
          kfDesc((size_t)m.maxKeyFrames * m.kpStride * 32, 0) {
      for (int k = 0; k < m.maxKeyFrames; k++) kfTcw[(size_t)k * 12] = kfTcw[(size_t)k * 12 + 5] = kfTcw[(size_t)k * 12 + 10] = 1.f;
      resize(m.mpBad.size());
    }
    void resize(size_t n) {   // after CovisibilityMap::NewMapPoint
      mpXw.resize(n * 3, 0.f); mpNormal.resize(n * 3, 0.f); mpMinDist.resize(n, 0.f); mpMaxDist.resize(n, 0.f); mpDesc.resize(n * 32, 0);
      mpRefKF.resize(n, 0); mpFound.resize(n, 1); mpVisible.resize(n, 1); mpFirstKFid.resize(n, 0); mpReplaced.resize(n, -1);
    }
    fb_point_refresh_args view() {
      fb_point_refresh_args a;
      memset(&a, 0, sizeof(a));
      a.n_levels = (int32_t)scaleFactors.size(); a.kf_Tcw = kfTcw.data(); a.kf_bad = kfBad.data(); a.kf_desc = kfDesc.data();
      a.scale_factors = scaleFactors.data(); a.mp_xw = mpXw.data(); a.mp_ref_kf = mpRefKF.data(); a.mp_normal = mpNormal.data();
      a.mp_min_dist = mpMinDist.data(); a.mp_max_dist = mpMaxDist.data(); a.mp_desc = mpDesc.data();
      return a;
    }
  };
  // pMP->UpdateNormalAndDepth() and / or pMP->ComputeDistinctiveDescriptors() for the listed points (NULL: every point)
  void RefreshPoints(fb_covis *g, PointTables &t, const std::vector<int> *points = nullptr,
                     int what = FB_REFRESH_NORMAL_DEPTH | FB_REFRESH_DESCRIPTOR) const {
    const fb_covis_map m = view();
    fb_point_refresh_args a = t.view();
    a.what = what;
    if (points) { a.d_list = points->data(); a.n_list = (int32_t)points->size(); }
    if (points && points->empty()) return;
    check(fb_covis_refresh_points(g, &m, &a));
  }
  // The point loop of LocalMapping::ProcessNewKeyFrame for the key frame in `slot` (kfN, kfMapPoints, kfOctave, kfDesc and
  // its pose are filled).  The edge list grows by kfN[slot] entries, new edges first, then tombstones; `recent` is
  // mlpRecentAddedMapPoints.  Returns the number of new edges.
  int ProcessNewKeyFrame(fb_covis *g, PointTables &t, int slot, std::vector<int> &recent) {
    const int N = kfN[slot];
    const fb_covis_map m = view();
    const size_t n0 = obsKf.size(), r0 = recent.size();
    obsMp.resize(n0 + N, -1); obsKf.resize(n0 + N, -1); obsIdx.resize(n0 + N, -1);
    recent.resize(r0 + N, -1);
    fb_covis_map grown = m;                                                         // the same arrays after the resize
    grown.obs_mp = obsMp.data(); grown.obs_kf = obsKf.data(); grown.obs_idx = obsIdx.data();
    fb_new_keyframe_args a;
    memset(&a, 0, sizeof(a));
    int32_t nAdded = 0, nRecent = (int32_t)r0;
    a.slot = slot; a.n_features = N; a.obs_cap = (int32_t)obsKf.size(); a.obs_mp = obsMp.data(); a.obs_kf = obsKf.data(); a.obs_idx = obsIdx.data();
    a.d_n_added = &nAdded; a.recent_cap = (int32_t)recent.size(); a.d_recent = recent.data(); a.d_n_recent = &nRecent; a.refresh = t.view();
    check(fb_covis_process_new_keyframe(g, &grown, &a));
    recent.resize(nRecent);
    return nAdded;
  }
  struct Culled {
    std::vector<int> points;                          // got SetBadFlag(), in list order: mpMap->EraseMapPoint for each
    struct Row { int kf, point, idx, edge; };         // the erased observations, per point in ascending kfOrder
    std::vector<Row> erased;
  };
  // LocalMapping::MapPointCulling over `recent` (in/out); edits mpBad, obsKf and kfMapPoints like MapPoint::SetBadFlag
  Culled MapPointCulling(fb_covis *g, const PointTables &t, int currentKFid, int nThObs, std::vector<int> &recent) {
    Culled out;
    if (recent.empty()) return out;
    const fb_covis_map m = view();
    fb_map_point_culling_args a;
    memset(&a, 0, sizeof(a));
    int32_t nRecent = (int32_t)recent.size(), nCulled = 0, nErased = 0;
    std::vector<int32_t> culled(recent.size(), -1), rows(obsKf.size() * 4 + 4, -1);
    a.cur_kf_id = currentKFid; a.n_th_obs = nThObs; a.mp_first_kf_id = t.mpFirstKFid.data(); a.mp_found = t.mpFound.data();
    a.mp_visible = t.mpVisible.data(); a.recent_cap = nRecent; a.d_recent = recent.data(); a.d_n_recent = &nRecent;
    a.kf_mp = kfMapPoints.data(); a.mp_bad = mpBad.data(); a.obs_kf = obsKf.data(); a.d_n_culled = &nCulled; a.d_culled = culled.data();
    a.d_n_erased = &nErased; a.erased_cap = (int32_t)obsKf.size(); a.d_erased = rows.data();
    check(fb_covis_map_point_culling(g, &m, &a));
    recent.resize(nRecent);
    out.points.assign(culled.begin(), culled.begin() + nCulled);
    for (int r = 0; r < nErased; r++) out.erased.push_back({rows[(size_t)r * 4], rows[(size_t)r * 4 + 1], rows[(size_t)r * 4 + 2], rows[(size_t)r * 4 + 3]});
    return out;
  }

  // ---- MapPoint::Replace, the loop fusion and SearchAndFuse of LoopClosing (MapPoint.cc:177-215; LoopClosing.cc:545-560, :616-642) ----
  struct Fused {
    std::vector<std::pair<int, int> > replaced;       // (from, to) in execution order: mpMap->EraseMapPoint(from) for each
    struct Row { int kf, point, idx, edge; };         // the new observations in execution order
    std::vector<Row> added;
    std::vector<int> nFused;                          // SearchAndFuse: the return value of each Fuse
  };
  // from[i]->Replace(to[i]) one after another; from[i] < 0 is skipped.  Edits kfMapPoints, mpBad, obsMp, obsKf, mpFound,
  // mpVisible, mpReplaced and mpDesc.
  Fused ReplacePoints(fb_covis *g, PointTables &t, const std::vector<int> &from, const std::vector<int> &to) {
    Fused out;
    if (from.empty() || from.size() != to.size()) return out;
    const fb_covis_map m = view();
    fb_replace_points_args a;
    memset(&a, 0, sizeof(a));
    int32_t nRep = 0;
    std::vector<int32_t> rows(from.size() * 2, -1);
    a.n_pairs = (int32_t)from.size(); a.d_from = from.data(); a.d_to = to.data();
    a.map = fuseView(t, &nRep, rows);
    check(fb_covis_replace_points(g, &m, &a));
    for (int r = 0; r < nRep; r++) out.replaced.push_back(std::make_pair(rows[(size_t)r * 2], rows[(size_t)r * 2 + 1]));
    return out;
  }
  // The loop fusion for mpCurrentKF = cur and mvpCurrentMatchedPoints as point indices (-1 = NULL; kfN[cur] entries).  The
  // edge list grows by kfN[cur] entries, new edges first, then tombstones.
  Fused LoopFuse(fb_covis *g, PointTables &t, int cur, const std::vector<int> &matched) {
    Fused out;
    const int N = kfN[cur];
    if ((int)matched.size() != N) throw std::runtime_error("LoopFuse: matched.size() != kfN[cur]");
    const int32_t n0 = (int32_t)obsKf.size();
    obsMp.resize((size_t)n0 + N, -1); obsKf.resize((size_t)n0 + N, -1); obsIdx.resize((size_t)n0 + N, -1);
    fb_covis_map m = view();
    m.n_obs = n0;
    fb_loop_fuse_args a;
    memset(&a, 0, sizeof(a));
    int32_t nRep = 0, nAdded = 0;
    std::vector<int32_t> rows((size_t)N * 2 + 2, -1), added((size_t)N * 4 + 4, -1);
    a.cur_slot = cur; a.n_features = N; a.d_matched = matched.data(); a.obs_cap = (int32_t)obsKf.size(); a.obs_idx = obsIdx.data();
    a.d_n_added = &nAdded; a.added_cap = N; a.d_added = added.data();
    a.map = fuseView(t, &nRep, rows);
    check(fb_covis_loop_fuse(g, &m, &a));
    collect(out, nRep, rows, nAdded, added);
    return out;
  }
  // What Fuse reads of a key frame that is the same for all (KeyFrame.h members), and mvKeysUn by slot
  struct FuseTarget {
    fb_camera cam;
    fb_grid_geom grid;
    float scaleFactors[FB_MAX_LEVELS], invLevelSigma2[FB_MAX_LEVELS], logScaleFactor;
    int nLevels;
    std::vector<fb_keypoint> keysUn;                  // [K][kpStride]
  };
  // LoopClosing::SearchAndFuse: slots / Scw ([n][12], rows 0..2 of toCvMat(CorrectedSim3)) in the order of CorrectedPosesMap,
  // loopPoints = mvpLoopMapPoints.  The edge list grows by slots.size() * kpStride entries.
  Fused SearchAndFuse(fb_covis *g, PointTables &t, const FuseTarget &target, const std::vector<int> &slots, const std::vector<float> &Scw,
                      const std::vector<int> &loopPoints, float th = 4.0f) {
    Fused out;
    const size_t nSet = slots.size(), grow = nSet * (size_t)kpStride;
    if (nSet == 0) return out;
    if (Scw.size() != nSet * 12) throw std::runtime_error("SearchAndFuse: Scw.size() != 12 * slots.size()");
    const int32_t n0 = (int32_t)obsKf.size();
    obsMp.resize((size_t)n0 + grow, -1); obsKf.resize((size_t)n0 + grow, -1); obsIdx.resize((size_t)n0 + grow, -1);
    fb_covis_map m = view();
    m.n_obs = n0;
    fb_search_and_fuse_args a;
    memset(&a, 0, sizeof(a));
    int32_t nRep = 0, nAdded = 0;
    std::vector<int32_t> rows(nSet * loopPoints.size() * 2 + 2, -1), added(grow * 4 + 4, -1), nFused(nSet, 0);
    a.n_set = (int32_t)nSet; a.d_set_slots = slots.data(); a.d_set_Scw = Scw.data(); a.n_loop = (int32_t)loopPoints.size();
    a.d_loop_mp = loopPoints.data(); a.th = th; a.cam = target.cam; a.grid = target.grid; a.log_scale_factor = target.logScaleFactor;
    a.n_levels = target.nLevels; a.kf_keys_un = target.keysUn.data();
    memcpy(a.scale_factors, target.scaleFactors, sizeof(a.scale_factors));
    memcpy(a.inv_level_sigma2, target.invLevelSigma2, sizeof(a.inv_level_sigma2));
    a.mp_xw = t.mpXw.data(); a.mp_normal = t.mpNormal.data(); a.mp_min_dist = t.mpMinDist.data(); a.mp_max_dist = t.mpMaxDist.data();
    a.obs_cap = (int32_t)obsKf.size(); a.obs_idx = obsIdx.data(); a.d_n_fused = nFused.data(); a.d_n_added = &nAdded;
    a.added_cap = (int32_t)grow; a.d_added = added.data();
    a.map = fuseView(t, &nRep, rows);
    check(fb_covis_search_and_fuse(g, &m, &a));
    collect(out, nRep, rows, nAdded, added);
    out.nFused.assign(nFused.begin(), nFused.end());
    return out;
  }

  // ---- LocalMapping::SearchInNeighbors (LocalMapping.cc:478-558) ----
  // vpTargetKFs of :481-503 for mpCurrentKeyFrame = cur from the handle's graph, in the reference's order with its duplicates
  std::vector<int> FuseTargets(fb_covis *g, const PointTables &t, int cur, int nn = 20, int nn2 = 5) const {
    const int32_t cap = nn * (1 + nn2);
    std::vector<int32_t> targets((size_t)cap + 1, -1);
    int32_t n = 0;
    check(fb_covis_fuse_targets(g, cur, nn, nn2, t.kfBad.data(), cap, &n, targets.data()));
    return std::vector<int>(targets.begin(), targets.begin() + std::min(n, cap));
  }
  struct Neighbors : Fused {                          // nFused: one per target, then the one of Fuse(cur, candidates)
    std::vector<int> candidates;                      // vpFuseCandidates
    int nCounter = 0, front = -1;                     // of the closing UpdateConnections, as UpdateConnections returns them
  };
  // :506-557 for the targets of FuseTargets: Fuse into each target, the candidates, Fuse into cur, the refresh of cur's points
  // (mpNormal, mpMinDist, mpMaxDist, mpDesc) and UpdateConnections(cur).  The edge list grows by newEdgeCap entries (default:
  // kpStride per Fuse call), new edges first, then tombstones.  UpdateBirdConnections stays the caller's next call.
  Neighbors SearchInNeighbors(fb_covis *g, PointTables &t, const FuseTarget &target, int cur, const std::vector<int> &targets, float th = 3.0f,
                              int newEdgeCap = -1) {
    Neighbors out;
    const size_t nT = targets.size(), grow = newEdgeCap >= 0 ? (size_t)newEdgeCap : (nT + 1) * (size_t)kpStride, nMp = mpBad.size();
    const int32_t n0 = (int32_t)obsKf.size();
    obsMp.resize((size_t)n0 + grow, -1); obsKf.resize((size_t)n0 + grow, -1); obsIdx.resize((size_t)n0 + grow, -1);
    fb_covis_map m = view();
    m.n_obs = n0;
    fb_search_in_neighbors_args a;
    memset(&a, 0, sizeof(a));
    int32_t nRep = 0, nAdded = 0, nCand = 0, nTargets = (int32_t)nT, nCounter = 0, front = -1;
    std::vector<int32_t> rows(nMp * 2 + 2, -1), added(grow * 4 + 4, -1), nFused(nT + 1, 0), cand(nMp + 1, -1), tg(targets.begin(), targets.end());
    tg.push_back(-1);
    a.cur_slot = cur; a.n_features = kfN[cur]; a.n_targets = nTargets; a.d_n_targets = &nTargets; a.d_targets = tg.data(); a.th = th;
    a.cam = target.cam; a.grid = target.grid; a.log_scale_factor = target.logScaleFactor; a.n_levels = target.nLevels;
    a.kf_keys_un = target.keysUn.data();
    memcpy(a.scale_factors, target.scaleFactors, sizeof(a.scale_factors));
    memcpy(a.inv_level_sigma2, target.invLevelSigma2, sizeof(a.inv_level_sigma2));
    a.kf_Tcw = t.kfTcw.data(); a.mp_xw = t.mpXw.data(); a.mp_normal = t.mpNormal.data(); a.mp_min_dist = t.mpMinDist.data();
    a.mp_max_dist = t.mpMaxDist.data(); a.mp_ref_kf = t.mpRefKF.data();
    a.obs_cap = (int32_t)obsKf.size(); a.obs_idx = obsIdx.data(); a.new_edge_cap = (int32_t)grow; a.d_n_fused = nFused.data();
    a.cand_cap = (int32_t)nMp; a.d_n_candidates = &nCand; a.d_candidates = cand.data();
    a.d_n_added = &nAdded; a.added_cap = (int32_t)grow; a.d_added = added.data(); a.d_n_counter = &nCounter; a.d_front = &front;
    a.map = fuseView(t, &nRep, rows);
    check(fb_covis_search_in_neighbors(g, &m, &a));
    collect(out, nRep, rows, nAdded, added);
    out.nFused.assign(nFused.begin(), nFused.end());
    out.candidates.assign(cand.begin(), cand.begin() + std::min((size_t)std::max(nCand, 0), nMp));
    out.nCounter = nCounter; out.front = front;
    return out;
  }

 private:
  fb_point_fuse_arrays fuseView(PointTables &t, int32_t *nRep, std::vector<int32_t> &rows) {
    fb_point_fuse_arrays f;
    memset(&f, 0, sizeof(f));
    f.kf_mp = kfMapPoints.data(); f.mp_bad = mpBad.data(); f.obs_mp = obsMp.data(); f.obs_kf = obsKf.data();
    f.mp_found = t.mpFound.data(); f.mp_visible = t.mpVisible.data(); f.mp_replaced = t.mpReplaced.data();
    f.kf_bad = t.kfBad.data(); f.kf_desc = t.kfDesc.data(); f.mp_desc = t.mpDesc.data();
    f.d_n_replaced = nRep; f.replaced_cap = (int32_t)(rows.size() / 2); f.d_replaced = rows.data();
    return f;
  }
  static void collect(Fused &out, int nRep, const std::vector<int32_t> &rows, int nAdded, const std::vector<int32_t> &added) {
    for (int r = 0; r < nRep && (size_t)r * 2 + 1 < rows.size(); r++) out.replaced.push_back(std::make_pair(rows[(size_t)r * 2], rows[(size_t)r * 2 + 1]));
    for (int r = 0; r < nAdded && (size_t)r * 4 + 3 < added.size(); r++)
      out.added.push_back({added[(size_t)r * 4], added[(size_t)r * 4 + 1], added[(size_t)r * 4 + 2], added[(size_t)r * 4 + 3]});
  }

 public:
  // The bird block of Map::AddKeyFrame(pKF) (Map.cc:41-46) with Map::UpdateLocalBirdMap (:97-153): localKFbird (front first)
  // is updated in place and localMapPointBirds is returned, in the std::set's order when mpbOrder ((uintptr_t)pMPB per bird
  // point) is given, else in index order.  `tables` is WindowTables::view() with the bird side; the camera centres come
  // from its kf_Tcw.
  std::vector<int> UpdateLocalBirdMap(fb_covis *g, const fb_covis_kf_tables &tables, int pKF, std::vector<int> &localKFbird,
                                      const std::vector<uint64_t> *mpbOrder = nullptr) const {
    const fb_covis_map m = view();
    fb_local_bird_map_args a;
    memset(&a, 0, sizeof(a));
    std::vector<int32_t> kfs((size_t)maxKeyFrames, -1), pts((size_t)tables.n_mpb + 1, -1);
    int32_t nKf = (int32_t)std::min(localKFbird.size(), kfs.size()), nPts = 0, overflow = 0;
    std::copy(localKFbird.begin(), localKFbird.begin() + nKf, kfs.begin());
    a.new_slot = pKF; a.d_mpb_order = mpbOrder ? mpbOrder->data() : nullptr;
    a.cap_kf = maxKeyFrames; a.d_local_kf_bird = kfs.data(); a.d_n_local_kf_bird = &nKf;
    a.cap_mpb = tables.n_mpb; a.d_local_mpb = pts.data(); a.d_n_local_mpb = &nPts; a.d_overflow = &overflow;
    check(fb_covis_local_bird_map(g, &m, &tables, &a));
    localKFbird.assign(kfs.begin(), kfs.begin() + nKf);
    return std::vector<int>(pts.begin(), pts.begin() + nPts);
  }

  // ---- loop closing between the device calls (LoopClosing.cc:147-228, :355-375, :571-589) ----
  // The consistency check of DetectLoop for vpCandidateKFs as slots: mvConsistentGroups lives on the handle;
  // -> mvpEnoughConsistentCandidates.  nGroups / overflow: the header, when wanted.
  std::vector<int> DetectLoop(fb_covis *g, const std::vector<int> &candidates, int consistencyTh = 3, int *nGroups = nullptr,
                              bool *overflow = nullptr) const {
    std::vector<int32_t> cand((size_t)maxKeyFrames, -1), enough((size_t)maxKeyFrames, -1);
    int32_t n = (int32_t)std::min(candidates.size(), cand.size()), nEnough = 0;
    std::copy(candidates.begin(), candidates.begin() + n, cand.begin());
    fb_loop_groups_header h;
    memset(&h, 0, sizeof(h));
    check(fb_covis_detect_loop(g, &n, cand.data(), consistencyTh, &nEnough, enough.data(), &h));
    if (nGroups) *nGroups = h.n_groups;
    if (overflow) *overflow = h.overflow != 0;
    return std::vector<int>(enough.begin(), enough.begin() + nEnough);
  }
  // mvpLoopMapPoints of mpMatchedKF = matched, as point indices
  std::vector<int> LoopMapPoints(fb_covis *g, int matched) const {
    const fb_covis_map m = view();
    std::vector<int32_t> pts((size_t)m.n_mp + 1, -1);
    int32_t n = 0, overflow = 0;
    check(fb_covis_loop_map_points(g, &m, matched, m.n_mp, &n, pts.data(), &overflow));
    return std::vector<int>(pts.begin(), pts.begin() + n);
  }
  // The pass over mvpCurrentConnectedKFs = connectedKFs that ends CorrectLoop: UpdateConnections of every member, and
  // LoopConnections[member] per list position, each in the std::set's order.  updated: (KFcounter.size(), front) per member.
  std::vector<std::vector<int>> LoopConnections(fb_covis *g, const std::vector<int> &connectedKFs,
                                                std::vector<std::pair<int, int>> *updated = nullptr) const {
    const fb_covis_map m = view();
    const int32_t n = (int32_t)connectedKFs.size();
    std::vector<std::vector<int>> rows((size_t)n);
    if (n == 0) return rows;
    std::vector<int32_t> nCounter((size_t)n, 0), front((size_t)n, -1), off((size_t)n + 1, 0), slots((size_t)n * maxKeyFrames, -1);
    fb_loop_connections_header h;
    memset(&h, 0, sizeof(h));
    fb_loop_connections_args a;
    memset(&a, 0, sizeof(a));
    a.set_cap = n; a.d_n_set = &n; a.d_set = connectedKFs.data(); a.d_n_counter = nCounter.data(); a.d_front = front.data();
    a.lc_cap = (int32_t)slots.size(); a.d_lc_off = off.data(); a.d_lc_slots = slots.data(); a.d_header = &h;
    check(fb_covis_loop_connections(g, &m, &a));
    for (int j = 0; j < n; j++) rows[(size_t)j].assign(slots.begin() + off[(size_t)j], slots.begin() + off[(size_t)j + 1]);
    if (updated) {
      updated->clear();
      for (int j = 0; j < n; j++) updated->push_back(std::make_pair((int)nCounter[(size_t)j], (int)front[(size_t)j]));
    }
    return rows;
  }
};

class CovisibilityGraph {
 public:
  explicit CovisibilityGraph(int max_keyframes) : K_(max_keyframes) { check(fb_covis_create(max_keyframes, &g_)); }
  ~CovisibilityGraph() { fb_covis_destroy(g_); }
  CovisibilityGraph(const CovisibilityGraph &) = delete;
  CovisibilityGraph &operator=(const CovisibilityGraph &) = delete;
  fb_covis *handle() const { return g_; }

  struct Updated { int nCounter, front; };          // KFcounter.size(), mvpOrderedConnectedKeyFrames.front() (-1 = empty)
  // pKF->UpdateConnections() for each listed key frame, one after the other
  std::vector<Updated> UpdateConnections(const CovisibilityMap &map, const std::vector<int> &slots) {
    const fb_covis_map m = map.view();
    std::vector<int32_t> n(slots.size()), f(slots.size());
    check(fb_covis_update_connections(g_, &m, (int32_t)slots.size(), slots.data(), n.data(), f.data()));
    std::vector<Updated> r(slots.size());
    for (size_t i = 0; i < r.size(); i++) r[i] = {n[i], f[i]};
    return r;
  }
  Updated UpdateConnections(const CovisibilityMap &map, int slot) { return UpdateConnections(map, std::vector<int>(1, slot))[0]; }
  struct BirdUpdated { int nBirdCounter, front; };  // the bird KFcounter.size(), mvpBirdConnectedKeyFrames.front() (-1 = empty)
  // pKF->UpdateBirdConnections(nowState) for each listed key frame (KeyFrame.cc:418-562), as UpdateConnections calls it: with
  // `front` (the result of UpdateConnections for the same slots) a key frame whose front counter was empty acts only when
  // nowState >= 3 (:608-609); NULL = every key frame acts.  `tables` is WindowTables::view() with the bird side; kfFrameId
  // (mnFrameId) and kfInMap (the key frame is in mpMap) are read when nowState >= 3.  The parents it sets are in the
  // handle's tree (fb_covis_tree_get).
  std::vector<BirdUpdated> UpdateBirdConnections(const CovisibilityMap &map, const fb_covis_kf_tables &tables, const std::vector<int> &slots,
                                                 const std::vector<Updated> *front, int nowState, int id0Slot,
                                                 const std::vector<int32_t> &kfFrameId, const std::vector<uint8_t> &kfInMap) {
    const fb_covis_map m = map.view();
    std::vector<int32_t> nc(slots.size()), n(slots.size()), f(slots.size());
    if (front) for (size_t i = 0; i < slots.size(); i++) nc[i] = (*front)[i].nCounter;
    check(fb_covis_update_bird_connections(g_, &m, &tables, (int32_t)slots.size(), slots.data(), front ? nc.data() : nullptr, nowState, id0Slot,
                                           kfFrameId.empty() ? nullptr : kfFrameId.data(), kfInMap.empty() ? nullptr : kfInMap.data(),
                                           n.data(), f.data()));
    std::vector<BirdUpdated> r(slots.size());
    for (size_t i = 0; i < r.size(); i++) r[i] = {n[i], f[i]};
    return r;
  }
  std::vector<int> GetBirdConnectedBirdKeyFrames(int slot, std::vector<int> *weights = nullptr) {
    int32_t n = 0;
    std::vector<int32_t> s(K_), w(K_);
    check(fb_covis_bird_connected(g_, slot, &n, s.data(), w.data()));
    if (weights) weights->assign(w.begin(), w.begin() + n);
    return std::vector<int>(s.begin(), s.begin() + n);
  }
  void AddConnection(int slot, int pKF, int weight) { check(fb_covis_add_connection_dev(g_, slot, pKF, weight, nullptr)); }
  void EraseConnection(int slot, int pKF) { check(fb_covis_erase_connection_dev(g_, slot, pKF, nullptr)); }
  void SetBadFlag(int slot) { check(fb_covis_erase_keyframe_dev(g_, slot, nullptr)); }   // the graph part (:797-798, :807-808)
  void clear() { check(fb_covis_clear(g_, nullptr)); }

  std::vector<int> GetVectorCovisibleKeyFrames(int slot, std::vector<int> *orderedWeights = nullptr) {
    int32_t n = 0;
    std::vector<int32_t> s(K_), w(K_);
    check(fb_covis_ordered(g_, slot, &n, s.data(), w.data()));
    if (orderedWeights) orderedWeights->assign(w.begin(), w.begin() + n);
    return std::vector<int>(s.begin(), s.begin() + n);
  }
  std::vector<int> GetBestCovisibilityKeyFrames(int slot, int N) {
    std::vector<int> v = GetVectorCovisibleKeyFrames(slot);
    if ((int)v.size() > N) v.resize(N);
    return v;
  }
  std::vector<int> GetCovisiblesByWeight(int slot, int w) {
    int32_t n = 0;
    std::vector<int32_t> s(K_);
    check(fb_covis_by_weight(g_, slot, w, &n, s.data()));
    return std::vector<int>(s.begin(), s.begin() + n);
  }
  std::vector<int> GetConnectedKeyFrames(int slot) {   // the std::set's order: ascending kfOrder
    int32_t n = 0;
    std::vector<int32_t> s(K_);
    check(fb_covis_connected(g_, slot, &n, s.data()));
    return std::vector<int>(s.begin(), s.begin() + n);
  }
  int GetWeight(int slot, int pKF) {
    int32_t w = 0;
    check(fb_covis_weight(g_, slot, pKF, &w));
    return w;
  }
  // GetBestCovisibilityKeyFrames(10) of every slot, as KeyFrameDatabase::SetBestCovisibilityKeyFrames takes them
  void UpdateKeyFrameDatabase(KeyFrameDatabase &db) {
    std::vector<int32_t> rows((size_t)K_ * FB_KFDB_COVIS, -1);
    check(fb_covis_kfdb_rows(g_, 0, nullptr, rows.data()));
    for (int s = 0; s < K_; s++) {
      std::vector<int> v;
      for (int c = 0; c < FB_KFDB_COVIS && rows[(size_t)s * FB_KFDB_COVIS + c] >= 0; c++) v.push_back(rows[(size_t)s * FB_KFDB_COVIS + c]);
      db.SetBestCovisibilityKeyFrames(s, v);
    }
  }

  struct Culling {                                  // in the order of GetVectorCovisibleKeyFrames() of the current key frame
    std::vector<int> slots, nRedundantObservations, nMPs;
    std::vector<uint8_t> culled;                    // SetBadFlag() was called on it
    std::vector<uint8_t> mpBadAfter;                // isBad() of every map point after the call's SetBadFlag()s
  };
  // LocalMapping::KeyFrameCulling (LocalMapping.cc:656-729); the caller then runs the real SetBadFlag per culled slot
  Culling KeyFrameCulling(const CovisibilityMap &map, int currentKF, int id0Slot, const std::vector<uint8_t> &notErase) {
    const fb_covis_map m = map.view();
    int32_t n = 0;
    std::vector<int32_t> s(K_), r(K_), p(K_);
    std::vector<uint8_t> c(K_), bad(map.mpBad.size() + 1);
    check(fb_covis_keyframe_culling(g_, &m, currentKF, id0Slot, notErase.empty() ? nullptr : notErase.data(), &n, s.data(), r.data(),
                                    p.data(), c.data(), bad.data()));
    Culling out;
    out.slots.assign(s.begin(), s.begin() + n); out.nRedundantObservations.assign(r.begin(), r.begin() + n);
    out.nMPs.assign(p.begin(), p.begin() + n); out.culled.assign(c.begin(), c.begin() + n);
    out.mpBadAfter.assign(bad.begin(), bad.begin() + map.mpBad.size());
    return out;
  }

 private:
  fb_covis *g_ = nullptr;
  int K_;
};

// ---- the local-BA window: head and tail of Optimizer::LocalBundleAdjustmentWithOdom (Optimizer.cc:2139-2227, :2574-2669) ----
// WindowTables is what the window reads of the caller's key frames and points next to CovisibilityMap; the bird side is
// used when birdStride > 0.  LocalWindow::Run is the whole call with host pointers: collect the window
// (fb_covis_local_window), the caller's odometry edges between the local key frames (:2419-2495), fb_local_ba, then the
// write-back and the erase lists.  A caller whose map lies in HBM makes the same four steps with the *_dev calls.
struct WindowTables {
  int birdStride = 0;
  std::vector<float> kfTcw, mpXw, invLevelSigma2;     // [K][12], [points][3], [levels]
  std::vector<uint8_t> kfBad, kfInit;                 // isBad(), isInit
  std::vector<fb_keypoint> kfKeysUn;                  // [K][kpStride]
  std::vector<int32_t> kfNb, kfMapPointsBird;         // [K], [K][birdStride]
  std::vector<uint8_t> kfBirdOctave, mpbBad;
  std::vector<float> kfBirdXc, mpbXw;                 // [K][birdStride][3], [bird points][3]
  std::vector<int32_t> bobsMpb, bobsKf, bobsIdx;
  WindowTables(const CovisibilityMap &m, int nLevels, int birdStride_ = 0)
      : birdStride(birdStride_), kfTcw((size_t)m.maxKeyFrames * 12, 0.f), invLevelSigma2(nLevels, 1.f), kfBad(m.maxKeyFrames, 0),
        kfInit(m.maxKeyFrames, 0), kfKeysUn((size_t)m.maxKeyFrames * m.kpStride), kfNb(m.maxKeyFrames, 0),
        kfMapPointsBird((size_t)m.maxKeyFrames * birdStride_, -1), kfBirdOctave((size_t)m.maxKeyFrames * birdStride_, 0),
        kfBirdXc((size_t)m.maxKeyFrames * birdStride_ * 3, 0.f) {}
  fb_covis_kf_tables view() {
    fb_covis_kf_tables t;
    memset(&t, 0, sizeof(t));
    t.kf_Tcw = kfTcw.data(); t.kf_bad = kfBad.data(); t.kf_init = kfInit.data(); t.kf_keys_un = kfKeysUn.data();
    t.n_levels = (int32_t)invLevelSigma2.size(); t.inv_level_sigma2 = invLevelSigma2.data(); t.mp_xw = mpXw.data();
    if (birdStride > 0) {
      t.bird_stride = birdStride; t.kf_nb = kfNb.data(); t.kf_mpb = kfMapPointsBird.data(); t.kf_bird_octave = kfBirdOctave.data();
      t.kf_bird_xc = kfBirdXc.data(); t.n_mpb = (int32_t)mpbBad.size(); t.mpb_bad = mpbBad.data(); t.mpb_xw = mpbXw.data();
      t.n_bobs = (int32_t)bobsKf.size(); t.bobs_mpb = bobsMpb.data(); t.bobs_kf = bobsKf.data(); t.bobs_idx = bobsIdx.data();
    }
    return t;
  }
};

class LocalWindow {
 public:
  struct Erase { int kf, point, idx, edge; };          // pKFi->EraseMapPointMatch(point at idx); point->EraseObservation(pKFi); obs_kf[edge] = -1
  struct OdomEdge { int i, j; float Tij[12]; double info; };   // i, j: positions in localKeyFrames()
  int nLocal = 0, nFixed = 0;
  std::vector<int32_t> kfSlot, mpIndex, mpbIndex, obsKf, obsMp, obsSrc, bobsKf, bobsMpb, bobsSrc;
  std::vector<uint8_t> kfFixed, obsOutlier, bobsOutlier;
  std::vector<float> kfTcw, mpXw, mpbXw, obsUv, obsInvSigma2, bobsXc, bobsInvSigma2;
  std::vector<Erase> toErase, toEraseBird;

  // lLocalKeyFrames, lLocalMapPoints, lFixedCameras and the edges
  void Collect(CovisibilityGraph &g, const CovisibilityMap &map, WindowTables &tables, int currentKF, bool bHaveBird) {
    const fb_covis_map m = map.view();
    const fb_covis_kf_tables t = tables.view();
    const bool bird = bHaveBird && tables.birdStride > 0;
    const size_t nKf = map.maxKeyFrames, nMp = map.mpBad.size(), nObs = map.obsKf.size(), nMpb = bird ? tables.mpbBad.size() : 0,
                 nBobs = bird ? tables.bobsKf.size() : 0;
    kfSlot.assign(nKf, -1); kfFixed.assign(nKf, 0); kfTcw.assign(nKf * 12, 0.f); mpIndex.assign(nMp + 1, -1); mpXw.assign(nMp * 3 + 1, 0.f);
    obsKf.assign(nObs + 1, -1); obsMp.assign(nObs + 1, -1); obsSrc.assign(nObs + 1, -1); obsUv.assign(nObs * 2 + 1, 0.f);
    obsInvSigma2.assign(nObs + 1, 0.f); mpbIndex.assign(nMpb + 1, -1); mpbXw.assign(nMpb * 3 + 1, 0.f); bobsKf.assign(nBobs + 1, -1);
    bobsMpb.assign(nBobs + 1, -1); bobsSrc.assign(nBobs + 1, -1); bobsXc.assign(nBobs * 3 + 1, 0.f); bobsInvSigma2.assign(nBobs + 1, 0.f);
    fb_covis_window w;
    memset(&w, 0, sizeof(w));
    w.cap_kf = (int32_t)nKf; w.cap_mp = (int32_t)nMp; w.cap_obs = (int32_t)nObs; w.cap_mpb = (int32_t)nMpb; w.cap_bobs = (int32_t)nBobs;
    w.kf_slot = kfSlot.data(); w.kf_fixed = kfFixed.data(); w.kf_Tcw = kfTcw.data(); w.mp_index = mpIndex.data(); w.mp_xw = mpXw.data();
    w.obs_kf = obsKf.data(); w.obs_mp = obsMp.data(); w.obs_src = obsSrc.data(); w.obs_uv = obsUv.data(); w.obs_inv_sigma2 = obsInvSigma2.data();
    w.mpb_index = mpbIndex.data(); w.mpb_xw = mpbXw.data(); w.bobs_kf = bobsKf.data(); w.bobs_mpb = bobsMpb.data(); w.bobs_src = bobsSrc.data();
    w.bobs_xc = bobsXc.data(); w.bobs_inv_sigma2 = bobsInvSigma2.data();
    fb_covis_window_header h;
    w.header = &h;
    check(fb_covis_local_window(g.handle(), &m, &t, currentKF, bird ? 1 : 0, &w));
    nLocal = h.n_local; nFixed = h.n_fixed;
    kfSlot.resize(nLocal + nFixed); kfFixed.resize(nLocal + nFixed); kfTcw.resize((size_t)(nLocal + nFixed) * 12);
    mpIndex.resize(h.n_mp); mpXw.resize((size_t)h.n_mp * 3); mpbIndex.resize(h.n_mpb); mpbXw.resize((size_t)h.n_mpb * 3);
    obsKf.resize(h.n_obs); obsMp.resize(h.n_obs); obsSrc.resize(h.n_obs); obsUv.resize((size_t)h.n_obs * 2); obsInvSigma2.resize(h.n_obs);
    bobsKf.resize(h.n_bobs); bobsMpb.resize(h.n_bobs); bobsSrc.resize(h.n_bobs); bobsXc.resize((size_t)h.n_bobs * 3); bobsInvSigma2.resize(h.n_bobs);
  }
  std::vector<int> localKeyFrames() const { return std::vector<int>(kfSlot.begin(), kfSlot.begin() + nLocal); }
  std::vector<int> fixedCameras() const { return std::vector<int>(kfSlot.begin() + nLocal, kfSlot.end()); }

  // the optimisation on the collected window (fb_local_ba; a defaults to the camera and weights the caller filled in)
  void Optimize(fb_local_ba_args a, const std::vector<OdomEdge> &odom, const volatile uint8_t *pbStopFlag = nullptr) {
    std::vector<int32_t> oi, oj;
    std::vector<float> oT;
    std::vector<double> oInfo;
    for (const OdomEdge &e : odom) { oi.push_back(e.i); oj.push_back(e.j); oT.insert(oT.end(), e.Tij, e.Tij + 12); oInfo.push_back(e.info); }
    obsOutlier.assign(obsKf.size() + 1, 0); bobsOutlier.assign(bobsKf.size() + 1, 0);
    a.n_kf = nLocal + nFixed; a.kf_Tcw = kfTcw.data(); a.kf_fixed = kfFixed.data(); a.n_mp = (int32_t)mpIndex.size(); a.mp_xw = mpXw.data();
    a.n_mpb = (int32_t)mpbIndex.size(); a.mpb_xw = mpbXw.data(); a.n_obs = (int32_t)obsKf.size(); a.obs_kf = obsKf.data(); a.obs_mp = obsMp.data();
    a.obs_uv = obsUv.data(); a.obs_inv_sigma2 = obsInvSigma2.data(); a.n_bobs = (int32_t)bobsKf.size(); a.bobs_kf = bobsKf.data();
    a.bobs_mpb = bobsMpb.data(); a.bobs_xc = bobsXc.data(); a.bobs_inv_sigma2 = bobsInvSigma2.data(); a.n_odom = (int32_t)oi.size();
    a.odom_kf_i = oi.data(); a.odom_kf_j = oj.data(); a.odom_Tij = oT.data(); a.odom_info = oInfo.data(); a.stop_flag = pbStopFlag;
    a.obs_outlier = obsOutlier.data(); a.bobs_outlier = bobsOutlier.data();
    check(fb_local_ba(&a));
  }

  // :2574-2669: vToErase / vToEraseBird in edge order, SetPose of the local key frames, SetWorldPos of the local points
  void WriteBack(const CovisibilityMap &map, WindowTables &tables) {
    toErase.clear(); toEraseBird.clear();
    for (size_t i = 0; i < obsKf.size() && i < obsOutlier.size(); i++)
      if (obsOutlier[i]) toErase.push_back({kfSlot[obsKf[i]], mpIndex[obsMp[i]], map.obsIdx[obsSrc[i]], obsSrc[i]});
    for (size_t i = 0; i < bobsKf.size() && i < bobsOutlier.size(); i++)
      if (bobsOutlier[i]) toEraseBird.push_back({kfSlot[bobsKf[i]], mpbIndex[bobsMpb[i]], tables.bobsIdx[bobsSrc[i]], bobsSrc[i]});
    for (int k = 0; k < nLocal; k++) std::copy(kfTcw.begin() + (size_t)k * 12, kfTcw.begin() + (size_t)k * 12 + 12, tables.kfTcw.begin() + (size_t)kfSlot[k] * 12);
    for (size_t j = 0; j < mpIndex.size(); j++) std::copy(mpXw.begin() + j * 3, mpXw.begin() + j * 3 + 3, tables.mpXw.begin() + (size_t)mpIndex[j] * 3);
    for (size_t j = 0; j < mpbIndex.size(); j++) std::copy(mpbXw.begin() + j * 3, mpbXw.begin() + j * 3 + 3, tables.mpbXw.begin() + (size_t)mpbIndex[j] * 3);
  }
};

// ---- Sim3Solver (include/Sim3Solver.h) ---------------------------------------------------------------------------------
// One candidate per object, as in the reference.  The first iterate() runs fb_sim3_solver once: every iteration up to
// mRansacMaxIts lands in a table, and iterate(n, ...) replays rows (mnIterations, mnIterations + n] of it, so
// LoopClosing's round-robin iterate(5, ...) and its "go on after a failed OptimizeSim3" behave as in the reference.
// The 3 x mRansacMaxIts RandomInt values are drawn when the table is filled (INTEGRATION.md 7 on what that means for the
// random stream).
struct Sim3KeyFrame {             // what Sim3Solver reads of a KeyFrame
  int N = 0;                      // features
  const fb_keypoint *mvKeysUn = nullptr;
  const uint8_t *mpValid = nullptr;        // [N] GetMapPointMatches()[i] && !isBad()
  const float *mpWorldPos = nullptr;       // [N][3] GetWorldPos()
  const int32_t *indexInKeyFrame = nullptr;  // [N] GetIndexInKeyFrame(this key frame), or NULL = i
  const float *Tcw = nullptr;              // [12] GetRotation | GetTranslation
  float fx = 0, fy = 0, cx = 0, cy = 0;    // mK
  long mnFrameId = 0;
};

// the key-frame pair of fb_sim3_solver_args / fb_optimize_sim3_args: n_cand = 1 (one pKF2), kf1 / kf2 / mp1 / mp2, the
// cameras, T1w / T2w and kf2_index.  n1 must outlive the call (kf1.n_kf points at it).
template <typename Args>
inline void fill_sim3_pair(Args &a, const Sim3KeyFrame &kf1, const Sim3KeyFrame &kf2, const int32_t *n1) {
  const Sim3KeyFrame *kf[2] = {&kf1, &kf2};
  fb_kf_target *k[2] = {&a.kf1, &a.kf2};
  fb_mp_list *m[2] = {&a.mp1, &a.mp2};
  for (int i = 0; i < 2; i++) {
    k[i]->kf_stride = kf[i]->N; k[i]->kf_kps = kf[i]->mvKeysUn;
    k[i]->cam.fx = kf[i]->fx; k[i]->cam.fy = kf[i]->fy; k[i]->cam.cx = kf[i]->cx; k[i]->cam.cy = kf[i]->cy;
    m[i]->mp_stride = kf[i]->N; m[i]->mp_valid = kf[i]->mpValid; m[i]->mp_xw = kf[i]->mpWorldPos;
  }
  a.n_cand = 1;
  a.kf1.n_kf = n1;
  a.T1w = kf1.Tcw; a.T2w = kf2.Tcw; a.kf2_index = kf2.indexInKeyFrame;
}

class Sim3Solver {
 public:
  typedef int (*RandomIntFn)(int min, int max);
  // DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp)
  static int RandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
  }
  // vnMatches12[i1] = feature of pKF2 whose MapPoint is vpMatched12[i1], or -1 (fb_match_bow_kf's matches12)
  Sim3Solver(const Sim3KeyFrame &kf1, const Sim3KeyFrame &kf2, const std::vector<int32_t> &vnMatches12, bool bFixScale,
             const float *mvLevelSigma2, int nLevels, RandomIntFn randomInt = &Sim3Solver::RandomInt)
      : kf1_(kf1), kf2_(kf2), m12_(vnMatches12), fixScale_(bFixScale), rand_(randomInt) {
    for (int l = 0; l < FB_MAX_LEVELS; l++) sigma2_[l] = l < nLevels ? mvLevelSigma2[l] : 0.0f;
    mN1 = (int)m12_.size();
    if (mN1 != kf1.N || kf1.N < 1 || kf2.N < 1) throw std::runtime_error("Sim3Solver: vpMatched12.size() must equal pKF1->N, and both key frames need features");
    N = 0;  // the constructor's count (Sim3Solver.cc:62-103) with fb_sim3_solver's skip rule, needed here for the range of the draws
    for (int i1 = 0; i1 < mN1; i1++) {
      const int j = m12_[i1];
      if (j < 0 || j >= kf2.N || !kf1.mpValid[i1] || !kf2.mpValid[j]) continue;
      const int k1 = kf1.indexInKeyFrame ? kf1.indexInKeyFrame[i1] : i1, k2 = kf2.indexInKeyFrame ? kf2.indexInKeyFrame[j] : j;
      if (k1 < 0 || k2 < 0 || k1 >= kf1.N || k2 >= kf2.N) continue;
      const int o1 = kf1.mvKeysUn[k1].octave, o2 = kf2.mvKeysUn[k2].octave;
      if (o1 < 0 || o1 >= FB_MAX_LEVELS || o2 < 0 || o2 >= FB_MAX_LEVELS) continue;  // (the reference would read out of bounds)
      N++;
    }
    SetRansacParameters();
  }

  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    maxIterations_ = maxIterations;
    const float epsilon = (float)mRansacMinInliers / N;
    int nIterations;
    if (mRansacMinInliers == N) {
      nIterations = 1;
    } else {
      const double x = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(epsilon, 3)));
      nIterations = x < (double)maxIterations ? (int)x : maxIterations;
    }
    mRansacMaxIts = std::max(1, std::min(nIterations, maxIterations));
    mnIterations = 0;
    filled_ = false;
  }

  // true = the reference returned mBestT12 (GetEstimated* hold it); false = the empty cv::Mat
  bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    if (N < mRansacMinInliers) {
      bNoMore = true;
      return false;
    }
    if (!filled_) fill();
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
      nCurrentIterations++;
      mnIterations++;
      const int k = mnIterations - 1;
      if (ninl_[k] >= mnBestInliers) {
        mnBestInliers = ninl_[k];
        best_ = k;
        if (accept_[k]) {
          nInliers = ninl_[k];
          for (int i = 0; i < N; i++)
            if ((mask_[(size_t)k * mw_ + i / 32] >> (i % 32)) & 1u) vbInliers[idx1_[i]] = true;
          return true;
        }
      }
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    return false;
  }
  bool find(std::vector<bool> &vbInliers12, int &nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
  }
  const float *GetEstimatedRotation() const { return &R_[(size_t)best_ * 9]; }     // row-major 3x3
  const float *GetEstimatedTranslation() const { return &t_[(size_t)best_ * 3]; }
  float GetEstimatedScale() const { return s_[best_]; }
  int iterations() const { return mnIterations; }
  int maxIterations() const { return mRansacMaxIts; }
  int correspondences() const { return N; }

 private:
  void fill() {
    const int s1 = kf1_.N;
    mw_ = (s1 + 31) / 32;
    std::vector<int32_t> m12(s1, -1), rnd((size_t)FB_SIM3_MAX_HYP * 3, 0);
    std::copy(m12_.begin(), m12_.end(), m12.begin());
    for (int k = 0; k < mRansacMaxIts; k++)
      for (int j = 0; j < 3; j++) rnd[(size_t)k * 3 + j] = rand_(0, N - j - 1);
    // (Sim3Solver.cc:192: inside the frame-id window more than 15 inliers are enough)
    int32_t above = mRansacMinInliers;
    if (kf1_.mnFrameId > 1126 && kf1_.mnFrameId < 1136) above = std::min(mRansacMinInliers, 15);
    const int32_t n1 = kf1_.N;
    idx1_.assign(s1, -1);
    s_.assign(FB_SIM3_MAX_HYP, 0.f); R_.assign((size_t)FB_SIM3_MAX_HYP * 9, 0.f); t_.assign((size_t)FB_SIM3_MAX_HYP * 3, 0.f);
    ninl_.assign(FB_SIM3_MAX_HYP, 0); accept_.assign(FB_SIM3_MAX_HYP, 0); mask_.assign((size_t)FB_SIM3_MAX_HYP * mw_, 0u);
    int32_t Ndev = 0, maxIts = 0, done = 0, first = 0, noMore = 0;
    fb_sim3_solver_args a;
    memset(&a, 0, sizeof(a));
    fill_sim3_pair(a, kf1_, kf2_, &n1);
    a.kf1_index = kf1_.indexInKeyFrame;
    a.matches12 = m12.data();
    for (int l = 0; l < FB_MAX_LEVELS; l++) a.level_sigma2[l] = sigma2_[l];
    a.fix_scale = fixScale_ ? 1 : 0;
    a.ransac_prob = mRansacProb; a.min_inliers = mRansacMinInliers; a.max_iterations = maxIterations_;
    a.accept_above = &above; a.rand_idx = rnd.data();
    a.N = &Ndev; a.indices1 = idx1_.data(); a.max_its = &maxIts; a.n_hyp_done = &done; a.first_accept = &first; a.no_more = &noMore;
    a.s = s_.data(); a.R = R_.data(); a.t = t_.data(); a.n_inliers = ninl_.data(); a.accept = accept_.data(); a.inlier_mask = mask_.data();
    check(fb_sim3_solver(&a));
    if (Ndev != N || maxIts != mRansacMaxIts) throw std::runtime_error("Sim3Solver: the device's N / mRansacMaxIts differ from the host's");
    filled_ = true;
  }
  Sim3KeyFrame kf1_, kf2_;
  std::vector<int32_t> m12_;
  bool fixScale_;
  RandomIntFn rand_;
  float sigma2_[FB_MAX_LEVELS];
  int mN1 = 0, N = 0, mw_ = 0;
  double mRansacProb = 0.99;
  int mRansacMinInliers = 6, mRansacMaxIts = 300, maxIterations_ = 300, mnIterations = 0, mnBestInliers = 0, best_ = 0;
  bool filled_ = false;
  std::vector<int32_t> idx1_, ninl_;
  std::vector<float> s_, R_, t_;
  std::vector<uint8_t> accept_;
  std::vector<uint32_t> mask_;
};

inline int Optimizer::OptimizeSim3(const Sim3KeyFrame &kf1, const Sim3KeyFrame &kf2, std::vector<int32_t> &vnMatches1, const float *R12,
                                   const float *t12, float s12, Sim3 &g2oS12, float th2, bool bFixScale,
                                   const float *mvInvLevelSigma2, int nLevels, Sim3 *mg2oScw, float *Scw) {
  if ((int)vnMatches1.size() != kf1.N || kf1.N < 1 || kf2.N < 1)
    throw std::runtime_error("OptimizeSim3: vpMatches1.size() must equal pKF1->N, and both key frames need features");
  const int32_t n1 = kf1.N;
  int32_t nIn = 0, nCorr = 0, nBad = 0;
  Sim3 scw;
  float scwRows[12];
  fb_optimize_sim3_args a;
  memset(&a, 0, sizeof(a));
  fill_sim3_pair(a, kf1, kf2, &n1);
  for (int l = 0; l < FB_MAX_LEVELS; l++) a.inv_level_sigma2[l] = l < nLevels ? mvInvLevelSigma2[l] : 0.0f;
  a.matches12 = vnMatches1.data();
  a.s12 = &s12; a.R12 = R12; a.t12 = t12; a.hyp_stride = 1;
  a.th2 = th2; a.fix_scale = bFixScale ? 1 : 0;
  a.n_inliers = &nIn; a.n_correspondences = &nCorr; a.n_bad = &nBad;
  a.q = g2oS12.q; a.t = g2oS12.t; a.s = &g2oS12.s;
  a.scw_q = scw.q; a.scw_t = scw.t; a.scw_s = &scw.s; a.Scw = scwRows;
  check(fb_optimize_sim3(&a));
  if (mg2oScw) *mg2oScw = scw;
  if (Scw) memcpy(Scw, scwRows, sizeof(scwRows));
  return nIn;
}

}  // namespace fishbird
#endif
