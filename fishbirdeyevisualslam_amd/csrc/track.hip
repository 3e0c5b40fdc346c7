// track.hip -- the device-resident Frame (fb_frame) and the per-frame tracking chain on gfx950.
//
// Replaces, as ONE device-resident sequence whose steps hand their results over in HBM (reference file:line):
//   Frame::Frame(...)                      src/Frame.cc:262-379   (extract, undistort, bird filter, cam XYZ, grids, member init)
//   Frame::SetPose / UpdatePoseMatrices    src/Frame.cc:421-433
//   Tracking::TrackWithMotionModel         src/Tracking.cc:1312-1385  (pose prediction, M9, M3, pose optimisation, outlier discard)
//   Tracking::TrackLocalMap                src/Tracking.cc:1387-1441  (M8 + FilterBirdOutlierInFront :1825-1914,
//                                                                      SearchLocalPoints :1947-1997, pose optimisation, inlier count)
//   end of Tracking::Track                 src/Tracking.cc:690-701, 721-725 (clean VO matches, drop outliers)
//
// The matchers, the extractor and the pose optimiser are the kernels of match.hip / orb.hip / pose.hip, reached through
// their *_dev entry points; this file adds the Frame state and the glue the reference does with pointer walks between
// them (mvpMapPoints bookkeeping, edge construction, MapPointBird creation).  Glue kernels are streaming maps over
// <= ~2000 slots per frame: one lane per slot, grid (slots / 256, batch), or one workgroup per sequence where a serial
// rule needs a block-wide scan / reduction.  They are latency-, not bandwidth-bound; what matters is the launch count
// per frame (17 + the extractor's), so commits ride in the kernel that follows them.
//
// The text: track_plan.h lays the handle's memory out (host code), track_kernels.inc holds the glue kernels,
// track_stages.inc the stages that launch them; here are the handle, Frame construction and the C entry points.
#include "fb_common.h"
#include "fb_frame_geom.h"
#include "fb_primitives.h"

#include <cmath>
#include <new>

#include "track_plan.h"
#include "track_kernels.inc"

namespace {
// host-side pointer blocks of the scratch no glue kernel takes as a struct
struct M9Scratch { uint8_t *valid; float *xw; uint8_t *desc; int32_t *n; uint8_t *ones; };
struct M8Scratch { int32_t *m12, *dist, *n, *nd; };
struct PreGuidance { int32_t *n; fb_keypoint *kps; uint8_t *desc, *keep; };  // the bird extractor's output when the guidance filter follows it
struct BowDev { int32_t *nw; uint32_t *ids; double *vals; int32_t *fv_nn; uint32_t *fv_ids; int32_t *fv_start, *fv_items; };
}  // namespace

struct fb_frame {
  fb_frame_params P;
  int cap = 0, B = 0;
  fb_orb_tables tab;
  fb_grid_geom gF, gB;
  fb_camera cam;
  float logScale = 0.f;
  SigmaTab sig;
  FramePlan plan;
  fb::DevBuf arena[FA_COUNT];  // FA_BOW: by the first fb_frame_compute_bow_dev (ensure_bow)
  // typed pointers into the arenas, set once by bind() / ensure_bow()
  FrameDev F;                              // the members the glue kernels take by value
  int32_t *cs, *ci, *bcs, *bci, *counts;   // the other members: mGrid, mGridBirdview, the counter block
  BowDev bw{};                             // mBowVec / mFeatVec (Frame.h:128-129)
  M3Scratch m3; LocalScratch loc; EdgeOut E; M9Scratch m9; M8Scratch m8; PreGuidance pre;
  int32_t *m_front, *m_bird, *m_local;     // what a matcher found, until a commit folds it into mp / mpb
  uint8_t *bow_has_mp;
  void *m2_ws;
  bool bowDone = false;   // !mBowVec.empty() (in the order the calls were enqueued)
  int minInliers = 30;    // the threshold the last end-of-Track clean-up used (fb_frame_drop_outliers_dev follows it)
  // cv::cornerSubPix on the bird key points (Frame.cc:345-352): half window 0 = not run (fb_frame_set_bird_subpix)
  int subpixHalf = 0, subpixIters = 40;
  double subpixEps = 0.001;
  // extractorBird->compute at the refined positions (Frame.cc:352-355, fb_frame_set_bird_redescribe): runs only with subpix on
  bool redescribe = false, redescribed = false;  // the switch; the last extraction ran it
  fb::DevBuf describeStatus;                     // [B][cap] FB_DESCRIBE_*, plan_redescribe_status(); allocated by the switch
  // cv::ORB's detector instead of ORBextractor on the bird image (Frame.cc:337-340, fb_frame_set_bird_detector)
  int detectMode = FB_BIRD_DETECT_ORBEXTRACTOR, detectThr = 20;
  // images from host callers
  fb::DevBuf img_f, img_b, img_c, img_m;
  uint8_t *pin = nullptr;
  size_t pinBytes = 0;
  int32_t *pinCounts = nullptr;
  hipStream_t sBird = nullptr;
  hipEvent_t evFork = nullptr, evJoin = nullptr, evCopy = nullptr;
  ~fb_frame() {
    if (evFork) (void)hipEventDestroy(evFork);
    if (evJoin) (void)hipEventDestroy(evJoin);
    if (evCopy) (void)hipEventDestroy(evCopy);
    if (sBird) (void)hipStreamDestroy(sBird);
    if (pin) (void)hipHostFree(pin);
    if (pinCounts) (void)hipHostFree(pinCounts);
  }
  template <typename T> T *at(int id) const {
    const FrameRegion &R = plan.r[id];
    return reinterpret_cast<T *>(static_cast<uint8_t *>(arena[R.arena].p) + R.off);
  }
  void bind() {  // members and scratch
    F.cap = cap;
    F.map_cap = P.map_cap; F.seen_mark = at<uint8_t>(FR_seen_mark);
    F.n = at<int32_t>(FR_n); F.kps = at<fb_keypoint>(FR_kps); F.kps_un = at<fb_keypoint>(FR_kps_un); F.desc = at<uint8_t>(FR_desc);
    F.mp = at<int32_t>(FR_mp); F.outlier = at<uint8_t>(FR_outlier);
    F.nb = at<int32_t>(FR_nb); F.bkps = at<fb_keypoint>(FR_bkps); F.bdesc = at<uint8_t>(FR_bdesc); F.bcam = at<float>(FR_bcam);
    F.mpb = at<int32_t>(FR_mpb); F.boutlier = at<uint8_t>(FR_boutlier);
    F.Tcw = at<float>(FR_Tcw);
    cs = at<int32_t>(FR_cs); ci = at<int32_t>(FR_ci); bcs = at<int32_t>(FR_bcs); bci = at<int32_t>(FR_bci); counts = at<int32_t>(FR_counts);
    m3 = {at<uint8_t>(FR_m3_valid), at<uint8_t>(FR_m3_obs), at<float>(FR_m3_xw), at<uint8_t>(FR_m3_desc), at<int32_t>(FR_m3_oct), at<float>(FR_m3_ang)};
    loc = {at<uint8_t>(FR_l_seen), at<uint8_t>(FR_l_blocked), at<uint8_t>(FR_l_inview), at<uint8_t>(FR_l_obs), at<float>(FR_l_proj),
           at<int32_t>(FR_l_level), at<float>(FR_l_cos), at<uint8_t>(FR_l_desc), at<int32_t>(FR_l_n)};
    E = {at<float>(FR_e_fxw), at<float>(FR_e_fobs), at<float>(FR_e_finf), at<uint8_t>(FR_e_fvalid),
         at<float>(FR_e_bxw), at<float>(FR_e_bxc), at<float>(FR_e_binf), at<uint8_t>(FR_e_bvalid)};
    m9 = {at<uint8_t>(FR_m9_valid), at<float>(FR_m9_xw), at<uint8_t>(FR_m9_desc), at<int32_t>(FR_m9_n), at<uint8_t>(FR_ones)};
    m8 = {at<int32_t>(FR_m8_m12), at<int32_t>(FR_m8_dist), at<int32_t>(FR_m8_n), at<int32_t>(FR_m8_nd)};
    pre = {at<int32_t>(FR_nb_pre), at<fb_keypoint>(FR_bkps_pre), at<uint8_t>(FR_bdesc_pre), at<uint8_t>(FR_guidance_keep)};
    m_front = at<int32_t>(FR_m_front); m_bird = at<int32_t>(FR_m_bird); m_local = at<int32_t>(FR_m_local);
    bow_has_mp = at<uint8_t>(FR_bow_has_mp);
    m2_ws = at<void>(FR_m2_ws);
  }
  int ensure_bow() {
    if (arena[FA_BOW].p) return FB_OK;
    FB_TRY(arena[FA_BOW].alloc(plan.arena_bytes[FA_BOW], true));
    bw = {at<int32_t>(FR_bow_nw), at<uint32_t>(FR_bow_ids), at<double>(FR_bow_vals), at<int32_t>(FR_fv_nn), at<uint32_t>(FR_fv_ids),
          at<int32_t>(FR_fv_start), at<int32_t>(FR_fv_items)};
    return FB_OK;
  }
  int32_t *cnt(int slot) const { return counts + (size_t)slot * B; }
};

#include "track_stages.inc"

extern "C" {

int fb_frame_create(const fb_frame_params *p, fb_frame **out) {
  FB_ARG(p && out && p->batch >= 1 && p->batch <= 65535);
  FB_ARG(p->front_width > 0 && p->front_height > 0 && p->bird_width > 0 && p->bird_height > 0);
  FB_ARG(p->orb.nlevels >= 1 && p->orb.nlevels <= FB_MAX_LEVELS && p->orb.nfeatures > 0 && p->orb.scale_factor > 1.0f);
  FB_ARG(p->map_cap >= 1 && p->local_mp_cap >= 1 && p->local_mpb_cap >= 1);
  FB_ARG(p->bird_nfeatures >= 0 && p->bird_nfeatures <= p->orb.nfeatures);
  FB_TRY(fb::check_device());
  fb_frame *f = new (std::nothrow) fb_frame();
  if (!f) { fb::set_error("fb_frame_create: out of memory"); return FB_ERR_HIP; }
  f->P = *p;
  f->B = p->batch;
  f->cap = fb_orb_capacity(&p->orb);
  {  // the extractor's level tables (mvScaleFactors ... mvInvLevelSigma2, Frame.cc:299-306)
    fb_orb *o = nullptr;
    int rc = fb_orb_create(&p->orb, &o);
    if (rc != FB_OK) { delete f; return rc; }
    fb_orb_get_tables(o, &f->tab);
    fb_orb_destroy(o);
  }
  for (int i = 0; i < FB_MAX_LEVELS; i++) f->sig.inv_sigma2[i] = f->tab.inv_level_sigma2[i];
  f->logScale = (float)log((double)p->orb.scale_factor);  // mfLogScaleFactor = log(mfScaleFactor), Frame.cc:301
  float bounds[4];
  {  // ComputeImageBounds + grid cell sizes (Frame.cc:271-283)
    int rc = fb_image_bounds(p->front_width, p->front_height, p->K, p->D, bounds);
    if (rc != FB_OK) { delete f; return rc; }
  }
  f->gF.min_x = bounds[0]; f->gF.min_y = bounds[2];
  f->gF.inv_w = 64.0f / (bounds[1] - bounds[0]);  // FRAME_GRID_COLS / (mnMaxX - mnMinX), Frame.h:38-39
  f->gF.inv_h = 48.0f / (bounds[3] - bounds[2]);
  f->gF.cols = 64; f->gF.rows = 48;
  f->gB.min_x = 0.f; f->gB.min_y = 0.f;
  f->gB.inv_w = 32.0f / (float)p->bird_width;     // FRAME_GRID_BIRD, Frame.h:40
  f->gB.inv_h = 32.0f / (float)p->bird_height;
  f->gB.cols = 32; f->gB.rows = 32;
  f->cam.fx = p->K[0]; f->cam.fy = p->K[1]; f->cam.cx = p->K[2]; f->cam.cy = p->K[3];
  f->cam.min_x = bounds[0]; f->cam.max_x = bounds[1]; f->cam.min_y = bounds[2]; f->cam.max_y = bounds[3];
  // the arenas at their exact size: a handle lives long, and a power-of-two class of a whole arena could double it
  int rc = plan_frame(*p, f->cap, &f->plan);
  if (rc == FB_OK) rc = f->arena[FA_MEMBERS].alloc(f->plan.arena_bytes[FA_MEMBERS], true);
  if (rc == FB_OK) rc = f->arena[FA_SCRATCH].alloc(f->plan.arena_bytes[FA_SCRATCH], true);
  if (rc != FB_OK) { delete f; return rc; }
  f->bind();
  hipError_t e = hipSuccess;
  for (int i = 0; i < FR_COUNT && e == hipSuccess; i++)
    if (f->plan.r[i].fill != FILL_NONE) e = hipMemset(f->at<void>(i), f->plan.r[i].fill, f->plan.r[i].bytes);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->sBird, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&f->evFork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&f->evJoin, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&f->evCopy, hipEventDisableTiming);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&f->pinCounts), ((size_t)f->B * FB_CNT_COUNT + (size_t)f->B * 12) * 4, hipHostMallocDefault);
  if (e != hipSuccess) {
    fb::set_error("fb_frame_create: %s", hipGetErrorString(e));
    (void)hipGetLastError();
    delete f;
    return FB_ERR_HIP;
  }
  *out = f;
  return FB_OK;
}

void fb_frame_destroy(fb_frame *f) { delete f; }

int fb_frame_extract_dev(fb_frame *f, fb_orb *of, fb_orb *ob, const uint8_t *d_front, int front_stride, size_t front_image_stride,
                         const uint8_t *d_bird, int bird_stride, size_t bird_image_stride, const uint8_t *d_contour,
                         const uint8_t *d_mask, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && of && ob && of != ob && d_front && d_bird);
  FB_ARG(front_stride >= f->P.front_width && bird_stride >= f->P.bird_width);
  FB_ARG(!d_mask || d_contour);  // the detect mask rides in the contour kernel
  if (d_contour) FB_ARG(bird_image_stride == (size_t)bird_stride * f->P.bird_height);  // contour / mask share the bird image's geometry
  // (while every kernel is bracketed for a per-kernel table -- fb_prof_enable without fb_prof_only -- the bird chain stays on
  // the caller's stream, so that the table shows each kernel on its own)
  const bool fork = !(fb::g_prof_on && fb::g_prof_only < 0);
  hipStream_t s = fb::as_stream(stream), sb = fork ? f->sBird : s;
  const int B = f->B, cap = f->cap;
  const FrameDev &F = f->F;
  f->bowDone = false;                         // a new Frame: mBowVec empty
  FB_TRY(fb_orb_set_output_stride(of, cap));  // both extractors write into the frame's arrays (one stride)
  FB_TRY(fb_orb_set_output_stride(ob, cap));
  // bird chain on the handle's stream, beside the front chain
  if (fork) {
    FB_HIP(hipEventRecord(f->evFork, s));
    FB_HIP(hipStreamWaitEvent(sb, f->evFork, 0));
  }
  {
    fb_keypoint *k0 = d_contour ? f->pre.kps : F.bkps;
    uint8_t *d0 = d_contour ? f->pre.desc : F.bdesc;
    int32_t *n0 = d_contour ? f->pre.n : F.nb;
    const bool cvorb = f->detectMode == FB_BIRD_DETECT_CVORB;
    if (cvorb) {  // Frame.cc:337-340: cv::ORB::detect(bird, mask); the descriptors follow at the end of the chain
      fb_orb_detect_args E;
      memset(&E, 0, sizeof(E));
      E.batch = B; E.width = f->P.bird_width; E.height = f->P.bird_height; E.stride = bird_stride; E.image_stride = bird_image_stride;
      E.images = d_bird; E.mask = d_mask; E.mask_stride = bird_stride; E.fast_threshold = f->detectThr;
      E.kp_stride = cap; E.kps = k0; E.n = n0;
      FB_TRY(fb_orb_detect_masks_dev(ob, &E, d_mask ? bird_image_stride : 0, sb));
    } else {
      FB_TRY(fb_orb_extract_batch_dev(ob, d_bird, B, f->P.bird_width, f->P.bird_height, bird_stride, bird_image_stride, k0, d0, n0, sb));
    }
    if (d_contour) {
      fb_bird_guidance_args G;
      memset(&G, 0, sizeof(G));
      G.batch = B; G.kp_stride = cap; G.cols = f->P.bird_width; G.rows = f->P.bird_height; G.pitch = bird_stride;
      G.contour = d_contour; G.mask = cvorb ? nullptr : d_mask; G.n_in = n0; G.kps_in = k0; G.desc_in = cvorb ? nullptr : d0;
      G.n_out = F.nb; G.kps_out = F.bkps; G.desc_out = cvorb ? nullptr : F.bdesc;
      G.keep = f->pre.keep;  // [batch][cap]: the verdicts are computed by many workgroups
      FB_TRY(fb_bird_guidance_dev(&G, sb));
    }
    if (f->subpixHalf > 0) {  // Frame.cc:345-352: mvKeysBird[k].pt refined before the camera positions and the grid
      fb_corner_subpix_args S;
      memset(&S, 0, sizeof(S));
      S.batch = B; S.kp_stride = cap; S.cols = f->P.bird_width; S.rows = f->P.bird_height; S.pitch = bird_stride;
      S.image_stride = bird_image_stride; S.image = d_bird; S.n = F.nb; S.kps = F.bkps;
      S.half_win_x = S.half_win_y = f->subpixHalf; S.max_iter = f->subpixIters; S.eps = f->subpixEps;
      FB_TRY(fb_corner_subpix_dev(&S, sb));
      if (f->redescribe && !cvorb) {  // Frame.cc:352-355: the descriptors of the refined positions, on the bird extractor's blurred pyramid
        fb_orb_describe_args R;
        memset(&R, 0, sizeof(R));
        R.batch = B; R.kp_stride = cap; R.n = F.nb; R.kps = F.bkps; R.desc = F.bdesc; R.status = f->describeStatus.as<uint8_t>();
        R.angle_mode = FB_DESCRIBE_KEEP_ANGLE;
        FB_TRY(fb_orb_describe_dev(ob, &R, sb));
      }
    }
    if (cvorb) {  // Frame.cc:352-355: extractorBird->compute, here the only source of the descriptors
      fb_orb_describe_args R;
      memset(&R, 0, sizeof(R));
      R.batch = B; R.kp_stride = cap; R.n = F.nb; R.kps = F.bkps; R.desc = F.bdesc; R.status = f->describeStatus.as<uint8_t>();
      R.angle_mode = FB_DESCRIBE_KEEP_ANGLE;
      FB_TRY(fb_orb_describe_dev(ob, &R, sb));
    }
    f->redescribed = cvorb || (f->subpixHalf > 0 && f->redescribe);
    FB_TRY(fb_bird_keys_to_cam_dev(F.bkps, F.nb, B, cap, f->P.bird_width, f->P.bird_height, f->P.pixel2meter, f->P.rear_axle_to_center,
                                   f->P.Tcb, F.bcam, sb));
    FB_TRY(fb_grid_build_batch_dev(F.bkps, F.nb, B, cap, &f->gB, f->bcs, f->bci, sb));
    if (fork) FB_HIP(hipEventRecord(f->evJoin, sb));
  }
  FB_TRY(fb_orb_extract_batch_dev(of, d_front, B, f->P.front_width, f->P.front_height, front_stride, front_image_stride, F.kps, F.desc, F.n, s));
  FB_TRY(fb_undistort_keypoints_dev(F.kps, F.n, B, cap, f->P.K, f->P.D, F.kps_un, s));
  FB_TRY(fb_grid_build_batch_dev(F.kps_un, F.n, B, cap, &f->gF, f->cs, f->ci, s));
  { fb::ProfScope prof_(fb::P_TRACK_GLUE, s);
    k_frame_reset<<<slot_grid(f), TT, 0, s>>>(F, f->counts, B); }
  FB_HIP(hipGetLastError());
  if (fork) FB_HIP(hipStreamWaitEvent(s, f->evJoin, 0));
  return FB_OK;
}

int fb_frame_extract(fb_frame *f, fb_orb *of, fb_orb *ob, const uint8_t *front, int front_stride, const uint8_t *bird,
                     int bird_stride, const uint8_t *contour, const uint8_t *mask, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && front && bird && front_stride >= f->P.front_width && bird_stride >= f->P.bird_width);
  const size_t B = f->B, fb_ = (size_t)front_stride * f->P.front_height, bb = (size_t)bird_stride * f->P.bird_height;
  const size_t need = B * (fb_ + 3 * bb);
  hipStream_t s = fb::as_stream(stream);
  if (f->pinBytes < need) {
    if (f->pin) { FB_HIP(hipStreamSynchronize(s)); FB_HIP(hipHostFree(f->pin)); f->pin = nullptr; f->pinBytes = 0; }
    FB_HIP(hipHostMalloc(reinterpret_cast<void **>(&f->pin), need, hipHostMallocDefault));
    f->pinBytes = need;
    FB_TRY(f->img_f.alloc(B * fb_)); FB_TRY(f->img_b.alloc(B * bb)); FB_TRY(f->img_c.alloc(B * bb)); FB_TRY(f->img_m.alloc(B * bb));
  } else {
    // the previous call's copies out of the staging block must be done before it is overwritten
    FB_HIP(hipEventSynchronize(f->evCopy));
  }
  uint8_t *pf = f->pin, *pb = pf + B * fb_, *pc = pb + B * bb, *pm = pc + B * bb;
  const uint8_t *df = static_cast<uint8_t *>(f->img_f.p), *db = static_cast<uint8_t *>(f->img_b.p);
  const uint8_t *dc = static_cast<uint8_t *>(f->img_c.p), *dm = static_cast<uint8_t *>(f->img_m.p);
  memcpy(pf, front, B * fb_);
  memcpy(pb, bird, B * bb);
  if (contour) memcpy(pc, contour, B * bb);
  if (mask) memcpy(pm, mask, B * bb);
  FB_HIP(hipMemcpyAsync(f->img_f.p, pf, B * fb_, hipMemcpyHostToDevice, s));
  FB_HIP(hipMemcpyAsync(f->img_b.p, pb, B * bb, hipMemcpyHostToDevice, s));
  if (contour) FB_HIP(hipMemcpyAsync(f->img_c.p, pc, B * bb, hipMemcpyHostToDevice, s));
  if (mask) FB_HIP(hipMemcpyAsync(f->img_m.p, pm, B * bb, hipMemcpyHostToDevice, s));
  FB_HIP(hipEventRecord(f->evCopy, s));
  return fb_frame_extract_dev(f, of, ob, df, front_stride, fb_, db, bird_stride, bb, contour ? dc : nullptr, mask ? dm : nullptr, stream);
}

int fb_frame_set_bird_subpix(fb_frame *f, int32_t half_win, int32_t max_iter, double eps) {
  FB_ARG(f && half_win >= 0 && half_win <= 8);
  if (half_win > 0) FB_ARG(max_iter >= 1 && max_iter <= 100 && eps >= 0.0);  // what fb_corner_subpix_dev accepts
  f->subpixHalf = half_win;
  if (half_win > 0) { f->subpixIters = max_iter; f->subpixEps = eps; }
  return FB_OK;
}

int fb_frame_set_bird_redescribe(fb_frame *f, int32_t on) {
  FB_ARG(f);
  if (on && !f->describeStatus.p) {
    FB_TRY(fb::check_device());
    FB_TRY(f->describeStatus.alloc(plan_redescribe_status(f->P, f->cap), true));
  }
  f->redescribe = on != 0;
  return FB_OK;
}

int fb_frame_set_bird_detector(fb_frame *f, int32_t mode, int32_t fast_threshold) {
  FB_ARG(f && (mode == FB_BIRD_DETECT_ORBEXTRACTOR || mode == FB_BIRD_DETECT_CVORB));
  if (mode == FB_BIRD_DETECT_CVORB) {
    FB_ARG(fast_threshold >= 1 && fast_threshold <= 255);
    if (!f->describeStatus.p) {
      FB_TRY(fb::check_device());
      FB_TRY(f->describeStatus.alloc(plan_redescribe_status(f->P, f->cap), true));
    }
    f->detectThr = fast_threshold;
  }
  f->detectMode = mode;
  return FB_OK;
}

int fb_frame_download_bird_describe_status(fb_frame *f, uint8_t *host_status, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && host_status);
  if (!f->redescribed) { fb::set_error("fb_frame_download_bird_describe_status: the frame's last extraction did not re-describe"); return FB_ERR_ARG; }
  hipStream_t s = fb::as_stream(stream);
  FB_HIP(hipMemcpyAsync(host_status, f->describeStatus.p, plan_redescribe_status(f->P, f->cap), hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  return FB_OK;
}

int fb_frame_download_bird_grid(fb_frame *f, int32_t *host_cell_start, int32_t *host_cell_items, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && host_cell_start && host_cell_items);
  hipStream_t s = fb::as_stream(stream);
  FB_HIP(hipMemcpyAsync(host_cell_start, f->bcs, f->plan.r[FR_bcs].bytes, hipMemcpyDeviceToHost, s));
  FB_HIP(hipMemcpyAsync(host_cell_items, f->bci, f->plan.r[FR_bci].bytes, hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  return FB_OK;
}

int fb_frame_set_pose_dev(fb_frame *f, const float *d_Tcw, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && d_Tcw);
  FB_HIP(hipMemcpyAsync(f->F.Tcw, d_Tcw, f->plan.r[FR_Tcw].bytes, hipMemcpyDeviceToDevice, fb::as_stream(stream)));
  return FB_OK;
}

int fb_frame_predict_pose_dev(fb_frame *cur, const fb_frame *last, const float *d_delta, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && last && d_delta && cur != last && cur->B == last->B);
  fb::ProfScope prof_(fb::P_TRACK_GLUE, fb::as_stream(stream));
  k_predict_pose<<<(cur->B + 63) / 64, 64, 0, fb::as_stream(stream)>>>(d_delta, last->F.Tcw, cur->F.Tcw, cur->B);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_frame_clear_map_points_dev(fb_frame *f, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f);
  k_clear_mp<<<slot_grid(f), TT, 0, fb::as_stream(stream)>>>(f->F);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_frame_set_map_points_dev(fb_frame *f, const int32_t *d_mp, const int32_t *d_mpb, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && (d_mp || d_mpb));
  k_set_map_points<<<slot_grid(f), TT, 0, fb::as_stream(stream)>>>(f->F, d_mp, d_mpb);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_frame_bird_mappoint_match_dev(fb_frame *cur, const fb_map_points_bird *mpb, const int32_t *d_local, const int32_t *d_n_local,
                                     int window_size, float filter_size, const fb_matcher_params *matcher, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && bird_ok(mpb) && matcher && (!d_local || d_n_local));
  FB_ARG(d_local || mpb->stride <= cur->P.local_mpb_cap);
  hipStream_t s = fb::as_stream(stream);
  FB_TRY(m9_impl(cur, mpb, d_local, d_n_local, window_size, filter_size, matcher, s));
  return launch_commit(cur, commit_m9(cur, d_local), s);
}

int fb_frame_search_by_projection_dev(fb_frame *cur, const fb_frame *last, const fb_map_points *map, float th,
                                      const fb_matcher_params *matcher, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && last && cur != last && cur->B == last->B && cur->cap == last->cap && map_ok(cur, map) && matcher);
  hipStream_t s = fb::as_stream(stream);
  FB_TRY(m3_impl(cur, last, map, th, matcher, s));
  Commit C;
  memset(&C, 0, sizeof(C));
  C.kind = 1; C.match = cur->m_front; C.src_mp = last->F.mp; C.src_stride = cur->cap;
  return launch_commit(cur, C, s);
}

int fb_frame_pose_optimization_dev(fb_frame *f, const fb_map_points *map, const fb_map_points_bird *mpb, int mode, float wB,
                                   float wF, int which, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && map_ok(f, map) && bird_ok(mpb));
  Commit C;
  memset(&C, 0, sizeof(C));
  return edges_and_pose(f, map, mpb, mode, wB, wF, which, C, fb::as_stream(stream));
}

int fb_frame_discard_outliers_dev(fb_frame *f, const fb_map_points *map, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && map_ok(f, map));
  return discard_impl(f, map, FB_CNT_PROJ_MATCHES, 0, fb::as_stream(stream));
}

int fb_frame_match_bird_points_dev(fb_frame *cur, fb_frame *ref, fb_map_points_bird *mpb, int window_size, float filter_size,
                                   const fb_matcher_params *matcher, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && ref && cur != ref && cur->B == ref->B && cur->cap == ref->cap && bird_ok(mpb) && matcher);
  return bird_points_impl(cur, ref, mpb, window_size, filter_size, matcher, 0, fb::as_stream(stream));
}

int fb_frame_search_local_points_dev(fb_frame *f, const fb_map_points *map, const int32_t *d_local, const int32_t *d_n_local,
                                     float th, const fb_matcher_params *matcher, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && map_ok(f, map) && matcher && (!d_local || d_n_local));
  FB_ARG(d_local || map->stride <= f->P.local_mp_cap);
  hipStream_t s = fb::as_stream(stream);
  FB_TRY(local_impl(f, map, d_local, d_n_local, th, matcher, s));
  Commit C;
  memset(&C, 0, sizeof(C));
  C.kind = 2; C.match = f->m_local; C.src_mp = d_local; C.src_stride = f->P.local_mp_cap;
  return launch_commit(f, C, s);
}

int fb_frame_finish_dev(fb_frame *f, const fb_map_points *map, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && map_ok(f, map));
  return finish_impl(f, map, nullptr, 0, 0, fb::as_stream(stream));
}

int fb_frame_drop_outliers_dev(fb_frame *f, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f);
  fb::ProfScope prof_(fb::P_TRACK_GLUE, fb::as_stream(stream));
  k_drop_outliers<<<f->B, WG, 0, fb::as_stream(stream)>>>(f->F, f->counts, f->B, f->minInliers);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_frame_track_motion_model_dev(fb_frame *cur, fb_frame *last, const fb_track_args *T, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && last && cur != last && cur->B == last->B && cur->cap == last->cap && track_args_ok(cur, T) && T->d_delta);
  return motion_model_impl(cur, last, T, fb::as_stream(stream));
}

int fb_frame_track_local_map_dev(fb_frame *cur, fb_frame *ref, const fb_track_args *T, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && ref && cur != ref && cur->B == ref->B && cur->cap == ref->cap && track_args_ok(cur, T));
  return local_map_impl(cur, ref, T, fb::as_stream(stream), T->gate_local_map != 0);
}

int fb_frame_track_dev(fb_frame *cur, fb_frame *last, const fb_track_args *T, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && last && cur != last && cur->B == last->B && cur->cap == last->cap && track_args_ok(cur, T) && T->d_delta);
  FB_TRY(motion_model_impl(cur, last, T, fb::as_stream(stream)));
  return local_map_impl(cur, last, T, fb::as_stream(stream), true);   // if (bOK) bOK = TrackLocalMap(), per sequence
}

// Tracking::UpdateLocalMap (Tracking.cc:1394) on the frame's own mvpMapPoints
static fb_local_map_args frame_local_map_args(const fb_frame *cur, const fb_local_map_args *a) {
  fb_local_map_args A = *a;
  A.batch = cur->B; A.kp_stride = cur->cap; A.d_n = cur->F.n; A.d_map_point = cur->F.mp;
  A.cap_mp = cur->P.local_mp_cap;
  return A;
}

int fb_frame_update_local_map_dev(fb_frame *cur, fb_covis *g, const fb_covis_map *map, const fb_local_map_args *a, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && g && map && a);
  const fb_local_map_args A = frame_local_map_args(cur, a);
  return fb_covis_local_map_dev(g, map, &A, stream);
}

int fb_frame_track_graph_dev(fb_frame *cur, fb_frame *last, const fb_track_args *T, fb_covis *g, const fb_covis_map *map,
                             const fb_local_map_args *a, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && last && cur != last && cur->B == last->B && cur->cap == last->cap && track_args_ok(cur, T) && T->d_delta);
  FB_ARG(g && map && a && a->d_local_mp && T->d_local_mp == a->d_local_mp && T->d_n_local_mp == a->d_n_local_mp);
  fb_local_map_args A = frame_local_map_args(cur, a);
  A.d_gate_row = cur->cnt(FB_CNT_MATCHES_MAP); A.gate_min = 10;       // if (bOK) bOK = TrackLocalMap(), per sequence
  FB_TRY(motion_model_impl(cur, last, T, fb::as_stream(stream)));
  FB_TRY(fb_covis_local_map_dev(g, map, &A, stream));
  return local_map_impl(cur, last, T, fb::as_stream(stream), true);
}

// a frame's BoW arrays as the transform's argument block (levelsup = 4, Frame.cc:633)
static void bow_args(const fb_frame *f, fb_bow_transform_args *A) {
  memset(A, 0, sizeof(*A));
  A->batch = f->B; A->f_stride = f->cap; A->n_f = f->F.n; A->desc = f->F.desc; A->levelsup = 4;
  A->n_words = f->bw.nw; A->bow_ids = f->bw.ids; A->bow_vals = f->bw.vals;
  A->fv_n_nodes = f->bw.fv_nn; A->fv_node_ids = f->bw.fv_ids; A->fv_node_start = f->bw.fv_start; A->fv_items = f->bw.fv_items;
}

int fb_frame_compute_bow_dev(fb_frame *f, const fb_vocabulary *voc, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && voc);
  if (f->bowDone) return FB_OK;  // if (mBowVec.empty()), Frame.cc:630
  FB_TRY(f->ensure_bow());
  fb_bow_transform_args A;
  bow_args(f, &A);
  FB_TRY(fb_bow_transform_dev(voc, &A, stream));
  f->bowDone = true;
  return FB_OK;
}

int fb_frame_track_using_bird_dev(fb_frame *cur, fb_frame *src, fb_frame *ref, const fb_track_args *T, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && src && ref && cur != src && cur != ref && cur->B == src->B && cur->cap == src->cap && cur->B == ref->B && cur->cap == ref->cap);
  FB_ARG(track_args_ok(cur, T) && T->d_delta);
  hipStream_t s = fb::as_stream(stream);
  fb_map_points_bird mpb = T->mpb;
  FB_TRY(fb_frame_predict_pose_dev(cur, src, T->d_delta, s));                                          // :2016-2034
  FB_TRY(m9_impl(cur, &mpb, T->d_local_mpb, T->d_n_local_mpb, 10, 0.05f, &M09, s));                    // :2036
  FB_TRY(launch_commit(cur, commit_m9(cur, T->d_local_mpb), s));
  FB_TRY(bird_points_impl(cur, ref, &mpb, 10, 0.05f, &M09, 11, s));                                    // :2038-2053: only where numPt <= 10
  Commit C;
  memset(&C, 0, sizeof(C));
  C.no_front = 1;
  FB_TRY(edges_and_pose(cur, &T->map, &mpb, FB_POSE_BIRD, 1.0f, 1.0f, 0, C, s));                       // BirdOptimization(&mCurrentFrame, 1.0)
  return bird_points_impl(cur, ref, &mpb, 10, 0.05f, &M09, 0, s);                                      // :2056
}

// KeyFrame(Frame&): the members arena, and the BoW arena when the source has computed it.  (The member layout follows from
// batch, capacity and map_cap alone, so the two plans agree; the padding between regions travels along.)
int fb_frame_copy_dev(fb_frame *dst, const fb_frame *src, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(dst && src && dst != src && dst->B == src->B && dst->cap == src->cap && dst->P.map_cap == src->P.map_cap);
  hipStream_t s = fb::as_stream(stream);
  if (src->bowDone) FB_TRY(dst->ensure_bow());
  FB_HIP(hipMemcpyAsync(dst->arena[FA_MEMBERS].p, src->arena[FA_MEMBERS].p, src->plan.arena_bytes[FA_MEMBERS], hipMemcpyDeviceToDevice, s));
  if (src->bowDone) FB_HIP(hipMemcpyAsync(dst->arena[FA_BOW].p, src->arena[FA_BOW].p, src->plan.arena_bytes[FA_BOW], hipMemcpyDeviceToDevice, s));
  dst->bowDone = src->bowDone;
  return FB_OK;
}

int fb_frame_bow_view_dev(fb_frame *f, fb_bow_transform_args *v) {
  FB_ARG(f && v && f->bowDone);
  bow_args(f, v);
  return FB_OK;
}

int fb_frame_search_by_bow_dev(fb_frame *cur, const fb_frame *kf, const fb_map_points *map, const fb_matcher_params *matcher,
                               int min_matches, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && kf && cur != kf && cur->B == kf->B && cur->cap == kf->cap && map_ok(cur, map) && matcher && min_matches >= 0);
  if (!cur->bowDone || !kf->bowDone) { fb::set_error("fb_frame_search_by_bow: ComputeBoW has not run on both frames"); return FB_ERR_ARG; }
  hipStream_t s = fb::as_stream(stream);
  FB_TRY(bow_impl(cur, kf, map, matcher, s));
  return launch_commit(cur, commit_bow(cur, kf, min_matches), s);
}

int fb_frame_track_reference_dev(fb_frame *cur, fb_frame *kf, fb_frame *ref, const fb_vocabulary *voc, const fb_track_args *T,
                                 void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(cur && kf && ref && voc && cur != kf && cur != ref && cur->B == kf->B && cur->cap == kf->cap && cur->B == ref->B && cur->cap == ref->cap);
  FB_ARG(track_args_ok(cur, T) && T->d_delta);
  if (!kf->bowDone) { fb::set_error("fb_frame_track_reference: the key frame's BoW is not computed (KeyFrame::ComputeBoW)"); return FB_ERR_ARG; }
  hipStream_t s = fb::as_stream(stream);
  fb_map_points_bird mpb = T->mpb;
  FB_TRY(fb_frame_predict_pose_dev(cur, kf, T->d_delta, s));                                           // :1185-1186
  FB_TRY(m9_impl(cur, &mpb, T->d_local_mpb, T->d_n_local_mpb, 10, 0.05f, &M09, s));                    // :1193-1194
  FB_TRY(launch_commit(cur, commit_m9(cur, T->d_local_mpb), s));
  FB_TRY(bird_points_impl(cur, ref, &mpb, 10, 0.05f, &M09, 10, s));                                    // :1196-1200
  FB_TRY(fb_frame_compute_bow_dev(cur, voc, s));                                                       // :1203
  FB_TRY(bow_impl(cur, kf, &T->map, &M07, s));                                                         // :1207-1210
  FB_TRY(edges_and_pose(cur, &T->map, &mpb, FB_POSE_FRONT_BIRD, T->wB, T->wF, 0, commit_bow(cur, kf, 15), s));  // :1212-1220
  return discard_impl(cur, &T->map, FB_CNT_BOW_MATCHES, 15, s);                                        // :1222-1241
}

int fb_frame_view_dev(fb_frame *f, fb_frame_view *v) {
  FB_ARG(f && v);
  const FrameDev &F = f->F;
  v->batch = f->B; v->kp_stride = f->cap;
  v->n = F.n; v->kps = F.kps; v->kps_un = F.kps_un; v->desc = F.desc; v->map_point = F.mp; v->outlier = F.outlier;
  v->n_bird = F.nb; v->kps_bird = F.bkps; v->desc_bird = F.bdesc; v->bird_cam_xyz = F.bcam; v->map_point_bird = F.mpb;
  v->bird_outlier = F.boutlier;
  v->Tcw = F.Tcw; v->counts = f->counts;
  return FB_OK;
}

int fb_frame_download(fb_frame *f, const fb_frame_view *h, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && h);
  hipStream_t s = fb::as_stream(stream);
  const struct { void *dst; int region; } rows[] = {
      {h->n, FR_n}, {h->kps, FR_kps}, {h->kps_un, FR_kps_un}, {h->desc, FR_desc}, {h->map_point, FR_mp}, {h->outlier, FR_outlier},
      {h->n_bird, FR_nb}, {h->kps_bird, FR_bkps}, {h->desc_bird, FR_bdesc}, {h->bird_cam_xyz, FR_bcam}, {h->map_point_bird, FR_mpb},
      {h->bird_outlier, FR_boutlier}, {h->Tcw, FR_Tcw}, {h->counts, FR_counts}};
  for (const auto &w : rows)
    if (w.dst) FB_HIP(hipMemcpyAsync(w.dst, f->at<void>(w.region), f->plan.r[w.region].bytes, hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  return FB_OK;
}

int fb_frame_counts(fb_frame *f, int32_t *host_counts, float *host_Tcw, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(f && host_counts);
  hipStream_t s = fb::as_stream(stream);
  const size_t B = f->B, nc = B * FB_CNT_COUNT;
  FB_HIP(hipMemcpyAsync(f->pinCounts, f->counts, nc * 4, hipMemcpyDeviceToHost, s));
  if (host_Tcw) FB_HIP(hipMemcpyAsync(f->pinCounts + nc, f->F.Tcw, B * 48, hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  memcpy(host_counts, f->pinCounts, nc * 4);
  if (host_Tcw) memcpy(host_Tcw, f->pinCounts + nc, B * 48);
  return FB_OK;
}

}  // extern "C"
