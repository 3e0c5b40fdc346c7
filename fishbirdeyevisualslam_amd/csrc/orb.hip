// orb.hip -- ORBextractor as CDNA4 kernels (gfx950), batched over equally sized images.
//
// Replaces (reference file:line):
//   ORBextractor::ORBextractor        src/ORBextractor.cc:410-470   (host tables)
//   ORBextractor::ComputePyramid      :1107-1132   -> k_resize (one launch per level >= 1)
//   ComputeKeyPointsOctTree cell loop :765-832     -> k_fast   (one wave per run of 30-px cells,
//        cv::FAST 9-16 score + 3x3 NMS + ini/min threshold fallback on an LDS tile)
//   DistributeOctTree / DivideNode    :481-763     -> k_octree (one workgroup per image level)
//   GaussianBlur :1086                              -> k_blur   (whole level, separable 7x7, dot4)
//   IC_Angle / computeOrbDescriptor   :77-147      -> k_describe (one wave per two key points: raw and
//        blurred patches staged in LDS -> moments, 256 rBRIEF tests)
//   ORBextractor::operator()          :1043-1105   -> fb_orb_extract*
//   computeDescriptors on a caller's key points (cv::ORB::compute)   -> k_describe_at (one wave per key point, the level
//        from its record) -> fb_orb_describe*
//   cv::ORB::detect (OpenCV 3 orb.cpp computeKeyPoints: FAST, Harris, retainBest, IC_Angle)   -> k_det_fast, k_det_select,
//        k_det_emit on the same raw pyramid -> fb_orb_detect*
//
// HBM layout per image: level 0 is the caller's image (never copied); levels 1..n-1 live in
// one pitched buffer (pitch % 64 == 0), the blurred levels in a second one of the same geometry.
// FAST candidates are packed x | y<<12 | score<<24 into per-cell runs of a per-level array sized
// for the NMS worst case, so no kernel can overflow a buffer.
//
// OpenCV semantics (not vendored in the reference -> "parity unpinned") are
// those of oracle/orb_oracle.cpp; this file must agree with it bit for bit.
#include <climits>

#include "fb_common.h"
#include "fb_fast_score.h"
#include "fb_primitives.h"

#include "orb_plan.h"
#include "orb_describe_at_plan.h"
#include "orb_detect_plan.h"

namespace {

// The 256 tests are stored one dword each: x0 | y0 << 8 | x1 << 16 | y1 << 24, every coordinate biased by PAT_BIAS into a
// byte.  k_describe unpacks them with v_cvt_f32_ubyte0..3 and subtracts the bias, which is exact in float: the rotation
// sees the same values as with a float table, and a lane fetches 16 B of pattern instead of 64 B.
constexpr int PATTERN_XY[1024] = {
#include "orb_pattern.inc"
};
constexpr int pattern_extreme(bool wantMax) {
  int m = PATTERN_XY[0];
  for (int i = 1; i < 1024; i++) m = wantMax ? (PATTERN_XY[i] > m ? PATTERN_XY[i] : m) : (PATTERN_XY[i] < m ? PATTERN_XY[i] : m);
  return m;
}
constexpr int PAT_BIAS = -pattern_extreme(false);
static_assert(PAT_BIAS >= 0 && pattern_extreme(true) + PAT_BIAS <= 255, "a pattern coordinate does not fit a biased byte");
struct PackedPattern { uint32_t test[256]; };
constexpr PackedPattern pack_pattern() {
  PackedPattern p{};
  for (int t = 0; t < 256; t++)
    for (int k = 0; k < 4; k++) p.test[t] |= (uint32_t)(PATTERN_XY[t * 4 + k] + PAT_BIAS) << (8 * k);
  return p;
}
__constant__ PackedPattern c_pattern = pack_pattern();

}  // namespace

// the kernels, in pipeline order
#include "orb_pyramid.inc"
#include "orb_fast.inc"
#include "orb_octree.inc"
#include "orb_describe.inc"
#include "orb_describe_at.inc"
#include "orb_detect.inc"

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
namespace {

// Everything that is valid for one (w, h, batchCap): prepare() builds a new one beside the handle's and moves it in whole.
struct Workspace {
  int w = 0, h = 0, batchCap = 0;
  OrbK K = {};
  int maxNodes = 0;
  size_t octreeLds = 0;
  bool rowsOK[FB_MAX_LEVELS] = {}, mergeOK[FB_MAX_LEVELS] = {};  // see resize_rows_ok / resize_merge_ok
  ResizeTabs rt[FB_MAX_LEVELS] = {};
  fb::DevBuf pyr, blur, cand, cellCand, cellCount, nodeOf, counts, lvlOut, tabs, angTab, timers;
};

// What fb_orb_detect adds for one (w, h, batchCap), built by its first call at that size (orb_detect_plan.h)
struct DetectWs {
  int w = 0, h = 0, batchCap = 0, maskCap = 0;  // maskCap: mask pyramids `maskpyr` holds
  DetK K = {};
  fb::DevBuf map, hist, pos, resp, cnt, maskpyr;
};

}  // namespace

struct fb_orb {
  fb_orb_params p;
  fb_orb_tables t;
  // FB_ORB_SIDE_MIN: k_blur on a stream of its own (see BlurSchedule); created on first use
  hipStream_t sideStream = nullptr;
  hipEvent_t evFork = nullptr, evJoin = nullptr;
  hipEvent_t evLevel[FB_MAX_LEVELS] = {};  // evLevel[l]: the resize that writes level l has been enqueued on the caller's stream
  ~fb_orb() {
    if (evFork) (void)hipEventDestroy(evFork);
    if (evJoin) (void)hipEventDestroy(evJoin);
    for (hipEvent_t e : evLevel)
      if (e) (void)hipEventDestroy(e);
    if (sideStream) (void)hipStreamDestroy(sideStream);
  }
  int kpStride = 0;  // fb_orb_set_output_stride (0 = the capacity)
  Workspace ws;
  DetectWs det;
  // last call (for fb_orb_get_level and fb_orb_describe)
  int lastBatch = 0;
  const uint8_t *lastImg = nullptr;
  long long lastImgStride = 0;
  int lastPitch0 = 0;
  int lastRoute[FB_MAX_LEVELS] = {};  // the resize kernel that built level l >= 1: 0 k_resize, 1 k_resize_rows, 2 k_resize_merge
  fb::DevBuf ownedImg;
};

namespace {

// one call of fb_orb_extract_batch_dev
struct OrbCall {
  const uint8_t *img;   // level 0: the caller's images
  long long imgStride;
  int pitch0, batch;
  hipStream_t s;        // the caller's stream
};

// level l >= 1 from level l - 1
void launch_resize(fb_orb *o, int l, const OrbCall &c) {
  const Workspace &ws = o->ws;
  const OrbK &K = ws.K;
  const LevelInfo &D = K.L[l], &S = K.L[l - 1];
  const uint8_t *src = (l == 1) ? c.img : ws.pyr.as<uint8_t>() + S.off;
  const long long sstr = (l == 1) ? c.imgStride : K.pyrStride;
  const int spitch = (l == 1) ? c.pitch0 : S.pitch;
  uint8_t *dst = ws.pyr.as<uint8_t>() + D.off;
  const dim3 blk(64, 4);
  auto grid = [&](int rowsPerThread) { return dim3((D.pitch / 4 + 63) / 64, (D.h + 4 * rowsPerThread - 1) / (4 * rowsPerThread), c.batch); };
  fb::ProfScope prof_(fb::P_RESIZE, c.s);
  const bool rows = ws.rowsOK[l] && spitch >= 12 && ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)spitch | (uintptr_t)sstr) & 3) == 0;
  o->lastRoute[l] = rows ? (ws.mergeOK[l] ? 2 : 1) : 0;  // fb_orb_debug_resize_route
  if (rows && ws.mergeOK[l])
    k_resize_merge<<<grid(RM_ROWS), blk, 0, c.s>>>(src, sstr, S.w, S.h, spitch, dst, K.pyrStride, D.w, D.h, D.pitch, ws.rt[l]);
  else if (rows)
    k_resize_rows<<<grid(RESIZE_ROWS), blk, 0, c.s>>>(src, sstr, S.w, S.h, spitch, dst, K.pyrStride, D.w, D.h, D.pitch, ws.rt[l]);
  else
    k_resize<<<grid(1), blk, 0, c.s>>>(src, sstr, S.w, S.h, spitch, dst, K.pyrStride, D.w, D.h, D.pitch, ws.rt[l]);
}

// the Gaussian blur of the levels [l0, l1) on stream st
void launch_blur(fb_orb *o, const OrbCall &c, int l0, int l1, hipStream_t st) {
#ifndef FB_ORB_ABLATE_BLUR  // probe build only (profiles/probes/ablate_blur.sh): what the step costs without the blur launch (results are then wrong)
  const OrbK &K = o->ws.K;
  const int strips = K.blurStrips[l1] - K.blurStrips[l0];
  if (strips <= 0) return;  // levels too small to hold a key point
  fb::ProfScope prof_(fb::P_BLUR, st);
  k_blur<<<dim3((strips + 3) / 4, c.batch), 256, 0, st>>>(K, l0, l1, c.img, c.imgStride, c.pitch0, o->ws.pyr.as<uint8_t>(), o->ws.blur.as<uint8_t>());
#endif
}

// When and where the Gaussian blur of a call runs.  It needs only the raw levels, so it is launched right behind the last
// resize, before k_fast.  By default it stays on the caller's stream at every batch size: in the B = 256 step (front, bird and
// pose streams side by side) a fork to a side stream costs more than the overlap returns, wherever the fork is placed and
// however the levels are grouped (profiles/blur_schedule_ab.json).  The fork is still there for a caller whose extractor has
// the GPU to itself (one stream: the blur then runs beside k_fast and the quadtree): FB_ORB_SIDE_MIN = smallest batch that
// forks (default: never), and a set bit l of FB_ORB_BLUR_CUTS starts a new group of levels at level l, each group launched
// behind the resize of its last level (default 0: one launch over [0, nlevels)).
struct BlurSchedule {
  fb_orb *o;
  const OrbCall &c;
  bool fork;
  unsigned cuts;
  hipStream_t sBlur;
  int blurFrom = 0;  // first level that no launch covers yet

  BlurSchedule(fb_orb *o_, const OrbCall &c_) : o(o_), c(c_), sBlur(c_.s) {
    static const int sideMin = [] {
      const char *e = getenv("FB_ORB_SIDE_MIN");
      return e ? atoi(e) : INT_MAX;
    }();
    static const unsigned cutsEnv = [] {
      const char *e = getenv("FB_ORB_BLUR_CUTS");
      return e ? (unsigned)strtoul(e, nullptr, 0) : 0u;
    }();
    // (c) when every kernel is bracketed for the per-kernel table (fb_prof_enable without fb_prof_only) everything stays on
    //     the caller's stream and the blur is ONE launch over [0, nlevels), so that the table shows each kernel on its own
    const bool profAll = fb::g_prof_on && fb::g_prof_only < 0;
    fork = c.batch >= sideMin && !profAll;
    cuts = profAll ? 0u : cutsEnv;
  }

  int begin(hipStream_t s) {
    if (!fork) return FB_OK;
    if (!o->sideStream) {
      if (!o->evFork) FB_HIP(hipEventCreateWithFlags(&o->evFork, hipEventDisableTiming));
      if (!o->evJoin) FB_HIP(hipEventCreateWithFlags(&o->evJoin, hipEventDisableTiming));
      for (int l = 1; l < FB_MAX_LEVELS; l++)
        if (!o->evLevel[l]) FB_HIP(hipEventCreateWithFlags(&o->evLevel[l], hipEventDisableTiming));
      FB_HIP(hipStreamCreateWithFlags(&o->sideStream, hipStreamNonBlocking));
    }
    sBlur = o->sideStream;
    // (a) the blur of this call writes ws.blur, which k_describe of the previous call on this handle may still read: evFork is
    //     recorded on `s` behind that k_describe, and every launch on the side stream waits for evFork or for a later event
    //     of `s` (evLevel, below)
    FB_HIP(hipEventRecord(o->evFork, s));
    FB_HIP(hipStreamWaitEvent(sBlur, o->evFork, 0));
    return FB_OK;
  }

  // level l (its resize, for l >= 1) has just been enqueued on the caller's stream: launches the group that ends with it, if
  // one does
  int behind_level(int l) {
    const int nl = o->ws.K.nlevels;
    if (l + 1 < nl && !((cuts >> (l + 1)) & 1u)) return FB_OK;
    if (fork && l > 0) {
      FB_HIP(hipEventRecord(o->evLevel[l], c.s));
      FB_HIP(hipStreamWaitEvent(sBlur, o->evLevel[l], 0));
    }
    launch_blur(o, c, blurFrom, l + 1, sBlur);
    blurFrom = l + 1;
    if (fork && l + 1 == nl) FB_HIP(hipEventRecord(o->evJoin, sBlur));  // behind the last blur launch, for (b)
    return FB_OK;
  }

  // (b) the level-0 blur reads the caller's images: `s` waits for evJoin before k_describe (which needs the blurred levels
  //     complete anyway), so whatever the caller records on `s` after this call lies behind every read of the images
  int join_before_describe(hipStream_t s) {
    if (fork) FB_HIP(hipStreamWaitEvent(s, o->evJoin, 0));
    return FB_OK;
  }
};

template <int TP>
void launch_fast(fb_orb *o, const OrbCall &c) {
  const Workspace &ws = o->ws;
  const OrbK &K = ws.K;
  fb::ProfScope prof_(TP == 44 ? fb::P_FAST : TP == 56 ? fb::P_FAST56 : fb::P_FAST72, c.s);
  const dim3 grd((K.totalGroups + 7) / 8 * 8, c.batch);
  const size_t lds = (size_t)2 * K.fastTileBytes + 2 * K.fastMaxPix;
  const auto kern = K.dbg == 20 ? k_fast<TP, true> : k_fast<TP, false>;  // FB_FAST_DBG=20: the instantiation that times its phases
  kern<<<grd, 64, lds, c.s>>>(K, c.img, c.imgStride, c.pitch0, ws.pyr.as<uint8_t>(), ws.cellCand.as<uint32_t>(), ws.cellCount.as<int>());
}
void launch_fast(fb_orb *o, const OrbCall &c) {
  const OrbK &K = o->ws.K;
  if (K.totalCells == 0) return;
  if (K.fastTP == 44) launch_fast<44>(o, c);
  else if (K.fastTP == 56) launch_fast<56>(o, c);
  else launch_fast<FAST_MAX_TILE>(o, c);
}

template <int NT>
void launch_octree(fb_orb *o, const OrbCall &c) {
  const Workspace &ws = o->ws;
  int *candCount = ws.counts.as<int>(), *lvlCount = candCount + (size_t)ws.batchCap * ws.K.nlevels;
  fb::ProfScope prof_(fb::P_OCTREE, c.s);
  k_octree<NT><<<dim3(c.batch, ws.K.nlevels), NT, ws.octreeLds, c.s>>>(ws.K, ws.cellCand.as<uint32_t>(), ws.cellCount.as<int>(), ws.cand.as<uint32_t>(), candCount,
                                                                       ws.nodeOf.as<uint16_t>(), ws.lvlOut.as<uint32_t>(), lvlCount, ws.maxNodes);
}
void launch_octree(fb_orb *o, const OrbCall &c) {
  static const int octWideMax = getenv("FB_OCT_WIDE_MAX") ? atoi(getenv("FB_OCT_WIDE_MAX")) : 512;
  // few workgroups: 1024 threads each (two such workgroups fill a CU's wave slots)
  if (o->ws.K.nlevels * c.batch <= octWideMax) launch_octree<1024>(o, c);
  else launch_octree<256>(o, c);
}
// The dynamic LDS limit is an attribute of the kernel, not of a handle: it is raised to the most any plan can ask for, so that
// handles with different quadtree sizes do not lower it for each other.  (A template like the launcher, and below it: the
// kernels are then instantiated, and laid out in the code object, in pipeline order.)
template <int NT>
int allow_octree_lds() {
  FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_octree<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)OCTREE_LDS_MAX));
  return FB_OK;
}

void launch_describe(fb_orb *o, const OrbCall &c, fb_keypoint *d_keypoints, uint8_t *d_descriptors, int32_t *d_n) {
  const Workspace &ws = o->ws;
  const OrbK &K = ws.K;
  const int *lvlCount = ws.counts.as<int>() + (size_t)ws.batchCap * K.nlevels;
  fb::ProfScope prof_(fb::P_DESCRIBE, c.s);
  k_describe<<<dim3((K.descBase[K.nlevels] + 7) / 8 * 8, c.batch), 64 * DESC_WPB, 0, c.s>>>(K, c.img, c.imgStride, c.pitch0, ws.pyr.as<uint8_t>(), ws.blur.as<uint8_t>(),
                                                                                          ws.angTab.as<uint4>(), ws.lvlOut.as<uint32_t>(), lvlCount, d_keypoints,
                                                                                          d_descriptors, d_n);
}

// the buffers of plan P for `batch` images, the tables uploaded; on an error `ws` is simply dropped by the caller
int build_workspace(const OrbPlan &P, int batch, Workspace &ws) {
  ws.K = P.K;
  ws.K.dbg = getenv("FB_FAST_DBG") ? atoi(getenv("FB_FAST_DBG")) : 0;
  ws.maxNodes = P.maxNodes;
  ws.octreeLds = P.octreeLds;
  memcpy(ws.rowsOK, P.rowsOK, sizeof(ws.rowsOK));
  memcpy(ws.mergeOK, P.mergeOK, sizeof(ws.mergeOK));
  FB_TRY(ws.tabs.upload(P.tabBytes.data(), P.tabBytes.size()));
  for (int l = 1; l < P.K.nlevels; l++) {
    const uint8_t *base = ws.tabs.as<uint8_t>();
    ws.rt[l].xofs = reinterpret_cast<const int *>(base + P.tabOff[l][0]);
    ws.rt[l].ialpha = reinterpret_cast<const short *>(base + P.tabOff[l][1]);
    ws.rt[l].yofs = reinterpret_cast<const int *>(base + P.tabOff[l][2]);
    ws.rt[l].ibeta = reinterpret_cast<const short *>(base + P.tabOff[l][3]);
  }
  FB_TRY(ws.angTab.upload(P.angTab, sizeof(P.angTab)));
  const OrbSizes z = P.sizes(batch);
  FB_TRY(ws.pyr.alloc(z.pyr));
  FB_TRY(ws.blur.alloc(z.blur));
  FB_TRY(ws.cand.alloc(z.cand));
  FB_TRY(ws.cellCand.alloc(z.cellCand));
  FB_TRY(ws.cellCount.alloc(z.cellCount));
  FB_TRY(ws.nodeOf.alloc(z.nodeOf));
  FB_TRY(ws.counts.alloc(z.counts));
  FB_TRY(ws.timers.alloc(z.timers));
  FB_HIP(hipMemset(ws.timers.p, 0, z.timers));
  ws.K.timers = ws.timers.as<unsigned long long>();
  FB_TRY(ws.lvlOut.alloc(z.lvlOut));
  return FB_OK;
}

// (re)build the workspace for images of w x h, up to `batch` per call: plan, allocate (make_workspace), commit.  Until the
// commit nothing of the handle is written, so a refusal or a HIP error leaves it usable at its previous size.
bool workspace_fits(const fb_orb *o, int w, int h, int batch) { return o->ws.w == w && o->ws.h == h && batch <= o->ws.batchCap; }
int make_workspace(fb_orb *o, int w, int h, int batch, Workspace &ws) {
  OrbPlan P;
  FB_TRY(plan_orb(o->p, o->t, w, h, o->kpStride, P));
  FB_TRY(build_workspace(P, batch, ws));
  FB_TRY(allow_octree_lds<1024>());
  FB_TRY(allow_octree_lds<256>());
  ws.w = w; ws.h = h; ws.batchCap = batch;
  return FB_OK;
}
void commit_workspace(fb_orb *o, Workspace &ws) {
  o->ws = std::move(ws);  // the commit: moves of plain data and of buffer ownership, nothing that can fail
  o->lastBatch = 0;       // the new buffers hold no pyramid yet (fb_orb_describe)
}
int prepare(fb_orb *o, int w, int h, int batch) {
  if (workspace_fits(o, w, h, batch)) return FB_OK;
  Workspace ws;
  FB_TRY(make_workspace(o, w, h, batch, ws));
  commit_workspace(o, ws);
  return FB_OK;
}

// fb_orb_detect: the extractor's workspace AND the detector's buffers for images of w x h, up to `batch` per call and `masks`
// mask pyramids.  Both are planned and allocated before either is committed, so a refused call leaves the handle as it was.
int prepare_detect(fb_orb *o, int w, int h, int batch, int masks) {
  const bool needWs = !workspace_fits(o, w, h, batch);
  const bool needDet = !(o->det.w == w && o->det.h == h && batch <= o->det.batchCap && masks <= o->det.maskCap);
  Workspace ws;
  DetectWs d;
  if (needWs) FB_TRY(make_workspace(o, w, h, batch, ws));
  if (needDet) {
    OrbPlan P;
    FB_TRY(plan_orb(o->p, o->t, w, h, o->kpStride, P));
    DetPlan D;
    FB_TRY(plan_detect(P, o->t, D));
    d.K = D.K;
    // (never smaller than what the handle holds at this size: a call with fewer images or masks later fits again)
    const bool same = o->det.w == w && o->det.h == h;
    d.batchCap = same ? std::max(batch, o->det.batchCap) : batch;
    d.maskCap = same ? std::max(masks, o->det.maskCap) : masks;
    const DetSizes z = D.sizes(d.batchCap, d.maskCap);
    FB_TRY(d.map.alloc(z.map));
    FB_TRY(d.hist.alloc(z.hist));
    FB_TRY(d.pos.alloc(z.pos));
    FB_TRY(d.resp.alloc(z.resp));
    FB_TRY(d.cnt.alloc(z.cnt));
    FB_TRY(d.maskpyr.alloc(z.maskpyr));
    d.w = w; d.h = h;
  }
  if (needWs) commit_workspace(o, ws);
  if (needDet) o->det = std::move(d);
  return FB_OK;
}

// the mask pyramid(s) of one call: m_l = tozero_254(resize(m_{l-1})), with the image levels' own resize tables; `masks`
// pyramids, the caller's masks `maskImgStride` bytes apart
int launch_mask_pyramid(fb_orb *o, const fb_orb_detect_args *A, int masks, long long maskImgStride, hipStream_t s) {
  const Workspace &ws = o->ws;
  uint8_t *mp = o->det.maskpyr.as<uint8_t>();
  const long long mpStride = ws.K.pyrStride;
  for (int l = 1; l < ws.K.nlevels; l++) {
    const LevelInfo &D = ws.K.L[l], &S = ws.K.L[l - 1];
    const uint8_t *src = l == 1 ? A->mask : mp + S.off;
    const int spitch = l == 1 ? A->mask_stride : S.pitch;
    {
      fb::ProfScope prof_(fb::P_RESIZE, s);
      k_resize<<<dim3((D.pitch / 4 + 63) / 64, (D.h + 3) / 4, masks), dim3(64, 4), 0, s>>>(src, l == 1 ? maskImgStride : mpStride, S.w, S.h, spitch, mp + D.off, mpStride,
                                                                                         D.w, D.h, D.pitch, ws.rt[l]);
    }
    const int dwords = D.pitch / 4 * D.h;
    k_det_mask<<<dim3((dwords + 255) / 256, masks), 256, 0, s>>>(mp + D.off, mpStride, dwords);
  }
  FB_HIP(hipGetLastError());
  return FB_OK;
}

// fb_orb_describe[_dev]: the argument checks of orb_describe_at_plan.h against the handle's last extract call
int describe_check(const fb_orb *o, const fb_orb_describe_args *A, size_t *lds) {
  FB_ARG(o);
  return check_describe_at(A, o->lastBatch, o->ws.w, o->ws.h, "fb_orb_describe", lds);
}

}  // namespace

extern "C" {

int fb_orb_capacity(const fb_orb_params *params) {
  if (!params) return FB_ERR_ARG;
  return capacity_of(*params);
}

int fb_orb_set_output_stride(fb_orb *h, int kp_stride) {
  FB_ARG(h && (kp_stride == 0 || kp_stride >= capacity_of(h->p)));
  h->kpStride = kp_stride;
  h->ws.K.kpStride = kp_stride > 0 ? kp_stride : capacity_of(h->p);  // (the workspace itself does not depend on it)
  return FB_OK;
}

int fb_orb_create(const fb_orb_params *params, fb_orb **out) {
  FB_ARG(params && out);
  FB_ARG(params->nlevels >= 1 && params->nlevels <= FB_MAX_LEVELS);
  FB_ARG(params->nfeatures >= 1 && params->nfeatures <= 60000);
  FB_ARG(params->scale_factor > 1.0f);
  FB_ARG(params->min_th_fast >= 1 && params->ini_th_fast >= params->min_th_fast && params->ini_th_fast <= 254);
  fb_orb *o = new fb_orb();
  o->p = *params;
  make_tables(o->p, o->t);
  *out = o;
  return FB_OK;
}

void fb_orb_destroy(fb_orb *h) { delete h; }

int fb_orb_get_tables(const fb_orb *h, fb_orb_tables *out) {
  FB_ARG(h && out);
  *out = h->t;
  return FB_OK;
}

int fb_orb_extract_batch_dev(fb_orb *o, const uint8_t *d_images, int batch, int width, int height, int stride,
                             size_t image_stride, fb_keypoint *d_keypoints, uint8_t *d_descriptors, int32_t *d_n,
                             void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(o && d_images && d_keypoints && d_descriptors && d_n);
  FB_ARG(batch >= 1 && width >= 2 * EDGE_THRESHOLD + 7 && height >= 2 * EDGE_THRESHOLD + 7 && stride >= width);
  FB_TRY(prepare(o, width, height, batch));
  const OrbK &K = o->ws.K;
  const OrbCall c = {d_images, (long long)image_stride, stride, batch, fb::as_stream(stream)};
  BlurSchedule blur(o, c);
  FB_TRY(blur.begin(c.s));
  FB_HIP(hipMemsetAsync(o->ws.cellCount.p, 0, (size_t)batch * K.totalCells * 4, c.s));
  for (int l = 0; l < K.nlevels; l++) {  // pyramid, each group of levels blurred as soon as it is there
    if (l > 0) launch_resize(o, l, c);
    FB_TRY(blur.behind_level(l));
  }
  launch_fast(o, c);
  launch_octree(o, c);
  FB_TRY(blur.join_before_describe(c.s));
  launch_describe(o, c, d_keypoints, d_descriptors, d_n);
  FB_HIP(hipGetLastError());
  o->lastBatch = batch;
  o->lastImg = d_images;
  o->lastImgStride = (long long)image_stride;
  o->lastPitch0 = stride;
  return FB_OK;
}

int fb_orb_extract(fb_orb *o, const uint8_t *image, int width, int height, int stride, fb_keypoint *keypoints,
                   uint8_t *descriptors, int32_t *n_out) {
  FB_TRY(fb::check_device());
  FB_ARG(o && n_out);
  if (!image || width <= 0 || height <= 0) return FB_OK;  // _image.empty(): silent return, ORBextractor.cc:1046
  FB_ARG(keypoints && descriptors && stride >= width);
  const int cap = capacity_of(o->p);
  // one page-locked block per host thread carries the image in and [n | key points | descriptors | level counts] out: one
  // asynchronous copy each way and ONE synchronisation (five synchronous copies before)
  const size_t imgBytes = (size_t)stride * height, kpBytes = (size_t)cap * sizeof(fb_keypoint), dBytes = (size_t)cap * 32;
  const size_t oN = 0, oK = 256, oD = oK + ((kpBytes + 255) & ~(size_t)255), oC = oD + ((dBytes + 255) & ~(size_t)255), outBytes = oC + 256;
  const size_t imgArea = fb::Stager::up256(imgBytes);  // the output area starts 256-byte aligned (its level counts are ints)
  uint8_t *pin = static_cast<uint8_t *>(fb::pinned_scratch(imgArea + outBytes));
  if (!pin) return FB_ERR_HIP;
  fb::DevBuf dout;
  FB_TRY(dout.alloc(outBytes));
  if (o->ownedImg.bytes < imgBytes || !o->ownedImg.p) FB_TRY(o->ownedImg.alloc(imgBytes));
  memcpy(pin, image, imgBytes);
  // as ~Stager: on an error return after this point the copies and kernels may still use `pin` and `dout`
  struct SyncOnError {
    bool armed = true;
    ~SyncOnError() { if (armed) { (void)hipStreamSynchronize(nullptr); (void)hipGetLastError(); } }
  } guard;
  FB_HIP(hipMemcpyAsync(o->ownedImg.p, pin, imgBytes, hipMemcpyHostToDevice, nullptr));
  uint8_t *dbase = dout.as<uint8_t>();
  const int keepStride = o->kpStride;
  if (keepStride) FB_TRY(fb_orb_set_output_stride(o, 0));  // this call's arrays hold exactly `cap` entries
  const int rc = fb_orb_extract_batch_dev(o, o->ownedImg.as<uint8_t>(), 1, width, height, stride, imgBytes, reinterpret_cast<fb_keypoint *>(dbase + oK),
                                          dbase + oD, reinterpret_cast<int32_t *>(dbase + oN), nullptr);
  if (keepStride) (void)fb_orb_set_output_stride(o, keepStride);
  FB_TRY(rc);
  uint8_t *pout = pin + imgArea;
  FB_HIP(hipMemcpyAsync(pout, dbase, oC, hipMemcpyDeviceToHost, nullptr));
  FB_HIP(hipMemcpyAsync(pout + oC, o->ws.counts.as<int>() + (size_t)o->ws.batchCap * o->p.nlevels, (size_t)o->p.nlevels * 4, hipMemcpyDeviceToHost, nullptr));
  FB_HIP(hipStreamSynchronize(nullptr));
  guard.armed = false;
  memcpy(n_out, pout + oN, 4);
  {  // n_out is clamped to the capacity on the device; the per-level counts tell whether anything was cut off (the
     // quadtree can end a level with up to 4 x its number of root nodes: very wide strips with a tiny feature budget)
    const int *lc = reinterpret_cast<const int *>(pout + oC);
    int total = 0;
    for (int l = 0; l < o->p.nlevels; l++) total += lc[l];
    if (total > cap) {
      fb::set_error("keypoint capacity exceeded: the quadtree kept %d key points, fb_orb_capacity() is %d", total, cap);
      return FB_ERR_CAPACITY;
    }
  }
  memcpy(keypoints, pout + oK, (size_t)*n_out * sizeof(fb_keypoint));
  memcpy(descriptors, pout + oD, (size_t)*n_out * 32);
  return FB_OK;
}

// ---- computeDescriptors at key points the caller supplies (the rules are restated at fb_orb_describe_args) ----------------
int fb_orb_describe_dev(fb_orb *o, const fb_orb_describe_args *A, void *stream) {
  FB_TRY(fb::check_device());
  size_t lds = 0;
  FB_TRY(describe_check(o, A, &lds));
  if (A->batch == 0 || A->kp_stride == 0) return FB_OK;
  FB_ARG(((uintptr_t)A->kps | (uintptr_t)A->desc | (uintptr_t)A->n) % 4 == 0);
  const Workspace &ws = o->ws;
  DescAtK K;
  memset(&K, 0, sizeof(K));
  K.nlevels = ws.K.nlevels; K.kp_stride = A->kp_stride; K.angle_mode = A->angle_mode;
  K.pitch0 = A->stride; K.img_stride = (long long)A->image_stride; K.pyr_stride = ws.K.pyrStride; K.blur_stride = ws.K.blurStride;
  K.n = A->n; K.kps = A->kps; K.desc = A->desc; K.status = A->status;
  K.img0 = A->angle_mode == FB_DESCRIBE_IC_ANGLE ? A->images : nullptr;
  K.pyr = ws.pyr.as<uint8_t>(); K.blur = ws.blur.as<uint8_t>(); K.ang_tab = ws.angTab.p;
  for (int l = 0; l < K.nlevels; l++) {
    const LevelInfo &L = ws.K.L[l];
    K.L[l] = DescAtLevel{L.w, L.h, L.pitch, o->t.inv_scale_factor[l], L.off, L.boff};
  }
  hipStream_t s = fb::as_stream(stream);
  fb::ProfScope prof_(fb::P_DESCRIBE_AT, s);
  k_describe_at<<<dim3((A->kp_stride + DESCAT_WAVES - 1) / DESCAT_WAVES, A->batch), DESCAT_THREADS, lds, s>>>(K);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_orb_describe(fb_orb *o, const fb_orb_describe_args *H) {
  FB_TRY(fb::check_device());
  size_t lds = 0;
  FB_TRY(describe_check(o, H, &lds));
  if (H->batch == 0 || H->kp_stride == 0) return FB_OK;
  for (int b = 0; b < H->batch; b++) FB_ARG(H->n[b] >= 0 && H->n[b] <= H->kp_stride);
  fb_orb_describe_args D = *H;
  const DescAtStage z = describe_at_stage(*H, o->ws.h);
  fb::Stager st;
  if (z.images) st.in(D.images, z.images);
  else D.images = nullptr;
  st.in(D.n, z.n);
  // in/out: only .angle of an accepted key point is written (IC mode), and only the rows of accepted key points
  st.out(D.kps, z.kps, true);
  st.out(D.desc, z.desc, true);
  st.out(D.status, z.status, true);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_orb_describe_dev(o, &D, nullptr));
  return st.fetch(nullptr);
}

// ---- cv::ORB's detector on the handle's pyramid (the rules are restated at fb_orb_detect_args) ----------------------------
int fb_orb_detect_dev(fb_orb *o, const fb_orb_detect_args *A, void *stream) { return fb_orb_detect_masks_dev(o, A, 0, stream); }

int fb_orb_detect_masks_dev(fb_orb *o, const fb_orb_detect_args *A, size_t mask_image_stride, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(o);
  bool noop = false;
  FB_TRY(check_detect(A, mask_image_stride, "fb_orb_detect", &noop));
  if (noop) return FB_OK;
  FB_ARG(((uintptr_t)A->kps | (uintptr_t)A->n | (uintptr_t)A->n_true) % 4 == 0);
  const int masks = !A->mask ? 0 : mask_image_stride ? A->batch : 1;
  FB_TRY(prepare_detect(o, A->width, A->height, A->batch, std::max(masks, 1)));
  const Workspace &ws = o->ws;
  const OrbCall c = {A->images, (long long)A->image_stride, A->stride, A->batch, fb::as_stream(stream)};
  BlurSchedule blur(o, c);
  FB_TRY(blur.begin(c.s));
  FB_HIP(hipMemsetAsync(o->det.hist.p, 0, (size_t)A->batch * ws.K.nlevels * 256 * 4, c.s));
  for (int l = 0; l < ws.K.nlevels; l++) {  // the raw and the blurred pyramid, exactly as an extract call builds them
    if (l > 0) launch_resize(o, l, c);
    FB_TRY(blur.behind_level(l));
  }
  if (A->mask) FB_TRY(launch_mask_pyramid(o, A, masks, (long long)mask_image_stride, c.s));
  DetK K = o->det.K;
  K.thr = A->fast_threshold; K.pitch0 = A->stride; K.kp_stride = A->kp_stride; K.mask_pitch0 = A->mask_stride;
  K.img_stride = (long long)A->image_stride;
  K.mask_img_stride = (long long)mask_image_stride; K.maskpyr_stride = mask_image_stride ? ws.K.pyrStride : 0;
  K.img0 = A->images; K.pyr = ws.pyr.as<uint8_t>();
  K.mask0 = A->mask; K.maskpyr = o->det.maskpyr.as<uint8_t>();
  K.map = o->det.map.as<uint8_t>(); K.hist = o->det.hist.as<unsigned>(); K.pos = o->det.pos.as<uint32_t>();
  K.resp = o->det.resp.as<float>(); K.cnt = o->det.cnt.as<int32_t>(); K.ang_tab = ws.angTab.p;
  K.kps = A->kps; K.n = A->n; K.n_true = A->n_true;
  DetSelLds S;
  const size_t selLds = det_select_layout(S);
  if (K.tileBase[K.nlevels] > 0) {
    fb::ProfScope prof_(fb::P_DET_FAST, c.s);
    k_det_fast<<<dim3(K.tileBase[K.nlevels], A->batch), DET_FAST_THREADS, 0, c.s>>>(K);
  }
  {
    fb::ProfScope prof_(fb::P_DET_SELECT, c.s);
    k_det_select<<<dim3(K.nlevels, A->batch), DET_SEL_THREADS, selLds, c.s>>>(K);
  }
  FB_TRY(blur.join_before_describe(c.s));
  {
    fb::ProfScope prof_(fb::P_DET_EMIT, c.s);
    k_det_emit<<<dim3((A->kp_stride + DET_EMIT_WAVES - 1) / DET_EMIT_WAVES, A->batch), DET_EMIT_WAVES * 64, 0, c.s>>>(K);
  }
  FB_HIP(hipGetLastError());
  o->lastBatch = A->batch;  // the pyramids are this call's: fb_orb_describe and fb_orb_get_level work on them
  o->lastImg = A->images;
  o->lastImgStride = (long long)A->image_stride;
  o->lastPitch0 = A->stride;
  return FB_OK;
}

int fb_orb_detect(fb_orb *o, const fb_orb_detect_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(o);
  bool noop = false;
  FB_TRY(check_detect(H, 0, "fb_orb_detect", &noop));
  if (noop) return FB_OK;
  fb_orb_detect_args D = *H;
  const DetStage z = detect_stage(*H);
  fb::Stager st;
  st.in(D.images, z.images);
  st.in(D.mask, z.mask);
  st.out(D.kps, z.kps, true);  // in/out: the entries at or past n[b] keep the caller's contents
  st.out(D.n, z.n, false);
  st.out(D.n_true, z.n_true, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_orb_detect_dev(o, &D, nullptr));
  return st.fetch(nullptr);
}

int fb_orb_debug_timers(fb_orb *o, uint64_t *dst16) {
  FB_TRY(fb::check_device());
  FB_ARG(o && dst16 && o->ws.timers.p);
  FB_HIP(hipDeviceSynchronize());
  FB_HIP(hipMemcpy(dst16, o->ws.timers.p, 16 * 8, hipMemcpyDeviceToHost));
  FB_HIP(hipMemset(o->ws.timers.p, 0, 16 * 8));
  return FB_OK;
}

#ifdef FB_FAST_LISTHIST
// probe build only (profiles/probes/fast_list_lengths.py): dst128[0..63] = cells by length of the iniThFAST list,
// dst128[64..127] = redone cells by length of the minThFAST-only list; both in bins of 8, cleared by the call
extern "C" int fb_orb_debug_list_hist(fb_orb *o, uint64_t *dst128) {
  FB_TRY(fb::check_device());
  FB_ARG(o && dst128 && o->ws.timers.p);
  FB_HIP(hipDeviceSynchronize());
  FB_HIP(hipMemcpy(dst128, o->ws.timers.as<unsigned long long>() + 16, 128 * 8, hipMemcpyDeviceToHost));
  FB_HIP(hipMemset(o->ws.timers.as<unsigned long long>() + 16, 0, 128 * 8));
  return FB_OK;
}
#endif

int fb_orb_debug_candidates(fb_orb *o, int b, int level, uint32_t *dst, int cap) {
  FB_TRY(fb::check_device());
  FB_ARG(o && o->lastImg && level >= 0 && level < o->p.nlevels && b >= 0 && b < o->ws.batchCap);
  FB_HIP(hipDeviceSynchronize());
  int n = 0;
  FB_HIP(hipMemcpy(&n, o->ws.counts.as<int>() + (size_t)b * o->p.nlevels + level, 4, hipMemcpyDeviceToHost));
  const LevelInfo &L = o->ws.K.L[level];
  const int m = n < cap ? n : cap;
  if (dst && m > 0)
    FB_HIP(hipMemcpy(dst, o->ws.cand.as<uint32_t>() + (size_t)b * o->ws.K.candStride + L.candBase, (size_t)m * 4, hipMemcpyDeviceToHost));
  return n;
}

int fb_orb_debug_resize_route(fb_orb *o, int level) {
  FB_ARG(o && o->lastImg && level >= 1 && level < o->p.nlevels);
  return o->lastRoute[level];
}

int fb_orb_get_level(fb_orb *o, int b, int level, uint8_t *dst, int *w, int *hgt) {
  FB_TRY(fb::check_device());
  FB_ARG(o && w && hgt && o->lastImg && level >= 0 && level < o->p.nlevels && b >= 0 && b < o->ws.batchCap);
  const LevelInfo &L = o->ws.K.L[level];
  *w = L.w;
  *hgt = L.h;
  if (!dst) return FB_OK;
  FB_HIP(hipDeviceSynchronize());
  const uint8_t *src = level == 0 ? o->lastImg + (long long)b * o->lastImgStride
                                  : o->ws.pyr.as<uint8_t>() + (long long)b * o->ws.K.pyrStride + L.off;
  const int pitch = level == 0 ? o->lastPitch0 : L.pitch;
  FB_HIP(hipMemcpy2D(dst, L.w, src, pitch, L.w, L.h, hipMemcpyDeviceToHost));
  return FB_OK;
}

int fb_orb_get_blurred_level(fb_orb *o, int b, int level, uint8_t *dst) {
  FB_TRY(fb::check_device());
  FB_ARG(o && dst && o->lastImg && level >= 0 && level < o->p.nlevels && b >= 0 && b < o->ws.batchCap);
  const LevelInfo &L = o->ws.K.L[level];
  FB_HIP(hipDeviceSynchronize());
  const uint8_t *src = o->ws.blur.as<uint8_t>() + (long long)b * o->ws.K.blurStride + L.boff;
  FB_HIP(hipMemcpy2D(dst, L.w, src, L.pitch, L.w, L.h, hipMemcpyDeviceToHost));
  return FB_OK;
}

}  // extern "C"
