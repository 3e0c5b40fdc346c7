// orb_detect_plan.h -- what fb_orb_detect (cv::ORB's detector, orb_detect.inc) derives from the extractor's plan before it
// touches the GPU: the kernel argument block DetK, the tile grid of k_det_fast, the candidate workspace, the dynamic LDS of
// k_det_select, the argument checks of both entry points and the bytes the host entry point stages.  The rules themselves
// are restated at fb_orb_detect_args in fishbird.h.
//
// Workspace per image (beside the extractor's own, allocated by the first detect call at a size):
//   map    one byte per pixel of every level in the geometry of the blurred pyramid (LevelInfo::boff, pitch): the FAST score
//          of a pixel that survived the 3x3 suppression, the 31-px border and the mask, else 0.  The padding columns are 0.
//   hist   256 counters per level: the survivors by score (the first cut is read off it exactly)
//   pos / resp   the candidate lists of the levels, raster order: x | y << 12 | score << 24 and the Harris response.  A strict
//          3x3 maximum excludes its 8 neighbours, so a level holds at most ceil(w/2) * ceil(h/2) of them: det_cand_bound().
//   cnt    the key points each level ends with
// and the mask pyramid of the HANDLE (levels >= 1 in the geometry of the raw pyramid): one image's worth when the mask is
// shared by the batch, `batch` of them when every image has its own (fb_orb_detect_masks_dev).  It is rebuilt on every call
// that passes a mask: nothing is cached, so a caller may rewrite the mask between calls.  Like the pyramids it belongs to the
// handle, whose calls come from one caller at a time: two detect calls on two streams would race on it.
// k_det_fast writes every byte of the map rows of a live level on every call (a level's pitch is exactly its tiles' width),
// so the map needs no clearing.
//
// No HIP header: plain host/device code like orb_plan.h, on which it builds (tests/cpp/orb_detect_plan_test.cpp compiles both
// with g++).  Unnamed namespace: one translation unit at a time.
#ifndef FB_ORB_DETECT_PLAN_H_
#define FB_ORB_DETECT_PLAN_H_

#include "orb_plan.h"

namespace {

constexpr int DET_EDGE = 31;                    // cv::ORB edgeThreshold: a key point sits >= 31 px inside its level
constexpr int DET_HARRIS_R = 3;                 // HarrisResponses, blockSize 7: Sobel 3x3 at -3 .. +3 reads -4 .. +4
constexpr float DET_HARRIS_K = 0.04f;
constexpr float DET_S = 1.f / (4 * 7 * 255.f);  // HarrisResponses: scale = 1 / ((1 << 2) * blockSize * 255)
constexpr float DET_S4 = DET_S * DET_S * DET_S * DET_S;
constexpr float DET_PATCH = 31.f;               // KeyPoint::size on level 0
static_assert(DET_EDGE >= HALF_PATCH && DET_EDGE >= DET_HARRIS_R + 1, "neither IC_Angle nor the Harris block leaves the level");

// k_det_fast: a workgroup of 256 threads owns a tile of 64 x 16 pixels of one level.  It stages the raw pixels of the tile and
// 4 px around it (3 for the FAST ring of the scores one pixel outside the tile, which the suppression compares with),
// scores 66 x 18 pixels and suppresses 64 x 16, four adjacent pixels per thread, written as one dword of `map`.
constexpr int DET_TW = 64, DET_TH = 16, DET_FAST_THREADS = 256;
constexpr int DET_RAW_W = DET_TW + 8, DET_RAW_H = DET_TH + 8;  // 72 x 24 B
constexpr int DET_SC_W = DET_TW + 2, DET_SC_H = DET_TH + 2, DET_SC_PITCH = 68;
static_assert(DET_TW / 4 * DET_TH == DET_FAST_THREADS, "one dword of the tile per thread");
static_assert(DET_SC_PITCH >= DET_SC_W, "a score row holds the tile and its rim");

// k_det_select: one workgroup of 1024 threads per (image, level)
constexpr int DET_SEL_THREADS = 1024;
struct DetSelLds {
  size_t hist;  // int [256]  the level's score histogram, then the digit histogram of each radix pass
  size_t wv;    // int [DET_SEL_THREADS / 64]  scratch of fb::block_excl_scan
  size_t misc;  // int [4]  the cut of a pass, decided by thread 0
  size_t bytes;
};
FB_HD inline size_t det_select_layout(DetSelLds &L) {
  L.hist = 0;
  L.wv = L.hist + 256 * 4;
  L.misc = L.wv + (DET_SEL_THREADS / 64) * 4;
  L.bytes = L.misc + 4 * 4;
  return L.bytes;
}

// k_det_emit: one wave per output slot
constexpr int DET_EMIT_WAVES = 4;

// the NMS bound of one level
FB_HD inline int det_cand_bound(int w, int h) { return ((w + 1) / 2) * ((h + 1) / 2); }
// a level that cannot hold a key point (31 px on every side) yields nothing and is never scored
FB_HD inline bool det_level_live(int w, int h) { return w > 2 * DET_EDGE && h > 2 * DET_EDGE; }

struct DetLevel {
  int w, h, pitch;
  int K1, K2;           // retainBest #1 (FAST score) and #2 (Harris response): 2 N and N, N = mnFeaturesPerLevel
  int tilesX, candCap;
  float scale;          // mvScaleFactor[l]
  long long off;        // byte offset of the level in one image's raw pyramid (levels >= 1) = in the mask pyramid
  long long moff;       // byte offset of the level in one image's map
  long long candBase;   // element offset of the level in one image's pos / resp
};
struct DetK {
  int nlevels, thr, pitch0, kp_stride, mask_pitch0;
  long long img_stride, pyr_stride, map_stride, cand_stride;
  long long mask_img_stride, maskpyr_stride;  // bytes from one image's mask (mask levels) to the next; 0 = one mask for the batch
  int tileBase[FB_MAX_LEVELS + 1];  // first k_det_fast workgroup of each level
  const uint8_t *img0, *pyr;        // level 0 = the caller's images, levels >= 1 = the handle's pyramid
  const uint8_t *mask0, *maskpyr;   // level 0 = the caller's mask (null: no mask), levels >= 1 = the thresholded mask pyramid
  uint8_t *map;
  unsigned *hist;
  uint32_t *pos;
  float *resp;
  int32_t *cnt;
  const void *ang_tab;              // uint4 [64], the IC_Angle table of the handle's workspace (plan_angle_table)
  fb_keypoint *kps;
  int32_t *n, *n_true;
  DetLevel L[FB_MAX_LEVELS];
};

struct DetSizes { size_t map, hist, pos, resp, cnt, maskpyr; };  // bytes of every buffer for a batch
struct DetPlan {
  DetK K;  // the pointers and the per-call fields stay 0 here
  DetSizes sizes(size_t B, size_t masks) const {  // masks: mask pyramids held (1 = shared by the batch, B = one per image)
    DetSizes z;
    z.map = B * (size_t)K.map_stride + 256;
    z.hist = B * (size_t)K.nlevels * 256 * 4;
    z.pos = z.resp = B * (size_t)K.cand_stride * 4 + 16;
    z.cnt = B * (size_t)K.nlevels * 4;
    z.maskpyr = masks * (size_t)K.pyr_stride + 256;
    return z;
  }
};

// The detector's layout on the extractor's plan P (levels, pitches and offsets are the extractor's own).
inline int plan_detect(const OrbPlan &P, const fb_orb_tables &t, DetPlan &out) {
  DetPlan D;
  memset(&D.K, 0, sizeof(D.K));
  DetK &K = D.K;
  K.nlevels = P.K.nlevels;
  K.pyr_stride = P.K.pyrStride;
  K.map_stride = P.K.blurStride;
  long long cand = 0;
  int tiles = 0;
  for (int l = 0; l < K.nlevels; l++) {
    const LevelInfo &S = P.K.L[l];
    DetLevel &L = K.L[l];
    L.w = S.w; L.h = S.h; L.pitch = S.pitch;
    L.K2 = t.features_per_level[l];
    L.K1 = 2 * L.K2;
    L.scale = t.scale_factor[l];
    L.off = S.off; L.moff = S.boff;
    const bool live = det_level_live(L.w, L.h);
    L.tilesX = live ? L.pitch / DET_TW : 0;  // = ceil(w / 64): the tiles of a row cover the pitch exactly
    K.tileBase[l] = tiles;
    tiles += L.tilesX * (live ? (L.h + DET_TH - 1) / DET_TH : 0);
    L.candCap = live ? det_cand_bound(L.w, L.h) : 0;
    L.candBase = cand;
    cand += (L.candCap + 3) & ~3;
  }
  for (int l = K.nlevels; l <= FB_MAX_LEVELS; l++) K.tileBase[l] = tiles;
  K.cand_stride = cand;
  if (tiles >= (1 << 30)) { fb::set_error("fb_orb_detect: %d FAST tiles", tiles); return FB_ERR_CAPACITY; }
  out = D;
  return FB_OK;
}

// What both entry points refuse before anything is staged, allocated or enqueued.  *noop: batch 0, nothing to do.
inline int check_detect(const fb_orb_detect_args *A, size_t mask_image_stride, const char *what, bool *noop) {
  *noop = false;
  if (!A || A->batch < 0 || A->batch > 65535) { fb::set_error("%s: bad argument: batch %d", what, A ? A->batch : -1); return FB_ERR_ARG; }
  if (A->batch == 0) { *noop = true; return FB_OK; }
  if (!A->images || !A->kps || !A->n) { fb::set_error("%s: images, kps and n are required", what); return FB_ERR_ARG; }
  if (A->fast_threshold < 1 || A->fast_threshold > 255) { fb::set_error("%s: fast_threshold %d is outside 1..255", what, A->fast_threshold); return FB_ERR_ARG; }
  if (A->kp_stride <= 0) { fb::set_error("%s: kp_stride %d", what, A->kp_stride); return FB_ERR_ARG; }
  if (A->width < 2 * EDGE_THRESHOLD + 7 || A->height < 2 * EDGE_THRESHOLD + 7) {
    fb::set_error("%s: a %d x %d image is smaller than the extractor accepts", what, A->width, A->height);
    return FB_ERR_ARG;
  }
  if (A->stride < A->width || (A->batch > 1 && A->image_stride < (size_t)A->stride * (size_t)A->height)) {
    fb::set_error("%s: stride %d / image_stride %zu do not hold %d x %d images", what, A->stride, A->image_stride, A->width, A->height);
    return FB_ERR_ARG;
  }
  if (A->mask && A->mask_stride < A->width) { fb::set_error("%s: mask_stride %d is below the width %d", what, A->mask_stride, A->width); return FB_ERR_ARG; }
  if (A->mask && mask_image_stride != 0 && mask_image_stride < (size_t)A->mask_stride * (size_t)A->height) {
    fb::set_error("%s: mask_image_stride %zu does not hold a mask of %d rows of %d bytes", what, mask_image_stride, A->height, A->mask_stride);
    return FB_ERR_ARG;
  }
  return FB_OK;
}

// The bytes fb_orb_detect stages of each array (after check_detect, batch > 0); mask 0 = none given.
struct DetStage { size_t images, mask, kps, n, n_true; };
inline DetStage detect_stage(const fb_orb_detect_args &A) {
  const size_t B = (size_t)A.batch;
  DetStage z;
  z.images = (B - 1) * A.image_stride + (size_t)A.stride * (size_t)A.height;
  z.mask = A.mask ? (size_t)A.mask_stride * (size_t)A.height : 0;
  z.kps = B * (size_t)A.kp_stride * sizeof(fb_keypoint);
  z.n = z.n_true = B * 4;
  return z;
}

}  // namespace
#endif
