// orb_describe_at_plan.h -- the kernel arguments and the dynamic LDS of k_describe_at (orb_describe_at.inc), stated once: a
// workgroup is DESCAT_WAVES waves, a wave owns one key point and one private slice: the radius-18 blurred patch (37 rows of
// 10 dwords: x-18 .. x+18 after dword alignment), then, in IC-angle mode only, the radius-15 raw patch (31 rows of 9
// dwords).  1488 B per wave with the angle kept, 2608 B with IC_Angle: 5.8 / 10.2 KB per workgroup, no LDS opt-in.
//
// No HIP header: plain host/device code like subpix_plan.h.  The launcher calls plan_describe_at(), which returns the bytes
// or refuses; the kernel calls describe_at_layout() with the same angle mode and takes its pointers from it.
// Unnamed namespace: one translation unit at a time.
#ifndef FB_ORB_DESCRIBE_AT_PLAN_H_
#define FB_ORB_DESCRIBE_AT_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "../../include/fishbird.h"

#ifndef FB_HD
#define FB_HD
#endif

namespace fb {
void set_error(const char *fmt, ...);
}

namespace {

constexpr int DESCAT_WAVES = 4;                          // key points per workgroup (the waves never talk to each other)
constexpr int DESCAT_THREADS = DESCAT_WAVES * 64;
constexpr int DESCAT_EDGE = 19;                          // EDGE_THRESHOLD: a key point sits >= 19 px inside its level
constexpr int DESCAT_BL_R = 18, DESCAT_BL_ROWS = 2 * DESCAT_BL_R + 1, DESCAT_BL_DW = 10;     // 37 rows x 40 B
constexpr int DESCAT_RAW_R = 15, DESCAT_RAW_ROWS = 2 * DESCAT_RAW_R + 1, DESCAT_RAW_DW = 9;  // 31 rows x 36 B
constexpr size_t DESCAT_LDS_MAX = 64 * 1024;             // what a launch gets without an opt-in
// a patch starts up to 3 bytes into its first dword: the last column used is 3 + 2 r, inside the row
static_assert(3 + 2 * DESCAT_BL_R < DESCAT_BL_DW * 4 && 3 + 2 * DESCAT_RAW_R < DESCAT_RAW_DW * 4, "a staged row holds the patch at every alignment");

struct DescAtLds {
  size_t blur;   // uint32 [DESCAT_BL_ROWS][DESCAT_BL_DW]    byte offset inside the wave's slice
  size_t raw;    // uint32 [DESCAT_RAW_ROWS][DESCAT_RAW_DW]  (FB_DESCRIBE_IC_ANGLE only)
  size_t slice;  // bytes per wave, a multiple of 16
};
FB_HD inline size_t describe_at_layout(DescAtLds &L, int angle_mode) {
  L.blur = 0;
  L.raw = (L.blur + (size_t)DESCAT_BL_ROWS * DESCAT_BL_DW * 4 + 15) & ~(size_t)15;
  const size_t end = angle_mode == FB_DESCRIBE_IC_ANGLE ? L.raw + (size_t)DESCAT_RAW_ROWS * DESCAT_RAW_DW * 4 : L.raw;
  L.slice = (end + 15) & ~(size_t)15;
  return L.slice * DESCAT_WAVES;
}

inline int plan_describe_at(int angle_mode, const char *what, size_t *bytes) {
  if (angle_mode != FB_DESCRIBE_KEEP_ANGLE && angle_mode != FB_DESCRIBE_IC_ANGLE) {
    fb::set_error("%s: angle_mode %d is neither FB_DESCRIBE_KEEP_ANGLE nor FB_DESCRIBE_IC_ANGLE", what, angle_mode);
    return FB_ERR_ARG;
  }
  DescAtLds L;
  *bytes = describe_at_layout(L, angle_mode);
  if (*bytes > DESCAT_LDS_MAX) {
    fb::set_error("%s: %zu B of LDS", what, *bytes);
    return FB_ERR_CAPACITY;
  }
  return FB_OK;
}

// What both entry points refuse before anything is staged or enqueued.  last_batch, w, h: the handle's last extract call
// (last_batch 0 = none yet).  Plain host code, so that tests/cpp/describe_at_plan_test.cpp can run it under the sanitizers.
inline int check_describe_at(const fb_orb_describe_args *A, int last_batch, int w, int h, const char *what, size_t *lds) {
  if (!A || A->batch < 0 || A->batch > 65535 || A->kp_stride < 0) {
    fb::set_error("%s: bad argument: batch %d, kp_stride %d", what, A ? A->batch : -1, A ? A->kp_stride : -1);
    return FB_ERR_ARG;
  }
  const int rc = plan_describe_at(A->angle_mode, what, lds);
  if (rc != FB_OK) return rc;
  if (last_batch <= 0) { fb::set_error("%s: the handle has not extracted anything yet (no pyramid to describe on)", what); return FB_ERR_ARG; }
  if (A->batch > last_batch) { fb::set_error("%s: batch %d, the last extract call had %d images", what, A->batch, last_batch); return FB_ERR_ARG; }
  if (A->batch == 0 || A->kp_stride == 0) return FB_OK;
  if (!A->n || !A->kps || !A->desc) { fb::set_error("%s: n, kps and desc are required", what); return FB_ERR_ARG; }
  if (A->angle_mode == FB_DESCRIBE_IC_ANGLE) {
    if (!A->images) { fb::set_error("%s: FB_DESCRIBE_IC_ANGLE needs the images of the extract call (level 0 of the raw pyramid)", what); return FB_ERR_ARG; }
    if (A->stride < w || (A->batch > 1 && A->image_stride < (size_t)A->stride * (size_t)h)) {
      fb::set_error("%s: stride %d / image_stride %zu do not hold %d x %d images", what, A->stride, A->image_stride, w, h);
      return FB_ERR_ARG;
    }
  }
  return FB_OK;
}

// The bytes fb_orb_describe stages of each array (after check_describe_at, batch and kp_stride > 0); images 0 = not staged.
struct DescAtStage { size_t images, n, kps, desc, status; };
inline DescAtStage describe_at_stage(const fb_orb_describe_args &A, int h) {
  const size_t B = (size_t)A.batch, ks = (size_t)A.kp_stride;
  DescAtStage z;
  z.images = A.angle_mode == FB_DESCRIBE_IC_ANGLE ? (B - 1) * A.image_stride + (size_t)A.stride * (size_t)h : 0;
  z.n = B * 4; z.kps = B * ks * sizeof(fb_keypoint); z.desc = B * ks * 32; z.status = B * ks;
  return z;
}

// What the kernel needs of a pyramid level, and of the call.  (OrbK carries the quadtree's and k_fast's tables as well; the
// level is picked per wave from the key point's record, so only these six numbers are read.)
struct DescAtLevel {
  int w, h, pitch;
  float inv_scale;      // mvInvScaleFactor[l]
  long long off, boff;  // byte offsets of the level in one image's pyramid / blurred pyramid
};
struct DescAtK {
  int nlevels, kp_stride, angle_mode, pitch0;
  long long img_stride, pyr_stride, blur_stride;
  const int32_t *n;
  fb_keypoint *kps;
  uint8_t *desc, *status;
  const uint8_t *img0;  // the caller's images = level 0 of the raw pyramid (IC mode only)
  const uint8_t *pyr, *blur;
  const void *ang_tab;  // uint4 [64], the IC_Angle table of the handle's workspace (plan_angle_table)
  DescAtLevel L[FB_MAX_LEVELS];
};

}  // namespace
#endif
