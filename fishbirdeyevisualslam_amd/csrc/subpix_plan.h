// subpix_plan.h -- the dynamic LDS of k_corner_subpix (frame.hip), stated once: a workgroup is SUBPIX_WAVES waves, a wave owns
// one key point and one private slice: the (2w+3) x (2h+3) float patch of the current round, then the (2w+1) x (2h+1) float
// window weights, written once.  At the reference's 5 x 5 half window: 169 + 121 floats = 1160 B (1168 rounded) per wave.
//
// No HIP header: plain host/device code like match_plan.h.  The launcher calls plan_subpix(), which checks the window and
// returns the bytes or refuses; the kernel calls subpix_layout() with the same two numbers and takes its pointers from it.
// Unnamed namespace: one translation unit at a time.
#ifndef FB_SUBPIX_PLAN_H_
#define FB_SUBPIX_PLAN_H_

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

constexpr int SUBPIX_WAVES = 4;                      // key points per workgroup
constexpr int SUBPIX_THREADS = SUBPIX_WAVES * 64;
constexpr int SUBPIX_MAX_HALF = 8;                   // window up to 17 x 17, patch up to 19 x 19
constexpr int SUBPIX_MAX_ITERS = 100;                // OpenCV's MAX_ITERS
constexpr size_t SUBPIX_LDS_MAX = 64 * 1024;         // what a launch gets without an opt-in; the largest plan is 10.4 KB

struct SubpixLds {
  int pw, ph, ww, wh;   // patch and window extents
  size_t patch;         // float [ph][pw]   byte offset inside the wave's slice
  size_t weight;        // float [wh][ww]
  size_t slice;         // bytes per wave, a multiple of 16
};
FB_HD inline size_t subpix_layout(SubpixLds &L, int half_x, int half_y) {
  L.ww = 2 * half_x + 1; L.wh = 2 * half_y + 1;
  L.pw = L.ww + 2; L.ph = L.wh + 2;
  L.patch = 0;
  L.weight = L.patch + (size_t)L.pw * L.ph * 4;
  L.slice = (L.weight + (size_t)L.ww * L.wh * 4 + 15) & ~(size_t)15;
  return L.slice * SUBPIX_WAVES;
}

inline int plan_subpix(int half_x, int half_y, const char *what, SubpixLds *L, size_t *bytes) {
  if (half_x < 1 || half_x > SUBPIX_MAX_HALF || half_y < 1 || half_y > SUBPIX_MAX_HALF) {
    fb::set_error("%s: half window %d x %d outside 1..%d", what, half_x, half_y, SUBPIX_MAX_HALF);
    return FB_ERR_ARG;
  }
  *bytes = subpix_layout(*L, half_x, half_y);
  if (*bytes > SUBPIX_LDS_MAX) {
    fb::set_error("%s: %zu B of LDS for a %d x %d half window", what, *bytes, half_x, half_y);
    return FB_ERR_CAPACITY;
  }
  return FB_OK;
}
static_assert((size_t)((2 * SUBPIX_MAX_HALF + 3) * (2 * SUBPIX_MAX_HALF + 3) + (2 * SUBPIX_MAX_HALF + 1) * (2 * SUBPIX_MAX_HALF + 1)) * 4 + 16 <=
                  SUBPIX_LDS_MAX / SUBPIX_WAVES, "every accepted window fits without an LDS opt-in");

}  // namespace
#endif
