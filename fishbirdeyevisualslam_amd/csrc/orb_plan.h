// orb_plan.h -- what the ORB extractor derives from (parameters, image size) before it touches the GPU: the host tables of
// ORBextractor::ORBextractor, the kernel argument block OrbK, the resize and IC_Angle tables and the buffer sizes.
//
// No HIP header and no handle: plan_orb() is plain host code (tests/cpp/orb_plan_test.cpp compiles it with g++).  It fills a
// local OrbPlan and assigns the caller's only on success, so a refusal leaves a plan that was valid before exactly as it
// was; orb.hip allocates from the plan and commits plan and buffers to the handle together.  Everything sits in an unnamed
// namespace like the kernels that take OrbK by value: the header belongs to one translation unit at a time.
#ifndef FB_ORB_PLAN_H_
#define FB_ORB_PLAN_H_

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/fishbird.h"

#ifndef FB_HD
#define FB_HD
#endif
#include "fb_detmath.h"

namespace fb {
void set_error(const char *fmt, ...);
}

namespace {

constexpr int EDGE_THRESHOLD = 19;  // ORBextractor.cc:74
constexpr int HALF_PATCH = 15;      // :73
constexpr int PATCH_SIZE = 31;      // :72
constexpr int BORDER = EDGE_THRESHOLD - 3;  // minBorderX/Y, :773

constexpr int FAST_MAX_TILE = 72;  // k_fast: cell window <= wCell+6 <= 65 px, +3 alignment slack
constexpr int FAST_CPW = 4;  // k_fast: consecutive cells per wave; the tile of cell i+1 is in flight while cell i is processed
constexpr int DESC_WPB = 4;  // k_describe: waves per workgroup (they never talk to each other)
constexpr int DESC_KPW = 2;  // k_describe: consecutive slots per wave, all their patch loads in flight together
constexpr int BLUR_ROWS = 32;  // k_blur: rows of a wave's strip of 256 columns
constexpr size_t OCTREE_LDS_MAX = 160 * 1024 - 512;  // k_octree: 512 B of the 160 KiB stay with its static LDS (scan scratch, a few scalars)
#ifdef FB_FAST_LISTHIST
#define FB_ORB_TIMER_WORDS (16 + 128)  // + the list-length histograms of the probe build (fb_orb_debug_list_hist)
#else
#define FB_ORB_TIMER_WORDS 16
#endif

struct LevelInfo {
  int w, h, pitch;
  long long off;  // byte offset of the level inside one image's pyramid buffer (levels >= 1)
  int nCols, nRows, wCell, hCell, cellBase;
  int N;                 // mnFeaturesPerLevel
  long long candBase;    // element offset into one image's candidate array
  int candCap;
  int slotCap;           // candidate slots per FAST cell (k_fast writes cell c's survivors at candBase + c * slotCap)
  int outBase, outCap;   // element offset / capacity in one image's per-level keypoint array
  int nIni;
  float hX;
  float scale;
  int patchSize;         // (int)(PATCH_SIZE*scale), :836
  long long boff;        // byte offset of the level's blurred copy inside one image's blur buffer
};

struct OrbK {
  int nlevels, iniTh, minTh, totalCells, outStride, capOut;
  int kpStride;  // entries per image in the caller's key-point / descriptor arrays (= capOut unless fb_orb_set_output_stride)
  int fastTileBytes, fastMaxOut, fastMaxPix;  // LDS carve of k_fast
  int fastTP;                                 // tile pitch instantiation of k_fast (44 / 56 / 72)
  int dbg;  // FB_FAST_DBG ablation switch (0 = normal)
  unsigned long long *timers;  // FB_FAST_DBG=20: per-phase wave time of k_fast (fb_orb_debug_timers)
  int cellBase[FB_MAX_LEVELS + 1];  // first FAST cell of each level (contiguous copy for one scalar load)
  int grpBase[FB_MAX_LEVELS + 1];   // first k_fast wave of each level (a wave = FAST_CPW consecutive cells)
  int totalGroups;
  // k_describe: a workgroup serves DESC_WPB * DESC_KPW consecutive slots of ONE level's run of lvlOut
  int descBase[FB_MAX_LEVELS + 1];  // first k_describe workgroup of each level
  int runBase[FB_MAX_LEVELS];       // L[l].outBase / L[l].outCap again, contiguous: the record address needs nothing else
  int runCap[FB_MAX_LEVELS];
  long long pyrStride;   // bytes per image of levels >= 1
  long long blurStride;  // bytes per image of the blurred pyramid (all levels)
  int blurStrips[FB_MAX_LEVELS + 1];  // first k_blur strip of each level
  long long candStride;  // candidates per image
  int umax[16];
  LevelInfo L[FB_MAX_LEVELS];
};

struct ResizeTabs {  // per level >= 1, device pointers
  const int *xofs;
  const short *ialpha;
  const int *yofs;
  const short *ibeta;
};

struct ONode {  // a quadtree node of k_octree
  short x0, y0, x1, y1;
  int cnt;
};

inline void make_tables(const fb_orb_params &p, fb_orb_tables &t) {  // ORBextractor.cc:410-470
  memset(&t, 0, sizeof(t));
  const int nl = p.nlevels;
  t.scale_factor[0] = 1.0f;
  t.level_sigma2[0] = 1.0f;
  for (int i = 1; i < nl; i++) {
    t.scale_factor[i] = t.scale_factor[i - 1] * p.scale_factor;
    t.level_sigma2[i] = t.scale_factor[i] * t.scale_factor[i];
  }
  for (int i = 0; i < nl; i++) {
    t.inv_scale_factor[i] = 1.0f / t.scale_factor[i];
    t.inv_level_sigma2[i] = 1.0f / t.level_sigma2[i];
  }
  float factor = 1.0f / p.scale_factor;
  float nDesired = p.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nl));
  int sum = 0;
  for (int l = 0; l < nl - 1; l++) {
    t.features_per_level[l] = fb_cvround(nDesired);
    sum += t.features_per_level[l];
    nDesired *= factor;
  }
  t.features_per_level[nl - 1] = std::max(p.nfeatures - sum, 0);
  int umax[HALF_PATCH + 2] = {0};
  int v, v0;
  const int vmax = fb_cvfloor(HALF_PATCH * sqrtf(2.f) / 2 + 1);
  const int vmin = fb_cvceil(HALF_PATCH * sqrtf(2.f) / 2);
  const double hp2 = HALF_PATCH * HALF_PATCH;
  for (v = 0; v <= vmax; ++v) umax[v] = fb_cvround_d(sqrt(hp2 - v * v));
  for (v = HALF_PATCH, v0 = 0; v >= vmin; --v) {
    while (umax[v0] == umax[v0 + 1]) ++v0;
    umax[v] = v0;
    ++v0;
  }
  for (int i = 0; i <= HALF_PATCH; i++) t.umax[i] = umax[i];
}

inline int capacity_of(const fb_orb_params &p) { return p.nfeatures + 8 * p.nlevels; }

struct OrbSizes {  // bytes of every workspace buffer for a batch
  size_t pyr, blur, cand, cellCand, cellCount, nodeOf, counts, lvlOut, timers;
};

struct OrbPlan {
  OrbK K;  // timers and dbg stay 0 here: a device pointer and an environment switch, both filled at commit
  bool rowsOK[FB_MAX_LEVELS];   // k_resize_rows may build the level (given an aligned source)
  bool mergeOK[FB_MAX_LEVELS];  // k_resize_merge may
  std::vector<uint8_t> tabBytes;    // the resize tables of the levels >= 1, each 16-byte aligned
  size_t tabOff[FB_MAX_LEVELS][4];  // xofs, ialpha, yofs, ibeta of a level inside tabBytes
  uint32_t angTab[64 * 4];          // IC_Angle table of k_describe
  int maxNodes;      // quadtree nodes of the largest level
  size_t octreeLds;  // dynamic LDS of k_octree
  // The per-image strides are K.pyrStride, K.blurStride (bytes), K.candStride, K.totalCells, K.outStride (elements).
  OrbSizes sizes(size_t B) const {
    OrbSizes z;
    z.pyr = B * K.pyrStride + 256;
    z.blur = B * K.blurStride + 256;
    z.cand = z.cellCand = B * K.candStride * 4 + 16;
    z.cellCount = B * (size_t)K.totalCells * 4 + 16;
    z.nodeOf = B * K.candStride * 2 + 16;
    z.counts = B * K.nlevels * 4 * 2 + FB_MAX_LEVELS * 4;  // candCount | lvlCount | slack: k_describe reads FB_MAX_LEVELS counts per image
    z.lvlOut = B * K.outStride * 4 + 16;
    z.timers = FB_ORB_TIMER_WORDS * 8;
    return z;
  }
};

// ---- step 1: the geometry of one level (everything that does not depend on the levels before it) ----
inline int plan_level(const fb_orb_params &p, const fb_orb_tables &t, int w, int h, int l, LevelInfo &L) {
  const float scale = t.inv_scale_factor[l];
  L.w = fb_cvround((float)w * scale);   // ORBextractor.cc:1112
  L.h = fb_cvround((float)h * scale);
  if (l == 0) { L.w = w; L.h = h; }
  if (L.w < 1 || L.h < 1) {  // cv::resize to an empty Size asserts in the reference as well
    fb::set_error("pyramid level %d of a %dx%d image is empty (scale factor %.3f, %d levels)", l, w, h, (double)p.scale_factor, p.nlevels);
    return FB_ERR_ARG;
  }
  if (L.w >= 4096 || L.h >= 4096) { fb::set_error("image too large (level %d is %dx%d, limit 4095)", l, L.w, L.h); return FB_ERR_ARG; }
  L.pitch = (L.w + 63) & ~63;
  const int maxBX = L.w - BORDER, maxBY = L.h - BORDER;
  const float width = (float)(maxBX - BORDER), height = (float)(maxBY - BORDER);
  L.nCols = (int)(width / 30.f);
  L.nRows = (int)(height / 30.f);
  if (L.nCols <= 0 || L.nRows <= 0) { L.nCols = L.nRows = 0; L.wCell = L.hCell = 1; }
  else { L.wCell = (int)ceilf(width / L.nCols); L.hCell = (int)ceilf(height / L.nRows); }
  if (L.wCell + 6 > FAST_MAX_TILE - 3 || L.hCell + 6 > FAST_MAX_TILE) { fb::set_error("FAST cell %dx%d exceeds the LDS tile", L.wCell, L.hCell); return FB_ERR_CAPACITY; }
  if (L.nCols * L.nRows >= (1 << 20)) { fb::set_error("level %d has more than 2^20 FAST cells", l); return FB_ERR_CAPACITY; }
  L.N = t.features_per_level[l];
  L.slotCap = ((L.wCell + 1) / 2) * ((L.hCell + 1) / 2);  // strict 3x3 maxima: at most one per 2x2 pixels
  L.candCap = L.nCols * L.nRows * L.slotCap + 16;         // the NMS worst case of every cell
  if (L.candCap >= (1 << 24)) { fb::set_error("level %d: more than 2^24 FAST candidates possible", l); return FB_ERR_CAPACITY; }
  const int Wr = maxBX - BORDER, Hr = maxBY - BORDER;
  L.nIni = (Hr > 0) ? (int)roundf((float)Wr / Hr) : 0;   // ORBextractor.cc:542
  L.hX = L.nIni > 0 ? (float)Wr / L.nIni : 1.f;
  L.outCap = std::max(L.N + 3, 4 * L.nIni) + 4;
  L.scale = t.scale_factor[l];
  L.patchSize = (int)(PATCH_SIZE * t.scale_factor[l]);
  return FB_OK;
}

// ---- step 2: where each level lies inside one image's share of every buffer, and the per-image strides ----
inline void plan_offsets(OrbPlan &P) {
  OrbK &K = P.K;
  long long pyrOff = 0, candOff = 0, blurOff = 0;
  int cells = 0, outOff = 0, strips = 0;
  P.maxNodes = 0;
  for (int l = 0; l < K.nlevels; l++) {
    LevelInfo &L = K.L[l];
    L.off = pyrOff;
    if (l > 0) pyrOff += (long long)L.pitch * L.h;
    L.boff = blurOff;
    blurOff += (long long)L.pitch * L.h;
    K.blurStrips[l] = strips;
    // levels too small to hold a key point (19 px border on every side) are never sampled: no blur strips for them
    if (L.w >= 2 * EDGE_THRESHOLD && L.h >= 2 * EDGE_THRESHOLD) strips += ((L.w + 255) / 256) * ((L.h + BLUR_ROWS - 1) / BLUR_ROWS);
    L.cellBase = cells;
    cells += L.nCols * L.nRows;
    L.candBase = candOff;
    candOff += (L.candCap + 3) & ~3;
    L.outBase = outOff;
    outOff += L.outCap;
    P.maxNodes = std::max(P.maxNodes, L.outCap + 4);
  }
  for (int l = K.nlevels; l <= FB_MAX_LEVELS; l++) K.blurStrips[l] = strips;
  K.totalCells = cells;
  K.pyrStride = (pyrOff + 255) & ~255ll;
  K.blurStride = (blurOff + 255) & ~255ll;
  K.candStride = candOff;
  K.outStride = outOff;
}

// ---- step 3: the resize tables of one level (oracle resize_linear_u8) and which kernels may use them ----
// Same arithmetic as k_resize, restructured for throughput: a lane of k_resize_rows owns 4 adjacent destination pixels and
// walks RESIZE_ROWS destination rows with one 12-byte source window per row.
constexpr int RESIZE_ROWS = 8;
// the taps of every 4-pixel group: inside the 12-byte window, and within 8 bytes of the group's first tap (scale <= 2)
inline bool resize_rows_ok(const std::vector<int> &xofs) {
  const int dw = (int)xofs.size();
  bool ok = true;
  for (int dx4 = 0; dx4 < dw; dx4 += 4) {
    const int last = xofs[std::min(dx4 + 3, dw - 1)] + 1;
    ok = ok && (last - (xofs[dx4] & ~3)) <= 11 && (last - xofs[dx4]) <= 7;
  }
  return ok;
}
// k_resize_merge walks the SOURCE rows of a run of RM_ROWS destination rows once, all RM_SRC windows requested up front.
constexpr int RM_ROWS = 12, RM_SRC = 16;
// every run of RM_ROWS destination rows spans at most RM_SRC source rows, and a source row closes at most one destination row
inline bool resize_merge_ok(const std::vector<int> &yofs) {
  const int dh = (int)yofs.size();
  bool ok = true;
  for (int y0 = 0; y0 < dh && ok; y0 += RM_ROWS) {
    const int y1 = std::min(y0 + RM_ROWS, dh) - 1;
    ok = yofs[y0] >= 0 && yofs[y1] + 1 - yofs[y0] <= RM_SRC - 1;
    for (int y = y0; y < y1 && ok; y++) ok = yofs[y + 1] > yofs[y];
  }
  return ok;
}

inline void plan_resize_tables(OrbPlan &P, int l) {
  const LevelInfo &S = P.K.L[l - 1], &D = P.K.L[l];
  const int sw = S.w, sh = S.h, dw = D.w, dh = D.h;
  const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
  std::vector<int> xofs(dw, 0), yofs(dh, 0);
  std::vector<short> ialpha(dw * 2, 0), ibeta(dh * 2, 0);
  for (int dx = 0; dx < dw; dx++) {
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = fb_cvfloor(fx);
    fx -= sx;
    if (sx < 0) { fx = 0; sx = 0; }
    if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
    xofs[dx] = sx;
    ialpha[dx * 2] = (short)fb_cvround((1.f - fx) * 2048.f);
    ialpha[dx * 2 + 1] = (short)fb_cvround(fx * 2048.f);
  }
  for (int dy = 0; dy < dh; dy++) {
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    int sy = fb_cvfloor(fy);
    fy -= sy;
    yofs[dy] = sy;
    ibeta[dy * 2] = (short)fb_cvround((1.f - fy) * 2048.f);
    ibeta[dy * 2 + 1] = (short)fb_cvround(fy * 2048.f);
  }
  P.rowsOK[l] = resize_rows_ok(xofs);
  P.mergeOK[l] = P.rowsOK[l] && resize_merge_ok(yofs);
  auto append = [&](const void *src, size_t n) {
    const size_t off = (P.tabBytes.size() + 15) & ~(size_t)15;
    P.tabBytes.resize(off + n);
    memcpy(P.tabBytes.data() + off, src, n);
    return off;
  };
  P.tabOff[l][0] = append(xofs.data(), xofs.size() * 4);
  P.tabOff[l][1] = append(ialpha.data(), ialpha.size() * 2);
  P.tabOff[l][2] = append(yofs.data(), yofs.size() * 4);
  P.tabOff[l][3] = append(ibeta.data(), ibeta.size() * 2);
}

// ---- step 4: the LDS carve of k_fast, sized for the largest cell of this image size ----
inline void plan_fast_tile(OrbK &K) {
  int tileB = 0, maxOut = 0, maxPix = 0, tpNeed = 0;
  for (int l = 0; l < K.nlevels; l++) {
    const LevelInfo &L = K.L[l];
    if (L.nCols * L.nRows == 0) continue;
    const int tpMax = (L.wCell + 6 + 3 + 3) & ~3, chMax = L.hCell + 6;
    tpNeed = std::max(tpNeed, tpMax);
    tileB = std::max(tileB, chMax);
    maxOut = std::max(maxOut, L.slotCap);
    maxPix = std::max(maxPix, L.wCell * L.hCell);
  }
  K.fastTP = tpNeed <= 44 ? 44 : tpNeed <= 56 ? 56 : FAST_MAX_TILE;
  K.fastTileBytes = (std::max(K.fastTP * tileB, 4 * ((maxOut + 3) & ~3)) + 15) & ~15;
  K.fastTileBytes = std::max(K.fastTileBytes, (21 * K.fastTP + 15) & ~15);  // k_fast stages 40 / 42 rows unconditionally into tile + score tile
  K.fastMaxOut = (maxOut + 3) & ~3;
  K.fastMaxPix = (maxPix + 7) & ~7;
}

// ---- step 5: which level a k_fast wave / a k_describe workgroup belongs to ----
inline void plan_grids(OrbK &K) {
  int gsum = 0, wsum = 0;
  for (int l = 0; l <= FB_MAX_LEVELS; l++) {
    K.cellBase[l] = l < K.nlevels ? K.L[l].cellBase : K.totalCells;
    K.grpBase[l] = gsum;
    K.descBase[l] = wsum;  // whole workgroups per level, so that no k_describe wave straddles two levels
    if (l >= K.nlevels) continue;
    gsum += (K.L[l].nCols * K.L[l].nRows + FAST_CPW - 1) / FAST_CPW;
    K.runBase[l] = K.L[l].outBase;
    K.runCap[l] = K.L[l].outCap;
    wsum += (K.L[l].outCap + DESC_WPB * DESC_KPW - 1) / (DESC_WPB * DESC_KPW);
  }
  K.totalGroups = gsum;
}

// ---- step 6: LDS of k_octree: 2 lists + ccnt + cpos + npos + order + split + best ----
inline int plan_octree_lds(OrbPlan &P) {
  const size_t M = P.maxNodes;
  size_t lds = 2 * M * sizeof(ONode) + 4 * M * 4 + 4 * M * 2 + M * 2 + M * 2 + M;
  lds = ((lds + 7) & ~(size_t)7) + M * 8 + 16;
  size_t maxCells = 0;
  for (int l = 0; l < P.K.nlevels; l++) maxCells = std::max(maxCells, (size_t)P.K.L[l].nCols * P.K.L[l].nRows);
  lds = std::max(lds, (maxCells + 1) * 4 + 16);  // the per-cell offsets of the packing prologue alias the node lists
  if (lds > OCTREE_LDS_MAX) { fb::set_error("nfeatures too large for the LDS quadtree (%zu B)", lds); return FB_ERR_CAPACITY; }
  P.octreeLds = lds;
  return FB_OK;
}

// ---- step 7: IC_Angle table of k_describe: lane 2r+half owns half of patch row v = r-15; per byte j of its 16-byte span
// the weight |u| (low nibble) and the inclusion mask |u| <= umax[|v|] (bit 4; left half: u = j-15, u = 0 belongs to the
// right half).  An excluded byte is 0.
inline void plan_angle_table(OrbPlan &P) {
  for (int lane = 0; lane < 62; lane++) {
    const int v = (lane >> 1) - 15, half = lane & 1, dmax = P.K.umax[v < 0 ? -v : v];
    for (int j = 0; j < 16; j++) {
      const int au = half ? j : 15 - j;
      const bool inc = au <= dmax && (half || au != 0);
      if (!inc) continue;
      P.angTab[lane * 4 + (j >> 2)] |= ((uint32_t)au | 0x10u) << (8 * (j & 3));
    }
  }
}

// The workspace layout for images of w x h.  FB_OK, or the refusal's code with its message set and `out` untouched.
inline int plan_orb(const fb_orb_params &p, const fb_orb_tables &t, int w, int h, int kpStride, OrbPlan &out) {
  OrbPlan P;
  memset(&P.K, 0, sizeof(P.K));
  memset(P.rowsOK, 0, sizeof(P.rowsOK));
  memset(P.mergeOK, 0, sizeof(P.mergeOK));
  memset(P.tabOff, 0, sizeof(P.tabOff));
  memset(P.angTab, 0, sizeof(P.angTab));
  OrbK &K = P.K;
  K.nlevels = p.nlevels;
  K.iniTh = p.ini_th_fast;
  K.minTh = p.min_th_fast;
  K.capOut = capacity_of(p);
  K.kpStride = kpStride > 0 ? kpStride : K.capOut;
  for (int i = 0; i < 16; i++) K.umax[i] = t.umax[i];
  for (int l = 0; l < p.nlevels; l++) {
    const int rc = plan_level(p, t, w, h, l, K.L[l]);
    if (rc != FB_OK) return rc;
  }
  plan_offsets(P);
  for (int l = 1; l < p.nlevels; l++) plan_resize_tables(P, l);
  plan_fast_tile(K);
  plan_grids(K);
  const int rc = plan_octree_lds(P);
  if (rc != FB_OK) return rc;
  plan_angle_table(P);
  out = std::move(P);
  return FB_OK;
}

}  // namespace

#endif
