// match_plan.h -- the dynamic LDS of every matcher kernel (match.hip, match_kf.inc, match_bow.hip), stated once: where each
// array of a workgroup lies, how many bytes the launch asks for, and which variant of the kernel fits.
//
// No HIP header: plain host/device code (tests/cpp/match_plan_test.cpp compiles it with g++ and sweeps it).  A launcher calls
// one plan_*() function, which picks the variant and returns the bytes or refuses; the kernel calls the same *_layout()
// function with the arguments it already receives and takes every pointer from the offsets.  All offsets are bytes from the
// start of the workgroup's dynamic LDS.  DESIGN.md section 4 has the table kernel -> layout -> variants.
//
// Everything sits in an unnamed namespace like the kernels: the header belongs to one translation unit at a time.
#ifndef FB_MATCH_PLAN_H_
#define FB_MATCH_PLAN_H_

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

// ---- the budget and the refusal -------------------------------------------------------------------------------------------
constexpr size_t LDS_BYTES = 160 * 1024;         // what a workgroup may have on gfx950, dynamic + static
constexpr size_t LDS_STATIC_MAX = 512;           // no matcher kernel has more static __shared__ than this (asserted below)
constexpr size_t LDS_BUDGET = LDS_BYTES - LDS_STATIC_MAX;  // a variant is chosen when its dynamic bytes fit in this

FB_HD constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// Static __shared__ bytes of each kernel.  A kernel keeps its statics in one struct and has a static_assert of that struct's
// size, rounded to the 16-byte alignment of the dynamic LDS behind it, against the constant here; the two tail kernels add
// the scan scratch of grid_build_body.  (These are the group_segment_fixed_size figures of the code objects.)
constexpr size_t CLAIM_FLAGS_BYTES = 8, ROT_HIST_BYTES = 33 * 4, POSE_BYTES = 12 * 4, VEC3_BYTES = 3 * 4;
constexpr size_t SCAN_PART_BYTES_1024 = 1024 / 64 * 4, SCAN_PART_BYTES_256 = 256 / 64 * 4;  // grid_build_body<NT>: one int per wave
constexpr size_t STATIC_M3 = up16(CLAIM_FLAGS_BYTES + (FB_MAX_LEVELS + 1) * 4 + ROT_HIST_BYTES + POSE_BYTES);  // proj_frame_body
constexpr size_t STATIC_TAIL_FRONT = STATIC_M3 + SCAN_PART_BYTES_1024;
constexpr size_t STATIC_M4 = up16(CLAIM_FLAGS_BYTES + ROT_HIST_BYTES + POSE_BYTES + VEC3_BYTES);
constexpr size_t STATIC_M2 = up16(CLAIM_FLAGS_BYTES);       // k_proj_points, k_m2_resolve (k_m2_candidates has none)
constexpr size_t STATIC_BIRD_MP = up16(2 * POSE_BYTES + 4); // bird_mappoints_body
constexpr size_t STATIC_TAIL_BIRD = STATIC_BIRD_MP + SCAN_PART_BYTES_1024;
constexpr size_t STATIC_BIRDVIEW = up16(2 * 4 + ROT_HIST_BYTES);
constexpr size_t STATIC_GRID = SCAN_PART_BYTES_256;         // k_grid_build
constexpr size_t STATIC_FUSE = up16(POSE_BYTES + VEC3_BYTES);
constexpr size_t STATIC_PROJ_SIM3 = up16(POSE_BYTES + VEC3_BYTES + CLAIM_FLAGS_BYTES);
constexpr size_t STATIC_SIM3 = up16((9 + 9 + 3 + 3 + 12 + 12) * 4 + 4);
constexpr size_t STATIC_INIT = up16(2 * 4 + ROT_HIST_BYTES);
constexpr size_t STATIC_BOW = up16(CLAIM_FLAGS_BYTES + ROT_HIST_BYTES);
constexpr size_t STATIC_TRIANGULATION = up16(4 + ROT_HIST_BYTES + 2 * 4 + 9 * 4);
static_assert(STATIC_TAIL_FRONT <= LDS_STATIC_MAX && STATIC_TAIL_BIRD <= LDS_STATIC_MAX && STATIC_SIM3 <= LDS_STATIC_MAX &&
              STATIC_TRIANGULATION <= LDS_STATIC_MAX && STATIC_M4 <= LDS_STATIC_MAX && STATIC_BOW <= LDS_STATIC_MAX,
              "a variant that fits LDS_BUDGET must never be refused");

// The one refusal: dynamic + static LDS of the launch against the 160 KiB of a workgroup.
inline int check_lds(size_t dynBytes, size_t staticBytes, const char *what) {
  if (dynBytes + staticBytes > LDS_BYTES) {
    fb::set_error("%s: frame too large for the LDS-staged matcher (%zu B + %zu B static > 160 KiB)", what, dynBytes, staticBytes);
    return FB_ERR_CAPACITY;
  }
  return FB_OK;
}

// The slack that the launchers have always added behind a kernel's arrays (kept, not tightened).
constexpr size_t M3_SLACK = 4 * 4, CLAIMS_U16_SLACK = 2 * 4, INIT_SLACK = 2 * 4, BOW_SLACK = 16, TRIANGULATION_SLACK = 16;

// a kernel's array at byte offset `off` of its dynamic LDS
template <typename E>
FB_HD inline E *lds_at(uint8_t *smem, size_t off) { return reinterpret_cast<E *>(smem + off); }

// ---- the staged target frame ------------------------------------------------------------------------------------------------
// LDS carve for a target frame of n keypoints / ncell cells. All offsets 16-B aligned.
struct Carve {
  size_t desc, xy, oct, cs, items, end;
  bool hasOct;
  // withDesc = false: the descriptor table stays in HBM/L2 (frames too large for LDS, e.g. the 2*nFeatures
  // initialisation extractor); only the key point positions, octaves and the grid are staged
  FB_HD Carve(int n, int ncell, bool withDesc = true, bool withOct = true) {
    hasOct = withOct;
    desc = 0;
    xy = up16(desc + (withDesc ? (size_t)n * 32 : 0));
    oct = up16(xy + (size_t)n * 8);
    cs = up16(oct + (withOct ? (size_t)n : 0));
    items = up16(cs + (size_t)(ncell + 1) * 2);
    end = up16(items + (size_t)n * 4);
  }
};

// ---- a kernel's own arrays, behind the staged frame (`at` = Carve::end, or the end of a bare descriptor table) -------------
// Each function fills the offsets and returns the total: the dynamic LDS bytes of the launch.

// M3 (k_proj_frame, k_frame_tail_front)
struct M3Lds {
  size_t owners;   // int [2][cur_stride]
  size_t cache;    // uint32 [last_stride][cacheK]  dist << 16 | idx
  size_t assigns;  // u16 [2][last_stride]
  size_t perm;     // u16 [last_stride] queries sorted by octave (processing order)
  size_t meta;     // u8 [last_stride] cached count | complete << 7
};
FB_HD inline size_t m3_layout(M3Lds &L, size_t at, int cur_stride, int last_stride, int cacheK) {
  L.owners = at;
  L.cache = L.owners + (size_t)2 * cur_stride * 4;
  L.assigns = L.cache + (size_t)last_stride * cacheK * 4;
  L.perm = L.assigns + (size_t)2 * last_stride * 2;
  L.meta = L.perm + (size_t)last_stride * 2;
  return L.meta + (size_t)last_stride * 2 + M3_SLACK;  // (a byte per query is used; the launchers have always counted two)
}

// The users of fb::Claims: M4 (k_proj_kf) and k_proj_sim3 with 16-bit assignments, M2 (k_proj_points, k_m2_resolve) and BoW
// (k_match_bow_t, which also keeps F's feature-vector items) with 32-bit ones.  fb::commit_matches puts the match array over
// this round's owner array and the histogram bins over this round's assign array.
struct ClaimsLds {
  size_t owners;   // int [2][tStride]
  size_t assigns;  // AT [2][qStride]
  size_t fitems;   // int [fitemStride] (BoW)
};
FB_HD inline size_t claims_layout(ClaimsLds &L, size_t at, int tStride, int qStride, int assignBytes, size_t slack, int fitemStride = 0) {
  L.owners = at;
  L.assigns = L.owners + (size_t)2 * tStride * 4;
  L.fitems = L.assigns + (size_t)2 * qStride * assignBytes;
  return L.fitems + (size_t)fitemStride * 4 + slack;
}
FB_HD inline size_t bow_layout(ClaimsLds &L, bool descInLds, int f_stride, int kf_items, int f_items) {  // descriptor table at 0
  return claims_layout(L, descInLds ? (size_t)f_stride * 32 : 0, f_stride, kf_items, 4, BOW_SLACK, f_items);
}

// M9 (k_bird_mappoints, k_frame_tail_bird); in the tail the camera positions lie over the grid scratch, which is dead by then
struct BirdLds {
  size_t writer;  // int [cur_stride]
  size_t cam;     // float [cur_stride][3] (the tail, when camInLds)
};
FB_HD inline size_t bird_layout(BirdLds &L, size_t at, int cur_stride, bool camInLds) {
  L.writer = at;
  L.cam = L.writer + (size_t)cur_stride * 4;
  return L.cam + (camInLds ? (size_t)cur_stride * 12 : 0);
}

// M8 (k_birdview)
struct BirdviewLds { size_t m12, bins; };  // int [ref_stride] each
FB_HD inline size_t birdview_layout(BirdviewLds &L, size_t at, int ref_stride) {
  L.m12 = at;
  L.bins = L.m12 + (size_t)ref_stride * 4;
  return L.bins + (size_t)ref_stride * 4;
}

// k_sim3: both key frames are staged in turn inside the carve of the larger one; the two match arrays lie behind it
struct Sim3Lds { size_t match1, match2; };  // int [mp1 stride], int [mp2 stride]
FB_HD inline size_t sim3_layout(Sim3Lds &L, size_t at, int mp1_stride, int mp2_stride) {
  L.match1 = at;
  L.match2 = L.match1 + (size_t)mp1_stride * 4;
  return L.match2 + (size_t)mp2_stride * 4;
}

// k_init_match: the A and B side of every array swap each round; the commit reuses the B side (last over headB, bins over nextB)
struct InitLds {
  size_t headA, headB;                                      // int [f2_stride]
  size_t nextA, nextB, assignA, assignB, distA, distB;      // u16 [f1_stride]
};
FB_HD inline size_t init_layout(InitLds &L, size_t at, int f1_stride, int f2_stride) {
  const size_t q = (size_t)f1_stride * 2;
  L.headA = at;
  L.headB = L.headA + (size_t)f2_stride * 4;
  L.nextA = L.headB + (size_t)f2_stride * 4;
  L.nextB = L.nextA + q;
  L.assignA = L.nextB + q;
  L.assignB = L.assignA + q;
  L.distA = L.assignB + q;
  L.distB = L.distA + q;
  return L.distB + q + INIT_SLACK;
}

// k_match_triangulation: no grid, the descriptor table of KF2 (when in LDS) at 0
struct TriangulationLds {
  size_t k2;    // float4 [kf2_stride] x, y, angle, octave
  size_t m12;   // int [kf1_stride]
  size_t bins;  // int [kf1_stride]
};
FB_HD inline size_t triangulation_layout(TriangulationLds &L, bool descInLds, int kf1_stride, int kf2_stride) {
  L.k2 = descInLds ? (size_t)kf2_stride * 32 : 0;
  L.m12 = L.k2 + (size_t)kf2_stride * 16;
  L.bins = L.m12 + (size_t)kf1_stride * 4;
  return L.bins + (size_t)kf1_stride * 4 + TRIANGULATION_SLACK;
}

// k_fuse_search and k_m2_candidates have no arrays of their own: their layout is the Carve, their total Carve::end.

// AssignFeaturesToGrid (k_grid_build at 0; the two tail kernels at Carve::end, under the matcher's own arrays, which are first
// written after the grid has been staged)
struct GridLds {
  size_t cnt;    // int [ncell + 1]
  size_t fillp;  // int [ncell]
  size_t items;  // int [kp_stride] when itemsInLds
};
FB_HD inline size_t grid_layout(GridLds &L, size_t at, int ncell, int kp_stride, bool itemsInLds) {
  L.cnt = at;
  L.fillp = L.cnt + (size_t)(ncell + 1) * 4;
  L.items = L.fillp + (size_t)ncell * 4;
  return L.items + (itemsInLds ? (size_t)kp_stride * 4 : 0);
}

// ---- the launchers' decisions ----------------------------------------------------------------------------------------------

// The descriptor-table fallback: the table goes to LDS when the whole plan fits the budget, otherwise it stays in HBM / L2.
// total(withDesc) = the kernel's dynamic bytes with and without the table.
struct DescPlan { int descInLds; size_t bytes; };
template <typename Total>
inline int plan_desc(Total &&total, size_t staticBytes, const char *what, DescPlan *p) {
  p->descInLds = 1;
  p->bytes = total(true);
  if (p->bytes > LDS_BUDGET) { p->descInLds = 0; p->bytes = total(false); }
  return check_lds(p->bytes, staticBytes, what);
}
// ... for a kernel with `own` bytes behind a staged frame (own(at) = total of its layout function)
template <typename Own>
inline int plan_staged(int stride, int ncell, Own &&own, size_t staticBytes, const char *what, DescPlan *p) {
  return plan_desc([&](bool withDesc) { return own(Carve(stride, ncell, withDesc).end); }, staticBytes, what, p);
}

// AssignFeaturesToGrid: the items are scattered and sorted in LDS when they fit
struct GridPlan { int itemsInLds; size_t bytes; };
inline GridPlan plan_grid(size_t at, int ncell, int kp_stride) {
  GridLds L;
  GridPlan g{1, grid_layout(L, at, ncell, kp_stride, true)};
  if (g.bytes > LDS_BUDGET) { g.itemsInLds = 0; g.bytes = grid_layout(L, at, ncell, kp_stride, false); }
  return g;
}

// The M3 ladder: descriptors in LDS + cache, descriptors in LDS, cache only, neither.  noCache: the FB_M3_NO_CACHE switch.
// (The last rung is not checked here: the caller's check_lds() is, on its final byte count.)
constexpr int CACHE_K = 4;
struct M3Plan { int cacheK, descInLds; size_t bytes; };
inline M3Plan plan_m3_ladder(int cur_stride, int last_stride, int ncell, bool noCache) {
  M3Lds L;
  auto total = [&](bool withDesc, int cacheK) {
    return m3_layout(L, Carve(cur_stride, ncell, withDesc, false).end, cur_stride, last_stride, cacheK);
  };
  M3Plan p{noCache ? 0 : CACHE_K, 1, 0};
  p.bytes = total(true, p.cacheK);
  if (p.bytes > LDS_BUDGET) { p.cacheK = 0; p.bytes = total(true, 0); }
  if (p.bytes > LDS_BUDGET) { p.cacheK = CACHE_K; p.descInLds = 0; p.bytes = total(false, CACHE_K); }
  if (p.bytes > LDS_BUDGET) { p.cacheK = 0; p.bytes = total(false, 0); }
  return p;
}
inline int plan_m3(int cur_stride, int last_stride, int ncell, bool noCache, const char *what, M3Plan *p) {
  *p = plan_m3_ladder(cur_stride, last_stride, ncell, noCache);
  return check_lds(p->bytes, STATIC_M3, what);
}

// k_frame_tail_front: the M3 ladder; the grid scratch overlays the matcher's arrays and may be the larger of the two
struct TailFrontPlan { int cacheK, descInLds, itemsInLds; size_t bytes; };
inline int plan_tail_front(int cur_stride, int last_stride, int ncell, bool noCache, const char *what, TailFrontPlan *p) {
  const M3Plan m = plan_m3_ladder(cur_stride, last_stride, ncell, noCache);
  const GridPlan g = plan_grid(Carve(cur_stride, ncell, m.descInLds != 0, false).end, ncell, cur_stride);
  *p = TailFrontPlan{m.cacheK, m.descInLds, g.itemsInLds, g.bytes > m.bytes ? g.bytes : m.bytes};
  return check_lds(p->bytes, STATIC_TAIL_FRONT, what);
}

// k_frame_tail_bird: writer array + the camera positions in LDS when they fit beside the staged frame with its descriptors,
// else the plan of k_bird_mappoints; the grid scratch as in the front tail
struct TailBirdPlan { int descInLds, itemsInLds, camInLds; size_t bytes; };
inline int plan_tail_bird(int cur_stride, int ncell, const char *what, TailBirdPlan *p) {
  BirdLds L;
  DescPlan d{1, bird_layout(L, Carve(cur_stride, ncell, true).end, cur_stride, true)};
  int camInLds = 1;
  if (d.bytes > LDS_BUDGET) {
    camInLds = 0;
    const int rc = plan_staged(cur_stride, ncell, [&](size_t at) { return bird_layout(L, at, cur_stride, false); }, STATIC_TAIL_BIRD, what, &d);
    if (rc != FB_OK) return rc;
  }
  const GridPlan g = plan_grid(Carve(cur_stride, ncell, d.descInLds != 0).end, ncell, cur_stride);
  *p = TailBirdPlan{d.descInLds, g.itemsInLds, camInLds, g.bytes > d.bytes ? g.bytes : d.bytes};
  return check_lds(p->bytes, STATIC_TAIL_BIRD, what);
}

// M2: two phases (candidate lists by many workgroups, k_m2_candidates; the serial rule on the lists, k_m2_resolve; neither
// stages descriptors) when the caller gave a workspace and the resolve kernel fits, else the one-kernel version
struct M2Plan { int twoPhase, descInLds; size_t candBytes, bytes; };
inline int plan_m2(int cur_stride, int mp_stride, int ncell, bool haveWorkspace, const char *what, M2Plan *p) {
  ClaimsLds L;
  auto own = [&](size_t at) { return claims_layout(L, at, cur_stride, mp_stride, 4, 0); };
  p->candBytes = Carve(cur_stride, ncell, false).end;
  p->bytes = own(p->candBytes);
  p->descInLds = 0;
  p->twoPhase = haveWorkspace && p->bytes <= LDS_BUDGET;
  if (p->twoPhase) return FB_OK;
  DescPlan d;
  const int rc = plan_staged(cur_stride, ncell, own, STATIC_M2, what, &d);
  p->descInLds = d.descInLds;
  p->bytes = d.bytes;
  return rc;
}

}  // namespace
#endif
