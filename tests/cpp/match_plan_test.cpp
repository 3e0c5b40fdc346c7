// The matchers' LDS plan (fishbirdeyevisualslam_amd/csrc/match_plan.h) on the CPU.
// Sweep: target stride x query stride x ncell {front 64x48, bird 32x32, 1} x {cache, FB_M3_NO_CACHE}.  Per case and kernel
// family: every region starts at a multiple of its element's alignment (16 B for what is read as uint4 / float4), ends inside
// the launch's bytes, overlaps no region that is live with it, and the documented overlays (grid scratch over the matcher's
// arrays in the tails, commit_matches / k_init_match's commit on the B arrays, the camera copy over the dead grid scratch) are
// exactly those; variant and bytes equal the launchers' formulas of commit 4374f82, restated literally below (that list is
// the specification), except in the two windows that the plan closes on purpose:
//   W1  dynamic bytes <= 160 KiB < dynamic + the kernel's static LDS: launched before, FB_ERR_CAPACITY now
//   W2  fb_match_initialization, descriptors-in-LDS bytes in (160 KiB - 512, 160 KiB]: now descriptors in HBM
// Then the named cases: one concrete shape per variant, and one per window.
// usage: match_plan_test   -> prints "cases=<n> failures=<n>", exit status 1 if failures > 0
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../fishbirdeyevisualslam_amd/csrc/match_plan.h"

namespace fb {
void set_error(const char *, ...) {}
}

static long g_failures = 0, g_cases = 0;
#define CHECK(cond, ...)                                                 \
  do {                                                                   \
    if (!(cond)) {                                                       \
      if (g_failures++ < 30) {                                           \
        std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);  \
        std::printf(__VA_ARGS__);                                        \
        std::printf("\n");                                               \
      }                                                                  \
    }                                                                    \
  } while (0)

// ---- the launchers of commit 4374f82 (match.hip, match_kf.inc, match_bow.hip), literally ---------------------------------
static size_t old_up(size_t v) { return (v + 15) & ~(size_t)15; }
static size_t old_carve_end(int n, int ncell, bool withDesc = true, bool withOct = true) {
  size_t desc = 0;
  size_t xy = old_up(desc + (withDesc ? (size_t)n * 32 : 0));
  size_t oct = old_up(xy + (size_t)n * 8);
  size_t cs = old_up(oct + (withOct ? (size_t)n : 0));
  size_t items = old_up(cs + (size_t)(ncell + 1) * 2);
  return old_up(items + (size_t)n * 4);
}
static size_t old_match_lds_bytes(int cur_stride, int ncell, int extra_ints, bool withDesc = true, bool withOct = true) {
  return old_carve_end(cur_stride, ncell, withDesc, withOct) + (size_t)extra_ints * 4;
}
static const size_t OLD_LDS_BUDGET = 160 * 1024 - 512;
static const int OLD_CACHE_K = 4;
static int old_check_lds(size_t bytes) { return bytes > 160 * 1024 ? FB_ERR_CAPACITY : FB_OK; }
struct OldPlan { size_t bytes; int descInLds, rc; };
static OldPlan old_plan_lds(int cur_stride, int ncell, int extra_ints) {
  OldPlan p;
  p.descInLds = 1;
  p.bytes = old_carve_end(cur_stride, ncell, true) + (size_t)extra_ints * 4;
  if (p.bytes > OLD_LDS_BUDGET) {
    p.descInLds = 0;
    p.bytes = old_carve_end(cur_stride, ncell, false) + (size_t)extra_ints * 4;
  }
  p.rc = old_check_lds(p.bytes);
  return p;
}
static size_t old_grid_lds_ints(int ncell, int kp_stride, bool itemsInLds) {
  return (size_t)(2 * ncell + 1) + (itemsInLds ? (size_t)kp_stride : 0);
}
struct OldM3 { size_t lds; int cacheK, descInLds, itemsInLds, rc; };
static OldM3 old_m3(int cur_stride, int last_stride, int ncell, bool noCache, bool tail) {
  const int base_ints = 2 * cur_stride + 2 * last_stride + 4;
  int cacheK = noCache ? 0 : OLD_CACHE_K, descInLds = 1;
  size_t lds = old_match_lds_bytes(cur_stride, ncell, base_ints + cacheK * last_stride, true, false);
  if (lds > OLD_LDS_BUDGET) { cacheK = 0; lds = old_match_lds_bytes(cur_stride, ncell, base_ints, true, false); }
  if (lds > OLD_LDS_BUDGET) { cacheK = OLD_CACHE_K; descInLds = 0; lds = old_match_lds_bytes(cur_stride, ncell, base_ints + cacheK * last_stride, false, false); }
  if (lds > OLD_LDS_BUDGET) { cacheK = 0; lds = old_match_lds_bytes(cur_stride, ncell, base_ints, false, false); }
  int itemsInLds = 1;
  if (tail) {
    const size_t staged = old_carve_end(cur_stride, ncell, descInLds != 0, false);
    size_t gridLds = staged + old_grid_lds_ints(ncell, cur_stride, true) * 4;
    if (gridLds > OLD_LDS_BUDGET) { itemsInLds = 0; gridLds = staged + old_grid_lds_ints(ncell, cur_stride, false) * 4; }
    if (gridLds > lds) lds = gridLds;
  }
  return OldM3{lds, cacheK, descInLds, itemsInLds, old_check_lds(lds)};
}
struct OldTailBird { size_t lds; int descInLds, itemsInLds, camInLds, rc; };
static OldTailBird old_tail_bird(int cur_stride, int ncell) {
  int camInLds = 1;
  OldPlan lp;
  lp.descInLds = 1;
  lp.bytes = old_carve_end(cur_stride, ncell, true) + (size_t)cur_stride * 16;
  if (lp.bytes > OLD_LDS_BUDGET) {
    camInLds = 0;
    lp = old_plan_lds(cur_stride, ncell, cur_stride);
    if (lp.rc != FB_OK) return OldTailBird{lp.bytes, lp.descInLds, 1, 0, lp.rc};
  }
  const size_t staged = old_carve_end(cur_stride, ncell, lp.descInLds != 0);
  int itemsInLds = 1;
  size_t gridLds = staged + old_grid_lds_ints(ncell, cur_stride, true) * 4;
  if (gridLds > OLD_LDS_BUDGET) { itemsInLds = 0; gridLds = staged + old_grid_lds_ints(ncell, cur_stride, false) * 4; }
  size_t lds = lp.bytes > gridLds ? lp.bytes : gridLds;
  return OldTailBird{lds, lp.descInLds, itemsInLds, camInLds, old_check_lds(lds)};
}
struct OldGrid { size_t lds; int itemsInLds, rc; };
static OldGrid old_grid(int ncell, int kp_stride) {
  size_t lds = (size_t)(2 * ncell + 1) * 4 + (size_t)kp_stride * 4;
  int itemsInLds = 1;
  if (lds > OLD_LDS_BUDGET) { itemsInLds = 0; lds = (size_t)(2 * ncell + 1) * 4; }
  return OldGrid{lds, itemsInLds, old_check_lds(lds)};
}
struct OldM2 { int twoPhase, descInLds, rc; size_t ldsA, lds; };
static OldM2 old_m2(int cur_stride, int mp_stride, int ncell, bool haveWorkspace) {
  if (haveWorkspace) {
    const size_t ldsA = old_carve_end(cur_stride, ncell, false);
    const size_t ldsB = ldsA + ((size_t)2 * cur_stride + (size_t)2 * mp_stride) * 4;
    if (ldsB <= OLD_LDS_BUDGET) return OldM2{1, 0, FB_OK, ldsA, ldsB};
  }
  const OldPlan lp = old_plan_lds(cur_stride, ncell, 2 * cur_stride + 2 * mp_stride);
  return OldM2{0, lp.descInLds, lp.rc, 0, lp.bytes};
}
static OldPlan old_init(int f1_stride, int f2_stride, int ncell) {
  const int extra = 2 * f2_stride + 3 * f1_stride + 2;
  size_t lds = old_match_lds_bytes(f2_stride, ncell, extra);
  const int descInLds = lds <= 160 * 1024;
  if (!descInLds) lds = old_match_lds_bytes(f2_stride, ncell, extra, false);
  return OldPlan{lds, descInLds, old_check_lds(lds)};
}
static OldPlan old_bow(int f_stride, int kf_items, int f_items) {
  size_t lds = (size_t)f_stride * 32 + (size_t)f_stride * 8 + (size_t)kf_items * 8 + (size_t)f_items * 4 + 16;
  const int descInLds = lds <= 160 * 1024 - 512;
  if (!descInLds) lds -= (size_t)f_stride * 32;
  return OldPlan{lds, descInLds, old_check_lds(lds)};
}
static OldPlan old_triangulation(int kf1_stride, int kf2_stride) {
  size_t lds = (size_t)kf2_stride * 48 + (size_t)kf1_stride * 8 + 16;
  const int descInLds = lds <= 160 * 1024 - 512;
  if (!descInLds) lds -= (size_t)kf2_stride * 32;
  return OldPlan{lds, descInLds, old_check_lds(lds)};
}

// ---- regions ---------------------------------------------------------------------------------------------------------------
struct Reg { const char *name; size_t off, bytes, align; };
static bool overlap(const Reg &a, const Reg &b) { return a.bytes && b.bytes && a.off < b.off + b.bytes && b.off < a.off + a.bytes; }
static bool inside(const Reg &a, const Reg &host) { return a.off >= host.off && a.off + a.bytes <= host.off + host.bytes; }
// aligned, inside [0, total), pairwise disjoint
static void check_regions(const char *tag, const char *what, const std::vector<Reg> &R, size_t total) {
  for (size_t i = 0; i < R.size(); i++) {
    CHECK(R[i].off % R[i].align == 0, "%s: %s.%s at %zu, alignment %zu", tag, what, R[i].name, R[i].off, R[i].align);
    CHECK(R[i].off + R[i].bytes <= total, "%s: %s.%s is [%zu, +%zu) of %zu", tag, what, R[i].name, R[i].off, R[i].bytes, total);
    for (size_t j = 0; j < i; j++) CHECK(!overlap(R[i], R[j]), "%s: %s.%s and .%s overlap", tag, what, R[j].name, R[i].name);
  }
}
static std::vector<Reg> carve_regions(const Carve &cv, int n, int ncell, bool withDesc) {
  std::vector<Reg> R;
  R.push_back(Reg{"desc", cv.desc, withDesc ? (size_t)n * 32 : 0, 16});
  R.push_back(Reg{"xy", cv.xy, (size_t)n * 8, 16});
  R.push_back(Reg{"oct", cv.oct, cv.hasOct ? (size_t)n : 0, 16});
  R.push_back(Reg{"cs", cv.cs, (size_t)(ncell + 1) * 2, 16});
  R.push_back(Reg{"items", cv.items, (size_t)n * 4, 16});
  return R;
}
static void add(std::vector<Reg> &R, const std::vector<Reg> &more) { R.insert(R.end(), more.begin(), more.end()); }
// the grid scratch of a tail kernel: behind the staged frame, inside the launch, starting where the matcher's arrays start
static void check_tail_grid(const char *tag, const char *what, const Carve &cv, int n, int ncell, bool withDesc, bool itemsInLds, size_t total,
                            size_t ownStart) {
  GridLds G;
  const size_t gEnd = grid_layout(G, cv.end, ncell, n, itemsInLds);
  std::vector<Reg> R = carve_regions(cv, n, ncell, withDesc);
  add(R, {Reg{"grid.cnt", G.cnt, (size_t)(ncell + 1) * 4, 4}, Reg{"grid.fillp", G.fillp, (size_t)ncell * 4, 4},
          Reg{"grid.items", G.items, itemsInLds ? (size_t)n * 4 : 0, 4}});
  check_regions(tag, what, R, total);
  CHECK(gEnd <= total && G.cnt == ownStart && G.cnt == cv.end, "%s: %s: grid scratch [%zu, %zu), own arrays at %zu, %zu bytes", tag, what, G.cnt, gEnd, ownStart, total);
}

// what the parent decided against what the plan decides; the two windows
static bool in_w1(int oldRc, size_t oldBytes, size_t staticBytes) { return oldRc == FB_OK && oldBytes + staticBytes > LDS_BYTES; }
static void check_desc_plan(const char *tag, const char *what, const OldPlan &o, int rc, const DescPlan &p, size_t staticBytes) {
  CHECK(p.descInLds == o.descInLds && p.bytes == o.bytes, "%s: %s: descInLds %d / %zu B, the parent had %d / %zu B", tag, what, p.descInLds, p.bytes, o.descInLds, o.bytes);
  const int want = in_w1(o.rc, o.bytes, staticBytes) ? FB_ERR_CAPACITY : o.rc;
  CHECK(rc == want, "%s: %s: rc %d, expected %d (%zu B + %zu static)", tag, what, rc, want, o.bytes, staticBytes);
}

static void claims_regions(const char *tag, const char *what, const Carve &cv, int T, int ncell, bool withDesc, int Q, int assignBytes, size_t slack,
                           size_t total) {
  ClaimsLds L;
  const size_t t = claims_layout(L, cv.end, T, Q, assignBytes, slack);
  CHECK(t == total, "%s: %s: layout total %zu, plan %zu", tag, what, t, total);
  std::vector<Reg> R = carve_regions(cv, T, ncell, withDesc);
  const Reg owners{"owners", L.owners, (size_t)2 * T * 4, 4}, assigns{"assigns", L.assigns, (size_t)2 * Q * assignBytes, (size_t)assignBytes};
  add(R, {owners, assigns});
  check_regions(tag, what, R, total);
  // fb::commit_matches: the match array is this round's owner array, the bins this round's assign array (either half)
  for (int half = 0; half < 2; half++) {
    const Reg matchL{"matchL", L.owners + (size_t)half * T * 4, (size_t)T * 4, 4}, binQ{"binQ", L.assigns + (size_t)half * Q * assignBytes, (size_t)Q * assignBytes, 2};
    CHECK(inside(matchL, owners) && inside(binQ, assigns), "%s: %s: commit overlay leaves its arrays", tag, what);
  }
}

static void check_case(int T, int Q, int ncell, bool noCache) {
  char tag[128];
  std::snprintf(tag, sizeof(tag), "T=%d Q=%d ncell=%d noCache=%d", T, Q, ncell, (int)noCache);
  g_cases++;
  // the staged frame itself
  for (int v = 0; v < 4; v++) {
    const bool wd = v & 1, wo = v & 2;
    const Carve cv(T, ncell, wd, wo);
    check_regions(tag, "carve", carve_regions(cv, T, ncell, wd), cv.end);
    CHECK(cv.end % 16 == 0 && cv.end == old_carve_end(T, ncell, wd, wo), "%s: carve end %zu", tag, cv.end);
  }
  {  // M3 and the front tail
    const OldM3 o = old_m3(T, Q, ncell, noCache, false);
    M3Plan p;
    const int rc = plan_m3(T, Q, ncell, noCache, "m3", &p);
    CHECK(p.cacheK == o.cacheK && p.descInLds == o.descInLds && p.bytes == o.lds, "%s: M3 %d/%d/%zu, parent %d/%d/%zu", tag, p.cacheK, p.descInLds, p.bytes, o.cacheK, o.descInLds, o.lds);
    CHECK(rc == (in_w1(o.rc, o.lds, STATIC_M3) ? FB_ERR_CAPACITY : o.rc), "%s: M3 rc %d", tag, rc);
    const OldM3 ot = old_m3(T, Q, ncell, noCache, true);
    TailFrontPlan tp;
    const int rct = plan_tail_front(T, Q, ncell, noCache, "tail", &tp);
    CHECK(tp.cacheK == ot.cacheK && tp.descInLds == ot.descInLds && tp.itemsInLds == ot.itemsInLds && tp.bytes == ot.lds,
          "%s: front tail %d/%d/%d/%zu, parent %d/%d/%d/%zu", tag, tp.cacheK, tp.descInLds, tp.itemsInLds, tp.bytes, ot.cacheK, ot.descInLds, ot.itemsInLds, ot.lds);
    CHECK(rct == (in_w1(ot.rc, ot.lds, STATIC_TAIL_FRONT) ? FB_ERR_CAPACITY : ot.rc), "%s: front tail rc %d", tag, rct);
    const Carve cv(T, ncell, p.descInLds != 0, false);
    M3Lds L;
    const size_t total = m3_layout(L, cv.end, T, Q, p.cacheK);
    CHECK(total == p.bytes && total <= tp.bytes, "%s: M3 layout total %zu, plan %zu, tail %zu", tag, total, p.bytes, tp.bytes);
    std::vector<Reg> R = carve_regions(cv, T, ncell, p.descInLds != 0);
    const Reg owners{"owners", L.owners, (size_t)2 * T * 4, 4}, assigns{"assigns", L.assigns, (size_t)2 * Q * 2, 2};
    add(R, {owners, Reg{"cache", L.cache, (size_t)Q * p.cacheK * 4, 4}, assigns, Reg{"perm", L.perm, (size_t)Q * 2, 2}, Reg{"meta", L.meta, (size_t)Q, 1}});
    check_regions(tag, "M3", R, total);
    for (int half = 0; half < 2; half++) {
      const Reg matchL{"matchL", L.owners + (size_t)half * T * 4, (size_t)T * 4, 4}, binQ{"binQ", L.assigns + (size_t)half * Q * 2, (size_t)Q * 2, 2};
      CHECK(inside(matchL, owners) && inside(binQ, assigns), "%s: M3: commit overlay leaves its arrays", tag);
    }
    check_tail_grid(tag, "front tail grid", cv, T, ncell, tp.descInLds != 0, tp.itemsInLds != 0, tp.bytes, L.owners);
  }
  {  // the Claims users behind a staged frame: M4 / k_proj_sim3 (u16), M2 in one kernel and in two phases (int)
    const OldPlan o4 = old_plan_lds(T, ncell, 2 * T + Q + 2);
    DescPlan p4;
    ClaimsLds L;
    const int rc4 = plan_staged(T, ncell, [&](size_t at) { return claims_layout(L, at, T, Q, 2, CLAIMS_U16_SLACK); }, STATIC_M4, "m4", &p4);
    check_desc_plan(tag, "M4", o4, rc4, p4, STATIC_M4);
    claims_regions(tag, "M4", Carve(T, ncell, p4.descInLds != 0), T, ncell, p4.descInLds != 0, Q, 2, CLAIMS_U16_SLACK, p4.bytes);
    DescPlan ps;
    const int rcs = plan_staged(T, ncell, [&](size_t at) { return claims_layout(L, at, T, Q, 2, CLAIMS_U16_SLACK); }, STATIC_PROJ_SIM3, "proj_sim3", &ps);
    check_desc_plan(tag, "k_proj_sim3", o4, rcs, ps, STATIC_PROJ_SIM3);
    for (int ws = 0; ws < 2; ws++) {
      const OldM2 o2 = old_m2(T, Q, ncell, ws != 0);
      M2Plan p2;
      const int rc2 = plan_m2(T, Q, ncell, ws != 0, "m2", &p2);
      CHECK(p2.twoPhase == o2.twoPhase && p2.descInLds == o2.descInLds && p2.bytes == o2.lds && (!o2.twoPhase || p2.candBytes == o2.ldsA),
            "%s: M2 ws=%d: %d/%d/%zu/%zu, parent %d/%d/%zu/%zu", tag, ws, p2.twoPhase, p2.descInLds, p2.candBytes, p2.bytes, o2.twoPhase, o2.descInLds, o2.ldsA, o2.lds);
      CHECK(rc2 == (in_w1(o2.rc, o2.lds, STATIC_M2) ? FB_ERR_CAPACITY : o2.rc), "%s: M2 ws=%d rc %d", tag, ws, rc2);
      claims_regions(tag, "M2", Carve(T, ncell, p2.descInLds != 0), T, ncell, p2.descInLds != 0, Q, 4, 0, p2.bytes);
      if (p2.twoPhase) CHECK(p2.candBytes == Carve(T, ncell, false).end && p2.candBytes <= LDS_BUDGET, "%s: k_m2_candidates %zu B", tag, p2.candBytes);
    }
  }
  {  // M9 and the bird tail
    const OldPlan o = old_plan_lds(T, ncell, T);
    DescPlan p;
    BirdLds L;
    const int rc = plan_staged(T, ncell, [&](size_t at) { return bird_layout(L, at, T, false); }, STATIC_BIRD_MP, "m9", &p);
    check_desc_plan(tag, "M9", o, rc, p, STATIC_BIRD_MP);
    {
      const Carve cv(T, ncell, p.descInLds != 0);
      std::vector<Reg> R = carve_regions(cv, T, ncell, p.descInLds != 0);
      CHECK(bird_layout(L, cv.end, T, false) == p.bytes, "%s: M9 layout total", tag);
      add(R, {Reg{"writer", L.writer, (size_t)T * 4, 4}});
      check_regions(tag, "M9", R, p.bytes);
    }
    const OldTailBird ot = old_tail_bird(T, ncell);
    TailBirdPlan tp{0, 1, 0, 0};
    const int rct = plan_tail_bird(T, ncell, "tail", &tp);
    if (ot.rc == FB_OK || rct == FB_OK) {
      CHECK(tp.descInLds == ot.descInLds && tp.itemsInLds == ot.itemsInLds && tp.camInLds == ot.camInLds && tp.bytes == ot.lds,
            "%s: bird tail %d/%d/%d/%zu, parent %d/%d/%d/%zu", tag, tp.descInLds, tp.itemsInLds, tp.camInLds, tp.bytes, ot.descInLds, ot.itemsInLds, ot.camInLds, ot.lds);
      CHECK(rct == (in_w1(ot.rc, ot.lds, STATIC_TAIL_BIRD) ? FB_ERR_CAPACITY : ot.rc), "%s: bird tail rc %d", tag, rct);
      const Carve cv(T, ncell, tp.descInLds != 0);
      const size_t own = bird_layout(L, cv.end, T, tp.camInLds != 0);
      CHECK(own <= tp.bytes, "%s: bird tail: own arrays end at %zu of %zu", tag, own, tp.bytes);
      std::vector<Reg> R = carve_regions(cv, T, ncell, tp.descInLds != 0);
      const Reg cam{"cam", L.cam, tp.camInLds ? (size_t)T * 12 : 0, 4};
      add(R, {Reg{"writer", L.writer, (size_t)T * 4, 4}, cam});
      check_regions(tag, "bird tail", R, tp.bytes);
      check_tail_grid(tag, "bird tail grid", cv, T, ncell, tp.descInLds != 0, tp.itemsInLds != 0, tp.bytes, L.writer);
      // the camera copy is written after the grid scratch has died; it lies behind the staged frame, never inside it
      CHECK(cam.off >= cv.end, "%s: bird tail: cam at %zu inside the staged frame (%zu)", tag, cam.off, cv.end);
    } else {
      CHECK(rct == ot.rc, "%s: bird tail rc %d, parent %d", tag, rct, ot.rc);
    }
  }
  {  // M8
    const OldPlan o = old_plan_lds(T, ncell, 2 * Q);
    DescPlan p;
    BirdviewLds L;
    const int rc = plan_staged(T, ncell, [&](size_t at) { return birdview_layout(L, at, Q); }, STATIC_BIRDVIEW, "m8", &p);
    check_desc_plan(tag, "M8", o, rc, p, STATIC_BIRDVIEW);
    const Carve cv(T, ncell, p.descInLds != 0);
    birdview_layout(L, cv.end, Q);
    std::vector<Reg> R = carve_regions(cv, T, ncell, p.descInLds != 0);
    add(R, {Reg{"m12", L.m12, (size_t)Q * 4, 4}, Reg{"bins", L.bins, (size_t)Q * 4, 4}});
    check_regions(tag, "M8", R, p.bytes);
  }
  {  // k_sim3: key frames of stride T and (T + 1) / 2, both staged inside the carve of the larger
    const int T2 = (T + 1) / 2, nc2 = ncell > 1 ? ncell / 2 : 1, Q2 = Q / 2;
    const OldPlan o = old_plan_lds(T, ncell, Q + Q2);
    DescPlan p;
    Sim3Lds L;
    const int rc = plan_staged(T, ncell, [&](size_t at) { return sim3_layout(L, at, Q, Q2); }, STATIC_SIM3, "sim3", &p);
    check_desc_plan(tag, "k_sim3", o, rc, p, STATIC_SIM3);
    const Carve cv(T, ncell, p.descInLds != 0), cv2(T2, nc2, p.descInLds != 0);
    sim3_layout(L, cv.end, Q, Q2);
    CHECK(cv2.end <= cv.end, "%s: k_sim3: the smaller key frame ends at %zu, the carve at %zu", tag, cv2.end, cv.end);
    for (const Carve *c : {&cv, &cv2}) {
      std::vector<Reg> R = carve_regions(*c, c == &cv ? T : T2, c == &cv ? ncell : nc2, p.descInLds != 0);
      add(R, {Reg{"match1", L.match1, (size_t)Q * 4, 4}, Reg{"match2", L.match2, (size_t)Q2 * 4, 4}});
      check_regions(tag, "k_sim3", R, p.bytes);
    }
  }
  {  // k_init_match: target T, queries Q
    const OldPlan o = old_init(Q, T, ncell);
    DescPlan p;
    InitLds L;
    const int rc = plan_staged(T, ncell, [&](size_t at) { return init_layout(L, at, Q, T); }, STATIC_INIT, "init", &p);
    const size_t with = old_match_lds_bytes(T, ncell, 2 * T + 3 * Q + 2);
    if (with > LDS_BUDGET && with <= LDS_BYTES) {  // W2
      const size_t without = old_match_lds_bytes(T, ncell, 2 * T + 3 * Q + 2, false);
      CHECK(o.descInLds == 1 && p.descInLds == 0 && p.bytes == without && rc == FB_OK, "%s: k_init_match in W2: %d / %zu / rc %d", tag, p.descInLds, p.bytes, rc);
    } else {
      check_desc_plan(tag, "k_init_match", o, rc, p, STATIC_INIT);
    }
    const Carve cv(T, ncell, p.descInLds != 0);
    init_layout(L, cv.end, Q, T);
    std::vector<Reg> R = carve_regions(cv, T, ncell, p.descInLds != 0);
    const Reg headB{"headB", L.headB, (size_t)T * 4, 4}, nextB{"nextB", L.nextB, (size_t)Q * 2, 2};
    add(R, {Reg{"headA", L.headA, (size_t)T * 4, 4}, headB, Reg{"nextA", L.nextA, (size_t)Q * 2, 2}, nextB, Reg{"assignA", L.assignA, (size_t)Q * 2, 2},
            Reg{"assignB", L.assignB, (size_t)Q * 2, 2}, Reg{"distA", L.distA, (size_t)Q * 2, 2}, Reg{"distB", L.distB, (size_t)Q * 2, 2}});
    check_regions(tag, "k_init_match", R, p.bytes);
    // its commit: `last` is a head array, `bins` a next array (which of the two the rounds left as B)
    const Reg last{"last", L.headB, (size_t)T * 4, 4}, bins{"bins", L.nextB, (size_t)Q * 2, 2};
    CHECK(inside(last, headB) && inside(bins, nextB), "%s: k_init_match: commit overlay", tag);
  }
  {  // k_fuse_search: the staged frame alone
    const OldPlan o = old_plan_lds(T, ncell, 0);
    DescPlan p;
    const int rc = plan_staged(T, ncell, [](size_t at) { return at; }, STATIC_FUSE, "fuse", &p);
    check_desc_plan(tag, "k_fuse_search", o, rc, p, STATIC_FUSE);
    CHECK(p.bytes == Carve(T, ncell, p.descInLds != 0).end, "%s: k_fuse_search %zu B", tag, p.bytes);
  }
  {  // BoW: candidate side T (all of them in its feature vector), Q query items; triangulation: KF2 = T, KF1 = Q
    const OldPlan o = old_bow(T, Q, T);
    DescPlan p;
    ClaimsLds L;
    const int rc = plan_desc([&](bool wd) { return bow_layout(L, wd, T, Q, T); }, STATIC_BOW, "bow", &p);
    check_desc_plan(tag, "BoW", o, rc, p, STATIC_BOW);
    CHECK(bow_layout(L, p.descInLds != 0, T, Q, T) == p.bytes, "%s: BoW layout total", tag);
    const Reg owners{"owners", L.owners, (size_t)2 * T * 4, 4}, assigns{"assigns", L.assigns, (size_t)2 * Q * 4, 4};
    check_regions(tag, "BoW", {Reg{"desc", 0, p.descInLds ? (size_t)T * 32 : 0, 16}, owners, assigns, Reg{"fitems", L.fitems, (size_t)T * 4, 4}}, p.bytes);
    const OldPlan ot = old_triangulation(Q, T);
    DescPlan pt;
    TriangulationLds Lt;
    const int rct = plan_desc([&](bool wd) { return triangulation_layout(Lt, wd, Q, T); }, STATIC_TRIANGULATION, "tri", &pt);
    check_desc_plan(tag, "triangulation", ot, rct, pt, STATIC_TRIANGULATION);
    triangulation_layout(Lt, pt.descInLds != 0, Q, T);
    check_regions(tag, "triangulation", {Reg{"desc", 0, pt.descInLds ? (size_t)T * 32 : 0, 16}, Reg{"k2", Lt.k2, (size_t)T * 16, 16},
                                         Reg{"m12", Lt.m12, (size_t)Q * 4, 4}, Reg{"bins", Lt.bins, (size_t)Q * 4, 4}}, pt.bytes);
  }
  {  // k_grid_build
    const OldGrid o = old_grid(ncell, T);
    const GridPlan g = plan_grid(0, ncell, T);
    CHECK(g.itemsInLds == o.itemsInLds && g.bytes == o.lds, "%s: grid %d/%zu, parent %d/%zu", tag, g.itemsInLds, g.bytes, o.itemsInLds, o.lds);
    CHECK(check_lds(g.bytes, STATIC_GRID, "grid") == (in_w1(o.rc, o.lds, STATIC_GRID) ? FB_ERR_CAPACITY : o.rc), "%s: grid rc", tag);
    GridLds L;
    grid_layout(L, 0, ncell, T, g.itemsInLds != 0);
    check_regions(tag, "grid", {Reg{"cnt", L.cnt, (size_t)(ncell + 1) * 4, 4}, Reg{"fillp", L.fillp, (size_t)ncell * 4, 4},
                                Reg{"items", L.items, g.itemsInLds ? (size_t)T * 4 : 0, 4}}, g.bytes);
  }
}

// ---- named cases: one concrete shape per variant (computed from the parent's formulas), one per window --------------------
static const int FRONT = 64 * 48, BIRD = 32 * 32;
static void named_m3(const char *name, int cur, int last, int cacheK, int descInLds) {
  g_cases++;
  M3Plan p;
  const int rc = plan_m3(cur, last, FRONT, false, name, &p);
  const OldM3 o = old_m3(cur, last, FRONT, false, false);
  CHECK(rc == FB_OK && p.cacheK == cacheK && p.descInLds == descInLds, "%s: rc %d cacheK %d descInLds %d", name, rc, p.cacheK, p.descInLds);
  CHECK(o.cacheK == cacheK && o.descInLds == descInLds && o.lds == p.bytes, "%s: the parent had %d/%d/%zu", name, o.cacheK, o.descInLds, o.lds);
}
template <typename Plan, typename Old>
static void named_desc(const char *name, Plan plan, Old old, int descInLds) {
  g_cases++;
  DescPlan p;
  const int rc = plan(&p);
  const OldPlan o = old();
  CHECK(rc == FB_OK && p.descInLds == descInLds && o.descInLds == descInLds && o.bytes == p.bytes && o.rc == FB_OK,
        "%s: rc %d descInLds %d %zu B, parent %d %zu B", name, rc, p.descInLds, p.bytes, o.descInLds, o.bytes);
}

static void named_cases() {
  named_m3("M3 rung 1 (the bench: 2064 / 2064)", 2064, 2064, CACHE_K, 1);
  named_m3("M3 rung 2 (2000 / 2400)", 2000, 2400, 0, 1);
  named_m3("M3 rung 3 (3200 / 2900)", 3200, 2900, CACHE_K, 0);
  named_m3("M3 rung 4 (5000 / 4700)", 5000, 4700, 0, 0);
  {
    g_cases++;
    TailFrontPlan p;
    const int rc = plan_tail_front(2064, 2064, FRONT, false, "front tail, bench", &p);
    CHECK(rc == FB_OK && p.cacheK == CACHE_K && p.descInLds == 1 && p.itemsInLds == 1, "front tail at the bench's shape: %d/%d/%d", p.cacheK, p.descInLds, p.itemsInLds);
    g_cases++;
    const int rc0 = plan_tail_front(2800, 1400, FRONT, false, "front tail, items in HBM", &p);
    const OldM3 o = old_m3(2800, 1400, FRONT, false, true);
    CHECK(rc0 == FB_OK && p.itemsInLds == 0 && o.itemsInLds == 0 && o.rc == FB_OK && p.bytes == o.lds && p.descInLds == o.descInLds && p.cacheK == o.cacheK,
          "front tail 2800 / 1400: itemsInLds %d (parent %d), %zu B", p.itemsInLds, o.itemsInLds, p.bytes);
  }
  {  // bird tail: everything in LDS at the bench's bird stride; camera copy and items out of LDS at the pinned large shapes
    g_cases++;
    TailBirdPlan p;
    int rc = plan_tail_bird(2064, BIRD, "bird tail, bench", &p);
    CHECK(rc == FB_OK && p.descInLds == 1 && p.itemsInLds == 1 && p.camInLds == 1, "bird tail 2064: %d/%d/%d", p.descInLds, p.itemsInLds, p.camInLds);
    g_cases++;
    rc = plan_tail_bird(3000, BIRD, "bird tail, cam in HBM", &p);
    OldTailBird o = old_tail_bird(3000, BIRD);
    CHECK(rc == FB_OK && p.camInLds == 0 && p.descInLds == 1 && o.camInLds == 0 && o.descInLds == 1 && o.itemsInLds == p.itemsInLds && o.lds == p.bytes,
          "bird tail 3000: cam %d desc %d items %d", p.camInLds, p.descInLds, p.itemsInLds);
    g_cases++;
    rc = plan_tail_bird(3200, BIRD, "bird tail, items in HBM", &p);
    o = old_tail_bird(3200, BIRD);
    CHECK(rc == FB_OK && p.camInLds == 0 && p.itemsInLds == 0 && o.camInLds == 0 && o.itemsInLds == 0 && o.descInLds == p.descInLds && o.lds == p.bytes,
          "bird tail 3200: cam %d desc %d items %d", p.camInLds, p.descInLds, p.itemsInLds);
  }
  // both sides of descInLds
  for (int side = 1; side >= 0; side--) {
    const int T = side ? 2000 : 4000;
    named_desc(side ? "BoW 2000: descriptors in LDS" : "BoW 4000: descriptors in HBM",
               [&](DescPlan *p) { ClaimsLds L; return plan_desc([&](bool wd) { return bow_layout(L, wd, T, T, T); }, STATIC_BOW, "bow", p); },
               [&]() { return old_bow(T, T, T); }, side);
    named_desc(side ? "triangulation 2000: LDS" : "triangulation 4000: HBM",
               [&](DescPlan *p) { TriangulationLds L; return plan_desc([&](bool wd) { return triangulation_layout(L, wd, T, T); }, STATIC_TRIANGULATION, "tri", p); },
               [&]() { return old_triangulation(T, T); }, side);
    named_desc(side ? "k_sim3 2000: LDS" : "k_sim3 4000: HBM",
               [&](DescPlan *p) { Sim3Lds L; return plan_staged(T, FRONT, [&](size_t at) { return sim3_layout(L, at, T, T); }, STATIC_SIM3, "sim3", p); },
               [&]() { return old_plan_lds(T, FRONT, 2 * T); }, side);
    named_desc(side ? "k_init_match 2000: LDS" : "k_init_match 4000: HBM",
               [&](DescPlan *p) { InitLds L; return plan_staged(T, FRONT, [&](size_t at) { return init_layout(L, at, T, T); }, STATIC_INIT, "init", p); },
               [&]() { return old_init(T, T, FRONT); }, side);
    named_desc(side ? "k_fuse_search 2000: LDS" : "k_fuse_search 4000: HBM",
               [&](DescPlan *p) { return plan_staged(T, FRONT, [](size_t at) { return at; }, STATIC_FUSE, "fuse", p); },
               [&]() { return old_plan_lds(T, FRONT, 0); }, side);
  }
  {  // W1: the last rung of M3 between 160 KiB - static and 160 KiB.  cur 5000 on the front grid; the bytes grow by 8 per query.
    g_cases++;
    int found = -1;
    for (int last = 0; last < 20000 && found < 0; last++) {
      const OldM3 o = old_m3(5000, last, FRONT, false, false);
      if (o.rc == FB_OK && o.lds + STATIC_M3 > LDS_BYTES) found = last;
    }
    CHECK(found > 0, "no M3 shape in window W1");
    M3Plan p;
    const int rc = plan_m3(5000, found, FRONT, false, "W1", &p);
    const OldM3 o = old_m3(5000, found, FRONT, false, false);
    CHECK(rc == FB_ERR_CAPACITY && p.cacheK == 0 && p.descInLds == 0 && p.bytes == o.lds && o.rc == FB_OK && p.bytes <= LDS_BYTES && p.bytes > LDS_BUDGET,
          "W1 at 5000 / %d: rc %d, %zu B", found, rc, p.bytes);
    M3Plan q;  // one query fewer than the first refused shape is still launched
    CHECK(plan_m3(5000, found - 1, FRONT, false, "W1-", &q) == FB_OK, "W1: 5000 / %d refused", found - 1);
  }
  {  // W2: k_init_match with descriptors-in-LDS bytes in (160 KiB - 512, 160 KiB]: f2 = 2800 on the front grid, 6 B per query
    g_cases++;
    int found = -1;
    for (int f1 = 1; f1 < 20000 && found < 0; f1++) {
      const size_t with = old_match_lds_bytes(2800, FRONT, 2 * 2800 + 3 * f1 + 2);
      if (with > LDS_BUDGET && with <= LDS_BYTES) found = f1;
    }
    CHECK(found > 0, "no k_init_match shape in window W2");
    DescPlan p;
    InitLds L;
    const int rc = plan_staged(2800, FRONT, [&](size_t at) { return init_layout(L, at, found, 2800); }, STATIC_INIT, "W2", &p);
    const OldPlan o = old_init(found, 2800, FRONT);
    CHECK(rc == FB_OK && o.descInLds == 1 && p.descInLds == 0 && p.bytes == old_match_lds_bytes(2800, FRONT, 2 * 2800 + 3 * found + 2, false),
          "W2 at f2 2800 / f1 %d: rc %d descInLds %d (parent %d)", found, rc, p.descInLds, o.descInLds);
  }
}

int main() {
  const int targets[] = {1, 63, 64, 65, 1023, 1024, 1025, 2064, 2900, 3400, 4000, 8000, 65535};
  const int queries[] = {0, 1, 1024, 2400, 5000, 50000};
  const int cells[] = {FRONT, BIRD, 1};
  for (int T : targets)
    for (int Q : queries)
      for (int ncell : cells)
        for (int noCache = 0; noCache < 2; noCache++) check_case(T, Q, ncell, noCache != 0);
  named_cases();
  std::printf("cases=%ld failures=%ld\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
