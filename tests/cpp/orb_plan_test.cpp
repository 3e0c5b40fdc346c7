// The extractor's workspace plan (fishbirdeyevisualslam_amd/csrc/orb_plan.h) on the CPU: plan_orb() over a sweep of image
// sizes and pyramids.  Checks that the regions of one image never overlap or leave their stride, that the grid bases add up,
// that the LDS carves fit, that a refusal leaves the caller's plan byte for byte as it was, and the 640x480 known answers.
// usage: orb_plan_test   -> prints "cases=<n> refused=<n> failures=<n>", exit status 1 if failures > 0
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../fishbirdeyevisualslam_amd/csrc/orb_plan.h"

static std::string g_error;
namespace fb {
void set_error(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}
}  // namespace fb

static long g_failures = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      if (g_failures++ < 20) {                                \
        std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                             \
        std::printf("\n");                                    \
      }                                                       \
    }                                                         \
  } while (0)

struct Region { long long lo, hi; };

// every region inside [0, stride), no two overlapping
static void check_regions(const Region *r, int n, long long stride, const char *what, const char *tag) {
  for (int i = 0; i < n; i++) {
    CHECK(r[i].lo >= 0 && r[i].lo <= r[i].hi && r[i].hi <= stride, "%s: %s of level %d is [%lld, %lld), stride %lld", tag, what, i, r[i].lo, r[i].hi, stride);
    for (int j = 0; j < i; j++)
      CHECK(r[i].lo >= r[j].hi || r[j].lo >= r[i].hi || r[i].lo == r[i].hi || r[j].lo == r[j].hi, "%s: %s of levels %d and %d overlap", tag, what, j, i);
  }
}

static void check_plan(const OrbPlan &P, int w, int h, const char *tag) {
  const OrbK &K = P.K;
  const int nl = K.nlevels;
  Region pyr[FB_MAX_LEVELS], blur[FB_MAX_LEVELS], cand[FB_MAX_LEVELS], out[FB_MAX_LEVELS];
  int cells = 0, groups = 0, descWgs = 0, maxSlot = 0, maxPix = 0;
  CHECK(K.L[0].w == w && K.L[0].h == h, "%s: level 0 is %dx%d", tag, K.L[0].w, K.L[0].h);
  for (int l = 0; l < nl; l++) {
    const LevelInfo &L = K.L[l];
    const long long bytes = (long long)L.pitch * L.h;
    CHECK(L.w >= 1 && L.h >= 1 && L.pitch >= L.w && L.pitch % 64 == 0, "%s: level %d is %dx%d pitch %d", tag, l, L.w, L.h, L.pitch);
    pyr[l] = {L.off, L.off + (l > 0 ? bytes : 0)};  // level 0 is the caller's image
    blur[l] = {L.boff, L.boff + bytes};
    cand[l] = {L.candBase, L.candBase + L.candCap};
    out[l] = {L.outBase, (long long)L.outBase + L.outCap};
    const int nc = L.nCols * L.nRows;
    CHECK(L.candCap >= nc * L.slotCap, "%s: level %d candCap %d < %d cells x %d slots", tag, l, L.candCap, nc, L.slotCap);
    CHECK(L.slotCap >= ((L.wCell + 1) / 2) * ((L.hCell + 1) / 2), "%s: level %d slotCap %d", tag, l, L.slotCap);
    CHECK(L.wCell + 6 <= 65 && L.hCell + 6 <= 65, "%s: level %d cell %dx%d", tag, l, L.wCell, L.hCell);  // the FAST tile refusal is out of reach
    // the cells cover the detection area: the last cell's window ends at or beyond the border
    if (nc > 0) CHECK(L.nCols * L.wCell >= L.w - 2 * BORDER - 6 && L.nRows * L.hCell >= L.h - 2 * BORDER - 6, "%s: level %d cells do not cover the level", tag, l);
    CHECK(L.outCap >= L.N + 3 && L.outCap >= 4 * L.nIni && L.outCap + 4 <= P.maxNodes, "%s: level %d outCap %d (N %d, nIni %d, maxNodes %d)", tag, l, L.outCap, L.N, L.nIni, P.maxNodes);
    CHECK(K.cellBase[l] == cells && L.cellBase == cells, "%s: cellBase[%d] = %d / %d, expected %d", tag, l, K.cellBase[l], L.cellBase, cells);
    CHECK(K.grpBase[l] == groups, "%s: grpBase[%d] = %d, expected %d", tag, l, K.grpBase[l], groups);
    CHECK(K.descBase[l] == descWgs, "%s: descBase[%d] = %d, expected %d", tag, l, K.descBase[l], descWgs);
    CHECK(K.runBase[l] == L.outBase && K.runCap[l] == L.outCap, "%s: run of level %d", tag, l);
    CHECK(K.blurStrips[l] <= K.blurStrips[l + 1], "%s: blurStrips decrease at level %d", tag, l);
    cells += nc;
    groups += (nc + FAST_CPW - 1) / FAST_CPW;
    descWgs += (L.outCap + DESC_WPB * DESC_KPW - 1) / (DESC_WPB * DESC_KPW);
    maxSlot = std::max(maxSlot, nc ? L.slotCap : 0);
    maxPix = std::max(maxPix, nc ? L.wCell * L.hCell : 0);
    if (l == 0) continue;
    // the resize tables: 16-byte aligned, inside the packed block, taps inside the source level
    const LevelInfo &S = K.L[l - 1];
    const size_t n[4] = {(size_t)L.w * 4, (size_t)L.w * 4, (size_t)L.h * 4, (size_t)L.h * 4};
    for (int k = 0; k < 4; k++) CHECK(P.tabOff[l][k] % 16 == 0 && P.tabOff[l][k] + n[k] <= P.tabBytes.size() && (k == 0 && l == 1 ? true : P.tabOff[l][k] > 0), "%s: table %d of level %d at %zu of %zu", tag, k, l, P.tabOff[l][k], P.tabBytes.size());
    const int *xofs = reinterpret_cast<const int *>(P.tabBytes.data() + P.tabOff[l][0]);
    const int *yofs = reinterpret_cast<const int *>(P.tabBytes.data() + P.tabOff[l][2]);
    for (int x = 0; x < L.w; x++) CHECK(xofs[x] >= 0 && xofs[x] <= S.w - 1, "%s: xofs[%d] = %d of level %d", tag, x, xofs[x], l);
    for (int y = 0; y < L.h; y++) CHECK(yofs[y] >= -1 && yofs[y] <= S.h - 1, "%s: yofs[%d] = %d of level %d", tag, y, yofs[y], l);
    CHECK(!P.mergeOK[l] || P.rowsOK[l], "%s: level %d mergeOK without rowsOK", tag, l);
  }
  check_regions(pyr, nl, K.pyrStride, "pyramid", tag);
  check_regions(blur, nl, K.blurStride, "blurred pyramid", tag);
  check_regions(cand, nl, K.candStride, "candidates", tag);
  check_regions(out, nl, K.outStride, "level output", tag);
  CHECK(K.totalCells == cells && K.totalGroups == groups, "%s: totalCells %d / %d, totalGroups %d / %d", tag, K.totalCells, cells, K.totalGroups, groups);
  for (int l = nl; l <= FB_MAX_LEVELS; l++)
    CHECK(K.cellBase[l] == cells && K.grpBase[l] == groups && K.descBase[l] == descWgs, "%s: bases past the last level (%d)", tag, l);
  CHECK(P.octreeLds <= 160 * 1024 - 512, "%s: octreeLds %zu", tag, P.octreeLds);
  CHECK(P.octreeLds >= ((size_t)P.maxNodes * 45 + 16) && P.octreeLds >= 4 * ((size_t)cells / std::max(nl, 1)), "%s: octreeLds %zu for %d nodes", tag, P.octreeLds, P.maxNodes);
  // k_fast: the survivors overlay the tile, the lists hold every pixel of the largest cell
  CHECK(K.fastTP == 44 || K.fastTP == 56 || K.fastTP == FAST_MAX_TILE, "%s: fastTP %d", tag, K.fastTP);
  CHECK(K.fastMaxOut >= maxSlot && 4 * K.fastMaxOut <= K.fastTileBytes && K.fastMaxPix >= maxPix, "%s: k_fast carve %d %d %d", tag, K.fastTileBytes, K.fastMaxOut, K.fastMaxPix);
  CHECK(K.timers == nullptr && K.dbg == 0, "%s: timers / dbg are the commit's", tag);
  const OrbSizes z = P.sizes(3);
  CHECK(z.pyr >= 3 * (size_t)K.pyrStride && z.blur >= 3 * (size_t)K.blurStride && z.cand >= 3 * (size_t)K.candStride * 4 && z.nodeOf >= 3 * (size_t)K.candStride * 2 &&
            z.cellCount >= 3 * (size_t)cells * 4 && z.lvlOut >= 3 * (size_t)K.outStride * 4 && z.counts >= (size_t)(3 * nl * 2 + FB_MAX_LEVELS - nl) * 4,
        "%s: buffer sizes", tag);
}

static fb_orb_params params(int nfeatures, float scale, int nlevels) {
  fb_orb_params p;
  p.nfeatures = nfeatures; p.scale_factor = scale; p.nlevels = nlevels; p.ini_th_fast = 15; p.min_th_fast = 5;
  return p;
}

static long g_cases = 0, g_refused = 0;

static int run(const fb_orb_params &p, int w, int h, OrbPlan &P) {
  fb_orb_tables t;
  make_tables(p, t);
  char tag[96];
  std::snprintf(tag, sizeof(tag), "%dx%d nf=%d scale=%.3f nl=%d", w, h, p.nfeatures, (double)p.scale_factor, p.nlevels);
  g_error.clear();
  const int rc = plan_orb(p, t, w, h, 0, P);
  g_cases++;
  if (rc == FB_OK) check_plan(P, w, h, tag);
  else { g_refused++; CHECK(!g_error.empty(), "%s: refusal %d without a message", tag, rc); }
  return rc;
}

// a refusal returns `code` with `text` in its message and leaves a plan that was filled before exactly as it was
static void check_refusal(const fb_orb_params &p, int w, int h, int code, const char *text) {
  OrbPlan P;
  CHECK(run(params(2000, 1.2f, 8), 640, 480, P) == FB_OK, "640x480 is planned");
  std::vector<uint8_t> object(sizeof(OrbPlan)), tables = P.tabBytes;
  memcpy(object.data(), static_cast<const void *>(&P), sizeof(OrbPlan));
  const int rc = run(p, w, h, P);
  CHECK(rc == code && g_error.find(text) != std::string::npos, "%dx%d: expected %d \"%s\", got %d \"%s\"", w, h, code, text, rc, g_error.c_str());
  CHECK(memcmp(object.data(), static_cast<const void *>(&P), sizeof(OrbPlan)) == 0 && P.tabBytes == tables, "%dx%d: the refusal \"%s\" changed the plan", w, h, text);
}

static void known_answers() {
  const fb_orb_params p = params(2000, 1.2f, 8);
  fb_orb_tables t;
  make_tables(p, t);
  const int fpl[8] = {434, 362, 302, 251, 209, 175, 145, 122};
  const int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
  for (int i = 0; i < 8; i++) CHECK(t.features_per_level[i] == fpl[i], "features_per_level[%d] = %d", i, t.features_per_level[i]);
  for (int i = 0; i < 16; i++) CHECK(t.umax[i] == umax[i], "umax[%d] = %d", i, t.umax[i]);
  OrbPlan P;
  CHECK(run(p, 640, 480, P) == FB_OK, "640x480 is planned");
  CHECK(P.K.capOut == 2064 && P.K.kpStride == 2064 && capacity_of(p) == 2064, "capOut %d", P.K.capOut);
  for (int i = 0; i < 16; i++) CHECK(P.K.umax[i] == umax[i], "K.umax[%d] = %d", i, P.K.umax[i]);
  for (int i = 0; i < 8; i++) CHECK(P.K.L[i].N == fpl[i], "L[%d].N = %d", i, P.K.L[i].N);
  CHECK(P.K.L[1].w == 533 && P.K.L[1].h == 400 && P.K.L[7].w == 179 && P.K.L[7].h == 134, "levels 1 and 7 are %dx%d and %dx%d", P.K.L[1].w, P.K.L[1].h, P.K.L[7].w, P.K.L[7].h);
  CHECK(P.K.L[0].nCols == 20 && P.K.L[0].nRows == 14, "level 0 has %dx%d cells", P.K.L[0].nCols, P.K.L[0].nRows);  // 608 / 30, 448 / 30
  fb_orb_tables t2 = t;
  OrbPlan Q;
  CHECK(plan_orb(p, t2, 640, 480, 4096, Q) == FB_OK && Q.K.kpStride == 4096 && Q.K.capOut == 2064, "an output stride of 4096 gives kpStride %d", Q.K.kpStride);
}

// Which resize kernel may build each level >= 1 of the constructed image cases (tests/orb_image_cases.py), for an aligned
// source: g = not rowsOK (k_resize), r = rowsOK without mergeOK (k_resize_rows), m = mergeOK (k_resize_merge).  The same
// literals are held to the numpy restatement by tests/test_orb_image_cases.py, so orb_plan.h and the model answer to one list.
struct RouteRow { int w, h; float scale; int nlevels; const char *routes; };
static const RouteRow ROUTE_TABLE[] = {
    {131, 77, 1.25f, 3, "mm"},
    {131, 77, 1.26f, 3, "mm"},
    {131, 77, 1.3f, 3, "rr"},
    {131, 77, 2.0f, 3, "rr"},
    {131, 77, 2.01f, 3, "rr"},
    {131, 77, 2.5f, 3, "gg"},
    {131, 77, 3.0f, 3, "gg"},
    {131, 77, 4.0f, 2, "g"},
    {128, 96, 1.3334f, 2, "m"},
    {131, 77, 1.3f, 4, "rrr"},
    {64, 51, 1.25f, 8, "mmmmmmm"},
    {64, 45, 1.25f, 7, "mmmmmm"},
    {64, 48, 1.25f, 7, "mmmmmm"},
    {64, 56, 1.2f, 2, "m"},
    {64, 57, 1.2f, 2, "m"},
    {64, 59, 1.2f, 2, "m"},
    {45, 188, 2.25f, 5, "gggr"},
    {64, 67, 2.0f, 4, "rrr"},
    {64, 69, 2.0f, 4, "rrr"},
    {64, 46, 1.5f, 2, "r"},
    {64, 48, 1.5f, 2, "r"},
    {64, 49, 1.5f, 2, "r"},
    {100, 80, 2.0f, 7, "rrgmmm"},
    {100, 80, 2.0f, 8, "rrgmmmm"},
    {48, 64, 1.2f, 2, "m"},
    {49, 64, 1.2f, 2, "m"},
    {45, 64, 1.2f, 2, "m"},
    {47, 64, 1.2f, 2, "m"},
    {48, 64, 1.5f, 2, "r"},
    {49, 64, 1.5f, 2, "r"},
    {45, 64, 1.5f, 2, "r"},
    {46, 64, 1.5f, 2, "r"},
    {49, 64, 2.5f, 2, "g"},
    {52, 64, 2.5f, 2, "g"},
    {45, 64, 2.5f, 2, "g"},
    {47, 64, 2.5f, 2, "g"},
    {45, 48, 1.2f, 3, "mm"},
    {46, 48, 1.2f, 3, "mm"},
    {47, 48, 1.2f, 3, "mm"},
    {48, 48, 1.2f, 3, "mm"},
    {49, 48, 1.2f, 3, "mm"},
    {50, 48, 1.2f, 3, "mm"},
    {51, 48, 1.2f, 3, "mm"},
    {52, 48, 1.2f, 3, "mm"},
    {56, 48, 1.2f, 3, "mm"},
    {60, 48, 1.2f, 3, "mm"},
    {64, 48, 1.2f, 3, "mm"},
    {72, 48, 1.2f, 3, "mm"},
    {76, 48, 1.2f, 3, "mm"},
    {513, 45, 1.2f, 2, "m"},
    {64, 48, 1.2f, 2, "m"},
    {260, 45, 1.2f, 2, "m"},
    {50, 47, 1.5f, 2, "r"},
    {51, 46, 2.0f, 2, "r"},
    {45, 45, 1.2f, 1, ""},
    {46, 45, 1.2f, 1, ""},
    {47, 45, 1.2f, 1, ""},
    {48, 45, 1.2f, 1, ""},
    {49, 45, 1.2f, 1, ""},
    {50, 45, 1.2f, 1, ""},
    {51, 45, 1.2f, 1, ""},
    {52, 45, 1.2f, 1, ""},
    {255, 45, 1.2f, 1, ""},
    {256, 45, 1.2f, 1, ""},
    {257, 45, 1.2f, 1, ""},
    {258, 45, 1.2f, 1, ""},
    {259, 45, 1.2f, 1, ""},
    {260, 45, 1.2f, 1, ""},
    {263, 45, 1.2f, 1, ""},
    {264, 45, 1.2f, 1, ""},
    {511, 45, 1.2f, 1, ""},
    {512, 45, 1.2f, 1, ""},
    {513, 45, 1.2f, 1, ""},
    {48, 63, 1.2f, 1, ""},
    {48, 64, 1.2f, 1, ""},
    {48, 65, 1.2f, 1, ""},
    {48, 66, 1.2f, 1, ""},
    {48, 67, 1.2f, 1, ""},
    {48, 70, 1.2f, 1, ""},
    {48, 95, 1.2f, 1, ""},
    {48, 96, 1.2f, 1, ""},
    {48, 97, 1.2f, 1, ""},
    {45, 45, 1.027f, 8, "mmmmmmm"},
    {64, 52, 1.2f, 4, "mmm"},
    {132, 77, 1.25f, 3, "mm"},
    {132, 77, 2.0f, 3, "rr"},
    {132, 77, 2.5f, 3, "gg"},
};

static void route_table() {
  for (const RouteRow &r : ROUTE_TABLE) {
    OrbPlan P;
    if (run(params(300, r.scale, r.nlevels), r.w, r.h, P) != FB_OK) { CHECK(false, "%dx%d scale %.4f is refused", r.w, r.h, (double)r.scale); continue; }
    CHECK((int)strlen(r.routes) == r.nlevels - 1, "%dx%d scale %.4f: %zu routes for %d levels", r.w, r.h, (double)r.scale, strlen(r.routes), r.nlevels);
    for (int l = 1; l < r.nlevels; l++) {
      const char got = P.mergeOK[l] ? 'm' : P.rowsOK[l] ? 'r' : 'g';
      CHECK(got == r.routes[l - 1], "%dx%d scale %.4f level %d (%dx%d): plan says %c, table %c", r.w, r.h, (double)r.scale, l, P.K.L[l].w, P.K.L[l].h, got, r.routes[l - 1]);
    }
  }
}

int main() {
  OrbPlan P;
  // the sizes and parameter sets of the GPU tests
  const int sizes[][2] = {{640, 480}, {1280, 720}, {512, 512}, {333, 207}, {400, 300}, {320, 240}, {800, 600}, {3840, 2160}, {100, 80}, {501, 431}, {200, 160}, {256, 192}, {4095, 4095}, {45, 45}};
  for (const auto &s : sizes) {
    run(params(2000, 1.2f, 8), s[0], s[1], P);
    run(params(4000, 1.2f, 8), s[0], s[1], P);
    run(params(300, 1.2f, 4), s[0], s[1], P);
    run(params(1200, 1.5f, 5), s[0], s[1], P);
    run(params(800, 2.0f, 4), s[0], s[1], P);
    run(params(1500, 1.1f, 8), s[0], s[1], P);
    run(params(500, 2.0f, 7), s[0], s[1], P);
    for (int nf : {2363, 2660, 2700, 3000}) run(params(nf, 1.759f, 1), s[0], s[1], P);
  }
  // widths and heights through 45 .. 700 at four scale factors, 1 .. 8 levels
  const float scales[] = {1.1f, 1.2f, 1.5f, 2.0f};
  for (int w = 45; w <= 700; w += 41)
    for (int h = 45; h <= 700; h += 59)
      for (float sc : scales)
        for (int nl = 1; nl <= 8; nl++) run(params(1000, sc, nl), w, h, P);
  CHECK(g_refused > 0 && g_refused < g_cases / 2, "%ld of %ld cases refused", g_refused, g_cases);
  // The refusals that geometry reaches.  (The FAST tile refusal is not among them: a level has one cell per 30 px of its
  // detection area, so a cell is at most 59 px wide, which check_plan asserts for every level of the sweep.)
  check_refusal(params(500, 2.0f, 8), 60, 50, FB_ERR_ARG, "is empty");
  check_refusal(params(2000, 1.2f, 8), 4096, 100, FB_ERR_ARG, "image too large");
  check_refusal(params(2000, 1.2f, 8), 100, 4096, FB_ERR_ARG, "limit 4095");
  check_refusal(params(60000, 1.2f, 1), 640, 480, FB_ERR_CAPACITY, "nfeatures too large for the LDS quadtree");
  check_refusal(params(3000, 1.759f, 1), 501, 431, FB_ERR_CAPACITY, "nfeatures too large for the LDS quadtree");
  known_answers();
  route_table();
  std::printf("cases=%ld refused=%ld failures=%ld\n", g_cases, g_refused, g_failures);
  return g_failures ? 1 : 0;
}
