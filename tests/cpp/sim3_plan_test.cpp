// The plan of the two Sim3 stages (fishbirdeyevisualslam_amd/csrc/sim3_plan.h) on the CPU.
// Sweep: KF1 stride {1, 63, 64, 65, 2363, 2364, 3402, 3403, 65535} x n_cand {1, 12, 64}, once per stage.  Per case the
// variant, the dynamic LDS bytes and the workspace bytes equal the formulas of sim3_solver.hip / opt_sim3.hip at commit
// 25eb33f, restated literally below (that list is the specification), and dynamic + static LDS fit the 160 KiB of a workgroup
// whenever the LDS variant is chosen.
// Keep rule: s3::keep_pair against the literal nested conditions of those two files and a hand-written expectation, on a
// table with one row per skip clause and the row just inside each bound.  The table's source also fails the test when it is
// asked for a value whose index has not been guarded.
// Workspace refusal: the four outcomes, with the message text.
// usage: sim3_plan_test   -> prints "cases=<n> failures=<n>", exit status 1 if failures > 0
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../fishbirdeyevisualslam_amd/csrc/sim3_plan.h"

static char g_error[256];
namespace fb {
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}
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

// ---- the launchers of commit 25eb33f, literally -------------------------------------------------------------------------------
static size_t old_up256(size_t v) { return (v + 255) & ~(size_t)255; }
// sim3_solver.hip:50-51, 437-438
static size_t old_solver_ws_bytes(int C, int s1) { return old_up256((size_t)C * 12 * s1 * 4); }
static size_t old_solver_lds(int s1) { return (size_t)s1 * 12 * 4; }
static bool old_solver_in_lds(int s1) { return old_solver_lds(s1) <= 160 * 1024 - 512; }
// opt_sim3.hip:40, 63-64, 418, 434, 451
static const size_t OLD_OPT_LDS_BUDGET = 160 * 1024 - 40 * 1024;
static size_t old_opt_ws_bytes(int C, int s1) { return old_up256((size_t)C * 13 * s1 * 4); }
static bool old_opt_fits_lds(int s1) { return (size_t)s1 * 13 * 4 <= OLD_OPT_LDS_BUDGET; }
static size_t old_opt_workspace(int C, int s1) { return old_opt_fits_lds(s1) ? 256 : old_opt_ws_bytes(C, s1); }
static size_t old_opt_lds(int s1) { return (size_t)s1 * 13 * 4; }

static void sweep() {
  const int strides[] = {1, 63, 64, 65, 2363, 2364, 3402, 3403, 65535};
  const int cands[] = {1, 12, 64};
  for (int s1 : strides)
    for (int C : cands) {
      {
        g_cases++;
        const s3::LdsPlan p = s3::plan_solver(s1);
        CHECK(p.inLds == old_solver_in_lds(s1), "solver s1 %d", s1);
        CHECK(p.bytes == (old_solver_in_lds(s1) ? old_solver_lds(s1) : 0), "solver s1 %d bytes %zu", s1, p.bytes);
        CHECK(s3::solver_workspace(C, s1) == old_solver_ws_bytes(C, s1), "solver workspace s1 %d C %d", s1, C);
        CHECK(!p.inLds || p.bytes + s3::STATIC_HYPOTHESES <= 160 * 1024, "solver s1 %d: %zu B beside the statics", s1, p.bytes);
        CHECK(p.inLds == (s1 <= 3402), "solver s1 %d: the threshold is 3402 features", s1);
      }
      {
        g_cases++;
        const s3::LdsPlan p = s3::plan_optimize(s1);
        CHECK(p.inLds == old_opt_fits_lds(s1), "optimize s1 %d", s1);
        CHECK(p.bytes == (old_opt_fits_lds(s1) ? old_opt_lds(s1) : 0), "optimize s1 %d bytes %zu", s1, p.bytes);
        CHECK(s3::optimize_workspace(C, s1) == old_opt_workspace(C, s1), "optimize workspace s1 %d C %d", s1, C);
        CHECK(!p.inLds || p.bytes + s3::STATIC_OPTIMIZE <= 160 * 1024, "optimize s1 %d: %zu B beside the statics", s1, p.bytes);
        CHECK(p.inLds == (s1 <= 2363), "optimize s1 %d: the threshold is 2363 features", s1);
      }
    }
  // the figures the documents quote
  CHECK(s3::STATIC_OPTIMIZE == 32816 && s3::STATIC_PREPARE == 16 && s3::STATIC_HYPOTHESES == 0, "static LDS figures");
  CHECK(s3::SOLVER_LDS_BUDGET == 160 * 1024 - 512 && s3::OPT_LDS_BUDGET == 160 * 1024 - 40 * 1024, "budgets");
}

// ---- the keep rule ---------------------------------------------------------------------------------------------------------------
constexpr int S1 = 40, S2 = 50, ML = FB_MAX_LEVELS;
struct Row { const char *what; int j, valid1, valid2, k1, k2, o1, o2; bool kept; };
static const Row ROWS[] = {
    {"a kept pair", 7, 1, 1, 3, 9, 2, 3, true},
    {"j = -1", -1, 1, 1, 3, 9, 2, 3, false},
    {"j = 0", 0, 1, 1, 3, 9, 2, 3, true},
    {"j = s2", S2, 1, 1, 3, 9, 2, 3, false},
    {"j = s2 - 1", S2 - 1, 1, 1, 3, 9, 2, 3, true},
    {"j = s1 (< s2)", S1, 1, 1, 3, 9, 2, 3, true},
    {"mp_valid 0 on side 1", 7, 0, 1, 3, 9, 2, 3, false},
    {"mp_valid 0 on side 2", 7, 1, 0, 3, 9, 2, 3, false},
    {"k1 = -1", 7, 1, 1, -1, 9, 2, 3, false},
    {"k1 = 0", 7, 1, 1, 0, 9, 2, 3, true},
    {"k2 = -1", 7, 1, 1, 3, -1, 2, 3, false},
    {"k2 = 0", 7, 1, 1, 3, 0, 2, 3, true},
    {"k1 = s1", 7, 1, 1, S1, 9, 2, 3, false},
    {"k1 = s1 - 1", 7, 1, 1, S1 - 1, 9, 2, 3, true},
    {"k2 = s2", 7, 1, 1, 3, S2, 2, 3, false},
    {"k2 = s2 - 1", 7, 1, 1, 3, S2 - 1, 2, 3, true},
    {"k2 = s1 (< s2)", 7, 1, 1, 3, S1, 2, 3, true},
    {"octave -1 on side 1", 7, 1, 1, 3, 9, -1, 3, false},
    {"octave 0 on side 1", 7, 1, 1, 3, 9, 0, 3, true},
    {"octave -1 on side 2", 7, 1, 1, 3, 9, 2, -1, false},
    {"octave 0 on side 2", 7, 1, 1, 3, 9, 2, 0, true},
    {"octave FB_MAX_LEVELS on side 1", 7, 1, 1, 3, 9, ML, 3, false},
    {"octave FB_MAX_LEVELS - 1 on side 1", 7, 1, 1, 3, 9, ML - 1, 3, true},
    {"octave FB_MAX_LEVELS on side 2", 7, 1, 1, 3, 9, 2, ML, false},
    {"octave FB_MAX_LEVELS - 1 on side 2", 7, 1, 1, 3, 9, 2, ML - 1, true},
};

// the conditions of k_sim3_prepare (sim3_solver.hip:78-86) and of the gather of k_optimize_sim3 (opt_sim3.hip:224-231) at
// commit 25eb33f, with the loads replaced by the row's values
static bool literal_keep(const Row &t, int s1, int s2) {
  bool keep = false;
  const int j = t.j;
  if (j >= 0 && j < s2 && t.valid1 && t.valid2) {
    const int k1 = t.k1, k2 = t.k2;
    if (k1 >= 0 && k2 >= 0 && k1 < s1 && k2 < s2) {
      const int o1 = t.o1, o2 = t.o2;
      keep = o1 >= 0 && o1 < FB_MAX_LEVELS && o2 >= 0 && o2 < FB_MAX_LEVELS;
    }
  }
  return keep;
}

// the row as the arrays the kernels read: a value is handed out only for an index inside its array
struct RowSrc {
  const Row *t;
  bool valid1() const { return t->valid1 != 0; }
  bool valid2(int j) const { CHECK(j >= 0 && j < S2, "%s: mp_valid of KF2 read at %d", t->what, j); return t->valid2 != 0; }
  int k1() const { return t->k1; }
  int k2(int j) const { CHECK(j >= 0 && j < S2, "%s: kf2_index read at %d", t->what, j); return t->k2; }
  int o1(int k) const { CHECK(k >= 0 && k < S1, "%s: key point of KF1 read at %d", t->what, k); return t->o1; }
  int o2(int k) const { CHECK(k >= 0 && k < S2, "%s: key point of KF2 read at %d", t->what, k); return t->o2; }
};

static void keep_rule() {
  for (const Row &t : ROWS) {
    g_cases++;
    int k1 = -7, k2 = -7, o1 = -7, o2 = -7;
    const bool got = s3::keep_pair(t.j, S1, S2, RowSrc{&t}, &k1, &k2, &o1, &o2);
    CHECK(got == t.kept, "%s: keep_pair says %d", t.what, (int)got);
    CHECK(literal_keep(t, S1, S2) == t.kept, "%s: the literal loop says %d", t.what, (int)!t.kept);
    if (got) CHECK(k1 == t.k1 && k2 == t.k2 && o1 == t.o1 && o2 == t.o2, "%s: the kept pair's indices and octaves", t.what);
  }
}

static void workspace_refusal() {
  alignas(16) static unsigned char buf[64];
  struct Case { const void *p; size_t bytes, need; int rc; } cases[] = {
      {buf, 48, 48, FB_OK}, {nullptr, 48, 48, FB_ERR_ARG}, {buf, 47, 48, FB_ERR_ARG}, {buf + 8, 48, 48, FB_ERR_ARG}};
  for (const Case &c : cases) {
    g_cases++;
    g_error[0] = 0;
    const int rc = s3::check_workspace("fb_x_dev", c.p, c.bytes, c.need);
    CHECK(rc == c.rc, "check_workspace -> %d", rc);
    CHECK(std::strcmp(g_error, c.rc == FB_OK ? "" : "fb_x_dev: workspace of 48 bytes (16-byte aligned) needed") == 0, "message '%s'", g_error);
  }
}

int main() {
  sweep();
  keep_rule();
  workspace_refusal();
  std::printf("cases=%ld failures=%ld\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
