// The plan of the bundle adjustment (fishbirdeyevisualslam_amd/csrc/ba_plan.h) on the CPU.
// Sweep: free key frames {0, 1, 2, 21, 22, 23, 24, 42, 43, 682} x points {0, 1, 15, 16, 17, 100, 4096} x odometry edges
// {0, 1, 103, 104, 246, 247} x world {1, 2} x nwg_cap {2, 256}.  Per case every figure of the plan equals the formulas of
// plan(), alloc_solver() and dev_lm_prepare() as ba_driver.inc had them before ba_plan.h, restated literally below (that list is
// the specification), and the invariants hold that launcher and kernels rely on: lmPerWg a multiple of CHUNK that covers the
// points, the chosen Schur variant's accumulator tiles, dynamic + static LDS within a workgroup's 160 KiB for every kernel on
// the chosen path, 256-byte aligned slots that do not overlap.  The same sweep shows which Schur variants are reachable.
// Then the old two-step odometry rule against the single rule at every edge count up to 1000, and the hand derivation of
// tests/ba_cases.py (NWG_CAP_FOR_CHUNKS = 2 at 100 points: lmPerWg = 64, two workgroups).
// usage: ba_plan_test   -> prints "cases=<n> failures=<n>", exit status 1 if failures > 0
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../fishbirdeyevisualslam_amd/csrc/ba_plan.h"

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

// ---- the driver before ba_plan.h, literally ------------------------------------------------------------------------------------
struct OldPlan {
  int P6, NT, rows, nLinBlocks, nUpdBlocks, nWg, lmPerWg;
  size_t schurLds, solveLds;
  bool big;
  int schurMaxT;  // 9 / 20 / 34
  size_t odomLds, linLds;
  bool linGlobal;
  int nLin256, linGrid, nS;
  int oH, oB, oS, oM, stride;
};
static const size_t OLD_ODOMLIN = 78 * 8;  // sizeof(OdomLin): double A[36], Bm[36], err[6]
static OldPlan old_plan(int np, int npt, int n_kf, int nO, int world, int nwg_env) {
  const int LIN_THREADS_ = 128, CHUNK_ = 16, KPAD_ = 50, POSE_PARTS_ = 4;
  OldPlan P;
  P.P6 = 6 * np;
  P.NT = (P.P6 + 1 + 15) / 16;
  P.rows = P.NT * 16;
  P.nLinBlocks = (npt + LIN_THREADS_ - 1) / LIN_THREADS_;
  P.nUpdBlocks = (4 * npt + n_kf + LIN_THREADS_ - 1) / LIN_THREADS_;
  P.nWg = std::min(nwg_env, std::max(1, (npt + CHUNK_ - 1) / CHUNK_));
  P.lmPerWg = ((npt + P.nWg - 1) / P.nWg + CHUNK_ - 1) / CHUNK_ * CHUNK_;
  P.nWg = std::max(1, (npt + P.lmPerWg - 1) / std::max(P.lmPerWg, 1));
  P.schurLds = (size_t)2 * P.rows * KPAD_ * 8;
  P.solveLds = ((size_t)(P.P6 + 1) * (P.P6 + 1) + (size_t)(P.P6 + 1) * 6 + 96 + P.P6 + 2) * 8;
  P.big = P.schurLds > 160 * 1024 || P.solveLds > 160 * 1024 || P.P6 + 1 > 256;
  P.schurMaxT = P.NT <= 8 ? 9 : (P.NT <= 12 ? 20 : 34);
  // alloc_solver, then dev_lm_prepare
  P.odomLds = (size_t)std::max(nO, 1) * OLD_ODOMLIN;
  bool olGlobal = false;
  if (P.odomLds > 150 * 1024) { olGlobal = true; P.odomLds = 0; }
  P.linLds = olGlobal ? 0 : P.odomLds + (size_t)std::max(nO, 1) * 108 * 8;
  P.linGlobal = olGlobal;
  if (!P.linGlobal && P.linLds > 150 * 1024) P.linGlobal = true;
  P.nS = P.rows * P.rows;
  P.nLin256 = (4 * npt + 255) / 256;
  P.linGrid = P.nLin256 + POSE_PARTS_ * np + 1;
  P.oH = np * POSE_PARTS_ * 27; P.oB = P.oH + P.P6 * P.P6; P.oS = P.oB + P.P6; P.oM = P.oS + 4; P.stride = P.oM + world;
  return P;
}
static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t devbuf(size_t n) { return up256(n ? n : 1); }  // fb::DevBuf::alloc takes at least one byte

struct Ext { const char *name; size_t off, want; };  // a slot and the bytes the old driver gave its array (0: not allocated)

static void one_case(int np, int npt, int nO, int world, int cap) {
  g_cases++;
  const int n_kf = np + 2, nE = 3 * npt, P6 = 6 * np;
  const bool sharded = world > 1;
  BADims d{};
  d.odom = true; d.n_kf = n_kf; d.n_mp = npt; d.npt = npt; d.nF = nE; d.nB = 0; d.nE = nE; d.nO = nO; d.nOAll = nO; d.np = np;
  const BAPlan P = plan(d, sharded, false, 0, world, cap);
  const OldPlan O = old_plan(np, npt, n_kf, nO, world, cap);
#define TAGF "np %d npt %d nO %d world %d cap %d"
#define TAGA np, npt, nO, world, cap
#define TAG TAGF, TAGA
  CHECK(P.P6 == O.P6 && P.NT == O.NT && P.rows == O.rows, TAG);
  CHECK(P.nLinBlocks == O.nLinBlocks && P.nUpdBlocks == O.nUpdBlocks, TAG);
  CHECK(P.nWg == O.nWg && P.lmPerWg == O.lmPerWg, TAG);
  CHECK(P.big == O.big, TAG);
  CHECK(P.schurLds == O.schurLds && P.solveLds == O.solveLds, TAG);
  CHECK(P.nS == O.nS && P.nLin256 == O.nLin256 && P.linGrid == O.linGrid, TAG);
  CHECK((P.odomHome == ODOM_HBM) == O.linGlobal, TAG);
  CHECK((P.odomHome == ODOM_LDS) == ((size_t)std::max(nO, 1) * 1488 <= LIN_LDS_BUDGET), TAG);
  if (!O.linGlobal) CHECK(P.linLds == O.linLds, TAG);
  else CHECK(P.linLds == 0, TAG);
  CHECK(P.xb.oH == O.oH && P.xb.oB == O.oB && P.xb.oS == O.oS && P.xb.oM == O.oM && P.xb.stride == O.stride, TAG);
  CHECK(P.anything == (nE + nO > 0 && (np > 0 || npt > 0)), TAG);
  // invariants
  CHECK(P.lmPerWg % CHUNK == 0 && (long long)P.nWg * P.lmPerWg >= npt && P.nWg >= 1 && P.nWg <= std::max(cap, 1), TAG);
  if (!P.big) {
    CHECK(np <= MAX_FREE_KF_LDS, TAG);
    CHECK(schur_maxt(P.schur) == O.schurMaxT, "the variant the old selection took: " TAGF, TAGA);
    CHECK((P.NT * (P.NT + 1) / 2 + 3) / 4 <= schur_maxt(P.schur), TAG);
    CHECK(P.schurLds + STATIC_SCHUR <= LDS_BYTES && P.solveLds + STATIC_SOLVE <= LDS_BYTES, TAG);
    const SolveLds s = solve_lds(P6);
    CHECK(s.A == 0 && s.Up == (size_t)(P6 + 1) * (P6 + 1) && s.fact2 == s.Up + (size_t)(P6 + 1) * 6 && s.rhs == s.fact2 + 96 &&
              s.bytes == (s.rhs + P6 + 2) * 8, TAG);
    const SchurLds y = schur_lds(P.rows);
    CHECK(y.Yp == 0 && y.Wp == (size_t)P.rows * KPAD && y.bytes == 2 * y.Wp * 8, TAG);
  } else {
    CHECK(np > MAX_FREE_KF_LDS, TAG);
    CHECK((size_t)P6 * 8 + STATIC_BIG_SOLVE <= LDS_BYTES && STATIC_BIG_PANEL <= LDS_BYTES && STATIC_BIG_UPDATE <= LDS_BYTES, TAG);
  }
  if (P.odomHome == ODOM_LDS) {
    CHECK(P.linLds + STATIC_LIN <= LDS_BYTES, TAG);
    CHECK((size_t)lin_lds_records(nO) * sizeof(OdomLin) + (size_t)lin_lds_records(nO) * ODOM_TMP_DOUBLES * 8 == P.linLds, TAG);
  }
  // the scratch block: every array the old driver allocated on its own, at the old size
  const ScratchLayout C = scratch_layout(P);
  const size_t nE1 = std::max(nE, 1), npt1 = std::max(npt, 1);
  std::vector<Ext> ext = {
      {"e_chi2", C.e_chi2.off, up256(nE1 * 8)}, {"pose1", C.pose1.off, up256((size_t)n_kf * 56)}, {"pt1", C.pt1.off, up256(3 * npt1 * 8)}};
  for (const auto &l : C.lin) {
    ext.push_back({"Hll", l.Hll.off, up256(9 * npt1 * 8)}); ext.push_back({"bl", l.bl.off, up256(3 * npt1 * 8)});
    ext.push_back({"W", l.W.off, up256(18 * nE1 * 8)});
    ext.push_back({"Hpp", l.Hpp.off, up256(std::max<size_t>((size_t)P6 * P6, 1) * 8)}); ext.push_back({"bp", l.bp.off, up256(std::max<size_t>(P6, 1) * 8)});
    ext.push_back({"chiPart", l.chiPart.off, up256((size_t)(2 * O.nLinBlocks + 2) * 8)});
    ext.push_back({"maxPart", l.maxPart.off, up256((size_t)(2 * O.nLinBlocks + 2) * 8)});
  }
  ext.push_back({"Dinv", C.Dinv.off, devbuf((size_t)npt * 9 * 8)});
  ext.push_back({"Spart", C.Spart.off, devbuf(O.big ? 8 : (size_t)O.nWg * O.rows * O.rows * 8)});
  ext.push_back({"xp", C.xp.off, devbuf((size_t)std::max(P6, 1) * 8)});
  ext.push_back({"ok", C.ok.off, devbuf(8)});
  ext.push_back({"scale", C.scale.off, devbuf((size_t)O.nUpdBlocks * 8)});
  ext.push_back({"xb", C.xb.off, devbuf((size_t)(sharded ? 4 : 2) * O.stride * 8)});
  ext.push_back({"ol", C.ol.off, O.linGlobal ? devbuf((size_t)std::max(nO, 1) * OLD_ODOMLIN) : 0});
  ext.push_back({"bigS", C.bigS.off, O.big ? devbuf((size_t)P6 * P6 * 8 + (size_t)P6 * 8) : 0});
  ext.push_back({"bigM", C.bigM.off, O.big ? devbuf((size_t)P6 * P6 * 8 + (size_t)P6 * 8) : 0});
  ext.push_back({"bigU", C.bigU.off, O.big ? devbuf((size_t)P6 * 48 * 8) : 0});
  ext.push_back({"ex", C.ex.off, sharded ? devbuf(((size_t)npt * 3 + nE + 1) * 8) : 0});
  ext.push_back({"flags", C.flags.off, devbuf(nE1)});
  ext.push_back({"kfT", C.kfT.off, devbuf((size_t)n_kf * 48)});
  ext.push_back({"ptOut", C.ptOut.off, devbuf(npt1 * 12)});
  for (size_t i = 0; i < ext.size(); i++) {  // in carving order: aligned, and each slot ends where the next begins
    const size_t end = i + 1 < ext.size() ? ext[i + 1].off : C.bytes;
    CHECK(ext[i].off % 256 == 0, "%s: " TAGF, ext[i].name, TAGA);
    CHECK(end >= ext[i].off && end - ext[i].off == ext[i].want, "%s holds %zu, the old driver gave %zu: " TAGF, ext[i].name, end - ext[i].off, ext[i].want, TAGA);
  }
  // the staged graph: aligned, ascending, the header first
  const GraphLayout G = graph_layout(d);
  const size_t go[] = {G.poseIdx.off, G.fixed.off, G.o_i.off, G.o_j.off, G.o_Zinv.off, G.o_info.off, G.od_start.off, G.od_edges.off, G.ctl.off,
                       G.abort.off, G.lm_start.off, G.ps_start.off, G.e_pt.off, G.e_kf.off, G.e_pj.off, G.e_type.off, G.e_level.off, G.e_meas.off,
                       G.e_info.off, G.lm_edges.off, G.ps_edges.off, G.poses.off, G.pts.off, G.kfT.off, G.bytes};
  for (size_t i = 0; i + 1 < sizeof(go) / sizeof(go[0]); i++) CHECK(go[i] % 256 == 0 && go[i + 1] >= go[i], "graph slot %zu: " TAGF, i, TAGA);
  CHECK(G.headerBytes == G.lm_start.off && G.ps_start.off > G.lm_start.off && G.e_pt.off > G.ps_start.off, TAG);
#undef TAG
#undef TAGF
#undef TAGA
}

static bool g_reached[35];

int main() {
  static_assert(MAX_FREE_KF_LDS == 23, "the boundary the tests and the refusal's message name");
  static_assert(sizeof(OdomLin) == 624 && ODOM_TMP_DOUBLES * 8 == 864, "1488 bytes per odometry edge on the LDS route");
  const int kfs[] = {0, 1, 2, 21, 22, 23, 24, 42, 43, 682}, pts[] = {0, 1, 15, 16, 17, 100, 4096}, odo[] = {0, 1, 103, 104, 246, 247};
  for (int np : kfs)
    for (int npt : pts)
      for (int nO : odo)
        for (int world : {1, 2})
          for (int cap : {2, 256}) one_case(np, npt, nO, world, cap);
  // which Schur variants a call can reach: every LDS-resident size, through the OLD selection
  for (int np = 0; np <= 682; np++) {
    const OldPlan O = old_plan(np, 100, np + 2, 0, 1, 256);
    if (!O.big) g_reached[O.schurMaxT] = true;
    g_cases++;
    CHECK(O.big == (np > MAX_FREE_KF_LDS), "np %d", np);
    if (!O.big) CHECK(schur_maxt(schur_variant(O.NT)) == O.schurMaxT, "np %d", np);
  }
  g_cases++;
  CHECK(g_reached[9] && g_reached[20] && !g_reached[34], "reachable Schur variants: <9> %d <20> %d <34> %d", g_reached[9], g_reached[20], g_reached[34]);
  // the odometry records' home: the old two steps against the single rule
  for (int nO = 0; nO <= 1000; nO++) {
    g_cases++;
    const OldPlan O = old_plan(2, 100, 4, nO, 1, 256);
    CHECK((odom_home(nO) == ODOM_HBM) == O.linGlobal, "nO %d", nO);
    CHECK((odom_home(nO) == ODOM_LDS) == (nO <= 103), "nO %d", nO);
  }
  // tests/ba_cases.py NWG_CAP_FOR_CHUNKS: 100 points under a cap of 2 workgroups
  {
    g_cases++;
    BADims d{};
    d.n_kf = 6; d.npt = 100; d.nE = 300; d.np = 4;
    const BAPlan P = plan(d, false, false, 0, 1, 2);
    CHECK(P.lmPerWg == 64 && P.nWg == 2 && 100 - P.lmPerWg == 36, "lmPerWg %d nWg %d", P.lmPerWg, P.nWg);
    const BAPlan Q = plan(d, false, false, 0, 1, 256);
    CHECK(Q.lmPerWg == 16 && Q.nWg == 7, "lmPerWg %d nWg %d", Q.lmPerWg, Q.nWg);
  }
  // the schedule's slot counts (run_device_lm before ba_plan.h)
  {
    g_cases++;
    const BASched local = {5, 1, 1, 10}, global = {10, 1, 0, 0};
    CHECK(first_batch(local) == 5 + 10 + 1 + 1 + 2 && max_slots(local) == 2 + 10 * 15, "local");
    CHECK(first_batch(global) == 10 + 1 + 2 && max_slots(global) == 2 + 10 * 10, "global");
  }
  std::printf("cases=%ld failures=%ld\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
