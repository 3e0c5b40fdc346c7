// sim3_plan.h -- what the two Sim3 stages of LoopClosing::ComputeSim3 (sim3_solver.hip, opt_sim3.hip) decide about memory,
// stated once: the width of a correspondence record, the static LDS of each kernel, which variant of a kernel fits a KF1
// stride and how many dynamic bytes it asks for, the workspace of each stage, the workspace refusal, and the rule by which a
// matched pair is kept.  DESIGN.md 7c / 7c-2 point here for the two thresholds (3402 and 2363 features).
//
// It needs no HIP header: plain host/device code (tests/cpp/sim3_plan_test.cpp compiles it with g++ and sweeps it).  Both
// _workspace() entry points, both _dev launchers and both kernels take every figure from it.  The device walk over matches12
// and the large-LDS opt-in of the two stages are in fb_sim3_pairs.h.  (k_optimize_sim3 writes the keep rule out once more.)
//
// Everything sits in an unnamed namespace like the kernels: the header belongs to one translation unit at a time.
#ifndef FB_SIM3_PLAN_H_
#define FB_SIM3_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "../../include/fishbird.h"

#ifdef __HIPCC__
#include "fb_common.h"  // FB_HD as __host__ __device__, whichever header a file includes first
#endif
#ifndef FB_HD
#define FB_HD
#endif

namespace fb {
void set_error(const char *fmt, ...);
}

namespace {
namespace s3 {

// ---- records, threads, static LDS ------------------------------------------------------------------------------------------
constexpr int SOLVER_NF = 12;    // dwords per solver correspondence (fb_sim3_corr), field by field in the workspace
constexpr int OPT_NCOL = 13;     // dword columns of an OptimizeSim3 correspondence: P1c, P2c, obs1, obs2, two informations, i1
constexpr int PREP_THREADS = 256, OPT_THREADS = 256;  // the two kernels that walk matches12
constexpr size_t LDS_BYTES = 160 * 1024;              // what a workgroup may have on gfx950, dynamic + static

// Static __shared__ bytes of each kernel.  A kernel keeps its statics in one struct and has a static_assert of that struct's
// size against the constant here.  (These are the group_segment_fixed_size figures of the code objects.)
constexpr size_t SCAN_BYTES_256 = 256 / 64 * 4;       // fb::block_excl_scan / block_sum: one int per wave
constexpr size_t STATIC_PREPARE = SCAN_BYTES_256;     // k_sim3_prepare
constexpr size_t STATIC_HYPOTHESES = 0;               // k_sim3_hypotheses has only its dynamic array, k_sim3_accept no LDS
constexpr size_t OPT_STATE_BYTES = 4128;              // Sim3Lds: 4 + 30 estimates of 64 B, H / b / x, the 36 sums and their per-wave parts
constexpr size_t OPT_JACOBIAN_BYTES = (size_t)14 * OPT_THREADS * 8;  // [14][NT] doubles, one column per thread
constexpr size_t STATIC_OPTIMIZE = OPT_STATE_BYTES + OPT_JACOBIAN_BYTES + SCAN_BYTES_256;  // k_optimize_sim3: 32 816

// The share of the 160 KiB that each stage reserves for its statics; the columns may take the rest.
constexpr size_t SOLVER_STATIC_SHARE = 512, OPT_STATIC_SHARE = 40 * 1024;
static_assert(STATIC_HYPOTHESES <= SOLVER_STATIC_SHARE && STATIC_OPTIMIZE <= OPT_STATIC_SHARE,
              "a variant that is chosen must fit beside the kernel's statics");
constexpr size_t SOLVER_LDS_BUDGET = LDS_BYTES - SOLVER_STATIC_SHARE, OPT_LDS_BUDGET = LDS_BYTES - OPT_STATIC_SHARE;

// ---- the launchers' decisions ----------------------------------------------------------------------------------------------
// The number of kept pairs is only known on the device, so the dynamic LDS is sized for the KF1 stride s1.
struct LdsPlan { bool inLds; size_t bytes; };  // bytes = the dynamic LDS of the launch (0 for the workspace variant)
FB_HD inline LdsPlan plan_columns(int s1, int dwords, size_t budget) {
  const size_t b = (size_t)s1 * dwords * 4;
  return b <= budget ? LdsPlan{true, b} : LdsPlan{false, 0};
}
FB_HD inline LdsPlan plan_solver(int s1) { return plan_columns(s1, SOLVER_NF, SOLVER_LDS_BUDGET); }   // k_sim3_hypotheses: s1 <= 3402
FB_HD inline LdsPlan plan_optimize(int s1) { return plan_columns(s1, OPT_NCOL, OPT_LDS_BUDGET); }     // k_optimize_sim3: s1 <= 2363

FB_HD inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
// The solver always writes its records to the workspace (k_sim3_prepare -> k_sim3_hypotheses); OptimizeSim3 needs one only for
// a key frame whose columns stay out of LDS, otherwise a 256-byte token.
FB_HD inline size_t solver_workspace(int n_cand, int s1) { return up256((size_t)n_cand * SOLVER_NF * s1 * 4); }
FB_HD inline size_t optimize_workspace(int n_cand, int s1) {
  return plan_optimize(s1).inLds ? 256 : up256((size_t)n_cand * OPT_NCOL * s1 * 4);
}

// The one refusal of a workspace that is missing, too small or misaligned.
inline int check_workspace(const char *who, const void *ptr, size_t bytes, size_t need) {
  if (!ptr || bytes < need || ((uintptr_t)ptr % 16) != 0) {
    fb::set_error("%s: workspace of %zu bytes (16-byte aligned) needed", who, need);
    return FB_ERR_ARG;
  }
  return FB_OK;
}

// ---- which pair is kept ----------------------------------------------------------------------------------------------------
// j = matches12[i1].  The reference skips j < 0, a NULL / bad pMP1, a bad pMP2 and GetIndexInKeyFrame < 0 (Sim3Solver.cc:64-79,
// Optimizer.cc:1615-1650).  MEMORY SAFETY beyond the reference: j >= the KF2 stride, an index >= its
// key frame's stride and an octave outside [0, FB_MAX_LEVELS) skip too, and no such value is ever used as an index: `src` is
// asked for a value only after what guards its index has passed.
//   src.valid1(), src.valid2(j), src.k1(), src.k2(j), src.o1(k1), src.o2(k2)
template <typename Src>
FB_HD inline bool keep_pair(int j, int s1, int s2, const Src &src, int *k1, int *k2, int *o1, int *o2) {
  if (j < 0 || j >= s2) return false;                  // vpMatched12[i1]
  if (!src.valid1() || !src.valid2(j)) return false;   // pMP1, !isBad() x 2
  *k1 = src.k1();                                      // GetIndexInKeyFrame
  *k2 = src.k2(j);
  if (*k1 < 0 || *k2 < 0 || *k1 >= s1 || *k2 >= s2) return false;
  *o1 = src.o1(*k1);
  *o2 = src.o2(*k2);
  return *o1 >= 0 && *o1 < FB_MAX_LEVELS && *o2 >= 0 && *o2 < FB_MAX_LEVELS;
}

}  // namespace s3
}  // namespace

#endif
