// ba_plan.h -- what the bundle adjustment (ba.hip with ba_graph.inc, ba_big.inc, ba_driver.inc) decides about memory, stated
// once: the thread counts and panel widths, the three dynamic LDS layouts (solve, Schur panels, odometry role of the
// linearisation), each kernel's static LDS, the budget that picks the LDS-resident or the HBM-resident reduced system and the
// home of the odometry records, the exchange block, the two device blocks of a call (staged graph, scratch) and the plan of a
// call.  DESIGN.md "the BA's plan" has the derivations (23 free key frames, 103 odometry edges).
//
// It needs no HIP header: plain host/device code (tests/cpp/ba_plan_test.cpp compiles it with g++ and sweeps it).  The driver
// takes every byte count and every path from plan(); solve_lookahead, schur_body and k_ba_lin_c take their LDS pointers from
// the same layouts.  plan() reads no environment and sets no error: it is a function of its arguments.
//
// Everything sits in an unnamed namespace like the kernels: the header belongs to one translation unit at a time.
#ifndef FB_BA_PLAN_H_
#define FB_BA_PLAN_H_

#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#include "fb_common.h"  // FB_HD as __host__ __device__
#include "fb_se3.h"
#else
namespace fb { struct SE3 { double r[4], t[3]; }; }  // the layouts need its size only
#endif
#ifndef FB_HD
#define FB_HD
#endif

namespace {

using fb::SE3;
static_assert(sizeof(SE3) == 56, "GraphLayout and ScratchLayout carve poses of 7 doubles");

// ---- threads, panels, records ----------------------------------------------------------------------------------------------
constexpr int LIN_THREADS = 128;      // k_ba_update_c
constexpr int LIN_C_THREADS = 256;    // k_ba_lin_c: four lanes per landmark
constexpr int SCHUR_THREADS = 256;
constexpr int SOLVE_C_THREADS = 512;  // wave 0 factors the next diagonal block, seven waves share the trailing update
constexpr int CHUNK = 16;             // landmarks per MFMA panel (K = 48)
constexpr int KP = 3 * CHUNK;
constexpr int KPAD = KP + 2;          // LDS row stride in doubles (breaks the 2-way bank conflict of stride 48)
constexpr int POSE_PARTS = 4;         // workgroups of the linearisation per free key frame
constexpr int SUMPARTS_ELEMS = 64;
constexpr int BIG_NB = 48;            // panel width of the HBM-resident factorisation (8 key frames)
constexpr int MAX_P6 = 4096;          // k_big_solve keeps the vector in LDS: at most 682 free key frames (the driver refuses more)

struct OdomLin { double A[36], Bm[36], err[6]; };  // the linearisation of one odometry edge
// the odometry role's products, per edge, behind the records: adj(T2) | adj(T1^-1) | J adj(T2)
constexpr int ODOM_TMP_ADJ2 = 0, ODOM_TMP_ADJ1 = 36, ODOM_TMP_JADJ2 = 72, ODOM_TMP_DOUBLES = 108;

// The Levenberg-Marquardt state of a call in device memory (ba.hip explains the schedule); it rides in the staged graph.
struct BACtl {
  double lambda, ni, currentChi, iniChi;
  int phase;     // 0 = first optimize(), 1 = second optimize() (after the chi2 gate), 2 = finished
  int it, qmax, nBad;
  int cur;       // index of the accepted state and of its linearisation
  int needInit;  // this slot linearises the accepted state instead of running a trial
  int needGate;  // this slot starts with the chi2 gate
  int abort;     // terminate(): set by the host when it sees *pbStopFlag
  int trials, slots;
  int badArgs;   // device-side graph builder (fb_local_ba_dev): 1 = index out of range, 2 = duplicate (key frame, point)
  double trChi, trScale, trRho;  // FB_BA_TRACE: tempChi, scale and rho of the last trial (after an opening linearisation: chi2_0, max diagonal, 0)
};
// optimisation schedule: LocalBundleAdjustment[WithOdom] = optimize(5) robust, chi2 gate, optimize(10) plain
// (Optimizer.cc:2504-2560); BundleAdjustmentWithOdom = ONE optimize(nIterations), robust iff bRobust, no gate (:2048-2050).
// Host and kernels share it.  (The Huber delta travels in BADev.)
struct BASched { int its1, robust1, gate, its2; };
// a typical schedule takes one trial per iteration: its1 + its2 trials + the two opening linearisations; the longest one ten
// trials per iteration
FB_HD constexpr int first_batch(const BASched &sc) { return sc.its1 + (sc.gate ? sc.its2 + 1 : 0) + 1 + 2; }
FB_HD constexpr int max_slots(const BASched &sc) { return 2 + 10 * (sc.its1 + (sc.gate ? sc.its2 : 0)); }

// ---- LDS: layouts (offsets in doubles from the start of the dynamic LDS) and statics ------------------------------------------
constexpr size_t LDS_BYTES = 160 * 1024;  // what a workgroup may have on gfx950, dynamic + static

// solve_lookahead (k_ba_solve_c)
constexpr int SOLVE_FACT_DOUBLES = 48;  // 36 L (row-major, lower) | 6 d | 6 1/d of a factored diagonal block
struct SolveLds {
  size_t A;      // [P6 + 1][P6 + 1], lower triangle; row P6 = right-hand side
  size_t Up;     // [P6 + 1][6] panel u = l * d of the current step
  size_t fact2;  // two buffers (even / odd block) of SOLVE_FACT_DOUBLES
  size_t rhs;    // [P6] backward substitution (+ 2 spare)
  size_t bytes;
};
FB_HD constexpr SolveLds solve_lds(int P6) {
  const int ld = P6 + 1;
  SolveLds L{};
  L.A = 0;
  L.Up = L.A + (size_t)(P6 + 1) * ld;
  L.fact2 = L.Up + (size_t)(P6 + 1) * 6;
  L.rhs = L.fact2 + 2 * SOLVE_FACT_DOUBLES;
  L.bytes = (L.rhs + (size_t)(P6 + 2)) * 8;  // (converted explicitly: `L.rhs + P6` cost k_ba_solve_c a sign extension)
  return L;
}
// schur_body (k_ba_schur_c): the two panels, [rows][KPAD] each
struct SchurLds { size_t Yp, Wp, bytes; };
FB_HD constexpr SchurLds schur_lds(int rows) {
  SchurLds L{};
  L.Yp = 0;
  L.Wp = (size_t)rows * KPAD;
  L.bytes = (size_t)2 * rows * KPAD * 8;
  return L;
}
// The odometry role of k_ba_lin_c when the records live in LDS: OdomLin [lin_lds_records] at the start, then ODOM_TMP_DOUBLES
// per edge.  (Two functions and no struct: with the offsets in a struct the compiler gave k_ba_lin_c<false> 298 VGPRs for 207.)
FB_HD constexpr int lin_lds_records(int nO) { return nO > 1 ? nO : 1; }
FB_HD constexpr size_t lin_lds_bytes(int nO) { return (size_t)lin_lds_records(nO) * (sizeof(OdomLin) + ODOM_TMP_DOUBLES * 8); }

// Static __shared__ bytes of each kernel; every kernel has a static_assert of its declarations against the constant here.
constexpr size_t STATIC_SCHUR = 0;                                 // k_ba_schur_c has only the panels
constexpr size_t STATIC_SOLVE = 4;                                 // k_ba_solve_c: s_ok
constexpr size_t STATIC_LIN = (size_t)LIN_C_THREADS * 8;           // k_ba_lin_c: s_buf
constexpr size_t STATIC_SUMPARTS = (size_t)3 * SUMPARTS_ELEMS * 8; // k_ba_sumparts_c: three quarters of the partials
constexpr size_t STATIC_UPDATE = LIN_THREADS / 64 * 8;             // k_ba_update_c: one double per wave
constexpr size_t STATIC_PREX = 256 * 8;                            // k_ba_prex: s_m
constexpr size_t STATIC_CONTROL = (256 + 512 + 512) * 8;           // k_ba_control: s_m, s_chiP, s_scaleP
constexpr size_t BIG_TILE_BYTES = (size_t)BIG_NB * (BIG_NB + 1) * 8;
constexpr size_t STATIC_BIG_PANEL = BIG_TILE_BYTES + BIG_NB * 8 + 4;  // k_big_panel: Ld, dd, s_neg
constexpr size_t STATIC_BIG_UPDATE = 2 * BIG_TILE_BYTES;           // k_big_update: Lt, Ut
constexpr size_t STATIC_BIG_SOLVE = BIG_TILE_BYTES;                // k_big_solve: Lp (+ P6 doubles of dynamic LDS)
constexpr size_t STATIC_BLD_SCAN = 16 * 4 + 4;                     // k_bld_scan: s_w, s_run

// The share of the 160 KiB that a kernel keeps for its statics; its dynamic layout may take the rest.  The linearisation's
// 10 KiB is not derived (s_buf is 2 KiB): it keeps the 150 KiB budget the driver had, so the odometry threshold stays at 103 edges.
constexpr size_t LIN_STATIC_SHARE = 10 * 1024;
static_assert(STATIC_LIN <= LIN_STATIC_SHARE, "a route that is chosen must fit beside the kernel's statics");
constexpr size_t SOLVE_LDS_BUDGET = LDS_BYTES - STATIC_SOLVE, SCHUR_LDS_BUDGET = LDS_BYTES - STATIC_SCHUR,
                 LIN_LDS_BUDGET = LDS_BYTES - LIN_STATIC_SHARE;
static_assert(STATIC_BIG_SOLVE + (size_t)MAX_P6 * 8 <= LDS_BYTES, "k_big_solve: the vector of the largest system beside Lp");

// The reduced pose system stays in LDS while the solve and the Schur panels of np free key frames fit.
FB_HD constexpr int nt_of(int P6) { return (P6 + 1 + 15) / 16; }  // 16x16 tiles per side; the right-hand side is row P6
FB_HD constexpr bool fits_lds(int np) {
  return solve_lds(6 * np).bytes <= SOLVE_LDS_BUDGET && schur_lds(nt_of(6 * np) * 16).bytes <= SCHUR_LDS_BUDGET;
}
constexpr int max_free_kf_lds() {
  int np = 0;
  while (fits_lds(np + 1)) np++;
  return np;
}
constexpr int MAX_FREE_KF_LDS = max_free_kf_lds();
static_assert(MAX_FREE_KF_LDS == 23, "the solve sets the boundary: 163 128 B at P6 = 138, 177 096 B at P6 = 144");

// k_ba_schur_c<MAXT>: accumulator tiles per wave, compile-time so that the C tiles stay in registers.  The LDS-resident
// system has NT <= 9, so two instantiations exist.
enum SchurVariant { SCHUR_T9, SCHUR_T20 };  // NT <= 8 (up to 21 free key frames), NT = 9 (22 and 23)
FB_HD constexpr int schur_maxt(SchurVariant v) { return v == SCHUR_T9 ? 9 : 20; }
FB_HD constexpr SchurVariant schur_variant(int NT) { return NT <= 8 ? SCHUR_T9 : SCHUR_T20; }
static_assert((nt_of(6 * MAX_FREE_KF_LDS) * (nt_of(6 * MAX_FREE_KF_LDS) + 1) / 2 + 3) / 4 <= schur_maxt(SCHUR_T20),
              "the widest LDS-resident system's tiles, dealt to four waves");

enum OdomHome { ODOM_LDS, ODOM_HBM };  // HBM: records in the scratch block, the products serial on the edge's lane
FB_HD constexpr OdomHome odom_home(int nO) { return lin_lds_bytes(nO) <= LIN_LDS_BUDGET ? ODOM_LDS : ODOM_HBM; }

// ---- the exchange block ----------------------------------------------------------------------------------------------------
// One per linearisation buffer t, `stride` doubles apart: everything a rank contributes to the pose system of a linearisation,
// contiguous so that the sharded BA sums it over the ranks with ONE all-reduce:
//   [0, oH) key-frame parts (np x POSE_PARTS x 27) | [oH, oB) HppO (P6 x P6) | [oB, oS) bpO (P6) |
//   [oS, oM) chi2, scale term, abort request, spare | [oM, stride) max |diag Hll| of each rank (own slot, others 0)
struct XBLay {
  double *base;
  int stride, oH, oB, oS, oM;
  FB_HD double *at(int t) const { return base + (size_t)t * stride; }
};
FB_HD inline XBLay xb_layout(int np, int P6, int world) {
  XBLay x{};
  x.base = nullptr;
  x.oH = np * POSE_PARTS * 27; x.oB = x.oH + P6 * P6; x.oS = x.oB + P6; x.oM = x.oS + 4; x.stride = x.oM + world;
  return x;
}

// ---- the plan of a call ----------------------------------------------------------------------------------------------------
struct BADims {  // the sizes of the graph, from the arguments alone
  bool odom;
  int n_kf, n_mp, npt;  // npt = n_mp + n_mpb: bird points keep their slots even when unused
  int nF, nB, nE, nO;   // front / bird observations, both, odometry edges (sharded: they live on rank 0)
  int nOAll;            // odometry edges of the call, the same on every rank
  int np;               // free key frames
};
struct BAPlan {
  BADims d;
  bool sharded, devIn;
  int rank, world;
  int P6, NT, rows;
  int nLinBlocks, nUpdBlocks;  // LIN_THREADS landmarks each (sizes the chi2 / max partials); k_ba_update_c: four lanes per landmark + one per key frame
  int nWg, lmPerWg;            // k_ba_schur_c: workgroups and landmarks of each (a multiple of CHUNK)
  int nLin256, linGrid;        // k_ba_lin_c: workgroups of the landmark role (chi2 slot of the odometry role = nLin256), of all three roles
  int nS;                      // elements of one partial of the Schur complement
  size_t schurLds, solveLds, linLds;  // dynamic bytes of the three launches (linLds: 0 on the HBM route)
  bool big;       // beyond MAX_FREE_KF_LDS free key frames the reduced system no longer fits LDS: HBM-resident path of ba_big.inc
  SchurVariant schur;
  OdomHome odomHome;
  XBLay xb;       // offsets only
  bool anything;  // (sharded: nE is this rank's view; every rank holds all edges, so this agrees across the ranks)
};
// nwg_cap: the most workgroups k_ba_schur_c may have (256 unless FB_BA_NWG says otherwise).  The caller has refused P6 > MAX_P6.
FB_HD inline BAPlan plan(const BADims &d, bool sharded, bool devIn, int rank, int world, int nwg_cap) {
  BAPlan P{};
  P.d = d; P.sharded = sharded; P.devIn = devIn; P.rank = rank; P.world = world;
  P.P6 = 6 * d.np;
  P.NT = nt_of(P.P6);
  P.rows = P.NT * 16;
  P.nLinBlocks = (d.npt + LIN_THREADS - 1) / LIN_THREADS;
  P.nUpdBlocks = (4 * d.npt + d.n_kf + LIN_THREADS - 1) / LIN_THREADS;
  const int chunks = (d.npt + CHUNK - 1) / CHUNK;
  P.nWg = chunks < 1 ? 1 : chunks;
  if (nwg_cap < P.nWg) P.nWg = nwg_cap;
  P.lmPerWg = ((d.npt + P.nWg - 1) / P.nWg + CHUNK - 1) / CHUNK * CHUNK;
  P.nWg = (d.npt + P.lmPerWg - 1) / (P.lmPerWg > 1 ? P.lmPerWg : 1);
  if (P.nWg < 1) P.nWg = 1;
  P.nLin256 = (4 * d.npt + LIN_C_THREADS - 1) / LIN_C_THREADS;
  P.linGrid = P.nLin256 + POSE_PARTS * d.np + 1;
  P.nS = P.rows * P.rows;
  P.schurLds = schur_lds(P.rows).bytes;
  P.solveLds = solve_lds(P.P6).bytes;
  P.big = !fits_lds(d.np);
  P.schur = schur_variant(P.NT);
  P.odomHome = odom_home(d.nO);
  P.linLds = P.odomHome == ODOM_LDS ? lin_lds_bytes(d.nO) : 0;
  P.xb = xb_layout(d.np, P.P6, world);
  P.anything = d.nE + (d.odom ? d.nOAll : 0) > 0 && (d.np > 0 || d.npt > 0);
  return P;
}

// ---- the two device blocks of a call -------------------------------------------------------------------------------------------
template <typename T> struct Slot {  // an array of T at a byte offset of some block
  size_t off = 0;
  T *at(void *base) const { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + off); }
};
struct Carver {  // hands out consecutive 256-byte-aligned slots
  size_t bytes = 0;
  template <typename T> Slot<T> take(size_t count) {
    Slot<T> s;
    s.off = bytes;
    bytes += (count * sizeof(T) + 255) & ~(size_t)255;
    return s;
  }
};
inline size_t at_least_1(long long n) { return n > 1 ? (size_t)n : 1; }

// Everything the kernels read is laid out in ONE staging block and goes to the device with one copy (two dozen small
// synchronous copies were a quarter of a millisecond).  The small host-built arrays come first: the device-input variant
// uploads only this header (the control block and the abort word ride in it: no separate synchronous copies).
struct GraphLayout {
  Slot<int> poseIdx;  // [n_kf] free index or -1
  Slot<uint8_t> fixed;
  Slot<int> o_i, o_j; Slot<SE3> o_Zinv; Slot<double> o_info; Slot<int> od_start, od_edges;
  Slot<BACtl> ctl; Slot<int> abort;
  size_t headerBytes;
  Slot<int> lm_start, ps_start;  // ADJACENT, in this order: the device builder zeroes both with one memset up to e_pt
  Slot<int> e_pt, e_kf, e_pj; Slot<uint8_t> e_type, e_level; Slot<float> e_meas; Slot<double> e_info; Slot<int> lm_edges, ps_edges;
  Slot<SE3> poses; Slot<double> pts;
  Slot<float> kfT;  // the caller's float poses (fixed key frames are returned untouched)
  size_t bytes;
};
inline GraphLayout graph_layout(const BADims &d) {
  const size_t nE1 = at_least_1(d.nE), nO1 = at_least_1(d.nO), npt1 = at_least_1(d.npt);
  GraphLayout G;
  Carver c;
  G.poseIdx = c.take<int>(d.n_kf); G.fixed = c.take<uint8_t>(d.n_kf);
  G.o_i = c.take<int>(nO1); G.o_j = c.take<int>(nO1); G.o_Zinv = c.take<SE3>(nO1); G.o_info = c.take<double>(nO1);
  G.od_start = c.take<int>(d.np + 1); G.od_edges = c.take<int>(2 * nO1);
  G.ctl = c.take<BACtl>(1); G.abort = c.take<int>(4);
  G.headerBytes = c.bytes;
  G.lm_start = c.take<int>(d.npt + 1); G.ps_start = c.take<int>(d.np + 1);
  G.e_pt = c.take<int>(nE1); G.e_kf = c.take<int>(nE1); G.e_pj = c.take<int>(nE1);
  G.e_type = c.take<uint8_t>(nE1); G.e_level = c.take<uint8_t>(nE1);
  G.e_meas = c.take<float>(3 * nE1); G.e_info = c.take<double>(nE1);
  G.lm_edges = c.take<int>(nE1); G.ps_edges = c.take<int>(nE1);
  G.poses = c.take<SE3>(d.n_kf); G.pts = c.take<double>(3 * npt1); G.kfT = c.take<float>((size_t)12 * d.n_kf);
  G.bytes = c.bytes;
  return G;
}

// The second device block: everything the schedule writes.  The driver clears e_chi2 (gate_edge reads an edge's chi2 before a
// linearisation may have covered it), the first nS doubles of Spart (the lower tiles of the summed system are never written:
// keep them finite) and the exchange blocks (the odometry role relies on it for HppO).
struct ScratchLayout {
  Slot<double> e_chi2;
  Slot<SE3> pose1;  // state 1 (state 0 is the staged copy)
  Slot<double> pt1;
  struct { Slot<double> Hll, bl, W, Hpp, bp, chiPart, maxPart; } lin[2];
  Slot<double> Dinv, Spart, xp, ok, scale;  // [npt][9]; LDS-resident: [nWg][rows][rows]; [P6]; the solve's verdict; k_ba_update_c's partials
  Slot<double> xb;      // exchange blocks: raw [2][stride], sharded: + reduced [2][stride]
  Slot<OdomLin> ol;     // the odometry records on the HBM route
  Slot<double> bigS, bigM, bigU;  // HBM-resident system: S | r, M | rhs, the panel's L D
  Slot<double> ex;      // sharded result
  Slot<uint8_t> flags; Slot<float> kfT, ptOut;  // results
  size_t bytes;
};
inline ScratchLayout scratch_layout(const BAPlan &P) {
  const BADims &d = P.d;
  const size_t nE1 = at_least_1(d.nE), npt1 = at_least_1(d.npt), P6 = P.P6;
  ScratchLayout C;
  Carver c;
  C.e_chi2 = c.take<double>(nE1);
  C.pose1 = c.take<SE3>(d.n_kf); C.pt1 = c.take<double>(3 * npt1);
  for (auto &l : C.lin) {
    l.Hll = c.take<double>(9 * npt1); l.bl = c.take<double>(3 * npt1); l.W = c.take<double>(18 * nE1);
    l.Hpp = c.take<double>(at_least_1(P6 * P6)); l.bp = c.take<double>(at_least_1(P6));
    l.chiPart = c.take<double>(2 * P.nLinBlocks + 2); l.maxPart = c.take<double>(2 * P.nLinBlocks + 2);
  }
  C.Dinv = c.take<double>(9 * npt1);
  C.Spart = c.take<double>(P.big ? 1 : (size_t)P.nWg * P.nS);
  C.xp = c.take<double>(at_least_1(P6)); C.ok = c.take<double>(1); C.scale = c.take<double>(at_least_1(P.nUpdBlocks));
  C.xb = c.take<double>((size_t)(P.sharded ? 4 : 2) * P.xb.stride);
  C.ol = c.take<OdomLin>(P.odomHome == ODOM_HBM ? at_least_1(d.nO) : 0);
  C.bigS = c.take<double>(P.big ? P6 * P6 + P6 : 0); C.bigM = c.take<double>(P.big ? P6 * P6 + P6 : 0);
  C.bigU = c.take<double>(P.big ? P6 * BIG_NB : 0);
  C.ex = c.take<double>(P.sharded ? (size_t)d.npt * 3 + d.nE + 1 : 0);
  C.flags = c.take<uint8_t>(nE1); C.kfT = c.take<float>((size_t)12 * d.n_kf); C.ptOut = c.take<float>(3 * npt1);
  C.bytes = c.bytes;
  return C;
}

}  // namespace

#endif
