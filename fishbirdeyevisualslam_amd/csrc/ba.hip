// ba.hip -- Optimizer::LocalBundleAdjustment / LocalBundleAdjustmentWithOdom / BundleAdjustmentWithOdom on gfx950.
//
// Replaces (reference file:line):
//   Optimizer::LocalBundleAdjustment            src/Optimizer.cc:838-1165
//   Optimizer::LocalBundleAdjustmentWithOdom    src/Optimizer.cc:2137-2670
//   EdgeSE3ProjectXYZ                           Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:103-147
//   EdgeSE3ProjectXYZ2UVQuat / 2XYZQuat / EdgeSE3Quat   src/OdomG2oTypeQuat.cc:109-212
//   BaseBinaryEdge::constructQuadraticForm      Thirdparty/g2o/g2o/core/base_binary_edge.hpp:55-120
//   BlockSolver::solve (Schur complement)       core/block_solver.hpp:354-486
//   OptimizationAlgorithmLevenberg::solve       core/optimization_algorithm_levenberg.cpp:61-164
//
// One Levenberg-Marquardt schedule, resident on the device, drives every entry point.  Its state (lambda, chi2, iteration and
// trial counters, which of the two states is the accepted one) lives in a control block in HBM (BACtl); the host enqueues
// identical "slots" of kernels, every kernel reads the control block, and k_ba_control takes the accept / reject decision at
// the end of each slot.  The host forwards the abort flag (pbStopFlag) on a side stream and reads the control block back once
// per batch of slots -- after every slot when FB_BA_HOST_LM or FB_BA_TRACE is set (host-paced: same kernels, same order).
// Kernels of a slot (all fp64 like g2o):
//   k_ba_schur_c    THE MFMA KERNEL: S_part = sum_l (W_l D_l^-1) W_l^T and the reduced rhs, as dense
//                   LDS panels (6n x 3c per chunk of c landmarks) multiplied with
//                   v_mfma_f64_16x16x4_f64; upper-triangular 16x16 tiles only, like g2o
//   k_ba_sumparts_c the workgroup partials of the Schur complement summed in a fixed order
//   k_ba_solve_c    S = Hpp + lambda I - sum S_part, dense LDL^T in LDS with look-ahead, backward substitution in one wave
//                   (more than MAX_FREE_KF_LDS free key frames: the reduced system lives in HBM, the kernels of ba_big.inc take these three places)
//   k_ba_update_c   landmark back-substitution, exp-map pose update, trial state, scale term; the chi2 gate between the rounds
//   k_ba_lin_c      the linearisation at the trial state in one launch of three roles: four lanes per landmark (residuals,
//                   Huber weights, Hll, bl, the 6x3 blocks W_e, partial chi2), a quarter of a free key frame's edges per
//                   workgroup (parts of its Hpp diagonal block and bp), one workgroup for the pose-pose EdgeSE3Quat blocks
//   k_ba_control    sums the parts, takes the decision (sharded: k_ba_prex and an all-reduce precede it)
// This file holds the kernels; the host side of the translation unit is included at its end:
//   ba_exchange.inc  RCCL / callback transport of the landmark-sharded BA, fb_rccl_*
//   ba_big.inc       kernels and host pieces of the HBM-resident reduced system
//   ba_plan.h        constants, LDS layouts, the plan of a call, the layouts of its two device blocks (no HIP: swept on the CPU)
//   ba_graph.inc     host builder, device builder (k_bld_*), odometry CSR, argument agreement
//   ba_driver.inc    plan, device binding, the slot loop, result hand-over, local_ba_impl, the extern "C" entry points
#include "fb_common.h"
#include "fb_primitives.h"

#include <thread>
#include "fb_se3.h"
#include "ba_plan.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>

namespace {

using fb::SE3;

constexpr int T_PROJ = 0, T_XYZ = 1;
constexpr int POSE_THREADS = 256;
// thread counts, panel widths, LDS layouts and the records shared with the host: ba_plan.h

struct BADev {  // device pointers + sizes, passed by value
  int n_kf, np, npt, nE, nO, quat;
  double fx, fy, cx, cy, delta;
  const int *poseIdx;          // [n_kf] free index or -1
  const int *e_pt, *e_kf;      // [nE]
  const uint8_t *e_type;       // [nE]
  const int *e_pj;             // [nE] poseIdx[e_kf[e]] (one dependent load less on the landmark-centric paths)
  const float *e_meas;         // [nE][3] (the measurements arrive as floats: kept so, half the staging bytes)
  const double *e_info;        // [nE]
  uint8_t *e_level;            // [nE]
  double *e_chi2;              // [nE] chi2 of the last evaluation that covered the edge
  const int *lm_start, *lm_edges;  // CSR by landmark
  const int *ps_start, *ps_edges;  // CSR by free pose
  const int *o_i, *o_j;        // [nO]
  const SE3 *o_Zinv;           // [nO]
  const double *o_info;        // [nO]
  const int *od_start, *od_edges;  // CSR by free pose: incident odometry edges, ascending edge index
};

struct LinBuf {  // linearisation at one state
  double *Hll;   // [npt][9]
  double *bl;    // [npt][3]
  double *W;     // [nE][18]
  double *Hpp;   // [P6][P6]: the key frames' 6x6 diagonal blocks only (the pose-pose blocks are HppO of the exchange block)
  double *bp;    // [P6]
  double *chiPart;  // [nLin + 1] per workgroup of the landmark role (last = odom chi2)
  double *maxPart;  // [nLin] max |diag Hll| of the workgroup's landmarks (lambda_0 = 1e-5 max diag)
};

struct State {
  SE3 *pose;     // [n_kf]
  double *pt;    // [npt][3]
};

// fb::rcp_f64_newton serves the pivots of the reduced pose system: the BA is held to 1e-4 on poses and landmarks, and an
// IEEE division is ~35 dependent instructions on the critical path of every block step of k_ba_solve_c
using fb::rcp_f64_newton;
using fb::wave_sum;
using fb::dpp_f64;

// residual + Jacobians of one point-pose edge (vertex 0 = point, vertex 1 = pose)
struct EdgeLin {
  double err[3];
  double Ji[3][3];  // d err / d point
  double Jj[3][6];  // d err / d pose
};

__device__ __forceinline__ void edge_residual(const BADev &D, int type, const SE3 &T, const double *X, const double *meas,
                                              double p[3], double err[3]) {
  fb::se3_map(T, X, p);
  if (type == T_PROJ) {
    if (D.quat) {  // OdomG2oTypeQuat.cc:138-144
      err[0] = meas[0] - (D.fx * p[0] / p[2] + D.cx);
      err[1] = meas[1] - (D.fy * p[1] / p[2] + D.cy);
    } else {       // types_six_dof_expmap.cpp:141-147
      err[0] = meas[0] - ((p[0] / p[2]) * D.fx + D.cx);
      err[1] = meas[1] - ((p[1] / p[2]) * D.fy + D.cy);
    }
    err[2] = 0;
  } else {
    err[0] = meas[0] - p[0]; err[1] = meas[1] - p[1]; err[2] = meas[2] - p[2];
  }
}

__device__ __forceinline__ void edge_jacobians(const BADev &D, int type, const SE3 &T, const double p[3], EdgeLin &L) {
  double R[9];
  fb::quat_to_R(T.r, R);
  const double X = p[0], Y = p[1], Z = p[2];
  if (type == T_PROJ) {
    if (D.quat) {  // EdgeSE3ProjectXYZ2UVQuat::linearizeOplus, OdomG2oTypeQuat.cc:109-129
      const double z2 = Z * Z;
      const double jep[2][3] = {{-(D.fx / Z), -0.0, -(-D.fx * X / z2)}, {-0.0, -(D.fy / Z), -(-D.fy * Y / z2)}};
      const double jpk[3][6] = {{-0.0, Z, -Y, 1, 0, 0}, {-Z, -0.0, X, 0, 1, 0}, {Y, -X, -0.0, 0, 0, 1}};  // [-skew(p), I]
#pragma unroll
      for (int r = 0; r < 2; r++) {
#pragma unroll
        for (int c = 0; c < 6; c++) L.Jj[r][c] = jep[r][0] * jpk[0][c] + jep[r][1] * jpk[1][c] + jep[r][2] * jpk[2][c];
#pragma unroll
        for (int c = 0; c < 3; c++) L.Ji[r][c] = jep[r][0] * R[c] + jep[r][1] * R[3 + c] + jep[r][2] * R[6 + c];
      }
    } else {  // EdgeSE3ProjectXYZ::linearizeOplus, types_six_dof_expmap.cpp:103-139
      const double z_2 = Z * Z;
      const double tmp[2][3] = {{D.fx, 0, -X / Z * D.fx}, {0, D.fy, -Y / Z * D.fy}};
      const double s = -1. / Z;
#pragma unroll
      for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) L.Ji[r][c] = (s * tmp[r][0]) * R[c] + (s * tmp[r][1]) * R[3 + c] + (s * tmp[r][2]) * R[6 + c];
      L.Jj[0][0] = X * Y / z_2 * D.fx; L.Jj[0][1] = -(1 + (X * X / z_2)) * D.fx; L.Jj[0][2] = Y / Z * D.fx;
      L.Jj[0][3] = -1. / Z * D.fx;     L.Jj[0][4] = 0;                            L.Jj[0][5] = X / z_2 * D.fx;
      L.Jj[1][0] = (1 + Y * Y / z_2) * D.fy; L.Jj[1][1] = -X * Y / z_2 * D.fy;   L.Jj[1][2] = -X / Z * D.fy;
      L.Jj[1][3] = 0;                  L.Jj[1][4] = -1. / Z * D.fy;               L.Jj[1][5] = Y / z_2 * D.fy;
    }
#pragma unroll
    for (int c = 0; c < 6; c++) L.Jj[2][c] = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) L.Ji[2][c] = 0;
  } else {  // EdgeSE3ProjectXYZ2XYZQuat::linearizeOplus, OdomG2oTypeQuat.cc:157-169
    const double jj[3][6] = {{0, -Z, Y, -1, -0.0, -0.0}, {Z, 0, -X, -0.0, -1, -0.0}, {-Y, X, 0, -0.0, -0.0, -1}};
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
      for (int c = 0; c < 6; c++) L.Jj[r][c] = jj[r][c];
#pragma unroll
      for (int c = 0; c < 3; c++) L.Ji[r][c] = -R[r * 3 + c];
    }
  }
}

// one point-pose edge of the landmark at X: chi2, Huber weight, its terms of Hll / bl, and its 6x3 block W
__device__ __forceinline__ void lin_edge(const BADev &D, const LinBuf &B, const double (&X)[3], int e, int kf, int lvl, int type, double info,
                                         const double (&measv)[3], const SE3 &T, int robust, double (&H)[9], double (&b3)[3], double &chi) {
  double *W = B.W + (size_t)e * 18;
  const int pj = D.poseIdx[kf];
  if (lvl != 0) {
#pragma unroll
    for (int i = 0; i < 18; i++) W[i] = 0;
    return;
  }
  const double meas[3] = {measv[0], measv[1], measv[2]};
  double p[3];
  EdgeLin L;
  edge_residual(D, type, T, X, meas, p, L.err);
  edge_jacobians(D, type, T, p, L);
  double chi2 = 0;
#pragma unroll
  for (int r = 0; r < 3; r++) chi2 += L.err[r] * (info * L.err[r]);
  D.e_chi2[e] = chi2;
  double rho0 = chi2, rho1 = 1.;
  if (robust) fb::huber(chi2, D.delta, rho0, rho1);
  chi += rho0;
  const double w = rho1 * info;
  double orr[3];
#pragma unroll
  for (int r = 0; r < 3; r++) orr[r] = -(info * L.err[r]) * rho1;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double s = 0;
#pragma unroll
    for (int r = 0; r < 3; r++) s += L.Ji[r][i] * orr[r];
    b3[i] += s;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double h = 0;
#pragma unroll
      for (int r = 0; r < 3; r++) h += L.Ji[r][i] * w * L.Ji[r][j];
      H[3 * i + j] += h;
    }
  }
  if (pj >= 0) {
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double h = 0;
#pragma unroll
        for (int r = 0; r < 3; r++) h += L.Jj[r][i] * w * L.Ji[r][j];
        W[i * 3 + j] = h;
      }
  } else {
#pragma unroll
    for (int i = 0; i < 18; i++) W[i] = 0;
  }
}

// The landmark role of the linearisation, FOUR lanes per landmark: lane `sub` of a quad takes the landmark's edges sub,
// sub + 4, ...; Hll, bl and chi2 are summed over the quad with two DPP quad permutes ((a0 + a1) + (a2 + a3)).  A landmark has
// 2..10 observers, so one lane per landmark walked them serially with three dependent gathers each: the landmark role was
// the long pole of the linearisation launch.
template <int TH>
__device__ __forceinline__ void linearize_quad_body(const BADev &D, const State &S, const LinBuf &B, int robust, double *s_part) {
  const int g = blockIdx.x * TH + threadIdx.x, l = g >> 2, sub = g & 3;
  double chi = 0, hmax = 0;
  double H[9], b3[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < 9; i++) H[i] = 0;
  if (l < D.npt) {
    const double X[3] = {S.pt[3 * l], S.pt[3 * l + 1], S.pt[3 * l + 2]};
    const int cBeg = D.lm_start[l], cEnd = D.lm_start[l + 1];
    for (int c0 = cBeg + sub; c0 < cEnd; c0 += 8) {  // two edges of this lane per trip, their gathers issued together
      int ee[2], kfv[2], lvl[2], typ[2];
      double infov[2], measv[2][3];
      SE3 Tv[2];
#pragma unroll
      for (int u = 0; u < 2; u++) ee[u] = D.lm_edges[min(c0 + 4 * u, cEnd - 1)];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        kfv[u] = D.e_kf[ee[u]]; lvl[u] = D.e_level[ee[u]]; typ[u] = D.e_type[ee[u]]; infov[u] = D.e_info[ee[u]];
        measv[u][0] = D.e_meas[3 * ee[u]]; measv[u][1] = D.e_meas[3 * ee[u] + 1]; measv[u][2] = D.e_meas[3 * ee[u] + 2];
      }
#pragma unroll
      for (int u = 0; u < 2; u++) Tv[u] = S.pose[kfv[u]];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        if (c0 + 4 * u >= cEnd) break;
        lin_edge(D, B, X, ee[u], kfv[u], lvl[u], typ[u], infov[u], measv[u], Tv[u], robust, H, b3, chi);
      }
    }
  }
  // quad sums (every lane of the wave takes part: lanes beyond npt carry zeros)
#pragma unroll
  for (int i = 0; i < 9; i++) { H[i] += dpp_f64<0xB1>(H[i]); H[i] += dpp_f64<0x4E>(H[i]); }
#pragma unroll
  for (int i = 0; i < 3; i++) { b3[i] += dpp_f64<0xB1>(b3[i]); b3[i] += dpp_f64<0x4E>(b3[i]); }
  if (l < D.npt && sub == 0) {
#pragma unroll
    for (int i = 0; i < 9; i++) B.Hll[(size_t)9 * l + i] = H[i];
#pragma unroll
    for (int i = 0; i < 3; i++) B.bl[(size_t)3 * l + i] = b3[i];
    hmax = fmax(fmax(fabs(H[0]), fabs(H[4])), fabs(H[8]));
  }
  const double ws = wave_sum(chi);
  hmax = fb::wave_max(hmax);
  if ((threadIdx.x & 63) == 0) { s_part[threadIdx.x >> 6] = ws; s_part[TH / 64 + (threadIdx.x >> 6)] = hmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0, m = 0;
    for (int i = 0; i < TH / 64; i++) { s += s_part[i]; m = fmax(m, s_part[TH / 64 + i]); }
    B.chiPart[blockIdx.x] = s;
    B.maxPart[blockIdx.x] = m;
  }
}

// ------------------------------------------------------------------------------------------
// The key-frame role of the linearisation: this workgroup sums every nparts-th edge of free key frame k starting at `part`;
// its 27 sums (21 upper entries of the Hpp diagonal block, 6 of bp) go to partOut (k_ba_control adds the parts in order)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void pose_body(const BADev &D, const State &S, int robust, double (*s_part)[27], int k, int part, int nparts,
                                          double *partOut) {
  const int tid = threadIdx.x;
  double acc[27];
#pragma unroll
  for (int i = 0; i < 27; i++) acc[i] = 0;
  for (int c = D.ps_start[k] + part * POSE_THREADS + tid; c < D.ps_start[k + 1]; c += nparts * POSE_THREADS) {
    const int e = D.ps_edges[c];
    if (D.e_level[e] != 0) continue;
    const int type = D.e_type[e], l = D.e_pt[e];
    const SE3 T = S.pose[D.e_kf[e]];
    const double X[3] = {S.pt[3 * l], S.pt[3 * l + 1], S.pt[3 * l + 2]};
    const double meas[3] = {D.e_meas[3 * e], D.e_meas[3 * e + 1], D.e_meas[3 * e + 2]};
    double p[3];
    EdgeLin L;
    edge_residual(D, type, T, X, meas, p, L.err);
    edge_jacobians(D, type, T, p, L);
    const double info = D.e_info[e];
    double chi2 = 0;
#pragma unroll
    for (int r = 0; r < 3; r++) chi2 += L.err[r] * (info * L.err[r]);
    double rho0 = chi2, rho1 = 1.;
    if (robust) fb::huber(chi2, D.delta, rho0, rho1);
    const double w = rho1 * info;
    int h = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      double s = 0;
#pragma unroll
      for (int r = 0; r < 3; r++) s += L.Jj[r][i] * (-(info * L.err[r]) * rho1);
      acc[21 + i] += s;
#pragma unroll
      for (int j = i; j < 6; j++) {
        double v = 0;
#pragma unroll
        for (int r = 0; r < 3; r++) v += L.Jj[r][i] * w * L.Jj[r][j];
        acc[h] += v;
        h++;
      }
    }
  }
  {
    double v[32];
#pragma unroll
    for (int i = 0; i < 32; i++) v[i] = i < 27 ? acc[i] : 0.0;
    const int lane = tid & 63;
    const double s = fb::wave_column_sums32(v, lane);  // lane L: column L >> 1
    if ((lane & 1) == 0 && (lane >> 1) < 27) s_part[tid >> 6][lane >> 1] = s;
  }
  __syncthreads();
  if (tid < 27) {
    double s = 0;
    for (int w2 = 0; w2 < POSE_THREADS / 64; w2++) s += s_part[w2][tid];
    s_part[0][tid] = s;
  }
  __syncthreads();
  if (tid < 27) partOut[tid] = s_part[0][tid];
}

// ------------------------------------------------------------------------------------------
// The odometry role of the linearisation: EdgeSE3Quat (OdomG2oTypeQuat.cc:180-204). Phase a: one lane per edge computes the
// residual and Jacobians into LDS; phase b: one lane per (free pose, row) adds the pose-pose blocks into HppO / bpO
// in edge order (deterministic).
// ------------------------------------------------------------------------------------------
constexpr int ODOM_DENSE_CLEAR_P6 = 6 * MAX_FREE_KF_LDS;  // the largest LDS-resident system (ba_plan.h)

template <bool GLOBAL>  // GLOBAL: the per-edge linearisations live in HBM scratch (they do not fit LDS)
__device__ __forceinline__ void odom_body(const BADev &D, const State &S, const LinBuf &B, int P6, int chiSlot, OdomLin *ol, double *s_chi,
                                          double *HppO, double *bpO, double *tmp) {
  const int tid = threadIdx.x;
  double chi = 0;
  // tmp != nullptr (LDS, ODOM_TMP_DOUBLES per edge: adj(T2) | adj(T1^-1) | J adj(T2)): the two 6x6x6 products of an edge are
  // spread over 36 lanes each instead of running serially on the edge's lane (same sums in the same order)
  for (int e = tid; e < D.nO; e += 256) {
    const SE3 T1 = S.pose[D.o_i[e]], T2 = S.pose[D.o_j[e]];
    const SE3 d = fb::se3_mul(fb::se3_mul(D.o_Zinv[e], T1), fb::se3_inverse(T2));
    double er[6];
    fb::se3_log(d, er);
    double J[36], a2[36], a1[36], t1[36];
#pragma unroll
    for (int i = 0; i < 36; i++) J[i] = 0;
    const double w0 = er[0], w1 = er[1], w2 = er[2], u0 = er[3], u1 = er[4], u2 = er[5];
    // JRInv: 0.5*[[skew(w),0],[skew(u),skew(w)]] + I
    J[1] = -w2; J[2] = w1; J[6] = w2; J[8] = -w0; J[12] = -w1; J[13] = w0;
    J[21 + 1] = -w2; J[21 + 2] = w1; J[27] = w2; J[27 + 2] = -w0; J[33] = -w1; J[33 + 1] = w0;
    J[18 + 1] = -u2; J[18 + 2] = u1; J[24] = u2; J[24 + 2] = -u0; J[30] = -u1; J[30 + 1] = u0;
#pragma unroll
    for (int i = 0; i < 36; i++) J[i] = 0.5 * J[i];
#pragma unroll
    for (int i = 0; i < 6; i++) J[i * 6 + i] += 1.0;
    fb::se3_adj(T2, a2);
    fb::se3_adj(fb::se3_inverse(T1), a1);
    if (tmp) {
      double *q = tmp + (size_t)e * ODOM_TMP_DOUBLES;
      for (int i = 0; i < 36; i++) { q[ODOM_TMP_ADJ2 + i] = a2[i]; q[ODOM_TMP_ADJ1 + i] = a1[i]; }
    } else {
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
          double s = 0;
          for (int k = 0; k < 6; k++) s += J[i * 6 + k] * a2[k * 6 + j];
          t1[i * 6 + j] = s;
        }
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
          double s = 0;
          for (int k = 0; k < 6; k++) s += t1[i * 6 + k] * a1[k * 6 + j];
          ol[e].A[i * 6 + j] = s;
        }
    }
    for (int i = 0; i < 36; i++) ol[e].Bm[i] = -J[i];
    const double info = D.o_info[e];
    const bool act = !(D.poseIdx[D.o_i[e]] < 0 && D.poseIdx[D.o_j[e]] < 0);  // allVerticesFixed edges are not active
    for (int i = 0; i < 6; i++) { ol[e].err[i] = er[i]; if (act) chi += er[i] * (info * er[i]); }
  }
  if (tmp) {
    __syncthreads();
    for (int idx = tid; idx < D.nO * 36; idx += 256) {  // J adj(T2), J = -Bm
      const int e = idx / 36, ij = idx - e * 36, i = ij / 6, j = ij - i * 6;
      const double *q = tmp + (size_t)e * ODOM_TMP_DOUBLES;
      double s2 = 0;
      for (int k = 0; k < 6; k++) s2 += (-ol[e].Bm[i * 6 + k]) * q[ODOM_TMP_ADJ2 + k * 6 + j];
      tmp[(size_t)e * ODOM_TMP_DOUBLES + ODOM_TMP_JADJ2 + ij] = s2;
    }
    __syncthreads();
    for (int idx = tid; idx < D.nO * 36; idx += 256) {  // (J adj(T2)) adj(T1^-1)
      const int e = idx / 36, ij = idx - e * 36, i = ij / 6, j = ij - i * 6;
      const double *q = tmp + (size_t)e * ODOM_TMP_DOUBLES;
      double s2 = 0;
      for (int k = 0; k < 6; k++) s2 += q[ODOM_TMP_JADJ2 + i * 6 + k] * q[ODOM_TMP_ADJ1 + k * 6 + j];
      ol[e].A[ij] = s2;
    }
  }
  s_chi[tid] = chi;
  if (GLOBAL) __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    double s = 0;
    const int nl = D.nO < 256 ? D.nO : 256;  // lanes at or beyond nO hold 0: the same sum in the same order without them
    for (int i = 0; i < nl; i++) s += s_chi[i];
    B.chiPart[chiSlot] = s;
  }
  // phase b: lane (k, i) = row i of free pose k.  The row's diagonal block and right-hand side entry are accumulated in
  // registers over the incident edges and written once; an off-diagonal block is loaded, updated and stored as a group of six
  // (one memory round trip per block: the 72 dependent read-modify-writes per row this replaces were most of the role's time)
  // HppO / bpO are this role's own scratch; the diagonal blocks and bpO are stored whole below, the off-diagonal blocks are
  // cleared here.  LDS-resident system: all of HppO, with coalesced stores.  Beyond it P6 x P6 stores from this one workgroup
  // would take longer than the rest of the linearisation: HppO starts cleared and only the blocks of the odometry edges are ever
  // written, so a row clears just the blocks its edges are about to add into (four dependent gathers: slower at small P6)
  if (P6 <= ODOM_DENSE_CLEAR_P6) {
    for (int i = tid; i < P6 * P6; i += 256) HppO[i] = 0;
    __syncthreads();
  } else {
    for (int row = tid; row < P6; row += 256) {
      const int k = row / 6;
      for (int cc = D.od_start[k]; cc < D.od_start[k + 1]; cc++) {
        const int e = D.od_edges[cc];
        const int pe[2] = {D.poseIdx[D.o_i[e]], D.poseIdx[D.o_j[e]]};
        for (int side = 0; side < 2; side++)
          if (pe[side] >= 0 && pe[side] != k)
            for (int j = 0; j < 6; j++) HppO[(size_t)row * P6 + 6 * pe[side] + j] = 0;
      }
    }
  }
  for (int row = tid; row < P6; row += 256) {
    const int k = row / 6, i = row % 6;
    double dg[6] = {0, 0, 0, 0, 0, 0}, bacc = 0;
    for (int cc = D.od_start[k]; cc < D.od_start[k + 1]; cc++) {  // incident edges only, in edge order
      const int e = D.od_edges[cc];
      const int pi = D.poseIdx[D.o_i[e]], pj = D.poseIdx[D.o_j[e]];
      const double info = D.o_info[e];
      const OdomLin &o = ol[e];
      // this row belongs to vertex i (Jacobian A) or vertex j (Jacobian Bm)
      const double *Mine = (pi == k) ? o.A : o.Bm;
      double bsum = 0;
      for (int r = 0; r < 6; r++) bsum += Mine[r * 6 + i] * (-(info * o.err[r]));
      bacc += bsum;
      for (int side = 0; side < 2; side++) {
        const int pc = side == 0 ? pi : pj;
        if (pc < 0) continue;
        const double *Oth = side == 0 ? o.A : o.Bm;
        double v[6];
        for (int j = 0; j < 6; j++) {
          double s = 0;
          for (int r = 0; r < 6; r++) s += Mine[r * 6 + i] * info * Oth[r * 6 + j];
          v[j] = s;
        }
        if (pc == k) {
          for (int j = 0; j < 6; j++) dg[j] += v[j];
        } else {
          double *dst = HppO + (size_t)row * P6 + 6 * pc, t6[6];
          for (int j = 0; j < 6; j++) t6[j] = dst[j];
          for (int j = 0; j < 6; j++) dst[j] = t6[j] + v[j];
        }
      }
      if (pi == k && pj == k) {  // degenerate self edge: also the Bm rows
        double b2 = 0;
        for (int r = 0; r < 6; r++) b2 += o.Bm[r * 6 + i] * (-(info * o.err[r]));
        bacc += b2;
      }
    }
    for (int j = 0; j < 6; j++) HppO[(size_t)row * P6 + 6 * k + j] = dg[j];
    bpO[row] = bacc;
  }
}

// ------------------------------------------------------------------------------------------
// k_ba_schur_c: MFMA fp64 accumulation of the Schur complement.
//   C[NT*16][NT*16] (upper tiles) += Yp[rows][K] * Wp[rows][K]^T over chunks of CHUNK landmarks,
//   Yp = W_e * Dinv_l scattered at rows 6*pose.., columns 3*li..; Wp likewise with W_e;
//   Wp row P6 carries bl so that column P6 of C is the reduced right-hand side (coefficients).
// v_mfma_f64_16x16x4_f64 operand layout (lane L): a = A[L%16][L/16], b = B[L/16][L%16],
// c[r] = C[(L/16)+4*r][L%16]  (measured on gfx950, scratch probe; not the f32 16x16x4 layout).
// ------------------------------------------------------------------------------------------
typedef double double4_t __attribute__((ext_vector_type(4)));

template <int MAXT>  // accumulator tiles per wave (compile-time so the C tiles stay in registers)
__device__ __forceinline__ void schur_body(const BADev &D, const LinBuf &B, double lambda, double *Dinv, double *Spart,
                                           int P6, int NT, int lmPerWg, uint8_t *smem) {
  const int rows = NT * 16;
  const SchurLds lds = schur_lds(rows);
  double *Yp = reinterpret_cast<double *>(smem) + lds.Yp, *Wp = reinterpret_cast<double *>(smem) + lds.Wp;  // [rows][KPAD] each
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l0 = blockIdx.x * lmPerWg, l1 = min(l0 + lmPerWg, D.npt);
  // upper-triangular tiles, dealt round-robin to the 4 waves
  const int nTiles = NT * (NT + 1) / 2;
  double4_t acc[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; t++) acc[t] = (double4_t){0, 0, 0, 0};
  // the panels are sparse (a landmark touches only the rows of its observing key frames): zero them once, and after each
  // chunk's MFMA phase clear exactly the entries that chunk wrote instead of re-zeroing 2 x rows x KPAD doubles
  for (int i = tid; i < 2 * rows * KPAD; i += SCHUR_THREADS) Yp[i] = 0;
  __syncthreads();
  for (int c0 = l0; c0 < l1; c0 += CHUNK) {
    // 16 lanes per landmark of the chunk: every lane inverts D (cheap), lane 0 of the group publishes it, the
    // group's lanes scatter the landmark's edge blocks in parallel
    {
      const int li = tid >> 4, sub = tid & 15;
      const int l = c0 + li;
      if (l < l1) {
        double M[9];
#pragma unroll
        for (int i = 0; i < 9; i++) M[i] = B.Hll[(size_t)9 * l + i];
        M[0] += lambda; M[4] += lambda; M[8] += lambda;
        const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
        const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
        const double id = 1.0 / det;
        double Di[9];
        Di[0] = c00 * id; Di[1] = (M[2] * M[7] - M[1] * M[8]) * id; Di[2] = (M[1] * M[5] - M[2] * M[4]) * id;
        Di[3] = c01 * id; Di[4] = (M[0] * M[8] - M[2] * M[6]) * id; Di[5] = (M[2] * M[3] - M[0] * M[5]) * id;
        Di[6] = c02 * id; Di[7] = (M[1] * M[6] - M[0] * M[7]) * id; Di[8] = (M[0] * M[4] - M[1] * M[3]) * id;
        if (sub == 0) {
#pragma unroll
          for (int i = 0; i < 9; i++) Dinv[(size_t)9 * l + i] = Di[i];
#pragma unroll
          for (int c = 0; c < 3; c++) Wp[(size_t)P6 * KPAD + 3 * li + c] = B.bl[(size_t)3 * l + c];
        }
        for (int cc = D.lm_start[l] + sub; cc < D.lm_start[l + 1]; cc += 16) {
          const int e = D.lm_edges[cc];
          const int pj = D.e_pj[e];
          if (pj < 0 || D.e_level[e] != 0) continue;
          const double *W = B.W + (size_t)e * 18;
#pragma unroll
          for (int i = 0; i < 6; i++) {
            const double w0 = W[i * 3], w1 = W[i * 3 + 1], w2 = W[i * 3 + 2];
            double *yr = Yp + (size_t)(6 * pj + i) * KPAD + 3 * li;
            double *wr = Wp + (size_t)(6 * pj + i) * KPAD + 3 * li;
            wr[0] = w0; wr[1] = w1; wr[2] = w2;
            yr[0] = w0 * Di[0] + w1 * Di[3] + w2 * Di[6];
            yr[1] = w0 * Di[1] + w1 * Di[4] + w2 * Di[7];
            yr[2] = w0 * Di[2] + w1 * Di[5] + w2 * Di[8];
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < MAXT; t++) {
      const int tile = wv + 4 * t;
      if (tile < nTiles) {
        // tile -> (ti, tj), ti <= tj
        int ti = 0, rem = tile;
        while (rem >= NT - ti) { rem -= NT - ti; ti++; }
        const int tj = ti + rem;
        const double *ya = Yp + (size_t)(ti * 16 + (lane & 15)) * KPAD + (lane >> 4);
        const double *wb = Wp + (size_t)(tj * 16 + (lane & 15)) * KPAD + (lane >> 4);
        double4_t c = acc[t];
#pragma unroll
        for (int k0 = 0; k0 < KP; k0 += 4) c = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[k0], wb[k0], c, 0, 0, 0);
        acc[t] = c;
      }
    }
    __syncthreads();
    {  // clear what this chunk scattered (same traversal as above)
      const int li = tid >> 4, sub = tid & 15;
      const int l = c0 + li;
      if (l < l1) {
        if (sub == 0) {
#pragma unroll
          for (int c = 0; c < 3; c++) Wp[(size_t)P6 * KPAD + 3 * li + c] = 0;
        }
        for (int cc = D.lm_start[l] + sub; cc < D.lm_start[l + 1]; cc += 16) {
          const int e = D.lm_edges[cc];
          const int pj = D.e_pj[e];
          if (pj < 0 || D.e_level[e] != 0) continue;
#pragma unroll
          for (int i = 0; i < 6; i++) {
            double *yr = Yp + (size_t)(6 * pj + i) * KPAD + 3 * li;
            double *wr = Wp + (size_t)(6 * pj + i) * KPAD + 3 * li;
            yr[0] = 0; yr[1] = 0; yr[2] = 0;
            wr[0] = 0; wr[1] = 0; wr[2] = 0;
          }
        }
      }
    }
    __syncthreads();
  }
  // write this workgroup's partial (upper tiles) : Spart[wg][rows][rows]
  double *out = Spart + (size_t)blockIdx.x * rows * rows;
#pragma unroll
  for (int t = 0; t < MAXT; t++) {
    const int tile = wv + 4 * t;
    if (tile < nTiles) {
      int ti = 0, rem = tile;
      while (rem >= NT - ti) { rem -= NT - ti; ti++; }
      const int tj = ti + rem;
#pragma unroll
      for (int r = 0; r < 4; r++) out[(size_t)(ti * 16 + (lane >> 4) + 4 * r) * rows + tj * 16 + (lane & 15)] = acc[t][r];
    }
  }
}

// ------------------------------------------------------------------------------------------
// solve_lookahead (k_ba_solve_c): S = Hpp + lambda I - Spart, dense LDL^T in LDS (6x6 blocks, no pivoting, fails on a zero
// pivot) and the solves, arranged for latency -- this one workgroup sits on the critical path of every LM trial.
//  * the right-hand side rides along as row P6 of the matrix: its panel steps ARE the forward substitution, so after the
//    factorisation row P6 holds z = D^-1 L^-1 b and only the backward substitution remains;
//  * look-ahead: in the trailing update of step J wave 0 updates only the NEXT diagonal block, factors it (a chain of ~100
//    dependent fp64 operations) and publishes L, d, 1/d through LDS, while the other three waves update the rest of the
//    trailing matrix; every thread used to factor the block redundantly BETWEEN the barriers;
//  * two barriers per key frame instead of three.
// The dense Hpp is not materialised: B.Hpp holds the key frames' diagonal blocks only and HppO the odometry (pose-pose) blocks.
#ifdef FB_BA_STAMPS
__device__ unsigned long long g_ba_stamps[16];
#define BA_T0() unsigned long long bt_ = 0; if (threadIdx.x == 0) { __builtin_amdgcn_sched_barrier(0); bt_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#define BA_TICK(slot_) if (threadIdx.x == 0) { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); g_ba_stamps[slot_] += t_ - bt_; bt_ = t_; }
#else
#define BA_T0()
#define BA_TICK(slot_)
#endif
template <int TS>  // threads of the workgroup
__device__ __forceinline__ void solve_lookahead(const LinBuf &B, double lambda, const double *Spart, int P6, int NT, double *xp, double *okFlag,
                                                uint8_t *smem, int &s_ok, const double *HppO) {
  const int ld = P6 + 1, rows = NT * 16, tid = threadIdx.x;
  BA_T0()
  const SolveLds lds = solve_lds(P6);  // A: lower triangle, row P6 = right-hand side; Up: panel u = l * d; fact2: 36 L | 6 d | 6 1/d, twice; rhs
  double *A = reinterpret_cast<double *>(smem) + lds.A, *Up = reinterpret_cast<double *>(smem) + lds.Up;
  double *fact2 = reinterpret_cast<double *>(smem) + lds.fact2, *rhs = reinterpret_cast<double *>(smem) + lds.rhs;
  if (tid == 0) s_ok = 1;
  {
    // A[i][j] = S[j][i] for i >= j (the upper triangle, as g2o's solver reads it): 16 lanes walk a row j of the upper
    // triangle (contiguous in memory), 16 row groups, four rows in flight per thread.  (The phase stamps had a quarter of the
    // solve in this loop when it divided a flat index and waited for each element's three loads in turn.)
    const int tr = tid >> 4, tc = tid & 15;
    constexpr int MAXM = (6 * MAX_FREE_KF_LDS + 15) / 16;  // 16-wide segments of the longest row of an LDS-resident system
    for (int j = tr; j < P6; j += TS / 16) {
      const int jb = j / 6;
      const double *srow = Spart + (size_t)j * rows, *orow = HppO + (size_t)j * P6, *hrow = B.Hpp + (size_t)j * P6;
      // every load of the row segment is issued before the first use: unconditional loads at clamped indices (a predicated
      // load makes the compiler wait for each element in turn), the selection happens on the values
      double o[MAXM], sv[MAXM], hv[MAXM];
#pragma unroll
      for (int m = 0; m < MAXM; m++) o[m] = orow[min(j + tc + 16 * m, P6 - 1)];
#pragma unroll
      for (int m = 0; m < MAXM; m++) sv[m] = srow[min(j + tc + 16 * m, P6 - 1)];
#pragma unroll
      for (int m = 0; m < MAXM; m++) hv[m] = hrow[min(j + tc + 16 * m, P6 - 1)];
#pragma unroll
      for (int m = 0; m < MAXM; m++) {
        const int i = j + tc + 16 * m;
        double h = o[m] - sv[m];
        if (i < 6 * jb + 6) h += hv[m];  // same key frame: the diagonal block
        if (i == j) h += lambda;
        if (i < P6) A[(size_t)i * ld + j] = h;
      }
    }
  }
  for (int i = tid; i < P6; i += TS) A[(size_t)P6 * ld + i] = B.bp[i] - Spart[(size_t)i * rows + P6];
  __syncthreads();
  const int nb6 = P6 / 6;
  // factor the 6x6 diagonal block at c0 (wave-redundant in registers), lane `wlane` 0 publishes it
  auto factor_block = [&](int c0) {
#pragma clang fp contract(fast)
    double *fact = fact2 + SOLVE_FACT_DOUBLES * ((c0 / 6) & 1);  // wave 0 publishes block J + 1 while slower waves may still read block J's
    // the dependent chain of this routine is the critical path of every block step: fused multiply-adds and the products
    // U[c][m] = L[c][m] d[m] kept next to L halve its length (the BA is tolerance-held)
    double Lb[6][6], Ub[6][6], d[6], dinv[6];
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int c = 0; c <= r; c++) Lb[r][c] = A[(size_t)(c0 + r) * ld + c0 + c];
    bool neg = false;
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double dc = Lb[c][c];
#pragma unroll
      for (int m = 0; m < c; m++) dc -= Lb[c][m] * Ub[c][m];
      if (dc == 0) neg = true;  // SimplicialLDLT: the factorisation fails on a pivot that is exactly 0, negative pivots proceed
      d[c] = dc;
      const double inv = dc != 0 ? rcp_f64_newton(dc) : 0.0;
      dinv[c] = inv;
#pragma unroll
      for (int r = c + 1; r < 6; r++) {
        double v = Lb[r][c];
#pragma unroll
        for (int m = 0; m < c; m++) v -= Lb[r][m] * Ub[c][m];
        Ub[r][c] = v;          // u = l d
        Lb[r][c] = v * inv;
      }
    }
    if ((tid & 63) == 0) {
      if (neg) s_ok = 0;
#pragma unroll
      for (int r = 0; r < 6; r++) {
        A[(size_t)(c0 + r) * ld + c0 + r] = d[r];
        fact[36 + r] = d[r];
        fact[42 + r] = dinv[r];
#pragma unroll
        for (int c = 0; c < r; c++) { A[(size_t)(c0 + r) * ld + c0 + c] = Lb[r][c]; fact[r * 6 + c] = Lb[r][c]; }
      }
    }
  };
  // (Measured and dropped: wave 0 running ahead -- taking the next block's panel rows itself so that its factor chain
  // overlaps the panel of the others, with a software barrier among the panel waves.  Same time: the chain
  // [factor read -> panel rows -> block update -> 6x6 factor] of the next block is the critical path either way.)
  if (tid < 64 && nb6 > 0) factor_block(0);
  __syncthreads();
  BA_TICK(1)  // first factor
  for (int J = 0; J < nb6; J++) {
    const int c0 = 6 * J, c1 = c0 + 6;
    const double *fact = fact2 + 48 * (J & 1);
    double Lb[6][6], dinv[6];
#pragma unroll
    for (int r = 1; r < 6; r++)
#pragma unroll
      for (int c = 0; c < r; c++) Lb[r][c] = fact[r * 6 + c];
#pragma unroll
    for (int c = 0; c < 6; c++) dinv[c] = fact[42 + c];
    for (int i = c1 + tid; i <= P6; i += TS) {  // panel: row i of L below the block (row P6: forward substitution)
      double u[6];
#pragma unroll
      for (int c = 0; c < 6; c++) {
        double v = A[(size_t)i * ld + c0 + c];
#pragma unroll
        for (int m = 0; m < c; m++) v -= u[m] * Lb[c][m];
        u[c] = v;
      }
#pragma unroll
      for (int c = 0; c < 6; c++) {
        Up[(size_t)i * 6 + c] = u[c];
        A[(size_t)i * ld + c0 + c] = u[c] * dinv[c];  // dinv = 0 for a zero pivot
      }
    }
    BA_TICK(2)  // read fact + panel
    __syncthreads();
    BA_TICK(3)  // barrier after panel
    if (tid < 64) {  // wave 0: the next diagonal block first, then its factorisation
      if (c1 < P6) {
        if (tid < 21) {
          int r = 0, rem = tid;
          while (rem > r) { rem -= r + 1; r++; }  // tid -> (r, cc), cc <= r
          const int i = c1 + r, k = c1 + rem;
          double acc2 = 0;
#pragma unroll
          for (int c = 0; c < 6; c++) acc2 += Up[(size_t)i * 6 + c] * A[(size_t)k * ld + c0 + c];
          A[(size_t)i * ld + k] -= acc2;
        }
        factor_block(c1);
      }
      BA_TICK(4)  // wave 0: next diagonal block update + factorisation
    } else {  // the other waves: the rest of the trailing matrix, rows c1 + 6 .. P6 (row P6: columns < P6)
      const int q = tid - 64, tr = q >> 4, tc = q & 15;
      for (int i = c1 + 6 + tr; i <= P6; i += (TS - 64) / 16) {
        double u[6];
#pragma unroll
        for (int c = 0; c < 6; c++) u[c] = Up[(size_t)i * 6 + c];
        const int kEnd = i < P6 ? i : P6 - 1;
        for (int k = c1 + tc; k <= kEnd; k += 16) {
          double acc2 = 0;
#pragma unroll
          for (int c = 0; c < 6; c++) acc2 += u[c] * A[(size_t)k * ld + c0 + c];
          A[(size_t)i * ld + k] -= acc2;
        }
      }
    }
    __syncthreads();
    BA_TICK(5)  // wait for the trailing update of the other waves
  }
  // row P6 now holds z = D^-1 L^-1 b.  Backward substitution L^T x = z on ONE wave: 18 dependent block steps with two
  // workgroup barriers each cost more in barriers than in arithmetic; inside a wave the LDS operations are ordered, so the
  // steps need no barrier at all.
  if (tid < 64) {
    for (int i = tid; i < P6; i += 64) rhs[i] = A[(size_t)P6 * ld + i];
    for (int J = nb6 - 1; J >= 0; J--) {
      const int c0 = 6 * J;
      double xJ[6];
#pragma unroll
      for (int r = 5; r >= 0; r--) {
        double v = rhs[c0 + r];
#pragma unroll
        for (int m = 5; m > r; m--) v -= A[(size_t)(c0 + m) * ld + c0 + r] * xJ[m];
        xJ[r] = v;
      }
      __builtin_amdgcn_wave_barrier();  // every lane has read rhs[c0..c0+6) before it is overwritten below
      if (tid < 6) rhs[c0 + tid] = xJ[tid];
      for (int i = tid; i < c0; i += 64) {
        double v = rhs[i];
#pragma unroll
        for (int c = 0; c < 6; c++) v -= A[(size_t)(c0 + c) * ld + i] * xJ[c];
        rhs[i] = v;
      }
      __builtin_amdgcn_wave_barrier();
    }
    for (int i = tid; i < P6; i += 64) xp[i] = rhs[i];
  }
  __syncthreads();
  BA_TICK(6)  // backward substitution
#ifdef FB_BA_STAMPS
  if (tid == 0) g_ba_stamps[15] += 1;
#endif
  if (tid == 0) *okFlag = s_ok ? 1.0 : 0.0;
}

// ------------------------------------------------------------------------------------------
// k_ba_update_c: back-substitution, trial state, scale term sum x (lambda x + b)
// ------------------------------------------------------------------------------------------
// Four lanes per landmark (as in the linearisation): lane q takes the landmark's edges q, q + 4, ..., the partial sums meet
// in a two-step butterfly (the same value on all four lanes), lane q < 3 then finishes coordinate q.  One lane per landmark
// left the back-substitution of 10 k landmarks to 79 two-wave workgroups.  Threads [4 npt, 4 npt + n_kf) = key frames.
__device__ __forceinline__ void update_body(const BADev &D, const LinBuf &B, const State &cur, const State &trial, const double *Dinv,
                                            const double *xp, double lambda, double *scalePart, int countPoses, double *s_part) {
  const int g = blockIdx.x * LIN_THREADS + threadIdx.x;
  double sc = 0;
  if (g < 4 * D.npt) {
    const int l = g >> 2, q = g & 3;
    double cl[3] = {0, 0, 0};
    for (int cc = D.lm_start[l] + q; cc < D.lm_start[l + 1]; cc += 4) {
      const int e = D.lm_edges[cc];
      const int pj = D.e_pj[e];
      if (pj < 0 || D.e_level[e] != 0) continue;
      const double *W = B.W + (size_t)e * 18;
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 6; i++) cl[j] -= W[i * 3 + j] * xp[6 * pj + i];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
      cl[j] += __shfl_xor(cl[j], 1, 64);
      cl[j] += __shfl_xor(cl[j], 2, 64);
      cl[j] += B.bl[(size_t)3 * l + j];
    }
    if (q < 3) {
      const double *Di = Dinv + (size_t)9 * l;
      const double xl = Di[q * 3] * cl[0] + Di[q * 3 + 1] * cl[1] + Di[q * 3 + 2] * cl[2];
      trial.pt[3 * l + q] = cur.pt[3 * l + q] + xl;
      sc = xl * (lambda * xl + B.bl[(size_t)3 * l + q]);
    }
  } else if (g < 4 * D.npt + D.n_kf) {
    const int k = g - 4 * D.npt;
    const int pi = D.poseIdx[k];
    if (pi < 0) trial.pose[k] = cur.pose[k];
    else {
      double u[6];
#pragma unroll
      for (int i = 0; i < 6; i++) { u[i] = xp[6 * pi + i]; if (countPoses) sc += u[i] * (lambda * u[i] + B.bp[6 * pi + i]); }
      trial.pose[k] = fb::se3_mul(fb::se3_exp(u), cur.pose[k]);
    }
  }
  const double ws = wave_sum(sc);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int i = 0; i < LIN_THREADS / 64; i++) s += s_part[i];
    scalePart[blockIdx.x] = s;
  }
}

// Spart[0] = sum over the workgroup partials (sharded BA: the local sum that goes through the all-reduce)
// The buffers are [rows][rows] matrices of which only the upper 16x16 tiles (and with them column P6, the reduced
// right-hand side) are ever written and read: the lower tiles are skipped
// 256-thread workgroups: 64 consecutive elements x 4 quarters of the partials (a wave = one quarter, so its loads are
// contiguous); the quarters meet in LDS in a fixed order.  One thread per element over all nWg partials kept only 64
// workgroups busy on 19 MB.
__device__ __forceinline__ void sumparts_body(double *Spart, int nWg, int n, int rows) {
  __shared__ double s_q[3][SUMPARTS_ELEMS];
  static_assert(sizeof(s_q) == STATIC_SUMPARTS, "ba_plan.h states this kernel's static LDS");
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = blockIdx.x * SUMPARTS_ELEMS + lane;
  bool live = i < n;
  if (live) {
    const int r = i / rows, c = i - r * rows;
    live = (r >> 4) <= (c >> 4);
  }
  const int per = (nWg + 3) >> 2, w0 = q * per, w1 = min(nWg, w0 + per);
  // 4 independent chains per thread: a single running sum serialises the memory latencies
  double a[4] = {0, 0, 0, 0};
  if (live) {
    int w = w0;
    for (; w + 4 <= w1; w += 4) {
#pragma unroll
      for (int u = 0; u < 4; u++) a[u] += Spart[(size_t)(w + u) * n + i];
    }
    for (; w < w1; w++) a[0] += Spart[(size_t)w * n + i];
  }
  const double s = (a[0] + a[1]) + (a[2] + a[3]);
  if (q > 0) s_q[q - 1][lane] = s;
  __syncthreads();
  if (q == 0 && live) Spart[i] = ((s + s_q[0][lane]) + s_q[1][lane]) + s_q[2][lane];
}
// gating between the two optimisation rounds and the final outlier flags
// (Optimizer.cc:1059-1073,1102-1115 / 2534-2565,2573-2607)
__device__ __forceinline__ void gate_edge(const BADev &D, const State &S, int setLevel, uint8_t *outFlag, int e) {
  if (D.e_level[e] == 2) {  // edge owned by another rank of a sharded BA
    if (!setLevel) outFlag[e] = 0;
    return;
  }
  const int type = D.e_type[e], l = D.e_pt[e];
  const SE3 T = S.pose[D.e_kf[e]];
  const double X[3] = {S.pt[3 * l], S.pt[3 * l + 1], S.pt[3 * l + 2]};
  bool bad;
  if (type == T_PROJ) {
    double p[3];
    fb::se3_map(T, X, p);
    bad = D.e_chi2[e] > 5.991 || !(p[2] > 0.0);
  } else {
    if (setLevel) {  // e->computeError() first
      const double meas[3] = {D.e_meas[3 * e], D.e_meas[3 * e + 1], D.e_meas[3 * e + 2]};
      double p[3], err[3];
      edge_residual(D, type, T, X, meas, p, err);
      const double info = D.e_info[e];
      D.e_chi2[e] = err[0] * (info * err[0]) + err[1] * (info * err[1]) + err[2] * (info * err[2]);
    }
    bad = D.e_chi2[e] > 5.991;
  }
  if (setLevel) { if (bad) D.e_level[e] = 1; }
  else outFlag[e] = bad ? 1 : 0;
}

// ---- device-resident Levenberg-Marquardt ------------------------------------------------------------------------------
// The accept / reject logic of OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-164), the
// iteration loop of SparseOptimizer::optimize and the two-stage schedule of LocalBundleAdjustment[WithOdom]
// (Optimizer.cc:2504-2570: optimize(5) with kernels, chi2 gate, optimize(10) without) live in BACtl in device memory.  The
// host enqueues identical "slots" of kernels without reading anything back; every kernel of a slot looks at BACtl and
// does nothing once the schedule has finished.  A slot is either the linearisation that opens an optimize() (needInit:
// chi2_0, lambda_0 = 1e-5 max diag) or one LM trial: Schur + solve at (cur, lambda) -> trial state -> its linearisation ->
// k_ba_control decides.  pbStopFlag: the host writes `abort` from a side stream while it waits.  (BACtl, BASched and the
// exchange block XBLay are in ba_plan.h.)
struct St2 { State s[2]; };
struct Lb2 { LinBuf b[2]; };
template <int MAXT>
__global__ __launch_bounds__(SCHUR_THREADS) void k_ba_schur_c(BADev D, Lb2 lb, const BACtl *c, double *Dinv, double *Spart, int P6, int NT, int lmPerWg) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  if (c->phase == 2 || c->needInit) return;
  schur_body<MAXT>(D, lb.b[c->cur], c->lambda, Dinv, Spart, P6, NT, lmPerWg, smem);
}
__global__ void k_ba_sumparts_c(const BACtl *c, double *Spart, int nWg, int n, int rows) {
  if (c->phase == 2 || c->needInit) return;
  sumparts_body(Spart, nWg, n, rows);
}
__global__ __launch_bounds__(SOLVE_C_THREADS) void k_ba_solve_c(Lb2 lb, const BACtl *c, const double *Spart, int P6, int NT, double *xp, double *okFlag,
                                                                XBLay xb) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int s_ok;
  static_assert(sizeof(s_ok) == STATIC_SOLVE, "ba_plan.h states this kernel's static LDS");
  if (c->phase == 2 || c->needInit) return;
  solve_lookahead<SOLVE_C_THREADS>(lb.b[c->cur], c->lambda, Spart, P6, NT, xp, okFlag, smem, s_ok, xb.at(c->cur) + xb.oH);
}
__global__ __launch_bounds__(LIN_THREADS) void k_ba_update_c(BADev D, Lb2 lb, St2 st, const BACtl *c, const double *Dinv, const double *xp, double *scalePart,
                                                             int countPoses) {
  __shared__ double s_part[LIN_THREADS / 64];
  static_assert(sizeof(s_part) == STATIC_UPDATE, "ba_plan.h states this kernel's static LDS");
  if (c->phase == 2) return;
  if (c->needInit) {
    if (c->needGate)  // edges beyond chi2 5.991 (or behind the camera) go to level 1 (Optimizer.cc:1059-1073 / 2534-2565)
      for (int e = blockIdx.x * LIN_THREADS + threadIdx.x; e < D.nE; e += gridDim.x * LIN_THREADS) gate_edge(D, st.s[c->cur], 1, nullptr, e);
    return;
  }
  update_body(D, lb.b[c->cur], st.s[c->cur], st.s[1 - c->cur], Dinv, xp, c->lambda, scalePart, countPoses, s_part);
}
// The decision at the end of a slot (one workgroup): assemble the key frames' diagonal blocks and bp from the parts, sum the
// chi2 / scale partials in index order (thread 0, from LDS), maximum of the diagonal (computeLambdaInit,
// optimization_algorithm_levenberg.cpp:166-180), then the LM state machine.
// Sharded BA: the block of this rank is summed over the ranks between this kernel and the control kernel; the chi2 / scale
// partials are therefore added up here (index order), next to the abort request and this rank's max |diag Hll|.
__global__ __launch_bounds__(256) void k_ba_prex(BADev D, Lb2 lb, const BACtl *c, int nLin, int chiSlot, const double *scalePart, int nScale, XBLay xb,
                                                 const int *abortLocal, int rank, int world) {
  __shared__ double s_m[256];
  static_assert(sizeof(s_m) == STATIC_PREX, "ba_plan.h states this kernel's static LDS");
  const int tid = threadIdx.x;
  const int init = c->needInit, t = init ? c->cur : 1 - c->cur;
  double *X = xb.at(t);
  if (c->phase == 2) {  // keep taking part in the exchange with harmless numbers
    if (tid < 4) X[xb.oS + tid] = (tid == 2 && *abortLocal) ? 1.0 : 0.0;
    if (tid < world) X[xb.oM + tid] = 0.0;
    return;
  }
  const LinBuf &B = lb.b[t];
  double m = 0;
  if (init) for (int i = tid; i < nLin; i += 256) m = fmax(m, B.maxPart[i]);
  s_m[tid] = m;
  __syncthreads();
  if (tid != 0) return;
  double chi = 0;
  for (int i = 0; i < nLin; i++) chi += B.chiPart[i];
  chi += B.chiPart[chiSlot];
  double scale = 0;
  if (!init) for (int i = 0; i < nScale; i++) scale += scalePart[i];
  double mm = 0;
  for (int i = 0; i < 256; i++) mm = fmax(mm, s_m[i]);
  X[xb.oS] = chi; X[xb.oS + 1] = scale; X[xb.oS + 2] = *abortLocal ? 1.0 : 0.0; X[xb.oS + 3] = 0.0;
  for (int r = 0; r < world; r++) X[xb.oM + r] = r == rank ? mm : 0.0;
}

template <bool SHARDED>
__device__ __forceinline__ void control_body(const BADev &D, const Lb2 &lb, BACtl *c, const BASched &sc, int nLin, int chiSlot, const double *scalePart, int nScale,
                                             const double *okFlag, int P6, const XBLay &xb, const int *abortLocal, int world, double *s_m /*[256]*/,
                                             double *s_chiP /*[512]*/, double *s_scaleP /*[512]*/) {
  const int tid = threadIdx.x;
  if (c->phase == 2) { if (tid == 0) c->slots++; return; }
  const int init = c->needInit;
  const int t = init ? c->cur : 1 - c->cur;
  const LinBuf &B = lb.b[t];
  const double *XB = xb.at(t);
  const double *HppO = XB + xb.oH, *bpO = XB + xb.oB, *poseP = XB;
  double m = 0;
  for (int idx = tid; idx < D.np * 42; idx += 256) {  // 36 block entries + 6 bp entries per key frame
    const int k = idx / 42, r = idx - k * 42;
    const double *pp = poseP + (size_t)k * POSE_PARTS * 27;
    if (r < 36) {
      const int i = r / 6, j = r % 6;
      const int a = i < j ? i : j, b2 = i < j ? j : i;
      const int u = a * 6 - a * (a - 1) / 2 + (b2 - a);  // upper-triangular packing
      double v = 0;
      for (int q = 0; q < POSE_PARTS; q++) v += pp[q * 27 + u];
      B.Hpp[(size_t)(6 * k + i) * P6 + 6 * k + j] = v;
      if (i == j && init) m = fmax(m, fabs(v + HppO[(size_t)(6 * k + i) * P6 + 6 * k + i]));
    } else {
      const int i = r - 36;
      double v = 0;
      for (int q = 0; q < POSE_PARTS; q++) v += pp[q * 27 + 21 + i];
      B.bp[6 * k + i] = v + bpO[6 * k + i];
    }
  }
  if (!SHARDED) {
    for (int i = tid; i < min(nLin, 512); i += 256) s_chiP[i] = B.chiPart[i];
    if (!init) for (int i = tid; i < min(nScale, 512); i += 256) s_scaleP[i] = scalePart[i];
    if (init) for (int i = tid; i < nLin; i += 256) m = fmax(m, B.maxPart[i]);
  }
  s_m[tid] = m;
  __syncthreads();
  double chi = 0, scale = 0;
  if (!SHARDED && tid < 64) {
    // the partials in a fixed order: lane t adds entries t, t + 64, ..., then the butterfly over the wave (deterministic,
    // and a few hundred dependent additions on one lane were a third of this kernel)
    for (int i = tid; i < nLin; i += 64) chi += i < 512 ? s_chiP[i] : B.chiPart[i];
    if (!init) for (int i = tid; i < nScale; i += 64) scale += i < 512 ? s_scaleP[i] : scalePart[i];
    chi = wave_sum(chi);
    scale = wave_sum(scale);
  }
  if (tid != 0) return;
  int abortReq;
  if (SHARDED) {  // reduced over the ranks: identical on all of them, and so is every decision below
    chi = XB[xb.oS]; scale = XB[xb.oS + 1];
    abortReq = XB[xb.oS + 2] > 0.0;
  } else {
    chi += B.chiPart[chiSlot];
    abortReq = *abortLocal;
  }
  double maxDiag = 0;
  if (init) {
    for (int i = 0; i < 256; i++) maxDiag = fmax(maxDiag, s_m[i]);
    if (SHARDED) for (int r = 0; r < world; r++) maxDiag = fmax(maxDiag, XB[xb.oM + r]);
  }
  BACtl k = *c;
  k.abort = abortReq;
  const int its = k.phase == 0 ? sc.its1 : sc.its2;
  bool endOpt = false;
  k.slots++;
  k.needGate = 0;
  if (init) {
    k.needInit = 0;
    k.currentChi = chi; k.iniChi = chi;
    k.lambda = 1e-5 * maxDiag; k.ni = 2; k.nBad = 0; k.it = 0; k.qmax = 0;
    k.trChi = chi; k.trScale = maxDiag; k.trRho = 0;
    if (its <= 0 || k.abort) endOpt = true;
  } else {
    k.trials++;
    double tempChi = chi;
    if (*okFlag == 0.0) tempChi = 1.7976931348623157e308;  // solver failure (levenberg.cpp:126-127)
    double rho = k.currentChi - tempChi;
    rho /= scale + 1e-3;
    k.trChi = tempChi; k.trScale = scale + 1e-3; k.trRho = rho;
    if (rho > 0 && isfinite(tempChi)) {
      double alpha = 1. - pow((2 * rho - 1), 3);
      alpha = fmin(alpha, 2. / 3.);
      k.lambda *= fmax(1. / 3., alpha);
      k.ni = 2;
      k.currentChi = tempChi;
      k.cur = 1 - k.cur;  // discardTop: the trial state and its linearisation become current
    } else {
      k.lambda *= k.ni;
      k.ni *= 2;  // pop
    }
    k.qmax++;
    if (!(rho < 0 && k.qmax < 10 && !k.abort)) {  // the iteration is over
      if (k.qmax == 10 || rho == 0) endOpt = true;
      else {
        if ((k.iniChi - k.currentChi) * 1e3 < k.iniChi) k.nBad++;
        else k.nBad = 0;
        if (k.nBad >= 3) endOpt = true;
      }
      if (!endOpt) {
        k.it++;
        if (k.it >= its || k.abort) endOpt = true;
        else { k.iniChi = k.currentChi; k.qmax = 0; }
      }
    }
  }
  if (endOpt) {
    // the chi2 gate runs in the next slot's k_ba_update_c launch (that slot only linearises)
    if (k.phase == 0 && sc.gate && !k.abort && D.nE > 0) { k.phase = 1; k.needInit = 1; k.needGate = 1; }
    else k.phase = 2;
  }
  *c = k;
}

template <bool SHARDED>
__global__ __launch_bounds__(256) void k_ba_control(BADev D, Lb2 lb, BACtl *c, BASched sc, int nLin, int chiSlot, const double *scalePart, int nScale,
                                                    const double *okFlag, int P6, XBLay xb, const int *abortLocal, int world) {
  __shared__ double s_m[256];
  __shared__ double s_chiP[512], s_scaleP[512];
  static_assert(sizeof(s_m) + sizeof(s_chiP) + sizeof(s_scaleP) == STATIC_CONTROL, "ba_plan.h states this kernel's static LDS");
  control_body<SHARDED>(D, lb, c, sc, nLin, chiSlot, scalePart, nScale, okFlag, P6, xb, abortLocal, world, s_m, s_chiP, s_scaleP);
}

// The linearisation of a slot as ONE launch of 256-thread workgroups with three roles (they are independent of each
// other): blocks [0, nLin) = landmarks (Hll, bl, W, chi2); the next POSE_PARTS * np blocks = a quarter of the edges of one
// free key frame each (27 partial sums of its Hpp diagonal block and bp); the last block = the odometry edges (their
// pose-pose blocks HppO, bpO).  The dense Hpp is never materialised: k_ba_control adds the key-frame parts into the diagonal
// blocks and bp, k_ba_solve_c / k_big_assemble read diagonal blocks + HppO.  Scratch per linearisation buffer t: [HppO | bpO], poseP.
// (Measured and dropped: the workgroup that finishes last -- a ticket in BACtl behind a device-scope fence -- taking the slot's
// decision itself instead of a k_ba_control launch.  A device-scope release / acquire on this part writes back and invalidates
// the XCD's L2 (buffer_wbl2 sc1 / buffer_inv sc1), once per workgroup: the linearisation went from 21 to 49 us.)
template <bool GLOBAL>
__global__ __launch_bounds__(LIN_C_THREADS) void k_ba_lin_c(BADev D, St2 st, Lb2 lb, const BACtl *c, BASched sc, int P6, int nLin, int chiSlot, OdomLin *olGlobal,
                                                  XBLay xb) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ double s_buf[LIN_C_THREADS];
  static_assert(sizeof(s_buf) == STATIC_LIN, "ba_plan.h states this kernel's static LDS");
  if (c->phase == 2) return;
  const int t = c->needInit ? c->cur : 1 - c->cur;
  const int robust = c->phase == 0 ? sc.robust1 : 0;
  const int bx = blockIdx.x;
  if (bx < nLin) {
    linearize_quad_body<256>(D, st.s[t], lb.b[t], robust, s_buf);
  } else if (bx < nLin + POSE_PARTS * D.np) {
    const int q = bx - nLin, k = q / POSE_PARTS, part = q - k * POSE_PARTS;
    pose_body(D, st.s[t], robust, reinterpret_cast<double(*)[27]>(s_buf), k, part, POSE_PARTS, xb.at(t) + (size_t)q * 27);
  } else {
    OdomLin *ol = GLOBAL ? olGlobal : reinterpret_cast<OdomLin *>(smem);
    double *tmp = GLOBAL ? nullptr : reinterpret_cast<double *>(ol + lin_lds_records(D.nO));  // LDS route: the records, then the products' scratch
    odom_body<GLOBAL>(D, st.s[t], lb.b[t], P6, chiSlot, ol, s_buf, xb.at(t) + xb.oH, xb.at(t) + xb.oB, tmp);
  }
}


__global__ void k_ba_gate_final_c(BADev D, St2 st, const BACtl *c, uint8_t *outFlag) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < D.nE) gate_edge(D, st.s[c->cur], 0, outFlag, e);
}

// sharded result: every rank contributes its own landmarks (points as exported floats) and edge flags, the others zeros
__global__ void k_ba_final_pack(int npt, int nE, int rank, int world, const float *ptOut, const uint8_t *flags, double *ex) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < npt * 3) ex[g] = ((g / 3) % world == rank) ? (double)ptOut[g] : 0.0;
  else if (g < npt * 3 + nE) ex[g] = flags[g - npt * 3];
}
__global__ void k_ba_final_unpack(int npt, int nE, const double *ex, float *ptOut, uint8_t *flags) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < npt * 3) ptOut[g] = (float)ex[g];
  else if (g < npt * 3 + nE) flags[g - npt * 3] = ex[g] != 0.0;
}

__global__ void k_ba_export_c(int n_kf, int npt, St2 st, const BACtl *c, const uint8_t *fixed, float *kfT, float *ptOut) {
  const SE3 *pose = st.s[c->cur].pose;
  const double *pt = st.s[c->cur].pt;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n_kf) {
    if (!fixed[g]) fb::se3_to_float12(pose[g], kfT + 12 * g);
  } else if (g < n_kf + npt * 3) ptOut[g - n_kf] = (float)pt[g - n_kf];
}

}  // namespace

#define BA_UP(buf, vec) FB_TRY(buf.upload((vec).data(), (vec).size() * sizeof((vec)[0])))

#ifdef FB_BA_STAMPS
extern "C" int fb_ba_debug_stamps(uint64_t *dst16) {  // probe build only: copies and clears the phase accumulators of the solve
  unsigned long long h[16], z[16] = {0};
  FB_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_ba_stamps), sizeof(h)));
  FB_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_ba_stamps), z, sizeof(z)));
  for (int i = 0; i < 16; i++) dst16[i] = h[i];
  return FB_OK;
}
#endif

#include "ba_exchange.inc"
#include "ba_big.inc"
#include "ba_graph.inc"
#include "ba_driver.inc"
