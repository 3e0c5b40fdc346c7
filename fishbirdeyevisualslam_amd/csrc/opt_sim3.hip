// opt_sim3.hip -- Optimizer::OptimizeSim3 for every loop candidate of one key frame on gfx950 (fb_optimize_sim3*,
// include/fishbird.h): one launch, one workgroup per candidate, both rounds of Levenberg-Marquardt on the device.
//
// Replaces (reference file:line):
//   Optimizer::OptimizeSim3                         src/Optimizer.cc:1560-1775
//   mg2oScw = gScm * gSmw, mScw                     src/LoopClosing.cc:357, 364-368
//   VertexSim3Expmap::oplusImpl, cam_map1/2         Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h:60-88
//   EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ  types_seven_dof_expmap.h:138-167 (computeError; NO linearizeOplus)
//   BaseBinaryEdge::linearizeOplus (numeric)        core/base_binary_edge.hpp:130-173
//   BaseBinaryEdge::constructQuadraticForm          core/base_binary_edge.hpp:54-120, RobustKernelHuber
//   g2o::Sim3                                       types/sim3.h (fb_se3.h)
//   OptimizationAlgorithmLevenberg                  fb_lm.h, the schedule pose.hip runs
//
// Phases of a workgroup:
//   gather     the kept correspondences compacted in ascending i1 (block scan) into 13 dword columns: P1c, P2c (CV_32F
//              products), obs1, obs2, the two informations, i1.  The columns live in LDS, or in the caller's workspace for
//              a key frame whose columns do not fit.  A removed pair keeps its row with i1 complemented.
//   linearise  lanes 0..14 build the 14 perturbed estimates Sim3(+-delta e_d) * estimate, the estimate itself and all their
//              inverses into LDS; every thread then evaluates both edges of its rows at the 15 estimates, forms the two
//              2x7 central-difference Jacobians and adds chi2 (rho), the upper 7x7 and b: 36 sums, reduced through
//              wave_column_sums32 + wave_sum and one LDS hop.
//   trial      chi2 at estimate (+) dx needs the one Sim3: one sum.
//   decision   after each round the chi2 of every pair at the estimate the errors were last computed at, contraction off,
//              operation for operation what tests/opt_sim3_ref.py evaluates; the matches12 edits follow from it.
// Everything is fp64 like g2o, with true quotients: a difference of two projections is multiplied by 1 / (2e-9), so the
// reciprocal shortcuts of pose.hip are not taken here.
#include "fb_common.h"
#include "fb_lm.h"
#include "fb_se3.h"
#include "fb_sim3_pairs.h"

namespace {

constexpr int NT = s3::OPT_THREADS;     // one wave per SIMD: the whole register file for the 15-estimate edge pass
constexpr int NW = NT / 64;
constexpr int NCOL = s3::OPT_NCOL;      // dword columns of a correspondence
constexpr int NACC = 1 + 28 + 7;        // chi2, 28 x H upper, 7 x b

using fb::Sim3d;

struct Sim3Lds {  // the St of fb_lm.h
  static constexpr int DIM = 7;
  Sim3d T, Ttrial, Teval, T0;
  double H[49], b[7], x[7];
  double red[NACC];
  double part[NW][NACC];
  int ok2;
  Sim3d P[15], Pinv[15];  // [2 d] = Sim3(+delta e_d) * T, [2 d + 1] = Sim3(-delta e_d) * T, [14] = T
};

// Every static __shared__ byte of k_optimize_sim3 is its three objects S, s_J and s_wv.  They stay three objects: as members of
// one struct the compiler assigned the registers of the whole kernel anew and it ran 1 % longer.
static_assert(sizeof(Sim3Lds) == s3::OPT_STATE_BYTES && sizeof(Sim3Lds) + sizeof(double[14 * NT]) + sizeof(int[NW]) == s3::STATIC_OPTIMIZE,
              "sim3_plan.h states the static LDS of k_optimize_sim3");

struct SolveSim3 {
  int fix_scale;
  __device__ __forceinline__ bool solve(const double *H, double lambda, const double *b, double *x) const { return fb::ldlt<7>(H, lambda, b, x); }
  __device__ __forceinline__ Sim3d oplus(double *x, const Sim3d &T) const {  // oplusImpl: the update itself loses its scale
    if (fix_scale) x[6] = 0;
    return fb::sim3_mul(fb::sim3_exp(x), T);
  }
};

// one row of the columns (cols[f * cap + r])
struct Corr { float p1[3], p2[3], o1[2], o2[2], inf1, inf2; };
__device__ __forceinline__ Corr load_corr(const uint32_t *cols, int cap, int r) {
  Corr c;
  c.p1[0] = __uint_as_float(cols[0 * cap + r]); c.p1[1] = __uint_as_float(cols[1 * cap + r]); c.p1[2] = __uint_as_float(cols[2 * cap + r]);
  c.p2[0] = __uint_as_float(cols[3 * cap + r]); c.p2[1] = __uint_as_float(cols[4 * cap + r]); c.p2[2] = __uint_as_float(cols[5 * cap + r]);
  c.o1[0] = __uint_as_float(cols[6 * cap + r]); c.o1[1] = __uint_as_float(cols[7 * cap + r]);
  c.o2[0] = __uint_as_float(cols[8 * cap + r]); c.o2[1] = __uint_as_float(cols[9 * cap + r]);
  c.inf1 = __uint_as_float(cols[10 * cap + r]); c.inf2 = __uint_as_float(cols[11 * cap + r]);
  return c;
}

struct Cams { double fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2; };

// computeError of both edges at estimate S (Sinv = S.inverse()): e12 = obs1 - cam_map1(project(S.map(P2c))),
// e21 = obs2 - cam_map2(project(Sinv.map(P1c)))
__device__ __forceinline__ void edge_errors(const Sim3d &S, const Sim3d &Sinv, const Corr &c, const Cams &K, double (&e12)[2], double (&e21)[2]) {
  const double P2[3] = {c.p2[0], c.p2[1], c.p2[2]}, P1[3] = {c.p1[0], c.p1[1], c.p1[2]};
  double a[3], b[3];
  fb::sim3_map(S, P2, a);
  e12[0] = (double)c.o1[0] - ((a[0] / a[2]) * K.fx1 + K.cx1);
  e12[1] = (double)c.o1[1] - ((a[1] / a[2]) * K.fy1 + K.cy1);
  fb::sim3_map(Sinv, P1, b);
  e21[0] = (double)c.o2[0] - ((b[0] / b[2]) * K.fx2 + K.cx2);
  e21[1] = (double)c.o2[1] - ((b[1] / b[2]) * K.fy2 + K.cy2);
}

// The same for the DECISION (chi2() > th2): unfused, every operation in the order of tests/opt_sim3_ref.py, so that the
// masks are equal given the same estimate.  Eigen's q * v, then s * (.) + t (sim3.h:144); inverse() as sim3.h:233.
__device__ __forceinline__ void decision_map(const Sim3d &S, float x0, float x1, float x2, double (&p)[3]) {
#pragma clang fp contract(off)
  const double v0 = x0, v1 = x1, v2 = x2;
  const double qx = S.r.x, qy = S.r.y, qz = S.r.z, qw = S.r.w;
  double u0 = qy * v2 - qz * v1, u1 = qz * v0 - qx * v2, u2 = qx * v1 - qy * v0;
  u0 += u0; u1 += u1; u2 += u2;
  const double r0 = v0 + qw * u0 + (qy * u2 - qz * u1);
  const double r1 = v1 + qw * u1 + (qz * u0 - qx * u2);
  const double r2 = v2 + qw * u2 + (qx * u1 - qy * u0);
  p[0] = S.s * r0 + S.t[0];
  p[1] = S.s * r1 + S.t[1];
  p[2] = S.s * r2 + S.t[2];
}
__device__ __forceinline__ Sim3d decision_inverse(const Sim3d &a) {
#pragma clang fp contract(off)
  Sim3d r;
  const double qx = -a.r.x, qy = -a.r.y, qz = -a.r.z, qw = a.r.w;
  r.r.x = qx; r.r.y = qy; r.r.z = qz; r.r.w = qw;
  const double f = -1. / a.s;
  const double v0 = f * a.t[0], v1 = f * a.t[1], v2 = f * a.t[2];
  double u0 = qy * v2 - qz * v1, u1 = qz * v0 - qx * v2, u2 = qx * v1 - qy * v0;
  u0 += u0; u1 += u1; u2 += u2;
  r.t[0] = v0 + qw * u0 + (qy * u2 - qz * u1);
  r.t[1] = v1 + qw * u1 + (qz * u0 - qx * u2);
  r.t[2] = v2 + qw * u2 + (qx * u1 - qy * u0);
  r.s = 1. / a.s;
  return r;
}
__device__ __forceinline__ double decision_chi2(const Sim3d &S, float x0, float x1, float x2, float o0, float o1, double info,
                                                double fx, double fy, double cx, double cy) {
#pragma clang fp contract(off)
  double p[3];
  decision_map(S, x0, x1, x2, p);
  const double e0 = (double)o0 - ((p[0] / p[2]) * fx + cx);
  const double e1 = (double)o1 - ((p[1] / p[2]) * fy + cy);
  double s = 0;
  s += e0 * (info * e0);
  s += e1 * (info * e1);
  return s;
}

// one edge into the sums (base_binary_edge.hpp:91-113, the Sim3 vertex only): rho, b += J^T (rho' * -(info e)),
// H += J^T (rho' info) J
__device__ __forceinline__ void accumulate_edge(const double (&J)[2][7], const double (&err)[2], double info, double delta, double (&acc)[NACC]) {
  double chi2 = 0;
#pragma unroll
  for (int r = 0; r < 2; r++) chi2 += err[r] * (info * err[r]);
  double rho0, rho1;
  fb::huber(chi2, delta, rho0, rho1);
  acc[0] += rho0;
  const double w = rho1 * info;
  const double ie[2] = {info * err[0], info * err[1]};
  int hidx = 1;
#pragma unroll
  for (int i = 0; i < 7; i++) {
    acc[29 + i] -= rho1 * (J[0][i] * ie[0] + J[1][i] * ie[1]);
#pragma unroll
    for (int j = i; j < 7; j++) {
      acc[hidx] += J[0][i] * w * J[0][j] + J[1][i] * w * J[1][j];
      hidx++;
    }
  }
}

// computeError of one edge at M: obs - cam_map(project(M.map(P))); M = the estimate with P2c / obs1 / K1 for e12, its inverse
// with P1c / obs2 / K2 for e21
__device__ __forceinline__ void proj_error(const Sim3d &M, const float (&P)[3], const float (&o)[2], double fx, double fy, double cx,
                                           double cy, double (&e)[2]) {
  const double X[3] = {P[0], P[1], P[2]};
  double a[3];
  fb::sim3_map(M, X, a);
  e[0] = (double)o[0] - ((a[0] / a[2]) * fx + cx);
  e[1] = (double)o[1] - ((a[1] / a[2]) * fy + cy);
}

// One edge of a linearisation: the central differences over the 14 perturbed estimates M[0..13] (a ROLLED loop, so one pair
// of estimates and one pair of projections are live at a time), its error at M[14], then the 36 sums.  The 14 entries of
// the 2x7 Jacobian pass through this thread's own column of s_J ([14][NT] doubles: conflict-free), because a register array
// cannot be indexed by the loop counter.
__device__ __forceinline__ void linearise_edge(const Sim3d *M, const float (&P)[3], const float (&o)[2], double info, double fx, double fy,
                                               double cx, double cy, double delta, double *s_J, double (&acc)[NACC]) {
  const double scalar = 1.0 / (2 * 1e-9);
  const int tid = threadIdx.x;
#pragma unroll 1
  for (int d = 0; d < 7; d++) {
    double ep[2], em[2];
    proj_error(M[2 * d], P, o, fx, fy, cx, cy, ep);
    proj_error(M[2 * d + 1], P, o, fx, fy, cx, cy, em);
    s_J[(2 * d) * NT + tid] = scalar * (ep[0] - em[0]);
    s_J[(2 * d + 1) * NT + tid] = scalar * (ep[1] - em[1]);
  }
  double err[2], J[2][7];
  proj_error(M[14], P, o, fx, fy, cx, cy, err);
#pragma unroll
  for (int d = 0; d < 7; d++) { J[0][d] = s_J[(2 * d) * NT + tid]; J[1][d] = s_J[(2 * d + 1) * NT + tid]; }
  accumulate_edge(J, err, info, delta, acc);
}

template <bool IN_LDS>
__global__ __launch_bounds__(NT) void k_optimize_sim3(fb_optimize_sim3_args A, uint32_t *ws) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_cols[];
  __shared__ Sim3Lds S;
  __shared__ double s_J[14 * NT];  // a thread's Jacobian of the edge it is linearising
  __shared__ int s_wv[NW];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s1 = A.kf1.kf_stride, s2 = A.kf2.kf_stride, cap = s1;
  uint32_t *cols = IN_LDS ? s_cols : ws + (size_t)c * NCOL * s1;
  int32_t *m12 = A.matches12 + (size_t)c * s1;
  // ---- gather (Optimizer.cc:1613-1692).  The walk of s3::walk_pairs written out: through the shared function this kernel ran
  // 1 % longer.  Which pair is kept is s3::keep_pair with pKF1's index = i itself (:1624).
  int n1 = A.kf1.n_kf[0];
  n1 = n1 < 0 ? 0 : (n1 > s1 ? s1 : n1);
  int ncorr = 0;
  {
    const uint8_t *v2 = A.mp2.mp_valid + (size_t)c * s2;
    const float *xw2 = A.mp2.mp_xw + (size_t)c * s2 * 3;
    const fb_keypoint *kps2 = A.kf2.kf_kps + (size_t)c * s2;
    const int32_t *ix2 = A.kf2_index ? A.kf2_index + (size_t)c * s2 : nullptr;
    const float *T2 = A.T2w + (size_t)c * 12;
    for (int c0 = 0; c0 < n1; c0 += NT) {
      const int i1 = c0 + tid;
      bool keep = false;
      int j = -1, i2 = -1, o1 = 0, o2 = 0;
      if (i1 < n1) {
        j = m12[i1];
        if (j >= 0 && j < s2 && A.mp1.mp_valid[i1] && v2[j]) {   // vpMatches1[i], pMP1, !isBad() x 2
          i2 = ix2 ? ix2[j] : j;                                  // GetIndexInKeyFrame (:1624)
          if (i2 >= 0 && i2 < s2) {
            o1 = A.kf1.kf_kps[i1].octave;
            o2 = kps2[i2].octave;
            keep = o1 >= 0 && o1 < FB_MAX_LEVELS && o2 >= 0 && o2 < FB_MAX_LEVELS;
          }
        }
      }
      int tot;
      const int row = ncorr + fb::block_excl_scan<NT>(keep ? 1 : 0, s_wv, &tot);
      if (keep) {  // row < cap: at most one row per i1 < n1 <= s1
        const float *X1 = A.mp1.mp_xw + (size_t)i1 * 3, *X2 = xw2 + (size_t)j * 3;
        for (int q = 0; q < 3; q++) {
          cols[q * cap + row] = __float_as_uint(s3::rowmul(A.T1w, q, X1[0], X1[1], X1[2]));
          cols[(3 + q) * cap + row] = __float_as_uint(s3::rowmul(T2, q, X2[0], X2[1], X2[2]));
        }
        cols[6 * cap + row] = __float_as_uint(A.kf1.kf_kps[i1].x); cols[7 * cap + row] = __float_as_uint(A.kf1.kf_kps[i1].y);
        cols[8 * cap + row] = __float_as_uint(kps2[i2].x); cols[9 * cap + row] = __float_as_uint(kps2[i2].y);
        cols[10 * cap + row] = __float_as_uint(A.inv_level_sigma2[o1]);
        cols[11 * cap + row] = __float_as_uint(A.inv_level_sigma2[o2]);
        cols[12 * cap + row] = (uint32_t)i1;
      }
      ncorr += tot;
    }
  }
  int32_t *idx = reinterpret_cast<int32_t *>(cols + 12 * cap);  // i1 of an active pair, ~i1 of a removed one
  const int hs = A.hyp_stride > 0 ? A.hyp_stride : 1;
  if (tid == 0) {  // gScm = Sim3(toMatrix3d(R12), toVector3d(t12), s12) (LoopClosing.cc:357)
    const float *R = A.R12 + (size_t)c * hs * 9, *t = A.t12 + (size_t)c * hs * 3;
    const double Rd[9] = {R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]};
    S.T.r = fb::quat_from_R(Rd);
    S.T.t[0] = t[0]; S.T.t[1] = t[1]; S.T.t[2] = t[2];
    S.T.s = A.s12[(size_t)c * hs];
    S.T0 = S.T; S.Teval = S.T;
  }
  __syncthreads();  // the columns and the estimate

  Cams K;
  K.fx1 = A.kf1.cam.fx; K.fy1 = A.kf1.cam.fy; K.cx1 = A.kf1.cam.cx; K.cy1 = A.kf1.cam.cy;
  K.fx2 = A.kf2.cam.fx; K.fy2 = A.kf2.cam.fy; K.cx2 = A.kf2.cam.cx; K.cy2 = A.kf2.cam.cy;
  const double delta = (double)sqrtf(A.th2);  // const float deltaHuber = sqrt(th2)
  const double th2 = (double)A.th2;
  const SolveSim3 solve{A.fix_scale};

  // robust is always true here (both rounds keep the Huber kernel)
  auto eval = [&](const Sim3d &Tp, bool, bool linearise) {
    if (linearise) {
      if (tid < 15) {  // the estimates of the numeric Jacobian: push, oplus(+-delta e_d), pop (base_binary_edge.hpp:157-170)
        Sim3d P = Tp;
        if (tid < 14) {
          const double dl = (tid & 1) ? -1e-9 : 1e-9;
          double u[7];
#pragma unroll
          for (int d = 0; d < 7; d++) u[d] = (tid >> 1) == d ? dl : 0.0;
          P = solve.oplus(u, Tp);
        }
        S.P[tid] = P;
        S.Pinv[tid] = fb::sim3_inverse(P);
      }
      __syncthreads();
      double acc[NACC];
#pragma unroll
      for (int i = 0; i < NACC; i++) acc[i] = 0;
      for (int r = tid; r < ncorr; r += NT) {
        if (idx[r] < 0) continue;
        const Corr cr = load_corr(cols, cap, r);
        linearise_edge(S.P, cr.p2, cr.o1, (double)cr.inf1, K.fx1, K.fy1, K.cx1, K.cy1, delta, s_J, acc);     // e12
        linearise_edge(S.Pinv, cr.p1, cr.o2, (double)cr.inf2, K.fx2, K.fy2, K.cx2, K.cy2, delta, s_J, acc);  // e21
      }
      {
        double v[32];
#pragma unroll
        for (int i = 0; i < 32; i++) v[i] = acc[i];
        const double s = fb::wave_column_sums32(v, lane);
        if ((lane & 1) == 0) S.part[wv][lane >> 1] = s;
#pragma unroll
        for (int i = 32; i < NACC; i++) {
          const double t = fb::wave_sum(acc[i]);
          if (lane == 0) S.part[wv][i] = t;
        }
      }
      __syncthreads();
      if (tid < NACC) {
        double s = 0;
        for (int w = 0; w < NW; w++) s += S.part[w][tid];
        S.red[tid] = s;
      }
      __syncthreads();
    } else {
      const Sim3d T = Tp, Ti = fb::sim3_inverse(T);
      double chi = 0;
      for (int r = tid; r < ncorr; r += NT) {
        if (idx[r] < 0) continue;
        const Corr cr = load_corr(cols, cap, r);
        double e12[2], e21[2];
        edge_errors(T, Ti, cr, K, e12, e21);
        double c12 = 0, c21 = 0, rho1;
        c12 += e12[0] * ((double)cr.inf1 * e12[0]); c12 += e12[1] * ((double)cr.inf1 * e12[1]);
        c21 += e21[0] * ((double)cr.inf2 * e21[0]); c21 += e21[1] * ((double)cr.inf2 * e21[1]);
        double r12, r21;
        fb::huber(c12, delta, r12, rho1);
        fb::huber(c21, delta, r21, rho1);
        chi += r12;
        chi += r21;
      }
      chi = fb::wave_sum(chi);
      if (lane == 0) S.part[wv][0] = chi;
      __syncthreads();
      if (tid == 0) {
        double s = 0;
        for (int w = 0; w < NW; w++) s += S.part[w][0];
        S.red[0] = s;
      }
      __syncthreads();
    }
  };
  // e12.chi2() > th2 || e21.chi2() > th2 at the estimate the errors were last computed at (:1727, :1761); a bad pair
  // nulls vpMatches1 and, with `remove`, leaves the graph.  -> this thread's number of bad pairs
  auto classify = [&](bool remove) {
    const Sim3d T = S.Teval, Ti = decision_inverse(T);
    int bad = 0;
    for (int r = tid; r < ncorr; r += NT) {
      const int i1 = idx[r];
      if (i1 < 0) continue;
      const Corr cr = load_corr(cols, cap, r);
      const double c12 = decision_chi2(T, cr.p2[0], cr.p2[1], cr.p2[2], cr.o1[0], cr.o1[1], (double)cr.inf1, K.fx1, K.fy1, K.cx1, K.cy1);
      const double c21 = decision_chi2(Ti, cr.p1[0], cr.p1[1], cr.p1[2], cr.o2[0], cr.o2[1], (double)cr.inf2, K.fx2, K.fy2, K.cx2, K.cy2);
      if (c12 > th2 || c21 > th2) {
        m12[i1] = -1;
        if (remove) idx[r] = ~i1;
        bad++;
      }
    }
    return bad;
  };

  int nBad = 0, nIn = 0;
  bool written = false;  // g2oS12 = vSim3_recov->estimate() (:1772) was reached
  if (ncorr > 0) {
    fb::lm_optimize<false>(S, solve, tid == 0, true, eval, 5);           // optimize(5)
    nBad = fb::block_sum<NT>(classify(true), s_wv);
    if (ncorr - nBad >= 10) {                                            // :1745
      fb::lm_optimize<false>(S, solve, tid == 0, true, eval, nBad > 0 ? 10 : 5);  // initializeOptimization(); optimize(nMoreIterations)
      nIn = (ncorr - nBad) - fb::block_sum<NT>(classify(false), s_wv);
      written = true;
    }
  }
  if (tid == 0) {
    const Sim3d G = written ? S.T : S.T0;
    double *q = A.q + (size_t)c * 4, *t = A.t + (size_t)c * 3;
    q[0] = G.r.x; q[1] = G.r.y; q[2] = G.r.z; q[3] = G.r.w;
    t[0] = G.t[0]; t[1] = G.t[1]; t[2] = G.t[2];
    A.s[c] = G.s;
    // gSmw = Sim3(toMatrix3d(R2w), toVector3d(t2w), 1.0); mg2oScw = gScm * gSmw (LoopClosing.cc:364-366)
    const float *T2 = A.T2w + (size_t)c * 12;
    const double R2[9] = {T2[0], T2[1], T2[2], T2[4], T2[5], T2[6], T2[8], T2[9], T2[10]};
    Sim3d M;
    M.r = fb::quat_from_R(R2);
    M.t[0] = T2[3]; M.t[1] = T2[7]; M.t[2] = T2[11];
    M.s = 1.0;
    const Sim3d W = fb::sim3_mul(G, M);
    double *wq = A.scw_q + (size_t)c * 4, *wt = A.scw_t + (size_t)c * 3;
    wq[0] = W.r.x; wq[1] = W.r.y; wq[2] = W.r.z; wq[3] = W.r.w;
    wt[0] = W.t[0]; wt[1] = W.t[1]; wt[2] = W.t[2];
    A.scw_s[c] = W.s;
    double R[9];  // Converter::toCvMat(g2o::Sim3): toCvSE3(s * R, t)
    fb::quat_to_R(W.r, R);
    float *o = A.Scw + (size_t)c * 12;
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) o[i * 4 + j] = (float)(W.s * R[i * 3 + j]);
      o[i * 4 + 3] = (float)W.t[i];
    }
    A.n_inliers[c] = nIn;
    A.n_correspondences[c] = ncorr;
    A.n_bad[c] = nBad;
  }
}

int check_args(const fb_optimize_sim3_args *A) {
  FB_ARG(A != nullptr);
  FB_ARG(A->n_cand >= 1);
  FB_ARG(A->kf1.kf_stride >= 1 && A->kf2.kf_stride >= 1);
  FB_ARG(A->mp1.mp_stride == A->kf1.kf_stride && A->mp2.mp_stride == A->kf2.kf_stride);
  FB_ARG(A->kf1.n_kf && A->kf1.kf_kps && A->kf2.kf_kps);
  FB_ARG(A->mp1.mp_valid && A->mp1.mp_xw && A->mp2.mp_valid && A->mp2.mp_xw);
  FB_ARG(A->T1w && A->T2w && A->matches12 && A->s12 && A->R12 && A->t12);
  FB_ARG(A->hyp_stride >= 0);
  FB_ARG(A->th2 >= 0);
  FB_ARG(A->n_inliers && A->n_correspondences && A->n_bad && A->q && A->t && A->s && A->scw_q && A->scw_t && A->scw_s && A->Scw);
  return FB_OK;
}

}  // namespace

extern "C" {

size_t fb_optimize_sim3_workspace(int n_cand, int kf1_stride) {
  if (n_cand < 0 || kf1_stride < 0) return 0;
  return s3::optimize_workspace(n_cand, kf1_stride);
}

int fb_optimize_sim3_dev(const fb_optimize_sim3_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_TRY(check_args(A));
  const int C = A->n_cand, s1 = A->kf1.kf_stride;
  const s3::LdsPlan plan = s3::plan_optimize(s1);
  if (!plan.inLds) FB_TRY(s3::check_workspace("fb_optimize_sim3_dev", A->workspace, A->workspace_bytes, s3::optimize_workspace(C, s1)));
  const hipStream_t s = fb::as_stream(stream);
  fb::ProfScope prof_(fb::P_OPT_SIM3, s);
  if (plan.inLds) {
    FB_TRY(s3::allow_large_lds<&k_optimize_sim3<true>>(s3::OPT_LDS_BUDGET));
    k_optimize_sim3<true><<<C, NT, plan.bytes, s>>>(*A, nullptr);
  } else {
    k_optimize_sim3<false><<<C, NT, 0, s>>>(*A, static_cast<uint32_t *>(A->workspace));
  }
  FB_HIP(hipGetLastError());
  return FB_OK;
}

// host-pointer drop-in: one staged upload, the same kernel, one staged download (fb::Stager)
int fb_optimize_sim3(const fb_optimize_sim3_args *H) {
  FB_TRY(fb::check_device());
  FB_TRY(check_args(H));
  fb_optimize_sim3_args D = *H;
  const size_t C = H->n_cand, s1 = H->kf1.kf_stride, hs = H->hyp_stride > 0 ? H->hyp_stride : 1;
  fb::DevBuf ws;  // (declared first: it goes back to the pool after the Stager has waited)
  fb::Stager st;
  fb::stage_sim3_pair(st, D, C);
  st.in(D.s12, ((C - 1) * hs + 1) * 4); st.in(D.R12, ((C - 1) * hs + 1) * 36); st.in(D.t12, ((C - 1) * hs + 1) * 12);
  st.out(D.matches12, C * s1 * 4, true);
  st.out(D.n_inliers, C * 4, false); st.out(D.n_correspondences, C * 4, false); st.out(D.n_bad, C * 4, false);
  st.out(D.q, C * 32, false); st.out(D.t, C * 24, false); st.out(D.s, C * 8, false);
  st.out(D.scw_q, C * 32, false); st.out(D.scw_t, C * 24, false); st.out(D.scw_s, C * 8, false);
  st.out(D.Scw, C * 48, false);
  FB_TRY(st.commit(nullptr));
  D.workspace_bytes = fb_optimize_sim3_workspace((int)C, (int)s1);
  FB_TRY(ws.alloc(D.workspace_bytes));
  D.workspace = ws.p;
  FB_TRY(fb_optimize_sim3_dev(&D, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
