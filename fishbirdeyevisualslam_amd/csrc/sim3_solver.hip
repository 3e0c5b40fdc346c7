// sim3_solver.hip -- Sim3Solver on gfx950 (fb_sim3_solver*, include/fishbird.h).
//
// Replaces (reference file:line):
//   Sim3Solver::Sim3Solver            src/Sim3Solver.cc:37-112
//   Sim3Solver::SetRansacParameters   src/Sim3Solver.cc:114-138
//   Sim3Solver::iterate               src/Sim3Solver.cc:140-231 (as a table of every iteration, see the header)
//   Sim3Solver::ComputeSim3           src/Sim3Solver.cc:250-361 (Horn 1987)
//   Sim3Solver::CheckInliers/Project  src/Sim3Solver.cc:364-388, 406-427
//
// Three launches on the caller's stream, no host synchronisation (capturable):
//   k_sim3_prepare     one workgroup per candidate: the constructor as an ordered compaction in ascending i1 (block scan),
//                      N, mRansacMaxIts from a host-computed step table
//   k_sim3_hypotheses  one workgroup per (candidate, 16 hypotheses): the candidate's correspondences staged in LDS once,
//                      one wave per hypothesis: the three draws replayed, Horn's closed form (wave-uniform), then the 64
//                      lanes sweep the correspondences with both projections; inlier mask by wave ballot
//   k_sim3_accept      one wave per candidate: running maximum of the counts, the accept rule, first_accept
//
// Float / double seams: cv::Mat 3x3 * 3x1 (and 3x3 * 3x3) products without a transpose flag are float, ((a*x + b*y) + c*z),
// no FMA; Pr2*Pr1.t() accumulates in double and rounds once; cv::norm / Mat::dot accumulate in double.  cv::eigen of the
// symmetric 4x4 CV_32F matrix is a cyclic Jacobi in float, eigenvalues sorted descending (PARITY UNPINNED: OpenCV is not
// vendored).  The reference's atan2 -> angle-axis -> cv::Rodrigues round trip is not taken: the eigenvector goes to R as a
// quaternion in double, rounded once to float (the same rotation).  den == 0, |vec| == 0 and z == 0 give
// inf / NaN as in the reference, and every comparison with them is false.
#include "fb_common.h"
#include "fb_sim3_pairs.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int MAXH = FB_SIM3_MAX_HYP;
constexpr int PREP_THREADS = s3::PREP_THREADS;
constexpr int HYP_THREADS = 256;             // 4 waves
constexpr int HYP_PER_WAVE = 4;
constexpr int HYP_PER_BLOCK = HYP_THREADS / 64 * HYP_PER_WAVE;  // 16: 12 candidates x 300 -> 228 workgroups on 256 CUs
constexpr int NF = s3::SOLVER_NF;            // dwords per correspondence (fb_sim3_corr)
constexpr int JACOBI_SWEEPS = 8;

// SetRansacParameters as a step function of N: first_n[v] = the smallest N >= min_inliers (and <= the KF1 stride) whose
// mRansacMaxIts is at least v, INT_MAX when there is none.  Filled on the host with the reference's expression and the host's
// libm; mRansacMaxIts(N) = the number of v in 1..max_iterations with first_n[v] <= N (it does not decrease with N).
struct ItsTable { int32_t first_n[MAXH + 1]; };

struct WS {
  uint32_t *soa;  // [C][NF][s1]: the correspondences field by field (lane i reads consecutive words)
};

// ---- k_sim3_prepare -------------------------------------------------------------------------------------------------
struct PrepLds { int wv[PREP_THREADS / 64]; };  // the scan scratch of s3::walk_pairs
static_assert(sizeof(PrepLds) == s3::STATIC_PREPARE, "sim3_plan.h states the static LDS of k_sim3_prepare");

__global__ __launch_bounds__(PREP_THREADS) void k_sim3_prepare(fb_sim3_solver_args A, ItsTable its, WS W) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const int s1 = A.kf1.kf_stride;
  __shared__ PrepLds L;
  const int N = s3::walk_pairs<PREP_THREADS>(
      A.kf1, A.kf2, A.mp1, A.mp2, A.T1w, A.T2w, c, A.matches12, A.kf1_index, A.kf2_index, L.wv,
      [&](int row, int i1, int, int, int o1, int o2, const float (&P1c)[3], const float (&P2c)[3]) {
        fb_sim3_corr r;
        for (int q = 0; q < 3; q++) { r.x3dc1[q] = P1c[q]; r.x3dc2[q] = P2c[q]; }
        {  // FromCameraToImage (:429-447)
          const float invz = 1 / r.x3dc1[2];
          r.p1im1[0] = A.kf1.cam.fx * (r.x3dc1[0] * invz) + A.kf1.cam.cx;
          r.p1im1[1] = A.kf1.cam.fy * (r.x3dc1[1] * invz) + A.kf1.cam.cy;
        }
        {
          const float invz = 1 / r.x3dc2[2];
          r.p2im2[0] = A.kf2.cam.fx * (r.x3dc2[0] * invz) + A.kf2.cam.cx;
          r.p2im2[1] = A.kf2.cam.fy * (r.x3dc2[1] * invz) + A.kf2.cam.cy;
        }
        r.max_err1 = (int32_t)(9.210 * (double)A.level_sigma2[o1]);  // a double product stored into a size_t (:87-88)
        r.max_err2 = (int32_t)(9.210 * (double)A.level_sigma2[o2]);
        A.indices1[(size_t)c * s1 + row] = i1;
        if (A.corr) A.corr[(size_t)c * s1 + row] = r;
        const uint32_t *rw = reinterpret_cast<const uint32_t *>(&r);
        uint32_t *soa = W.soa + (size_t)c * NF * s1;
#pragma unroll
        for (int f = 0; f < NF; f++) soa[(size_t)f * s1 + row] = rw[f];
      });
  if (tid == 0) {
    int mi = 0;  // SetRansacParameters (:114-138); iterate returns at once when N < mRansacMinInliers (:146-150)
    if (N >= A.min_inliers)
      for (int v = 1; v <= A.max_iterations; v++) mi += its.first_n[v] <= N ? 1 : 0;
    A.N[c] = N;
    A.max_its[c] = N >= A.min_inliers ? mi : 0;
    A.n_hyp_done[c] = N >= A.min_inliers ? mi : 0;
  }
}

// ---- Horn 1987 on three correspondences (ComputeSim3, :250-361) ---------------------------------------------------------
struct Sim3 { float s, R[9], t[3], T12[12], T21[12]; };

// Eigenvector of the largest eigenvalue of the symmetric 4x4 a (float): cyclic Jacobi, a fixed number of sweeps over
// (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), only + - * / sqrt.  First maximum of the diagonal (eigenvalues sorted descending).
__device__ __forceinline__ void jacobi_eig4(float (&a)[4][4], float q[4]) {
  float V[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) V[r][c] = r == c ? 1.0f : 0.0f;
#pragma unroll 1
  for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int qq = p + 1; qq < 4; qq++) {
        const float apq = a[p][qq];
        if (apq == 0.0f) continue;
        const float zeta = (a[qq][qq] - a[p][p]) / (2.0f * apq);
        const float t = (zeta >= 0.0f ? 1.0f : -1.0f) / (fabsf(zeta) + sqrtf(1.0f + zeta * zeta));
        const float cs = 1.0f / sqrtf(1.0f + t * t), sn = cs * t;
#pragma unroll
        for (int k = 0; k < 4; k++) {  // A <- A J
          const float akp = a[k][p], akq = a[k][qq];
          a[k][p] = cs * akp - sn * akq;
          a[k][qq] = sn * akp + cs * akq;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {  // A <- J^T A
          const float apk = a[p][k], aqk = a[qq][k];
          a[p][k] = cs * apk - sn * aqk;
          a[qq][k] = sn * apk + cs * aqk;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float vp = V[k][p], vq = V[k][qq];
          V[k][p] = cs * vp - sn * vq;
          V[k][qq] = sn * vp + cs * vq;
        }
      }
  }
  float best = a[0][0];
  q[0] = V[0][0]; q[1] = V[1][0]; q[2] = V[2][0]; q[3] = V[3][0];
#pragma unroll
  for (int c = 1; c < 4; c++) {
    const bool up = a[c][c] > best;
    best = up ? a[c][c] : best;
#pragma unroll
    for (int r = 0; r < 4; r++) q[r] = up ? V[r][c] : q[r];
  }
}

// P1, P2: 3x3 with the samples as COLUMNS (P[r][i] = coordinate r of sample i)
__device__ __forceinline__ void compute_sim3(const float (&P1)[3][3], const float (&P2)[3][3], bool fixScale, Sim3 &o) {
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++) {  // cv::reduce(SUM) in float, C / P.cols as a scale by 1/3 in double
    O1[r] = (float)((double)((P1[r][0] + P1[r][1]) + P1[r][2]) * (1.0 / 3.0));
    O2[r] = (float)((double)((P2[r][0] + P2[r][1]) + P2[r][2]) * (1.0 / 3.0));
#pragma unroll
    for (int i = 0; i < 3; i++) { Pr1[r][i] = P1[r][i] - O1[r]; Pr2[r][i] = P2[r][i] - O2[r]; }
  }
  float M[3][3];  // M = Pr2 * Pr1.t(): double accumulation, one rounding
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++)
      M[i][j] = (float)(((double)Pr2[i][0] * (double)Pr1[j][0] + (double)Pr2[i][1] * (double)Pr1[j][1]) + (double)Pr2[i][2] * (double)Pr1[j][2]);
  const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
  const float N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
  const float N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
  float Nm[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
  float q[4];
  jacobi_eig4(Nm, q);
  {  // rotation of the quaternion (w, x, y, z) = q / |q|, in double, rounded once
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double n2 = ((w * w + x * x) + y * y) + z * z, k = 2.0 / n2;
    o.R[0] = (float)(1.0 - k * (y * y + z * z)); o.R[1] = (float)(k * (x * y - w * z)); o.R[2] = (float)(k * (x * z + w * y));
    o.R[3] = (float)(k * (x * y + w * z)); o.R[4] = (float)(1.0 - k * (x * x + z * z)); o.R[5] = (float)(k * (y * z - w * x));
    o.R[6] = (float)(k * (x * z - w * y)); o.R[7] = (float)(k * (y * z + w * x)); o.R[8] = (float)(1.0 - k * (x * x + y * y));
    if (((double)q[1] * q[1] + (double)q[2] * q[2]) + (double)q[3] * q[3] == 0.0) {  // vec / norm(vec) = 0/0 (:304)
      const float nan = __int_as_float(0x7fc00000);
#pragma unroll
      for (int e = 0; e < 9; e++) o.R[e] = nan;
    }
  }
  const float *R = o.R;
  if (!fixScale) {
    double nom = 0.0, den = 0.0;  // nom = Pr1.dot(P3) in double; den: double sum of the float squares of P3 = R * Pr2
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const float p3 = (R[i * 3] * Pr2[0][j] + R[i * 3 + 1] * Pr2[1][j]) + R[i * 3 + 2] * Pr2[2][j];
        nom = nom + (double)Pr1[i][j] * (double)p3;
        den = den + (double)(p3 * p3);
      }
    o.s = (float)(nom / den);
  } else {
    o.s = 1.0f;
  }
  const float s = o.s;
  const double sinv = 1.0 / (double)s;  // (1.0/ms12i) * mR12i.t()
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float u = (R[i * 3] * O2[0] + R[i * 3 + 1] * O2[1]) + R[i * 3 + 2] * O2[2];
    o.t[i] = O1[i] - s * u;  // t = O1 - s*R*O2
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      o.T12[i * 4 + j] = s * R[i * 3 + j];
      o.T21[i * 4 + j] = (float)((double)R[j * 3 + i] * sinv);
    }
    o.T12[i * 4 + 3] = o.t[i];
  }
#pragma unroll
  for (int i = 0; i < 3; i++)  // tinv = -sRinv * t
    o.T21[i * 4 + 3] = -((o.T21[i * 4] * o.t[0] + o.T21[i * 4 + 1] * o.t[1]) + o.T21[i * 4 + 2] * o.t[2]);
}

// Sim3Solver::Project (:406-427) + the squared distance of CheckInliers (:374-378): err = dist.dot(dist) stored as float.  (The
// walk's rowmul has the text of the copy this file had; its contract(off) pragma changes nothing in a file built unfused.)
__device__ __forceinline__ float reproj_err(const float *T, float X, float Y, float Z, float fx, float fy, float cx, float cy,
                                            float u0, float v0, bool firstMinusSecond) {
  const float xc = s3::rowmul(T, 0, X, Y, Z), yc = s3::rowmul(T, 1, X, Y, Z), zc = s3::rowmul(T, 2, X, Y, Z);
  const float invz = 1 / zc;
  const float u = fx * (xc * invz) + cx, v = fy * (yc * invz) + cy;
  const float dx = firstMinusSecond ? u0 - u : u - u0, dy = firstMinusSecond ? v0 - v : v - v0;
  return (float)((double)dx * (double)dx + (double)dy * (double)dy);
}

// ---- k_sim3_hypotheses ----------------------------------------------------------------------------------------------
template <bool IN_LDS>
__global__ __launch_bounds__(HYP_THREADS) void k_sim3_hypotheses(fb_sim3_solver_args A, WS W) {
  extern __shared__ uint32_t s_rec[];
  const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s1 = A.kf1.kf_stride;
  const int nh = A.n_hyp_done[c];
  const int k0 = blockIdx.x * HYP_PER_BLOCK;
  if (k0 >= nh) return;  // (uniform over the workgroup)
  const int N = A.N[c];
  const uint32_t *src = W.soa + (size_t)c * NF * s1;
  const uint32_t *rec = src;
  int fs = s1;  // words between two fields
  if (IN_LDS) {
    fs = N;
    for (int f = 0; f < NF; f++)
      for (int i = tid; i < N; i += HYP_THREADS) s_rec[f * N + i] = src[(size_t)f * s1 + i];
    __syncthreads();
    rec = s_rec;
  }
  const float *recf = reinterpret_cast<const float *>(rec);
  const int32_t *reci = reinterpret_cast<const int32_t *>(rec);
  const float fx1 = A.kf1.cam.fx, fy1 = A.kf1.cam.fy, cx1 = A.kf1.cam.cx, cy1 = A.kf1.cam.cy;
  const float fx2 = A.kf2.cam.fx, fy2 = A.kf2.cam.fy, cx2 = A.kf2.cam.cx, cy2 = A.kf2.cam.cy;
  const int mw = (s1 + 31) >> 5;
#pragma unroll 1
  for (int h = 0; h < HYP_PER_WAVE; h++) {
    const int k = k0 + h * (HYP_THREADS / 64) + wv;
    if (k >= nh) break;  // (uniform over the wave)
    // the three draws with swap-with-back removal (:163-177) on vAvailableIndices = 0..N-1
    const int32_t *rd = A.rand_idx + ((size_t)c * MAXH + k) * 3;
    int r0 = rd[0], r1 = rd[1], r2 = rd[2];
    r0 = r0 < 0 ? 0 : (r0 > N - 1 ? N - 1 : r0);
    r1 = r1 < 0 ? 0 : (r1 > N - 2 ? N - 2 : r1);
    r2 = r2 < 0 ? 0 : (r2 > N - 3 ? N - 3 : r2);
    const int i0 = r0;                                  // slot r0 then holds the back, N-1
    const int i1 = r1 == r0 ? N - 1 : r1;
    const int back2 = (N - 2) == r0 ? N - 1 : N - 2;   // the back after the first removal; slot r1 then holds it
    const int i2 = r2 == r1 ? back2 : (r2 == r0 ? N - 1 : r2);
    const int smp[3] = {i0, i1, i2};
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int r = 0; r < 3; r++) { P1[r][i] = recf[r * fs + smp[i]]; P2[r][i] = recf[(3 + r) * fs + smp[i]]; }
    Sim3 S;
    compute_sim3(P1, P2, A.fix_scale != 0, S);
    // CheckInliers (:364-388): set 2 through T12 with K1 against P1im1, set 1 through T21 with K2 against P2im2
    uint32_t *mask = A.inlier_mask + ((size_t)c * MAXH + k) * mw;
    int cnt = 0;
    for (int b = 0; b < N; b += 64) {
      const int i = b + lane;
      bool in = false;
      if (i < N) {
        const float e1 = reproj_err(S.T12, recf[3 * fs + i], recf[4 * fs + i], recf[5 * fs + i], fx1, fy1, cx1, cy1,
                                    recf[6 * fs + i], recf[7 * fs + i], true);
        const float e2 = reproj_err(S.T21, recf[i], recf[fs + i], recf[2 * fs + i], fx2, fy2, cx2, cy2,
                                    recf[8 * fs + i], recf[9 * fs + i], false);
        in = e1 < (float)reci[10 * fs + i] && e2 < (float)reci[11 * fs + i];  // a float against a size_t: the float comparison
      }
      const unsigned long long ball = __ballot(in);
      cnt += __popcll(ball);
      if (lane == 0) {
        mask[b >> 5] = (uint32_t)ball;
        if (b + 32 < N) mask[(b >> 5) + 1] = (uint32_t)(ball >> 32);
      }
    }
    if (lane == 0) {
      const size_t row = (size_t)c * MAXH + k;
      A.s[row] = S.s;
#pragma unroll
      for (int e = 0; e < 9; e++) A.R[row * 9 + e] = S.R[e];
#pragma unroll
      for (int e = 0; e < 3; e++) A.t[row * 3 + e] = S.t[e];
      A.n_inliers[row] = cnt;
    }
  }
}

// ---- k_sim3_accept --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sim3_accept(fb_sim3_solver_args A) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int nh = A.n_hyp_done[c];
  const int above = A.accept_above ? A.accept_above[c] : A.min_inliers;
  int run = 0, first = -1;  // mnBestInliers starts at 0
  for (int b = 0; b < MAXH; b += 64) {
    const int k = b + lane;
    const int n = k < nh ? A.n_inliers[(size_t)c * MAXH + k] : 0;
    int inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc = inc > t ? inc : t; }
    int before = __shfl_up(inc, 1, 64);
    before = lane == 0 ? run : (before > run ? before : run);
    const bool acc = k < nh && n >= before && n > above;  // mnInliersi >= mnBestInliers (:183) and the return rule (:192)
    if (k < MAXH) A.accept[(size_t)c * MAXH + k] = acc ? 1 : 0;
    const unsigned long long ball = __ballot(acc);
    if (first < 0 && ball) first = b + __ffsll((long long)ball) - 1;
    const int last = __shfl(inc, 63, 64);
    run = last > run ? last : run;
  }
  if (lane == 0) {
    A.first_accept[c] = first;
    A.no_more[c] = first < 0 ? 1 : 0;  // N < min_inliers (nh = 0), or mnIterations reached mRansacMaxIts without a return
  }
}

// SetRansacParameters (:125-135) for one N >= min_inliers, in the reference's float / double mix with the host's libm
int ransac_max_its(int N, double prob, int minInliers, int maxIterations) {
  const float epsilon = (float)minInliers / N;
  int nIterations;
  if (minInliers == N) {
    nIterations = 1;
  } else {
    const double x = std::ceil(std::log(1 - prob) / std::log(1 - std::pow((double)epsilon, 3.0)));
    nIterations = x < (double)maxIterations ? (int)x : maxIterations;  // (also when x is inf or NaN: min() with the cap)
  }
  return std::max(1, std::min(nIterations, maxIterations));
}

int check_args(const fb_sim3_solver_args *A) {
  FB_ARG(A && A->n_cand >= 1 && A->kf1.kf_stride > 0 && A->kf2.kf_stride > 0);
  FB_ARG(A->mp1.mp_stride == A->kf1.kf_stride && A->mp2.mp_stride == A->kf2.kf_stride);
  FB_ARG(A->min_inliers >= 3 && A->max_iterations >= 1 && A->max_iterations <= MAXH);
  FB_ARG(A->ransac_prob > 0.0 && A->ransac_prob < 1.0);
  FB_ARG(A->kf1.n_kf && A->kf1.kf_kps && A->kf2.kf_kps && A->mp1.mp_valid && A->mp1.mp_xw && A->mp2.mp_valid && A->mp2.mp_xw);
  FB_ARG(A->T1w && A->T2w && A->matches12 && A->rand_idx);
  FB_ARG(A->N && A->indices1 && A->max_its && A->n_hyp_done && A->first_accept && A->no_more);
  FB_ARG(A->s && A->R && A->t && A->n_inliers && A->accept && A->inlier_mask);
  return FB_OK;
}

}  // namespace

extern "C" {

size_t fb_sim3_solver_workspace(int n_cand, int n1_stride) {
  if (n_cand < 0 || n1_stride < 0) return 0;
  return s3::solver_workspace(n_cand, n1_stride);
}

int fb_sim3_solver_dev(const fb_sim3_solver_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_TRY(check_args(A));
  const int C = A->n_cand, s1 = A->kf1.kf_stride;
  FB_TRY(s3::check_workspace("fb_sim3_solver_dev", A->workspace, A->workspace_bytes, s3::solver_workspace(C, s1)));
  const hipStream_t s = fb::as_stream(stream);
  WS W;
  W.soa = static_cast<uint32_t *>(A->workspace);
  ItsTable its;
  for (int v = 0; v <= MAXH; v++) its.first_n[v] = INT_MAX;
  for (int N = A->min_inliers, top = 0; N <= s1 && top < A->max_iterations; N++) {  // (ends where the cap is reached: ~4 min_inliers)
    const int v = ransac_max_its(N, A->ransac_prob, A->min_inliers, A->max_iterations);
    for (; top < v; top++) its.first_n[top + 1] = N;
  }
  {
    fb::ProfScope prof_(fb::P_SIM3_PREP, s);
    k_sim3_prepare<<<C, PREP_THREADS, 0, s>>>(*A, its, W);
    FB_HIP(hipGetLastError());
  }
  {
    const s3::LdsPlan plan = s3::plan_solver(s1);
    const dim3 grid((A->max_iterations + HYP_PER_BLOCK - 1) / HYP_PER_BLOCK, C);
    if (plan.inLds) FB_TRY(s3::allow_large_lds<&k_sim3_hypotheses<true>>(s3::SOLVER_LDS_BUDGET));
    fb::ProfScope prof_(fb::P_SIM3_HYP, s);
    if (plan.inLds) k_sim3_hypotheses<true><<<grid, HYP_THREADS, plan.bytes, s>>>(*A, W);
    else k_sim3_hypotheses<false><<<grid, HYP_THREADS, 0, s>>>(*A, W);
    FB_HIP(hipGetLastError());
  }
  {
    fb::ProfScope prof_(fb::P_SIM3_ACCEPT, s);
    k_sim3_accept<<<C, 64, 0, s>>>(*A);
    FB_HIP(hipGetLastError());
  }
  return FB_OK;
}

// host-pointer drop-in: one staged upload, the same kernels, one staged download (fb::Stager)
int fb_sim3_solver(const fb_sim3_solver_args *H) {
  FB_TRY(fb::check_device());
  FB_TRY(check_args(H));
  fb_sim3_solver_args D = *H;
  const size_t C = H->n_cand, s1 = H->kf1.kf_stride, mw = (s1 + 31) / 32;
  fb::DevBuf ws;  // (declared first: it goes back to the pool after the Stager has waited)
  fb::Stager st;
  fb::stage_sim3_pair(st, D, C);
  st.in(D.kf1_index, s1 * 4);
  st.in(D.matches12, C * s1 * 4);
  st.in(D.accept_above, C * 4);
  st.in(D.rand_idx, C * MAXH * 3 * 4);
  st.out(D.N, C * 4, false);
  st.out(D.indices1, C * s1 * 4, true);  // copy-in: rows past N keep the caller's contents
  st.out(D.corr, C * s1 * sizeof(fb_sim3_corr), true);
  st.out(D.max_its, C * 4, false);
  st.out(D.n_hyp_done, C * 4, false);
  st.out(D.first_accept, C * 4, false);
  st.out(D.no_more, C * 4, false);
  st.out(D.s, C * MAXH * 4, true);       // rows past max_its keep the caller's contents
  st.out(D.R, C * MAXH * 36, true);
  st.out(D.t, C * MAXH * 12, true);
  st.out(D.n_inliers, C * MAXH * 4, true);
  st.out(D.accept, C * MAXH, false);
  st.out(D.inlier_mask, C * MAXH * mw * 4, true);
  FB_TRY(st.commit(nullptr));
  D.workspace_bytes = fb_sim3_solver_workspace((int)C, (int)s1);
  FB_TRY(ws.alloc(D.workspace_bytes));
  D.workspace = ws.p;
  FB_TRY(fb_sim3_solver_dev(&D, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
