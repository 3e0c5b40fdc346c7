// mapping.hip -- LocalMapping::CreateNewMapPoints on gfx950 (fb_create_new_map_points*, include/fishbird.h).
//
// Replaces (reference file:line):
//   LocalMapping::CreateNewMapPoints           src/LocalMapping.cc:231-476 (monocular branch)
//   LocalMapping::ComputeF12                   src/LocalMapping.cc:560-577
//   KeyFrame::ComputeSceneMedianDepth(2)       src/KeyFrame.cc:965-995
//   MapPoint::ComputeDistinctiveDescriptors    src/MapPoint.cc:242-307 (two observations)
//   MapPoint::UpdateNormalAndDepth             src/MapPoint.cc:330-371 (pKF1 = reference key frame)
//
// Four launches on the caller's stream, no host synchronisation (capturable):
//   k_np_prep              one workgroup per neighbour: camera centres, F12, baseline, exact median depth (radix select on
//                          order-preserving keys), the ratioBaselineDepth < 0.01 gate
//   k_match_triangulation  M7 (match_bow.hip) for every neighbour in one launch, KF1 shared, gated neighbours exit at once
//   k_np_claim             one lane per KF1 feature: walks the neighbours in covisibility order and keeps the first one whose
//                          match passes the parallax test, the triangulation and the checks (why this is the
//                          reference's serial loop)
//   k_np_emit              one workgroup per neighbour: ordered compaction by ascending idx1, the new points' fields and the
//                          in/out slot arrays
//
// Float / double seams (cv::Mat products, dot and norm): the products and dot products accumulate in double and round once
// to float (the convention of the project's other restatements of cv::Mat arithmetic, e.g. GetCameraCenter); cv::norm and
// cv::Mat::dot return double.  Parity with OpenCV itself is unpinned for the pieces OpenCV computes internally (3x3 inverse,
// the 4x4 SVD, Mat / scalar): OpenCV is not vendored.  The host restatement under tests/ repeats every expression below.
#include "fb_common.h"
#include "sim3_plan.h"  // s3::up256, s3::check_workspace

namespace fb {
int match_triangulation_shared(const fb_triangulation_args &A, const int32_t *skip, hipStream_t stream);  // match_bow.hip
}

namespace {

constexpr int MAXNB = FB_NEW_POINTS_MAX_NB;
constexpr int PREP_THREADS = 256;
constexpr int CLAIM_THREADS = 64;  // ~2000 serial lanes: spread over as many CUs as possible
constexpr int EMIT_THREADS = 1024;
constexpr int JACOBI_SWEEPS = 10;

struct NbStarts { int32_t s[MAXNB + 1]; };  // the host's nb_mp_start, as a kernel argument

struct WS {          // per neighbour arrays written by k_np_prep, packed the way fb_triangulation_args reads them
  float *F12;        // [n_nb][9]
  float *Cw1;        // [n_nb][3] pKF1's camera centre (the same for every neighbour)
  float *R2w;        // [n_nb][9]
  float *t2w;        // [n_nb][3]
  float *Ow2;        // [n_nb][3]
  int32_t *skip;     // [n_nb]
  int32_t *nmatch;   // [n_nb] M7's own counts (not the reference's: see nb_matches)
  int32_t *m12;      // [n_nb][kf1_stride]
  int32_t *win_nb;   // [kf1_stride]
  int32_t *win_idx2; // [kf1_stride]
  float *win_xw;     // [kf1_stride][3]
};

using s3::up256;

size_t carve(uint8_t *p, int n_nb, int s1, WS *w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { uint8_t *q = p ? p + off : nullptr; off += up256(bytes ? bytes : 1); return q; };
  WS d;
  d.F12 = reinterpret_cast<float *>(take((size_t)n_nb * 36));
  d.Cw1 = reinterpret_cast<float *>(take((size_t)n_nb * 12));
  d.R2w = reinterpret_cast<float *>(take((size_t)n_nb * 36));
  d.t2w = reinterpret_cast<float *>(take((size_t)n_nb * 12));
  d.Ow2 = reinterpret_cast<float *>(take((size_t)n_nb * 12));
  d.skip = reinterpret_cast<int32_t *>(take((size_t)n_nb * 4));
  d.nmatch = reinterpret_cast<int32_t *>(take((size_t)n_nb * 4));
  d.m12 = reinterpret_cast<int32_t *>(take((size_t)n_nb * s1 * 4));
  d.win_nb = reinterpret_cast<int32_t *>(take((size_t)s1 * 4));
  d.win_idx2 = reinterpret_cast<int32_t *>(take((size_t)s1 * 4));
  d.win_xw = reinterpret_cast<float *>(take((size_t)s1 * 12));
  if (w) *w = d;
  return off;
}

// ---- cv::Mat arithmetic in the form the reference's expressions take ------------------------------------------------
// sum_k a[k]*b[k] over three float pairs, in double, k ascending
__device__ __forceinline__ double dot3d(float a0, float a1, float a2, float b0, float b1, float b2) {
  return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}
__device__ __forceinline__ double norm3d(float a0, float a1, float a2) { return sqrt(dot3d(a0, a1, a2, a0, a1, a2)); }

// Ow = -Rcw^T tcw (KeyFrame::SetPose, KeyFrame.cc:110-111); T row-major 3x4
__device__ __forceinline__ void camera_center(const float *T, float O[3]) {
  for (int r = 0; r < 3; r++) O[r] = (float)(-dot3d(T[r], T[4 + r], T[8 + r], T[3], T[7], T[11]));
}

// C = A * B (3x3, row-major), one rounding per entry
__device__ __forceinline__ void gemm33(const float *A, const float *B, float *C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[i * 3 + j] = (float)dot3d(A[i * 3], A[i * 3 + 1], A[i * 3 + 2], B[j], B[3 + j], B[6 + j]);
}

// LocalMapping::ComputeF12 (LocalMapping.cc:560-577): K1^-T [t12]x R12 K2^-1, one key frame camera for both.
// K^-1 in closed form: cofactors in float over det3 (float) inverted in double.
__device__ void compute_F12(const float *T1, const float *T2, float fx, float fy, float cx, float cy, float F[9]) {
  float R12[9], t12[3];
  for (int i = 0; i < 3; i++)  // R12 = R1w * R2w^T
    for (int j = 0; j < 3; j++) R12[i * 3 + j] = (float)dot3d(T1[i * 4], T1[i * 4 + 1], T1[i * 4 + 2], T2[j * 4], T2[j * 4 + 1], T2[j * 4 + 2]);
  float M[9];  // -R1w * R2w^T (the scale -1 of the gemm is exact)
  for (int k = 0; k < 9; k++) M[k] = -R12[k];
  for (int r = 0; r < 3; r++)  // t12 = M * t2w + t1w (one gemm with beta = 1)
    t12[r] = (float)(dot3d(M[r * 3], M[r * 3 + 1], M[r * 3 + 2], T2[3], T2[7], T2[11]) + (double)T1[r * 4 + 3]);
  const float tx[9] = {0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f};  // SkewSymmetricMatrix
  const double d = 1.0 / (double)(fx * (fy * 1.0f - cy * 0.0f) - 0.0f * (0.0f * 1.0f - cy * 0.0f) + cx * (0.0f * 0.0f - fy * 0.0f));
  float Ki[9];
  Ki[0] = (float)((double)(fy * 1.0f - cy * 0.0f) * d);
  Ki[1] = (float)((double)(0.0f * 0.0f - 0.0f * 1.0f) * d);
  Ki[2] = (float)((double)(0.0f * cy - cx * fy) * d);
  Ki[3] = (float)((double)(cy * 0.0f - 0.0f * 1.0f) * d);
  Ki[4] = (float)((double)(fx * 1.0f - cx * 0.0f) * d);
  Ki[5] = (float)((double)(cx * 0.0f - fx * cy) * d);
  Ki[6] = (float)((double)(0.0f * 0.0f - fy * 0.0f) * d);
  Ki[7] = (float)((double)(0.0f * 0.0f - fx * 0.0f) * d);
  Ki[8] = (float)((double)(fx * fy - 0.0f * 0.0f) * d);
  const float KiT[9] = {Ki[0], Ki[3], Ki[6], Ki[1], Ki[4], Ki[7], Ki[2], Ki[5], Ki[8]};
  float P[9], Q[9];
  gemm33(KiT, tx, P);
  gemm33(P, R12, Q);
  gemm33(Q, Ki, F);
}

__device__ __forceinline__ uint32_t float_key(float f) {  // order-preserving (the median is taken in float order)
  if (f == 0.0f) f = 0.0f;                                 // -0 sorts with +0
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- one match (LocalMapping.cc:318-437, monocular) ------------------------------------------------------------------
enum { NP_OK = 0, NP_PARALLAX = 1, NP_W0 = 2, NP_BEHIND = 3, NP_CHI2 = 4, NP_DIST0 = 5, NP_SCALE = 6 };

struct Cam { float fx, fy, cx, cy, invfx, invfy; };

// Null vector of the 4x4 A (float) in double: one-sided Jacobi (Hestenes) with a fixed schedule of sweeps over the column
// pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); only + - * / sqrt, so a host restatement compiled without contraction repeats it
// bit for bit.  Returns V's column of the smallest column norm (first minimum).
__device__ __forceinline__ void jacobi_null4(const float (&Af)[4][4], double v[4]) {
  double a[4][4], V[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) { a[r][c] = (double)Af[r][c]; V[r][c] = r == c ? 1.0 : 0.0; }
#pragma unroll 1
  for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) { al = al + a[r][p] * a[r][p]; be = be + a[r][q] * a[r][q]; ga = ga + a[r][p] * a[r][q]; }
        if (ga == 0.0) continue;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const double ap = a[r][p], aq = a[r][q];
          a[r][p] = c * ap - s * aq;
          a[r][q] = s * ap + c * aq;
          const double vp = V[r][p], vq = V[r][q];
          V[r][p] = c * vp - s * vq;
          V[r][q] = s * vp + c * vq;
        }
      }
  }
  double best = 0.0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    double n = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) n = n + a[r][c] * a[r][c];
    if (c == 0 || n < best) { best = n; v[0] = V[0][c]; v[1] = V[1][c]; v[2] = V[2][c]; v[3] = V[3][c]; }
  }
}

__device__ int triangulate(const fb_keypoint &kp1, const fb_keypoint &kp2, const float *T1, const float *T2, const float *Ow1,
                           const float *Ow2, const Cam &K, const float *sf, const float *sig2, float ratioFactor, float X[3]) {
  // parallax (:318-329): xn = ((u-cx)*invf, (v-cy)*invf, 1); ray = Rwc * xn; cos as float of the double quotient
  const float xn1x = (kp1.x - K.cx) * K.invfx, xn1y = (kp1.y - K.cy) * K.invfy;
  const float xn2x = (kp2.x - K.cx) * K.invfx, xn2y = (kp2.y - K.cy) * K.invfy;
  float r1[3], r2[3];
  for (int r = 0; r < 3; r++) {
    r1[r] = (float)dot3d(T1[r], T1[4 + r], T1[8 + r], xn1x, xn1y, 1.0f);
    r2[r] = (float)dot3d(T2[r], T2[4 + r], T2[8 + r], xn2x, xn2y, 1.0f);
  }
  const float cosParallaxRays = (float)(dot3d(r1[0], r1[1], r1[2], r2[0], r2[1], r2[2]) / (norm3d(r1[0], r1[1], r1[2]) * norm3d(r2[0], r2[1], r2[2])));
  const float cosParallaxStereo = cosParallaxRays + 1;  // mono: both stereo terms equal it (:331-341)
  if (!(cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (double)cosParallaxRays < 0.9998)) return NP_PARALLAX;
  // linear triangulation (:346-362): A rows in float, null vector, x3D = v(0:3) / v(3)
  float A[4][4];
  for (int c = 0; c < 4; c++) {
    A[0][c] = xn1x * T1[8 + c] - T1[c];
    A[1][c] = xn1y * T1[8 + c] - T1[4 + c];
    A[2][c] = xn2x * T2[8 + c] - T2[c];
    A[3][c] = xn2y * T2[8 + c] - T2[4 + c];
  }
  double v[4];
  jacobi_null4(A, v);
  const float w = (float)v[3];
  if (w == 0) return NP_W0;                   // x3D.at<float>(3)==0 (:357)
  const float sc = (float)(1.0 / (double)w);  // Mat / double: a scale by 1/w
  X[0] = (float)v[0] * sc; X[1] = (float)v[1] * sc; X[2] = (float)v[2] * sc;
  // cheirality (:379-386): Rcw.row(2).dot(x3Dt) is double, + tcw(2) in double, stored as float
  const float z1 = (float)(dot3d(T1[8], T1[9], T1[10], X[0], X[1], X[2]) + (double)T1[11]);
  if (z1 <= 0) return NP_BEHIND;
  const float z2 = (float)(dot3d(T2[8], T2[9], T2[10], X[0], X[1], X[2]) + (double)T2[11]);
  if (z2 <= 0) return NP_BEHIND;
  // reprojection in KF1 and KF2 (:388-434): invz = 1.0/z in double, stored as float; chi2 compared in double
  {
    const float s2 = sig2[kp1.octave];
    const float x1 = (float)(dot3d(T1[0], T1[1], T1[2], X[0], X[1], X[2]) + (double)T1[3]);
    const float y1 = (float)(dot3d(T1[4], T1[5], T1[6], X[0], X[1], X[2]) + (double)T1[7]);
    const float invz1 = (float)(1.0 / (double)z1);
    const float u1 = K.fx * x1 * invz1 + K.cx, v1 = K.fy * y1 * invz1 + K.cy;
    const float ex = u1 - kp1.x, ey = v1 - kp1.y;
    if ((double)(ex * ex + ey * ey) > 5.991 * (double)s2) return NP_CHI2;
  }
  {
    const float s2 = sig2[kp2.octave];
    const float x2 = (float)(dot3d(T2[0], T2[1], T2[2], X[0], X[1], X[2]) + (double)T2[3]);
    const float y2 = (float)(dot3d(T2[4], T2[5], T2[6], X[0], X[1], X[2]) + (double)T2[7]);
    const float invz2 = (float)(1.0 / (double)z2);
    const float u2 = K.fx * x2 * invz2 + K.cx, v2 = K.fy * y2 * invz2 + K.cy;
    const float ex = u2 - kp2.x, ey = v2 - kp2.y;
    if ((double)(ex * ex + ey * ey) > 5.991 * (double)s2) return NP_CHI2;
  }
  // scale consistency (:439-455)
  const float dist1 = (float)norm3d(X[0] - Ow1[0], X[1] - Ow1[1], X[2] - Ow1[2]);
  const float dist2 = (float)norm3d(X[0] - Ow2[0], X[1] - Ow2[1], X[2] - Ow2[2]);
  if (dist1 == 0 || dist2 == 0) return NP_DIST0;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = sf[kp1.octave] / sf[kp2.octave];
  if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return NP_SCALE;
  return NP_OK;
}

// ---- k_np_prep ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PREP_THREADS) void k_np_prep(fb_new_points_args A, NbStarts S, WS W) {
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const float *T1 = A.Tcw1, *T2 = A.Tcw2 + (size_t)b * 12;
  __shared__ int s_hist[256];
  __shared__ uint32_t s_prefix, s_mask;
  __shared__ int s_k;
  const int m0 = S.s[b], n = S.s[b + 1] - S.s[b];  // n >= 1 (checked on the host)
  if (tid == 0) { s_prefix = 0; s_mask = 0; s_k = (n - 1) / 2; }  // vDepths[(size-1)/q], q = 2
  // ComputeSceneMedianDepth(2): z = Rcw.row(2).dot(x3Dw) + zcw as float; the k-th smallest by an 8-bit radix select
  for (int shift = 24; shift >= 0; shift -= 8) {
    s_hist[tid] = 0;  // PREP_THREADS == 256
    __syncthreads();
    const uint32_t prefix = s_prefix, mask = s_mask;
    for (int i = tid; i < n; i += nt) {
      const float *x = A.nb_mp_xw + (size_t)(m0 + i) * 3;
      const float z = (float)(dot3d(T2[8], T2[9], T2[10], x[0], x[1], x[2]) + (double)T2[11]);
      const uint32_t key = float_key(z);
      if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int k = s_k, cum = 0, d = 0;
      for (; d < 255; d++) {
        if (cum + s_hist[d] > k) break;
        cum += s_hist[d];
      }
      s_k = k - cum;
      s_prefix = prefix | ((uint32_t)d << shift);
      s_mask = mask | (255u << shift);
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const float median = key_float(s_prefix);
  float Ow1[3], Ow2[3];
  camera_center(T1, Ow1);
  camera_center(T2, Ow2);
  // baseline = cv::norm(Ow2 - Ow1) (:268-269); ratioBaselineDepth < 0.01 in double (:280-283)
  const float baseline = (float)norm3d(Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]);
  const float ratio = baseline / median;
  const int gated = (double)ratio < 0.01;
  compute_F12(T1, T2, A.fx, A.fy, A.cx, A.cy, W.F12 + (size_t)b * 9);
  for (int r = 0; r < 3; r++) {
    W.Cw1[b * 3 + r] = Ow1[r];
    W.Ow2[b * 3 + r] = Ow2[r];
    W.t2w[b * 3 + r] = T2[r * 4 + 3];
    for (int c = 0; c < 3; c++) W.R2w[b * 9 + r * 3 + c] = T2[r * 4 + c];
  }
  W.skip[b] = gated;
  A.nb_skipped[b] = gated;
  A.nb_matches[b] = 0;
  A.nb_new[b] = 0;
}

// ---- k_np_claim -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CLAIM_THREADS) void k_np_claim(fb_new_points_args A, WS W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.kf1_stride) return;
  int win = -1, w2 = -1;
  float X[3] = {0.0f, 0.0f, 0.0f};
  if (i < A.n1[0] && !A.has_mp1[i]) {
    const fb_keypoint kp1 = A.kps1[i];
    float T1[12];
    for (int k = 0; k < 12; k++) T1[k] = A.Tcw1[k];
    Cam K;
    K.fx = A.fx; K.fy = A.fy; K.cx = A.cx; K.cy = A.cy;
    K.invfx = 1.0f / A.fx; K.invfy = 1.0f / A.fy;  // Frame.cc: invfx = 1.0f/fx
    const float ratioFactor = 1.5f * A.scale_factor;  // :256
    for (int b = 0; b < A.n_nb; b++) {
      if (W.skip[b]) continue;
      const int m = W.m12[(size_t)b * A.kf1_stride + i];
      if (m < 0) continue;
      atomicAdd(&A.nb_matches[b], 1);  // vMatchedPairs of neighbour b holds idx1 (it was free when b was visited)
      const fb_keypoint kp2 = A.kps2[(size_t)b * A.kf2_stride + m];
      float T2[12];
      for (int k = 0; k < 12; k++) T2[k] = A.Tcw2[(size_t)b * 12 + k];
      if (triangulate(kp1, kp2, T1, T2, W.Cw1 + b * 3, W.Ow2 + b * 3, K, A.scale_factors, A.level_sigma2, ratioFactor, X) == NP_OK) {
        win = b;
        w2 = m;
        break;
      }
    }
  }
  W.win_nb[i] = win;
  W.win_idx2[i] = w2;
  if (win >= 0) {
    W.win_xw[(size_t)i * 3] = X[0]; W.win_xw[(size_t)i * 3 + 1] = X[1]; W.win_xw[(size_t)i * 3 + 2] = X[2];
    atomicAdd(&A.nb_new[win], 1);
  }
}

// ---- k_np_emit ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EMIT_THREADS) void k_np_emit(fb_new_points_args A, WS W) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  __shared__ int s_off, s_wave[EMIT_THREADS / 64];
  if (tid == 0) {
    int off = 0;
    for (int j = 0; j < b; j++) off += A.nb_new[j];
    s_off = off;
    if (b == A.n_nb - 1) *A.n_new = off + A.nb_new[b];
  }
  __syncthreads();
  if (A.nb_new[b] == 0) return;
  const float Ow1[3] = {W.Cw1[b * 3], W.Cw1[b * 3 + 1], W.Cw1[b * 3 + 2]}, Ow2[3] = {W.Ow2[b * 3], W.Ow2[b * 3 + 1], W.Ow2[b * 3 + 2]};
  const int before = A.nb_before_kf1[b];
  const float sfLast = A.scale_factors[A.n_levels - 1];
  int base = s_off;
  for (int c0 = 0; c0 < A.kf1_stride; c0 += EMIT_THREADS) {
    const int i = c0 + tid;
    const bool mine = i < A.kf1_stride && W.win_nb[i] == b;
    const unsigned long long ball = __ballot(mine);
    if (lane == 0) s_wave[wv] = __popcll(ball);
    __syncthreads();
    int pre = 0, tot = 0;
    for (int w = 0; w < EMIT_THREADS / 64; w++) { pre += w < wv ? s_wave[w] : 0; tot += s_wave[w]; }
    __syncthreads();
    if (mine) {
      const int row = base + pre + __popcll(ball & ((1ull << lane) - 1ull));
      const int idx2 = W.win_idx2[i];
      const float X[3] = {W.win_xw[(size_t)i * 3], W.win_xw[(size_t)i * 3 + 1], W.win_xw[(size_t)i * 3 + 2]};
      // UpdateNormalAndDepth (MapPoint.cc:330-371): normal = (n1/|n1| + n2/|n2|) / 2, distances from pKF1
      const float a0 = X[0] - Ow1[0], a1 = X[1] - Ow1[1], a2 = X[2] - Ow1[2];
      const float b0 = X[0] - Ow2[0], b1 = X[1] - Ow2[1], b2 = X[2] - Ow2[2];
      const double na = norm3d(a0, a1, a2), nb = norm3d(b0, b1, b2);
      const float sa = (float)(1.0 / na), sb = (float)(1.0 / nb);
      float *N = A.normal + (size_t)row * 3;
      N[0] = ((0.0f + a0 * sa) + b0 * sb) * 0.5f;  // normal starts at zeros (:349) and gains one term per observation
      N[1] = ((0.0f + a1 * sa) + b1 * sb) * 0.5f;
      N[2] = ((0.0f + a2 * sa) + b2 * sb) * 0.5f;
      const float dist = (float)na;
      const float maxd = dist * A.scale_factors[A.kps1[i].octave];
      A.max_dist[row] = maxd;
      A.min_dist[row] = maxd / sfLast;
      float *Xo = A.xw + (size_t)row * 3;
      Xo[0] = X[0]; Xo[1] = X[1]; Xo[2] = X[2];
      // ComputeDistinctiveDescriptors with two observations: the first in mObservations' (pointer) order
      const uint4 *src = reinterpret_cast<const uint4 *>(before ? A.desc2 + ((size_t)b * A.kf2_stride + idx2) * 32 : A.desc1 + (size_t)i * 32);
      uint4 *dst = reinterpret_cast<uint4 *>(A.desc + (size_t)row * 32);
      dst[0] = src[0];
      dst[1] = src[1];
      A.idx1[row] = i;
      A.nb[row] = b;
      A.idx2[row] = idx2;
      A.kf1_new[i] = row;
      A.has_mp1[i] = 1;
      A.has_mp2[(size_t)b * A.kf2_stride + idx2] = 1;
      atomicMax(&A.kf2_new[(size_t)b * A.kf2_stride + idx2], row);  // the later AddMapPoint wins the slot
    }
    base += tot;
  }
}

int check_args(const fb_new_points_args *A) {
  FB_ARG(A && A->n_nb >= 0 && A->n_nb <= MAXNB && A->kf1_stride > 0 && A->kf2_stride > 0);
  if (A->matcher.check_orientation != 0) {
    fb::set_error("fb_create_new_map_points: check_orientation must be 0 (ORBmatcher(0.6,false), LocalMapping.cc:239)");
    return FB_ERR_ARG;
  }
  FB_ARG(A->n_levels >= 1 && A->n_levels <= FB_MAX_LEVELS);
  if (A->n_nb > 0) {
    FB_ARG(A->nb_mp_start && A->nb_mp_start[0] == 0);
    for (int b = 0; b < A->n_nb; b++)
      if (A->nb_mp_start[b + 1] <= A->nb_mp_start[b]) {
        fb::set_error("fb_create_new_map_points: neighbour %d has no map point (ComputeSceneMedianDepth of an empty key frame)", b);
        return FB_ERR_ARG;
      }
  }
  return FB_OK;
}

}  // namespace

extern "C" {

size_t fb_create_new_map_points_workspace(int n_nb, int kf1_stride) {
  if (n_nb < 0 || kf1_stride < 0) return 0;
  return carve(nullptr, n_nb, kf1_stride, nullptr);
}

int fb_create_new_map_points_dev(const fb_new_points_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_TRY(check_args(A));
  FB_ARG(A->n1 && A->kps1 && A->desc1 && A->Tcw1 && A->has_mp1 && A->n_new && A->kf1_new);
  const hipStream_t s = fb::as_stream(stream);
  FB_HIP(hipMemsetAsync(A->kf1_new, 0xff, (size_t)A->kf1_stride * 4, s));
  if (A->n_nb == 0) {
    FB_HIP(hipMemsetAsync(A->n_new, 0, 4, s));
    return FB_OK;
  }
  FB_ARG(A->n2 && A->kps2 && A->desc2 && A->Tcw2 && A->has_mp2 && A->nb_mp_xw && A->nb_before_kf1 && A->xw && A->normal &&
         A->max_dist && A->min_dist && A->desc && A->idx1 && A->nb && A->idx2 && A->kf2_new && A->nb_matches && A->nb_new && A->nb_skipped);
  FB_TRY(s3::check_workspace("fb_create_new_map_points_dev", A->workspace, A->workspace_bytes, carve(nullptr, A->n_nb, A->kf1_stride, nullptr)));
  WS W;
  carve(static_cast<uint8_t *>(A->workspace), A->n_nb, A->kf1_stride, &W);
  NbStarts S;
  for (int b = 0; b <= A->n_nb; b++) S.s[b] = A->nb_mp_start[b];
  FB_HIP(hipMemsetAsync(A->kf2_new, 0xff, (size_t)A->n_nb * A->kf2_stride * 4, s));
  {
    fb::ProfScope prof_(fb::P_NP_PREP, s);
    k_np_prep<<<A->n_nb, PREP_THREADS, 0, s>>>(*A, S, W);
    FB_HIP(hipGetLastError());
  }
  fb_triangulation_args M{};
  M.batch = A->n_nb; M.kf1_stride = A->kf1_stride; M.kf2_stride = A->kf2_stride;
  M.n1 = A->n1; M.kps1 = A->kps1; M.desc1 = A->desc1; M.has_mp1 = A->has_mp1; M.fv1 = A->fv1;
  M.n2 = A->n2; M.kps2 = A->kps2; M.desc2 = A->desc2; M.has_mp2 = A->has_mp2; M.fv2 = A->fv2;
  M.F12 = W.F12; M.Cw1 = W.Cw1; M.R2w = W.R2w; M.t2w = W.t2w;  // written by k_np_prep
  M.fx = A->fx; M.fy = A->fy; M.cx = A->cx; M.cy = A->cy;
  for (int l = 0; l < FB_MAX_LEVELS; l++) { M.scale_factors[l] = A->scale_factors[l]; M.level_sigma2[l] = A->level_sigma2[l]; }
  M.matcher = A->matcher;
  M.matches12 = W.m12;
  M.nmatches = W.nmatch;
  FB_TRY(fb::match_triangulation_shared(M, W.skip, s));
  {
    fb::ProfScope prof_(fb::P_NP_CLAIM, s);
    k_np_claim<<<(A->kf1_stride + CLAIM_THREADS - 1) / CLAIM_THREADS, CLAIM_THREADS, 0, s>>>(*A, W);
    FB_HIP(hipGetLastError());
  }
  {
    fb::ProfScope prof_(fb::P_NP_EMIT, s);
    k_np_emit<<<A->n_nb, EMIT_THREADS, 0, s>>>(*A, W);
    FB_HIP(hipGetLastError());
  }
  return FB_OK;
}

// host-pointer drop-in: one staged upload, the same kernels, one staged download (fb::Stager)
int fb_create_new_map_points(const fb_new_points_args *H) {
  FB_TRY(fb::check_device());
  FB_TRY(check_args(H));
  FB_ARG(H->n1 && H->has_mp1 && H->n_new && H->kf1_new);
  fb_new_points_args D = *H;
  const size_t B = H->n_nb, s1 = H->kf1_stride, s2 = H->kf2_stride;
  const size_t nmp = B ? (size_t)H->nb_mp_start[B] : 0;
  fb::DevBuf ws;  // the call's workspace (declared first: it goes back to the pool after the Stager has waited)
  fb::Stager st;
  st.in(D.n1, 4); st.in(D.kps1, s1 * sizeof(fb_keypoint)); st.in(D.desc1, s1 * 32); st.in(D.Tcw1, 48);
  st.in(D.n2, B * 4); st.in(D.kps2, B * s2 * sizeof(fb_keypoint)); st.in(D.desc2, B * s2 * 32); st.in(D.Tcw2, B * 48);
  st.in(D.nb_mp_xw, nmp * 12); st.in(D.nb_before_kf1, B);  // (nb_mp_start is a host array in both entry points)
  fb::stage(st, D.fv1, 1);
  fb::stage(st, D.fv2, B);
  st.out(D.has_mp1, s1, true);
  st.out(D.has_mp2, B * s2, true);
  st.out(D.n_new, 4, false);
  st.out(D.xw, s1 * 12, true);  // copy-in: rows past n_new keep the caller's contents
  st.out(D.normal, s1 * 12, true);
  st.out(D.max_dist, s1 * 4, true);
  st.out(D.min_dist, s1 * 4, true);
  st.out(D.desc, s1 * 32, true);
  st.out(D.idx1, s1 * 4, true);
  st.out(D.nb, s1 * 4, true);
  st.out(D.idx2, s1 * 4, true);
  st.out(D.kf1_new, s1 * 4, false);
  st.out(D.kf2_new, B * s2 * 4, false);
  st.out(D.nb_matches, B * 4, false);
  st.out(D.nb_new, B * 4, false);
  st.out(D.nb_skipped, B * 4, false);
  FB_TRY(st.commit(nullptr));
  D.workspace_bytes = fb_create_new_map_points_workspace((int)B, (int)s1);
  FB_TRY(ws.alloc(D.workspace_bytes));
  D.workspace = ws.p;
  FB_TRY(fb_create_new_map_points_dev(&D, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
