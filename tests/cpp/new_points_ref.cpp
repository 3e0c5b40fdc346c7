// new_points_ref.cpp -- host restatement of LocalMapping::CreateNewMapPoints' arithmetic (monocular), TEST INFRASTRUCTURE.
// Built by tests/new_points_ref.py with g++ -ffp-contract=off; the serial loop over the neighbours (and the call of the
// oracle's SearchForTriangulation with the current has_mp1) lives there.  Reference lines: src/LocalMapping.cc.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {
struct Kp { float x, y, size, angle, response; int32_t octave; };  // fb_keypoint

// cv::Mat float products / dot: double accumulation, one rounding; cv::norm: double
double dot(const float *a, const float *b) {
  double s = (double)a[0] * (double)b[0];
  s = s + (double)a[1] * (double)b[1];
  s = s + (double)a[2] * (double)b[2];
  return s;
}
double nrm(const float *a) { return std::sqrt(dot(a, a)); }
void rowT(const float *T, int r, float o[3]) { o[0] = T[r * 4]; o[1] = T[r * 4 + 1]; o[2] = T[r * 4 + 2]; }
void colT(const float *T, int c, float o[3]) { o[0] = T[c]; o[1] = T[4 + c]; o[2] = T[8 + c]; }
void center(const float *T, float O[3]) {  // -Rcw^T tcw
  const float t[3] = {T[3], T[7], T[11]};
  for (int r = 0; r < 3; r++) { float c[3]; colT(T, r, c); O[r] = (float)(-dot(c, t)); }
}
void mul33(const float *A, const float *B, float *C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) { const float b[3] = {B[j], B[3 + j], B[6 + j]}; C[i * 3 + j] = (float)dot(A + i * 3, b); }
}
}  // namespace

extern "C" {

// ComputeSceneMedianDepth(2), the baseline gate and ComputeF12 for one neighbour (LocalMapping.cc:264-289, 560-577).
// Returns 1 when the neighbour is skipped.
int npr_neighbour(const float *T1, const float *T2, const float *xw, int n, float fx, float fy, float cx, float cy,
                  float *F12, float *Ow1, float *Ow2, float *median_out) {
  center(T1, Ow1);
  center(T2, Ow2);
  const float vb[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
  const float baseline = (float)nrm(vb);
  std::vector<float> depths;
  float r2[3];
  rowT(T2, 2, r2);
  for (int i = 0; i < n; i++) depths.push_back((float)(dot(r2, xw + 3 * i) + (double)T2[11]));
  std::sort(depths.begin(), depths.end());
  const float median = depths[(depths.size() - 1) / 2];
  *median_out = median;
  const float ratio = baseline / median;
  // F12 = K^-T [t12]x R12 K^-1
  float R12[9], M[9], t12[3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) { float a[3], b[3]; rowT(T1, i, a); rowT(T2, j, b); R12[i * 3 + j] = (float)dot(a, b); }
  for (int k = 0; k < 9; k++) M[k] = -R12[k];
  const float t2[3] = {T2[3], T2[7], T2[11]};
  for (int r = 0; r < 3; r++) t12[r] = (float)(dot(M + r * 3, t2) + (double)T1[r * 4 + 3]);
  const float S[9] = {0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f};
  // K^-1 by cofactors / det (K = [fx 0 cx; 0 fy cy; 0 0 1])
  const float k[9] = {fx, 0.0f, cx, 0.0f, fy, cy, 0.0f, 0.0f, 1.0f};
  const float det = k[0] * (k[4] * k[8] - k[5] * k[7]) - k[1] * (k[3] * k[8] - k[5] * k[6]) + k[2] * (k[3] * k[7] - k[4] * k[6]);
  const double id = 1.0 / (double)det;
  float Ki[9];
  Ki[0] = (float)((double)(k[4] * k[8] - k[5] * k[7]) * id);
  Ki[1] = (float)((double)(k[2] * k[7] - k[1] * k[8]) * id);
  Ki[2] = (float)((double)(k[1] * k[5] - k[2] * k[4]) * id);
  Ki[3] = (float)((double)(k[5] * k[6] - k[3] * k[8]) * id);
  Ki[4] = (float)((double)(k[0] * k[8] - k[2] * k[6]) * id);
  Ki[5] = (float)((double)(k[2] * k[3] - k[0] * k[5]) * id);
  Ki[6] = (float)((double)(k[3] * k[7] - k[4] * k[6]) * id);
  Ki[7] = (float)((double)(k[1] * k[6] - k[0] * k[7]) * id);
  Ki[8] = (float)((double)(k[0] * k[4] - k[1] * k[3]) * id);
  const float KiT[9] = {Ki[0], Ki[3], Ki[6], Ki[1], Ki[4], Ki[7], Ki[2], Ki[5], Ki[8]};
  float P[9], Q[9];
  mul33(KiT, S, P);
  mul33(P, R12, Q);
  mul33(Q, Ki, F12);
  return ratio < 0.01 ? 1 : 0;
}

// right singular vector of the smallest singular value: one-sided Jacobi, 10 sweeps of the pairs (p<q) in order
void npr_null_vector(const float *A16, double *v) {
  double a[4][4], V[4][4];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) { a[r][c] = A16[r * 4 + c]; V[r][c] = r == c ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 10; sweep++)
    for (int p = 0; p < 3; p++)
      for (int q = p + 1; q < 4; q++) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int r = 0; r < 4; r++) { al = al + a[r][p] * a[r][p]; be = be + a[r][q] * a[r][q]; ga = ga + a[r][p] * a[r][q]; }
        if (ga == 0.0) continue;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
        for (int r = 0; r < 4; r++) {
          const double ap = a[r][p], aq = a[r][q], vp = V[r][p], vq = V[r][q];
          a[r][p] = c * ap - s * aq; a[r][q] = s * ap + c * aq;
          V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
        }
      }
  int jb = 0;
  double best = 0.0;
  for (int c = 0; c < 4; c++) {
    double n = 0.0;
    for (int r = 0; r < 4; r++) n = n + a[r][c] * a[r][c];
    if (c == 0 || n < best) { best = n; jb = c; }
  }
  for (int r = 0; r < 4; r++) v[r] = V[r][jb];
}

// One match, LocalMapping.cc:313-455 (monocular).  0 = a new point, else the check that rejected it:
// 1 parallax, 2 w == 0, 3 behind a camera, 4 chi2, 5 zero distance, 6 scale.
int npr_triangulate(const Kp *kp1, const Kp *kp2, const float *T1, const float *T2, const float *Ow1, const float *Ow2,
                    float fx, float fy, float cx, float cy, const float *sf, const float *sig2, float scale_factor, float *X) {
  const float invfx = 1.0f / fx, invfy = 1.0f / fy;
  const float ratioFactor = 1.5f * scale_factor;
  const float xn1[3] = {(kp1->x - cx) * invfx, (kp1->y - cy) * invfy, 1.0f};
  const float xn2[3] = {(kp2->x - cx) * invfx, (kp2->y - cy) * invfy, 1.0f};
  float ray1[3], ray2[3];
  for (int r = 0; r < 3; r++) {
    float c1[3], c2[3];
    colT(T1, r, c1); colT(T2, r, c2);
    ray1[r] = (float)dot(c1, xn1);
    ray2[r] = (float)dot(c2, xn2);
  }
  const float cosParallaxRays = (float)(dot(ray1, ray2) / (nrm(ray1) * nrm(ray2)));
  float cosParallaxStereo = cosParallaxRays + 1;
  const float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
  cosParallaxStereo = std::min(cosParallaxStereo1, cosParallaxStereo2);
  if (!(cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && cosParallaxRays < 0.9998)) return 1;
  float A[16];
  for (int c = 0; c < 4; c++) {
    A[0 * 4 + c] = xn1[0] * T1[8 + c] - T1[c];
    A[1 * 4 + c] = xn1[1] * T1[8 + c] - T1[4 + c];
    A[2 * 4 + c] = xn2[0] * T2[8 + c] - T2[c];
    A[3 * 4 + c] = xn2[1] * T2[8 + c] - T2[4 + c];
  }
  double v[4];
  npr_null_vector(A, v);
  const float vf[4] = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  if (vf[3] == 0) return 2;
  const float alpha = (float)(1.0 / (double)vf[3]);
  for (int r = 0; r < 3; r++) X[r] = vf[r] * alpha;
  float row[3];
  rowT(T1, 2, row);
  const float z1 = (float)(dot(row, X) + (double)T1[11]);
  if (z1 <= 0) return 3;
  rowT(T2, 2, row);
  const float z2 = (float)(dot(row, X) + (double)T2[11]);
  if (z2 <= 0) return 3;
  {
    const float sigmaSquare1 = sig2[kp1->octave];
    rowT(T1, 0, row);
    const float x1 = (float)(dot(row, X) + (double)T1[3]);
    rowT(T1, 1, row);
    const float y1 = (float)(dot(row, X) + (double)T1[7]);
    const float invz1 = 1.0 / z1;
    const float u1 = fx * x1 * invz1 + cx, v1 = fy * y1 * invz1 + cy;
    const float errX1 = u1 - kp1->x, errY1 = v1 - kp1->y;
    if ((errX1 * errX1 + errY1 * errY1) > 5.991 * sigmaSquare1) return 4;
  }
  {
    const float sigmaSquare2 = sig2[kp2->octave];
    rowT(T2, 0, row);
    const float x2 = (float)(dot(row, X) + (double)T2[3]);
    rowT(T2, 1, row);
    const float y2 = (float)(dot(row, X) + (double)T2[7]);
    const float invz2 = 1.0 / z2;
    const float u2 = fx * x2 * invz2 + cx, v2 = fy * y2 * invz2 + cy;
    const float errX2 = u2 - kp2->x, errY2 = v2 - kp2->y;
    if ((errX2 * errX2 + errY2 * errY2) > 5.991 * sigmaSquare2) return 4;
  }
  const float n1[3] = {X[0] - Ow1[0], X[1] - Ow1[1], X[2] - Ow1[2]};
  const float n2[3] = {X[0] - Ow2[0], X[1] - Ow2[1], X[2] - Ow2[2]};
  const float dist1 = (float)nrm(n1), dist2 = (float)nrm(n2);
  if (dist1 == 0 || dist2 == 0) return 5;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = sf[kp1->octave] / sf[kp2->octave];
  if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return 6;
  return 0;
}

// UpdateNormalAndDepth for a two-observation point whose reference key frame is pKF1 (MapPoint.cc:330-371)
void npr_normal_depth(const float *X, const float *Ow1, const float *Ow2, float sf_octave1, float sf_last, float *normal,
                      float *max_dist, float *min_dist) {
  const float n1[3] = {X[0] - Ow1[0], X[1] - Ow1[1], X[2] - Ow1[2]};
  const float n2[3] = {X[0] - Ow2[0], X[1] - Ow2[1], X[2] - Ow2[2]};
  const double d1 = nrm(n1), d2 = nrm(n2);
  const float s1 = (float)(1.0 / d1), s2 = (float)(1.0 / d2);
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (int r = 0; r < 3; r++) acc[r] = acc[r] + n1[r] * s1;
  for (int r = 0; r < 3; r++) acc[r] = acc[r] + n2[r] * s2;
  for (int r = 0; r < 3; r++) normal[r] = acc[r] * 0.5f;
  const float dist = (float)d1;
  *max_dist = dist * sf_octave1;
  *min_dist = *max_dist / sf_last;
}

}  // extern "C"
