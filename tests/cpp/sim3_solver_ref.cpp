// sim3_solver_ref.cpp -- host restatement of the reference's Sim3Solver (src/Sim3Solver.cc), TEST INFRASTRUCTURE.
// Built by tests/sim3_solver_ref.py with g++ -O2 -ffp-contract=off, no dependencies.  The literal serial class: the
// constructor loop, SetRansacParameters, iterate() with its persistent state, ComputeSim3 step by step (libm atan2 / sin /
// cos for the angle-axis -> Rodrigues route) and CheckInliers.  RandomInt's return values come from a table indexed by the
// iteration, (rand[k][0..2] for mnIterations = k+1).  Every iteration is logged, with two figures the tests use to set
// aside razor-edge hypotheses: the smallest |err - thr| / thr over all correspondences and both sides, and the relative gap
// (l0 - l1) / l0 of the two largest eigenvalues of N.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct V3 { float v[3]; };
struct V2 { float v[2]; };

// cv::Mat 3x3 * 3x1 + 3x1 in float (the project's convention for products without a transpose flag)
V3 affine(const float *T /* row-major 3x4 */, const V3 &X) {
  V3 o;
  for (int r = 0; r < 3; r++) o.v[r] = ((T[r * 4] * X.v[0] + T[r * 4 + 1] * X.v[1]) + T[r * 4 + 2] * X.v[2]) + T[r * 4 + 3];
  return o;
}

// cv::eigen on a symmetric CV_32F 4x4: Jacobi in float, eigenvalues descending, eigenvectors as rows (restated as the cyclic
// Jacobi with eight sweeps; OpenCV is not vendored: parity unpinned)
void eigen4(const float Nin[4][4], float eval[4], float evec[4][4]) {
  float a[4][4], V[4][4];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) { a[r][c] = Nin[r][c]; V[r][c] = r == c ? 1.0f : 0.0f; }
  for (int sweep = 0; sweep < 8; sweep++)
    for (int p = 0; p < 3; p++)
      for (int q = p + 1; q < 4; q++) {
        const float apq = a[p][q];
        if (apq == 0.0f) continue;
        const float zeta = (a[q][q] - a[p][p]) / (2.0f * apq);
        const float t = (zeta >= 0.0f ? 1.0f : -1.0f) / (std::fabs(zeta) + std::sqrt(1.0f + zeta * zeta));
        const float c = 1.0f / std::sqrt(1.0f + t * t), s = c * t;
        for (int k = 0; k < 4; k++) {
          const float x = a[k][p], y = a[k][q];
          a[k][p] = c * x - s * y;
          a[k][q] = s * x + c * y;
        }
        for (int k = 0; k < 4; k++) {
          const float x = a[p][k], y = a[q][k];
          a[p][k] = c * x - s * y;
          a[q][k] = s * x + c * y;
        }
        for (int k = 0; k < 4; k++) {
          const float x = V[k][p], y = V[k][q];
          V[k][p] = c * x - s * y;
          V[k][q] = s * x + c * y;
        }
      }
  int order[4] = {0, 1, 2, 3};
  std::stable_sort(order, order + 4, [&](int i, int j) { return a[i][i] > a[j][j]; });
  for (int r = 0; r < 4; r++) {
    eval[r] = a[order[r]][order[r]];
    for (int c = 0; c < 4; c++) evec[r][c] = V[c][order[r]];
  }
}

struct Solver {
  // constructor state
  int mN1 = 0, N = 0;
  std::vector<int> mvnIndices1;
  std::vector<V3> mvX3Dc1, mvX3Dc2;
  std::vector<V2> mvP1im1, mvP2im2;
  std::vector<size_t> mvnMaxError1, mvnMaxError2, mvAllIndices;
  float K1[4], K2[4];
  bool mbFixScale = false;
  // ransac
  double mRansacProb = 0.99;
  int mRansacMinInliers = 6, mRansacMaxIts = 300, mnIterations = 0, mnBestInliers = 0;
  // current estimation
  float mR12i[9], mt12i[3], ms12i = 0, mT12i[12], mT21i[12];
  std::vector<bool> mvbInliersi, mvbBestInliers;
  int mnInliersi = 0;
  float mBestRotation[9], mBestTranslation[3], mBestScale = 0;
  double gap = 0, razor = 0;
  int nRazor = 0;  // correspondences of this iteration with |err - thr| / thr < 1e-4 on either side
  std::vector<bool> inBand;  // which ones
  // log of every iteration
  struct Row { float s, R[9], t[3]; int n; std::vector<bool> in, band; double razor, gap; int best, ret, nRazor; };
  std::vector<Row> log;

  void FromCameraToImage(const std::vector<V3> &P, std::vector<V2> &o, const float *K) {
    const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    o.clear();
    for (size_t i = 0; i < P.size(); i++) {
      const float invz = 1 / (P[i].v[2]);
      const float x = P[i].v[0] * invz;
      const float y = P[i].v[1] * invz;
      V2 p;
      p.v[0] = fx * x + cx;
      p.v[1] = fy * y + cy;
      o.push_back(p);
    }
  }

  void Project(const std::vector<V3> &P, std::vector<V2> &o, const float *T, const float *K) {
    const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    o.clear();
    for (size_t i = 0; i < P.size(); i++) {
      const V3 c = affine(T, P[i]);
      const float invz = 1 / (c.v[2]);
      const float x = c.v[0] * invz;
      const float y = c.v[1] * invz;
      V2 p;
      p.v[0] = fx * x + cx;
      p.v[1] = fy * y + cy;
      o.push_back(p);
    }
  }

  void SetRansacParameters(double probability, int minInliers, int maxIterations) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    N = (int)mvX3Dc1.size();
    mvbInliersi.resize(N);
    float epsilon = (float)mRansacMinInliers / N;
    int nIterations;
    if (mRansacMinInliers == N) {
      nIterations = 1;
    } else {
      const double x = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(epsilon, 3)));
      nIterations = x < (double)mRansacMaxIts ? (int)x : mRansacMaxIts;  // (int)inf is undefined: min() with the cap first
    }
    mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
    mnIterations = 0;
  }

  // P1, P2: 3x3, samples as columns
  void ComputeSim3(const float P1[3][3], const float P2[3][3]) {
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
    for (int r = 0; r < 3; r++) {  // cv::reduce(SUM) then C / P.cols
      const float s1 = (P1[r][0] + P1[r][1]) + P1[r][2], s2 = (P2[r][0] + P2[r][1]) + P2[r][2];
      O1[r] = (float)((double)s1 * (1.0 / 3.0));
      O2[r] = (float)((double)s2 * (1.0 / 3.0));
      for (int i = 0; i < 3; i++) { Pr1[r][i] = P1[r][i] - O1[r]; Pr2[r][i] = P2[r][i] - O2[r]; }
    }
    float M[3][3];  // Pr2 * Pr1.t()
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double acc = (double)Pr2[i][0] * (double)Pr1[j][0];
        acc = acc + (double)Pr2[i][1] * (double)Pr1[j][1];
        acc = acc + (double)Pr2[i][2] * (double)Pr1[j][2];
        M[i][j] = (float)acc;
      }
    double N11, N12, N13, N14, N22, N23, N24, N33, N34, N44;
    N11 = M[0][0] + M[1][1] + M[2][2];
    N12 = M[1][2] - M[2][1];
    N13 = M[2][0] - M[0][2];
    N14 = M[0][1] - M[1][0];
    N22 = M[0][0] - M[1][1] - M[2][2];
    N23 = M[0][1] + M[1][0];
    N24 = M[2][0] + M[0][2];
    N33 = -M[0][0] + M[1][1] - M[2][2];
    N34 = M[1][2] + M[2][1];
    N44 = -M[0][0] - M[1][1] + M[2][2];
    const float Nm[4][4] = {{(float)N11, (float)N12, (float)N13, (float)N14}, {(float)N12, (float)N22, (float)N23, (float)N24},
                            {(float)N13, (float)N23, (float)N33, (float)N34}, {(float)N14, (float)N24, (float)N34, (float)N44}};
    float eval[4], evec[4][4];
    eigen4(Nm, eval, evec);
    gap = ((double)eval[0] - (double)eval[1]) / (double)eval[0];
    float vec[3] = {evec[0][1], evec[0][2], evec[0][3]};
    const double nv = std::sqrt(((double)vec[0] * vec[0] + (double)vec[1] * vec[1]) + (double)vec[2] * vec[2]);  // cv::norm
    const double ang = std::atan2(nv, (double)evec[0][0]);
    const double alpha = (2 * ang) / nv;  // vec = 2*ang*vec/norm(vec): one scale of the float row
    for (int i = 0; i < 3; i++) vec[i] = (float)((double)vec[i] * alpha);
    {  // cv::Rodrigues(vec, R): double inside, stored as float
      double r[3] = {vec[0], vec[1], vec[2]};
      const double theta = std::sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
      if (theta < 2.220446049250313e-16) {
        for (int i = 0; i < 9; i++) mR12i[i] = (i % 4 == 0) ? 1.0f : 0.0f;
      } else {
        const double c = std::cos(theta), s = std::sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
        r[0] *= it; r[1] *= it; r[2] *= it;
        const double rrt[9] = {r[0] * r[0], r[0] * r[1], r[0] * r[2], r[0] * r[1], r[1] * r[1], r[1] * r[2], r[0] * r[2], r[1] * r[2], r[2] * r[2]};
        const double rx[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
        for (int i = 0; i < 9; i++) mR12i[i] = (float)(c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i] + s * rx[i]);
      }
    }
    float P3[3][3];  // mR12i * Pr2
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) P3[i][j] = (mR12i[i * 3] * Pr2[0][j] + mR12i[i * 3 + 1] * Pr2[1][j]) + mR12i[i * 3 + 2] * Pr2[2][j];
    if (!mbFixScale) {
      double nom = 0;  // Pr1.dot(P3)
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) nom += (double)Pr1[i][j] * (double)P3[i][j];
      double den = 0;  // cv::pow(P3, 2, aux_P3) in float, summed in double
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { const float sq = P3[i][j] * P3[i][j]; den += sq; }
      ms12i = (float)(nom / den);
    } else {
      ms12i = 1.0f;
    }
    for (int i = 0; i < 3; i++) {  // mt12i = O1 - ms12i*mR12i*O2
      const float ro = (mR12i[i * 3] * O2[0] + mR12i[i * 3 + 1] * O2[1]) + mR12i[i * 3 + 2] * O2[2];
      mt12i[i] = O1[i] - ms12i * ro;
    }
    for (int i = 0; i < 3; i++) {  // T12 = [sR | t]
      for (int j = 0; j < 3; j++) mT12i[i * 4 + j] = ms12i * mR12i[i * 3 + j];
      mT12i[i * 4 + 3] = mt12i[i];
    }
    const double inv = 1.0 / ms12i;  // sRinv = (1.0/ms12i)*mR12i.t(); tinv = -sRinv*mt12i
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) mT21i[i * 4 + j] = (float)((double)mR12i[j * 3 + i] * inv);
    for (int i = 0; i < 3; i++)
      mT21i[i * 4 + 3] = -((mT21i[i * 4] * mt12i[0] + mT21i[i * 4 + 1] * mt12i[1]) + mT21i[i * 4 + 2] * mt12i[2]);
  }

  void CheckInliers() {
    std::vector<V2> vP1im2, vP2im1;
    Project(mvX3Dc2, vP2im1, mT12i, K1);
    Project(mvX3Dc1, vP1im2, mT21i, K2);
    mnInliersi = 0;
    razor = 1e300;
    nRazor = 0;
    inBand.assign(mvP1im1.size(), false);
    for (size_t i = 0; i < mvP1im1.size(); i++) {
      const float d1[2] = {mvP1im1[i].v[0] - vP2im1[i].v[0], mvP1im1[i].v[1] - vP2im1[i].v[1]};
      const float d2[2] = {vP1im2[i].v[0] - mvP2im2[i].v[0], vP1im2[i].v[1] - mvP2im2[i].v[1]};
      const float err1 = (float)((double)d1[0] * (double)d1[0] + (double)d1[1] * (double)d1[1]);  // Mat::dot is double
      const float err2 = (float)((double)d2[0] * (double)d2[0] + (double)d2[1] * (double)d2[1]);
      if (err1 < mvnMaxError1[i] && err2 < mvnMaxError2[i]) {
        mvbInliersi[i] = true;
        mnInliersi++;
      } else {
        mvbInliersi[i] = false;
      }
      const double r1 = std::fabs((double)err1 - (double)mvnMaxError1[i]) / (double)mvnMaxError1[i];
      const double r2 = std::fabs((double)err2 - (double)mvnMaxError2[i]) / (double)mvnMaxError2[i];
      if (r1 < razor) razor = r1;  // (NaN never lowers it: a NaN error is an outlier on every implementation)
      if (r2 < razor) razor = r2;
      if (r1 < 1e-4 || r2 < 1e-4) { nRazor++; inBand[i] = true; }
    }
  }

  // -> 1 when iterate returned mBestT12 (non-empty)
  int iterate(int nIterations, const int32_t *rnd, int acceptAbove, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    if (N < mRansacMinInliers) {
      bNoMore = true;
      return 0;
    }
    std::vector<size_t> vAvailableIndices;
    float P3Dc1i[3][3], P3Dc2i[3][3];
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
      nCurrentIterations++;
      mnIterations++;
      vAvailableIndices = mvAllIndices;
      for (short i = 0; i < 3; ++i) {
        int randi = rnd[(mnIterations - 1) * 3 + i];  // DUtils::Random::RandomInt(0, vAvailableIndices.size()-1)
        int idx = (int)vAvailableIndices[randi];
        for (int r = 0; r < 3; r++) { P3Dc1i[r][i] = mvX3Dc1[idx].v[r]; P3Dc2i[r][i] = mvX3Dc2[idx].v[r]; }
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
      ComputeSim3(P3Dc1i, P3Dc2i);
      CheckInliers();
      Row row;
      row.s = ms12i;
      std::memcpy(row.R, mR12i, 36);
      std::memcpy(row.t, mt12i, 12);
      row.n = mnInliersi;
      row.in = mvbInliersi;
      row.razor = razor;
      row.gap = gap;
      row.nRazor = nRazor;
      row.band = inBand;
      row.best = 0;
      row.ret = 0;
      if (mnInliersi >= mnBestInliers) {
        row.best = 1;
        mvbBestInliers = mvbInliersi;
        mnBestInliers = mnInliersi;
        std::memcpy(mBestRotation, mR12i, 36);
        std::memcpy(mBestTranslation, mt12i, 12);
        mBestScale = ms12i;
        if (mnInliersi > acceptAbove) {  // > mRansacMinInliers, or > 15 inside the frame-id window (:192)
          nInliers = mnInliersi;
          for (int i = 0; i < N; i++)
            if (mvbInliersi[i]) vbInliers[mvnIndices1[i]] = true;
          row.ret = 1;
          log.push_back(row);
          return 1;
        }
      }
      log.push_back(row);
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    return 0;
  }
};

}  // namespace

extern "C" {

// The constructor (:37-112).  valid1[i1] = pMP1 && !isBad(); matches12[i1] = slot in KF2 of vpMatched12[i1] or -1;
// valid2[j] = !isBad() of that point; index1/index2 = GetIndexInKeyFrame (NULL = the slot itself).
void *s3r_create(int n1, const int32_t *matches12, const uint8_t *valid1, const uint8_t *valid2, const int32_t *index1, const int32_t *index2,
                 const int32_t *octave1, const int32_t *octave2, const float *xw1, const float *xw2, const float *T1, const float *T2,
                 const float *levelSigma2, const float *K1, const float *K2, int fixScale) {
  Solver *S = new Solver;
  S->mbFixScale = fixScale != 0;
  S->mN1 = n1;
  size_t idx = 0;
  for (int i1 = 0; i1 < n1; i1++) {
    if (matches12[i1] >= 0) {
      const int j = matches12[i1];
      if (!valid1[i1]) continue;  // !pMP1, or pMP1->isBad()
      if (!valid2[j]) continue;
      const int indexKF1 = index1 ? index1[i1] : i1;
      const int indexKF2 = index2 ? index2[j] : j;
      if (indexKF1 < 0 || indexKF2 < 0) continue;
      const float sigmaSquare1 = levelSigma2[octave1[indexKF1]];
      const float sigmaSquare2 = levelSigma2[octave2[indexKF2]];
      S->mvnMaxError1.push_back(9.210 * sigmaSquare1);
      S->mvnMaxError2.push_back(9.210 * sigmaSquare2);
      S->mvnIndices1.push_back(i1);
      V3 X1, X2;
      std::memcpy(X1.v, xw1 + (size_t)i1 * 3, 12);
      std::memcpy(X2.v, xw2 + (size_t)j * 3, 12);
      S->mvX3Dc1.push_back(affine(T1, X1));
      S->mvX3Dc2.push_back(affine(T2, X2));
      S->mvAllIndices.push_back(idx);
      idx++;
    }
  }
  std::memcpy(S->K1, K1, 16);
  std::memcpy(S->K2, K2, 16);
  S->FromCameraToImage(S->mvX3Dc1, S->mvP1im1, S->K1);
  S->FromCameraToImage(S->mvX3Dc2, S->mvP2im2, S->K2);
  S->SetRansacParameters(0.99, 6, 300);
  return S;
}
void s3r_destroy(void *h) { delete static_cast<Solver *>(h); }
int s3r_N(void *h) { return static_cast<Solver *>(h)->N; }
// corr rows as fb_sim3_corr: x3dc1[3] x3dc2[3] p1im1[2] p2im2[2] max_err1 max_err2 (12 dwords)
void s3r_correspondences(void *h, int32_t *indices1, uint32_t *corr) {
  Solver *S = static_cast<Solver *>(h);
  for (int i = 0; i < S->N; i++) {
    indices1[i] = S->mvnIndices1[i];
    float f[10] = {S->mvX3Dc1[i].v[0], S->mvX3Dc1[i].v[1], S->mvX3Dc1[i].v[2], S->mvX3Dc2[i].v[0], S->mvX3Dc2[i].v[1], S->mvX3Dc2[i].v[2],
                   S->mvP1im1[i].v[0], S->mvP1im1[i].v[1], S->mvP2im2[i].v[0], S->mvP2im2[i].v[1]};
    std::memcpy(corr + (size_t)i * 12, f, 40);
    corr[(size_t)i * 12 + 10] = (uint32_t)S->mvnMaxError1[i];
    corr[(size_t)i * 12 + 11] = (uint32_t)S->mvnMaxError2[i];
  }
}
int s3r_set_ransac(void *h, double p, int minInliers, int maxIts) {
  Solver *S = static_cast<Solver *>(h);
  S->SetRansacParameters(p, minInliers, maxIts);
  return S->mRansacMaxIts;
}
int s3r_iterations(void *h) { return static_cast<Solver *>(h)->mnIterations; }
// iterate(n, bNoMore, vbInliers, nInliers): rnd = [.][3] RandomInt values by iteration; vbInliers: mN1 bytes;
// sRt = s, R[9], t[3] of mBestT12 when it returns 1
int s3r_iterate(void *h, int n, const int32_t *rnd, int acceptAbove, int32_t *bNoMore, uint8_t *vbInliers, int32_t *nInliers, float *sRt) {
  Solver *S = static_cast<Solver *>(h);
  bool nm;
  std::vector<bool> vb;
  int ni;
  const int r = S->iterate(n, rnd, acceptAbove, nm, vb, ni);
  *bNoMore = nm ? 1 : 0;
  *nInliers = ni;
  for (int i = 0; i < S->mN1; i++) vbInliers[i] = vb[i] ? 1 : 0;
  if (r) {
    sRt[0] = S->mBestScale;
    std::memcpy(sRt + 1, S->mBestRotation, 36);
    std::memcpy(sRt + 10, S->mBestTranslation, 12);
  }
  return r;
}
int s3r_log_size(void *h) { return (int)static_cast<Solver *>(h)->log.size(); }
// rows of the log: s[n], R[n][9], t[n][3], n_inliers[n], is_best[n], returned[n], razor[n], gap[n], n_razor[n], mask[n][mask_words], band[n][mask_words] (the in-band correspondences)
void s3r_log(void *h, float *s, float *R, float *t, int32_t *ninl, uint8_t *best, uint8_t *ret, double *razor, double *gap, int32_t *nRazor, uint32_t *mask, uint32_t *band, int maskWords) {
  Solver *S = static_cast<Solver *>(h);
  for (size_t k = 0; k < S->log.size(); k++) {
    const Solver::Row &r = S->log[k];
    s[k] = r.s;
    std::memcpy(R + k * 9, r.R, 36);
    std::memcpy(t + k * 3, r.t, 12);
    ninl[k] = r.n;
    best[k] = (uint8_t)r.best;
    ret[k] = (uint8_t)r.ret;
    razor[k] = r.razor;
    gap[k] = r.gap;
    nRazor[k] = r.nRazor;
    for (int w = 0; w < maskWords; w++) mask[k * maskWords + w] = band[k * maskWords + w] = 0;
    for (size_t i = 0; i < r.in.size(); i++)
      if (r.in[i]) mask[k * maskWords + i / 32] |= 1u << (i % 32);
    for (size_t i = 0; i < r.band.size(); i++)
      if (r.band[i]) band[k * maskWords + i / 32] |= 1u << (i % 32);
  }
}
// cv::eigen of a symmetric 4x4 float matrix: eigenvalues descending, eigenvectors as rows
void s3r_eigen4(const float *N16, float *eval4, float *evec16) {
  float Nm[4][4], ev[4][4];
  std::memcpy(Nm, N16, 64);
  eigen4(Nm, eval4, ev);
  std::memcpy(evec16, ev, 64);
}
// ComputeSim3 on two 3x3 sample matrices (columns = samples) -> s, R, t
void s3r_compute_sim3(const float *P1, const float *P2, int fixScale, float *sRt) {
  Solver S;
  S.mbFixScale = fixScale != 0;
  float a[3][3], b[3][3];
  std::memcpy(a, P1, 36);
  std::memcpy(b, P2, 36);
  S.ComputeSim3(a, b);
  sRt[0] = S.ms12i;
  std::memcpy(sRt + 1, S.mR12i, 36);
  std::memcpy(sRt + 10, S.mt12i, 12);
}

}  // extern "C"
