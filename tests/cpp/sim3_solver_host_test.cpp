// sim3_solver_host_test.cpp -- drives fishbird::Sim3Solver (host/fishbird_host.hpp) the way LoopClosing::ComputeSim3 drives the
// reference's Sim3Solver: iterate(5, ...) round-robin over three candidates, going on after every return.  The same draws
// go to the CPU restatement of the reference class (tests/cpp/sim3_solver_ref.cpp, linked in) and the two return sequences
// must be the same.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fishbird_host.hpp"

extern "C" {
void *s3r_create(int n1, const int32_t *matches12, const uint8_t *valid1, const uint8_t *valid2, const int32_t *index1, const int32_t *index2,
                 const int32_t *octave1, const int32_t *octave2, const float *xw1, const float *xw2, const float *T1, const float *T2,
                 const float *levelSigma2, const float *K1, const float *K2, int fixScale);
void s3r_destroy(void *h);
int s3r_set_ransac(void *h, double p, int minInliers, int maxIts);
int s3r_iterate(void *h, int n, const int32_t *rnd, int acceptAbove, int32_t *bNoMore, uint8_t *vbInliers, int32_t *nInliers, float *sRt);
}

#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static unsigned g_state = 12345u;
static double uni() { g_state = g_state * 1664525u + 1013904223u; return (g_state >> 8) / 16777216.0; }
static std::vector<int32_t> *g_draws = nullptr;  // the draws of the candidate whose table is being filled
static int logged_random_int(int min, int max) {
  const int v = fishbird::Sim3Solver::RandomInt(min, max);
  g_draws->push_back(v);
  return v;
}

struct Cand {
  int n;
  std::vector<fb_keypoint> kps;
  std::vector<uint8_t> valid;
  std::vector<float> xw;
  std::vector<int32_t> oct;
  float T[12];
};

int main() {
  try {
    const int n1 = 400, C = 3;
    const float K[4] = {500.f, 500.f, 640.f, 360.f};
    float sigma2[8];
    { float s = 1.f; for (int l = 0; l < 8; l++) { sigma2[l] = s * s; s *= 1.2f; } }
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    Cand k1;
    k1.n = n1; k1.kps.resize(n1); k1.valid.assign(n1, 1); k1.xw.resize(n1 * 3); k1.oct.resize(n1);
    for (int i = 0; i < 12; i++) k1.T[i] = I[i];
    for (int i = 0; i < n1; i++) {
      const double z = 3 + 20 * uni();
      k1.xw[i * 3] = (float)((uni() - 0.5) * 2.0 * z); k1.xw[i * 3 + 1] = (float)((uni() - 0.5) * 1.2 * z); k1.xw[i * 3 + 2] = (float)z;
      k1.kps[i].octave = k1.oct[i] = (int)(uni() * 8) & 7;
      if (i % 37 == 0) k1.valid[i] = 0;  // NULL / bad points of KF1
    }
    std::vector<Cand> k2(C);
    std::vector<std::vector<int32_t>> m12(C, std::vector<int32_t>(n1, -1)), draws(C);
    const int want[3] = {150, 60, 17};  // the last one stays below min_inliers
    for (int c = 0; c < C; c++) {
      Cand &k = k2[c];
      k.n = n1; k.kps.resize(n1); k.valid.assign(n1, 1); k.xw.resize(n1 * 3); k.oct.resize(n1);
      const float sc = 1.f + 0.05f * c, th = 0.05f * (c + 1), cs = std::cos(th), sn = std::sin(th);
      const float T[12] = {cs, 0, sn, 0.3f * c, 0, 1, 0, -0.1f, -sn, 0, cs, 0.2f};
      for (int i = 0; i < 12; i++) k.T[i] = T[i];
      int made = 0;
      for (int i = 0; i < n1; i++) {
        k.kps[i].octave = k.oct[i] = (int)(uni() * 8) & 7;
        const bool outlier = uni() < 0.5;
        for (int r = 0; r < 3; r++)  // the candidate's map: a scaled copy of KF1's, outliers anywhere
          k.xw[i * 3 + r] = outlier ? (float)((uni() - 0.3) * 20) : k1.xw[i * 3 + r] * sc + (float)((uni() - 0.5) * 0.004);
        if (k1.valid[i] && made < want[c]) { m12[c][i] = i; made++; }
      }
    }
    fishbird::Sim3KeyFrame f1;
    f1.N = n1; f1.mvKeysUn = k1.kps.data(); f1.mpValid = k1.valid.data(); f1.mpWorldPos = k1.xw.data(); f1.Tcw = k1.T;
    f1.fx = K[0]; f1.fy = K[1]; f1.cx = K[2]; f1.cy = K[3];
    std::vector<fishbird::Sim3Solver *> dev(C);
    std::vector<void *> ref(C);
    std::vector<bool> discarded(C, false);
    for (int c = 0; c < C; c++) {
      fishbird::Sim3KeyFrame f2 = f1;
      f2.mvKeysUn = k2[c].kps.data(); f2.mpValid = k2[c].valid.data(); f2.mpWorldPos = k2[c].xw.data(); f2.Tcw = k2[c].T;
      dev[c] = new fishbird::Sim3Solver(f1, f2, m12[c], c == 1, sigma2, 8, &logged_random_int);
      dev[c]->SetRansacParameters(0.99, 20, 300);
      ref[c] = s3r_create(n1, m12[c].data(), k1.valid.data(), k2[c].valid.data(), nullptr, nullptr, k1.oct.data(), k2[c].oct.data(), k1.xw.data(),
                          k2[c].xw.data(), k1.T, k2[c].T, sigma2, K, K, c == 1);
      EXPECT(s3r_set_ransac(ref[c], 0.99, 20, 300) == dev[c]->maxIterations() || dev[c]->correspondences() < 20);
    }
    EXPECT(dev[0]->correspondences() == 150 && dev[2]->correspondences() == 17);
    int returns = 0, rounds = 0, left = C;
    while (left > 0 && rounds < 200) {  // LoopClosing.cc:290-391: round-robin, five iterations each
      rounds++;
      for (int c = 0; c < C; c++) {
        if (discarded[c]) continue;
        bool bNoMore;
        std::vector<bool> vb;
        int nInliers;
        g_draws = &draws[c];
        const bool got = dev[c]->iterate(5, bNoMore, vb, nInliers);
        draws[c].resize(300 * 3, 0);
        int32_t rNoMore, rInl;
        std::vector<uint8_t> rvb(n1);
        float srt[13];
        const int rgot = s3r_iterate(ref[c], 5, draws[c].data(), 20, &rNoMore, rvb.data(), &rInl, srt);
        EXPECT(got == (rgot != 0) && bNoMore == (rNoMore != 0) && nInliers == rInl);
        for (int i = 0; i < n1; i++) EXPECT(vb[i] == (rvb[i] != 0));
        if (got) {
          returns++;
          // the bounds of tests/test_sim3_solver_gpu.py (four times the measured worst difference of the two rotation routes)
          EXPECT(std::fabs(dev[c]->GetEstimatedScale() - srt[0]) <= 9.6e-7f * srt[0]);
          for (int e = 0; e < 9; e++) EXPECT(std::fabs(dev[c]->GetEstimatedRotation()[e] - srt[1 + e]) <= 9.6e-7f);
          const float tn = std::max(1.0f, std::sqrt(srt[10] * srt[10] + srt[11] * srt[11] + srt[12] * srt[12]));
          for (int e = 0; e < 3; e++) EXPECT(std::fabs(dev[c]->GetEstimatedTranslation()[e] - srt[10 + e]) <= 1.6e-5f * tn);
          if (c == 1) EXPECT(dev[c]->GetEstimatedScale() == 1.0f);
        }
        if (bNoMore) { discarded[c] = true; left--; }
      }
    }
    EXPECT(left == 0 && returns >= 2);
    for (int c = 0; c < C; c++) { delete dev[c]; s3r_destroy(ref[c]); }
    printf("sim3_solver_host_test ok (%d returns in %d rounds)\n", returns, rounds);
    return 0;
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 2;
  }
}
