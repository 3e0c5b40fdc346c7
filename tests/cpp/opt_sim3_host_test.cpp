// opt_sim3_host_test.cpp -- drives fishbird::Optimizer::OptimizeSim3 (host/fishbird_host.hpp) the way LoopClosing::ComputeSim3
// does: key frame 2 sees key frame 1's points through a known Sim3, the key points are the projections, four matches point
// at wrong features, the input Sim3 is the true one perturbed.  The shim must return the C entry point's result byte for
// byte, null exactly the wrong matches, come back near the true Sim3 and hand out mg2oScw = g2oS12 * Sim3(R2w, t2w, 1).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fishbird_host.hpp"

#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static unsigned g_state = 4242u;
static double uni() { g_state = g_state * 1664525u + 1013904223u; return (g_state >> 8) / 16777216.0; }

int main() {
  try {
    const int n = 120, nWrong = 4;
    const float fx = 500.f, fy = 500.f, cx = 640.f, cy = 360.f;
    float invSigma2[8];
    { float s = 1.f; for (int l = 0; l < 8; l++) { invSigma2[l] = 1.f / (s * s); s *= 1.2f; } }
    const float T1[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float T2[12] = {1, 0, 0, 0.1f, 0, 1, 0, -0.05f, 0, 0, 1, 0.2f};
    // X3Dc1 = s R X3Dc2 + t: a rotation about z by 0.02 rad, t, s
    const double sT = 1.05, cz = std::cos(0.02), sz = std::sin(0.02), tT[3] = {0.3, -0.1, 0.2};
    std::vector<fb_keypoint> kp1(n), kp2(n);
    std::vector<uint8_t> v1(n, 1), v2(n, 1);
    std::vector<float> xw1(n * 3), xw2(n * 3);
    std::vector<int32_t> m(n, -1);
    memset(kp1.data(), 0, n * sizeof(fb_keypoint));
    memset(kp2.data(), 0, n * sizeof(fb_keypoint));
    for (int i = 0; i < n; i++) {
      const double z = 4 + 15 * uni(), P1[3] = {(uni() - 0.5) * 1.6 * z, (uni() - 0.5) * 0.9 * z, z};
      // X3Dc2 = R^T (X3Dc1 - t) / s
      const double d[3] = {P1[0] - tT[0], P1[1] - tT[1], P1[2] - tT[2]};
      const double P2[3] = {(cz * d[0] + sz * d[1]) / sT, (-sz * d[0] + cz * d[1]) / sT, d[2] / sT};
      for (int k = 0; k < 3; k++) { xw1[i * 3 + k] = (float)P1[k]; xw2[i * 3 + k] = (float)(P2[k] - T2[k * 4 + 3]); }
      kp1[i].x = (float)(fx * P1[0] / P1[2] + cx + (uni() - 0.5)); kp1[i].y = (float)(fy * P1[1] / P1[2] + cy + (uni() - 0.5));
      kp2[i].x = (float)(fx * P2[0] / P2[2] + cx + (uni() - 0.5)); kp2[i].y = (float)(fy * P2[1] / P2[2] + cy + (uni() - 0.5));
      kp1[i].octave = (int)(uni() * 8) & 7; kp2[i].octave = (int)(uni() * 8) & 7;
    }
    for (int i = 0; i < 100; i++) m[i] = i;
    for (int i = 0; i < nWrong; i++) m[10 * i + 3] = 100 + i;  // features 100..119 of KF2 belong to other points
    v1[50] = 0;                                                  // a NULL / bad point of KF1: skipped, not nulled
    fishbird::Sim3KeyFrame k1, k2;
    k1.N = n; k1.mvKeysUn = kp1.data(); k1.mpValid = v1.data(); k1.mpWorldPos = xw1.data(); k1.Tcw = T1; k1.fx = fx; k1.fy = fy; k1.cx = cx; k1.cy = cy;
    k2 = k1;
    k2.mvKeysUn = kp2.data(); k2.mpValid = v2.data(); k2.mpWorldPos = xw2.data(); k2.Tcw = T2;
    const double c2 = std::cos(0.027), s2 = std::sin(0.027);
    const float R12[9] = {(float)c2, (float)-s2, 0, (float)s2, (float)c2, 0, 0, 0, 1}, t12[3] = {0.33f, -0.12f, 0.23f}, s12 = 1.07f;

    std::vector<int32_t> mShim = m;
    fishbird::Sim3 g, scw;
    float Scw[12];
    const int nIn = fishbird::Optimizer::OptimizeSim3(k1, k2, mShim, R12, t12, s12, g, 10.f, false, invSigma2, 8, &scw, Scw);

    // the C entry point on the same arrays
    std::vector<int32_t> mC = m;
    const int32_t n1 = n;
    int32_t cIn = 0, cCorr = 0, cBad = 0;
    double q[4], t[3], s, wq[4], wt[3], ws;
    float cScw[12];
    fb_optimize_sim3_args a;
    memset(&a, 0, sizeof(a));
    a.n_cand = 1;
    a.kf1.kf_stride = n; a.kf1.n_kf = &n1; a.kf1.kf_kps = kp1.data(); a.kf2.kf_stride = n; a.kf2.kf_kps = kp2.data();
    a.kf1.cam.fx = a.kf2.cam.fx = fx; a.kf1.cam.fy = a.kf2.cam.fy = fy; a.kf1.cam.cx = a.kf2.cam.cx = cx; a.kf1.cam.cy = a.kf2.cam.cy = cy;
    a.mp1.mp_stride = n; a.mp1.mp_valid = v1.data(); a.mp1.mp_xw = xw1.data();
    a.mp2.mp_stride = n; a.mp2.mp_valid = v2.data(); a.mp2.mp_xw = xw2.data();
    a.T1w = T1; a.T2w = T2;
    for (int l = 0; l < 8; l++) a.inv_level_sigma2[l] = invSigma2[l];
    a.matches12 = mC.data(); a.s12 = &s12; a.R12 = R12; a.t12 = t12; a.hyp_stride = 1; a.th2 = 10.f; a.fix_scale = 0;
    a.n_inliers = &cIn; a.n_correspondences = &cCorr; a.n_bad = &cBad;
    a.q = q; a.t = t; a.s = &s; a.scw_q = wq; a.scw_t = wt; a.scw_s = &ws; a.Scw = cScw;
    EXPECT(fb_optimize_sim3(&a) == 0);

    EXPECT(nIn == cIn && mShim == mC);
    EXPECT(memcmp(g.q, q, 32) == 0 && memcmp(g.t, t, 24) == 0 && g.s == s);
    EXPECT(memcmp(scw.q, wq, 32) == 0 && memcmp(scw.t, wt, 24) == 0 && scw.s == ws && memcmp(Scw, cScw, 48) == 0);
    EXPECT(cCorr == 99 && cBad == nWrong && nIn == 99 - nWrong);
    for (int i = 0; i < n; i++) {
      const bool wrong = i < 10 * nWrong && i % 10 == 3;
      EXPECT(mShim[i] == (wrong ? -1 : m[i]));
    }
    // near the generating Sim3 (half a pixel of uniform noise on 95 pairs)
    EXPECT(std::fabs(g.s - sT) < 5e-3 && std::fabs(g.t[0] - tT[0]) < 3e-2 && std::fabs(g.t[1] - tT[1]) < 3e-2 && std::fabs(g.t[2] - tT[2]) < 6e-2);
    EXPECT(std::fabs(2 * std::atan2(g.q[2], g.q[3]) - 0.02) < 2e-3);
    // mg2oScw = g2oS12 * Sim3(I, t2w, 1): same rotation and scale, t = s R t2w + t; Scw = [s R | t] in float
    EXPECT(scw.s == g.s && std::fabs(scw.q[2] - g.q[2]) < 1e-15 && std::fabs(scw.q[3] - g.q[3]) < 1e-15);
    EXPECT(std::fabs(Scw[3] - (float)scw.t[0]) == 0 && std::fabs(Scw[11] - (float)scw.t[2]) == 0);
    EXPECT(std::fabs(Scw[10] - (float)scw.s) < 1e-4f);  // R22 = 1 - 2 (x^2 + y^2), x = y ~ 1e-3
    printf("opt_sim3_host_test ok: nIn %d, s %.6f, t %.4f %.4f %.4f\n", nIn, g.s, g.t[0], g.t[1], g.t[2]);
    return 0;
  } catch (const std::exception &e) {
    printf("FAILED: %s\n", e.what());
    return 1;
  }
}
