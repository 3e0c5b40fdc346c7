// window_host_test.cpp -- drives fishbird::LocalWindow (host/fishbird_host.hpp) the way LocalMapping drives
// Optimizer::LocalBundleAdjustment: collect the window of the new key frame, optimise, write back, erase the outliers.
// The map's answers are known by construction.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "fishbird_host.hpp"

#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

typedef std::vector<int> V;

int main() {
  try {
    const int K = 8, S = 32, NP = 16;
    const float fx = 500.f, fy = 500.f, cx = 320.f, cy = 240.f;
    fishbird::CovisibilityMap map(K, S);
    const uint64_t order[K] = {0x7400, 0x7300, 0x7500, 0x7100, 0x7200, 0x7600, 0x7000, 0x7700};
    for (int s = 0; s < K; s++) map.kfOrder[s] = order[s];
    fishbird::WindowTables tab(map, 8);
    for (int l = 0; l < 8; l++) tab.invLevelSigma2[l] = 1.f / std::pow(1.44f, (float)l);
    // key frame k looks along +z from x = 0.3 k; 0 is the new key frame, 1 and 2 its neighbours, 3 sees six of the
    // points without being a neighbour (fixed), 4 is a bad key frame that sees them too
    float truth[K][12];
    for (int k = 0; k < K; k++) {
      const float T[12] = {1, 0, 0, -0.3f * k, 0, 1, 0, 0, 0, 0, 1, 0};
      for (int c = 0; c < 12; c++) { truth[k][c] = T[c]; tab.kfTcw[(size_t)k * 12 + c] = T[c]; }
    }
    float xw[NP][3];
    for (int i = 0; i < NP; i++) {
      map.NewMapPoint();
      xw[i][0] = (i % 4 - 1.5f) * 0.8f; xw[i][1] = (i / 4 - 1.5f) * 0.6f; xw[i][2] = 6.f + 0.25f * i;
      for (int c = 0; c < 3; c++) tab.mpXw.push_back(xw[i][c]);
    }
    auto observe = [&](int i, int kf, int octave) {
      const int idx = map.kfN[kf];
      map.AddObservation(i, kf, idx, octave);
      fb_keypoint &kp = tab.kfKeysUn[(size_t)kf * S + idx];
      const float x = xw[i][0] + truth[kf][3], y = xw[i][1], z = xw[i][2];
      kp.x = fx * x / z + cx; kp.y = fy * y / z + cy; kp.octave = octave; kp.size = 31.f; kp.angle = 0.f; kp.response = 1.f;
      return idx;
    };
    for (int i = 0; i < NP; i++) for (int kf = 0; kf < 3; kf++) observe(i, kf, i % 3);
    for (int i = 0; i < 6; i++) { observe(i, 3, 1); observe(i, 4, 1); }
    tab.kfBad[4] = 1;
    tab.kfInit[1] = 1;
    // one wrong measurement: point 3 in key frame 2 lies 40 pixels off.  Point 3 has four observers, the fixed camera among
    // them (0.9 m of baseline), so the other three agree on it and only this edge fails the chi2 test; a point of three
    // observers 0.3 m apart would absorb the error in its depth and lose two edges
    const int badPoint = 3, badIdx = 3;   // key frame 2 got point i at feature i
    tab.kfKeysUn[(size_t)2 * S + badIdx].x += 40.f;
    // the estimates of the free key frames and of the points are off
    tab.kfTcw[0 * 12 + 3] += 0.02f; tab.kfTcw[2 * 12 + 7] -= 0.015f;
    for (int i = 0; i < NP; i++) tab.mpXw[(size_t)i * 3 + 2] += 0.05f * ((i & 1) ? 1.f : -1.f);
    const std::vector<float> before = tab.kfTcw;

    fishbird::CovisibilityGraph g(K);
    g.UpdateConnections(map, V{0, 1, 2, 3, 4});
    EXPECT((g.GetVectorCovisibleKeyFrames(0) == V{2, 1}));            // 16 each: the larger pointer leads
    fishbird::LocalWindow win;
    win.Collect(g, map, tab, 0, false);
    EXPECT((win.localKeyFrames() == V{0, 2, 1}) && (win.fixedCameras() == V{3}));
    EXPECT((win.kfFixed == std::vector<uint8_t>{0, 0, 1, 1}));
    EXPECT(win.mpIndex.size() == (size_t)NP && win.mpIndex[0] == 0 && win.mpIndex[NP - 1] == NP - 1);
    EXPECT(win.obsKf.size() == (size_t)(3 * NP + 6));                  // the bad key frame's edges are left out
    // point 0: observers in ascending pointer order 3 (0x7100), 1 (0x7300), 0 (0x7400), 2 (0x7500) -> window indices 3, 2, 0, 1
    EXPECT(win.obsKf[0] == 3 && win.obsKf[1] == 2 && win.obsKf[2] == 0 && win.obsKf[3] == 1 && win.obsMp[3] == 0 && win.obsMp[4] == 1);
    EXPECT(map.obsKf[win.obsSrc[0]] == 3 && map.obsMp[win.obsSrc[0]] == 0);
    EXPECT(win.obsInvSigma2[0] == tab.invLevelSigma2[1] && win.obsUv[0] == tab.kfKeysUn[(size_t)3 * S + 0].x);

    fb_local_ba_args a;
    memset(&a, 0, sizeof(a));
    a.with_odom = 0; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.wF = 1.f; a.wB = 1.f; a.wP = 1.f;
    win.Optimize(a, {});
    win.WriteBack(map, tab);
    for (const fishbird::LocalWindow::Erase &e : win.toErase) printf("erase: key frame %d point %d feature %d edge %d\n", e.kf, e.point, e.idx, e.edge);
    EXPECT(win.toErase.size() == 1 && win.toErase[0].kf == 2 && win.toErase[0].point == badPoint && win.toErase[0].idx == badIdx);
    EXPECT(map.obsKf[win.toErase[0].edge] == 2 && map.obsMp[win.toErase[0].edge] == badPoint);
    for (int c = 0; c < 12; c++) {
      EXPECT(std::fabs(tab.kfTcw[0 * 12 + c] - truth[0][c]) < 0.01f && std::fabs(tab.kfTcw[2 * 12 + c] - truth[2][c]) < 0.0075f);   // half the planted error
      EXPECT(tab.kfTcw[1 * 12 + c] == before[1 * 12 + c] && tab.kfTcw[3 * 12 + c] == before[3 * 12 + c]);   // isInit, fixed
      EXPECT(tab.kfTcw[4 * 12 + c] == before[4 * 12 + c] && tab.kfTcw[5 * 12 + c] == before[5 * 12 + c]);   // outside the window
    }
    EXPECT(std::fabs(tab.kfTcw[0 * 12 + 3] - before[0 * 12 + 3]) > 5e-3f);                                   // it moved
    for (int i = 0; i < NP; i++) EXPECT(std::fabs(tab.mpXw[(size_t)i * 3 + 2] - xw[i][2]) < 0.05f);   // nearer than the planted 0.05
    printf("window_host_test ok\n");
    return 0;
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 2;
  }
}
