// loop_fuse_host_test.cpp -- drives fishbird::CovisibilityMap::ReplacePoints / LoopFuse / SearchAndFuse (host/fishbird_host.hpp,
// host pointers throughout) the way LoopClosing::CorrectLoop does, on a map whose answers are known by construction: the
// set key frame looks down +z from the origin with fx = fy = 100, so a point at (x, 0, 5) projects to (100 + 20 x, 100).
#include <cstdio>
#include <cstdlib>

#include "fishbird_host.hpp"

#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

typedef std::vector<int> V;
typedef fishbird::CovisibilityMap Map;

int main() {
  try {
    const int K = 3, S = 4;
    Map map(K, S);
    for (int s = 0; s < K; s++) map.kfOrder[s] = 0x7000 + 0x100 * s;
    const int pL = map.NewMapPoint(), pM = map.NewMapPoint(), pA = map.NewMapPoint(), pX = map.NewMapPoint(), pY = map.NewMapPoint();
    map.AddObservation(pL, 0, 0, 0);                                       // (point, key frame, feature, octave): the loop side
    map.AddObservation(pM, 0, 1, 0);
    map.AddObservation(pA, 1, 0, 0);                                       // the set key frame holds pA where pL will project
    map.AddObservation(pX, 2, 0, 0);
    map.AddObservation(pY, 2, 1, 0);
    map.AddObservation(pX, 0, 2, 0);
    map.kfN[1] = 2;                                                        // feature 1 of key frame 1 is empty
    Map::PointTables t(map, 4);
    for (int l = 0; l < 4; l++) t.scaleFactors[l] = 1.f + 0.2f * l;
    t.mpFound[pX] = 3; t.mpVisible[pX] = 7; t.mpFound[pY] = 10; t.mpVisible[pY] = 20;
    fishbird::CovisibilityGraph g(K);

    // Replace: pY is in key frame 2 already, so pX's slot there is nulled and that edge dropped; key frame 0's goes over
    Map::Fused r = map.ReplacePoints(g.handle(), t, V{-1, pX, pY}, V{pL, pY, pY});
    EXPECT(r.replaced.size() == 1 && r.replaced[0].first == pX && r.replaced[0].second == pY);
    EXPECT(map.mpBad[pX] == 1 && t.mpReplaced[pX] == pY && t.mpFound[pY] == 13 && t.mpVisible[pY] == 27);
    EXPECT(map.kfMapPoints[(size_t)2 * S + 0] == -1 && map.kfMapPoints[(size_t)0 * S + 2] == pY && map.kfMapPoints[(size_t)2 * S + 1] == pY);
    EXPECT(map.obsKf[3] == -1 && map.obsMp[5] == pY && map.obsKf[5] == 0);

    // the loop fusion for key frame 2: feature 0 is empty now and takes pL (a new edge); feature 1 holds pY -> Replace(pY -> pM)
    const size_t n0 = map.obsKf.size();
    r = map.LoopFuse(g.handle(), t, 2, V{pL, pM});
    EXPECT(map.obsKf.size() == n0 + 2);
    EXPECT(r.added.size() == 1 && r.added[0].kf == 2 && r.added[0].point == pL && r.added[0].idx == 0 && r.added[0].edge == (int)n0);
    EXPECT(map.obsMp[n0] == pL && map.obsKf[n0] == 2 && map.obsIdx[n0] == 0 && map.obsKf[n0 + 1] == -1);
    EXPECT(r.replaced.size() == 1 && r.replaced[0].first == pY && r.replaced[0].second == pM);
    EXPECT(map.kfMapPoints[(size_t)2 * S + 0] == pL && map.kfMapPoints[(size_t)2 * S + 1] == pM && map.mpBad[pY] == 1);
    EXPECT(map.kfMapPoints[(size_t)0 * S + 2] == -1);                      // pM is in key frame 0 already: pY's slot there is nulled

    // SearchAndFuse over the set {1}: pL projects onto feature 0 (held by pA -> Replace(pA -> pL)), pM onto the empty feature 1
    Map::FuseTarget target;
    memset(&target.cam, 0, sizeof(target.cam)); memset(&target.grid, 0, sizeof(target.grid));
    target.cam.fx = target.cam.fy = 100.f; target.cam.cx = target.cam.cy = 100.f; target.cam.max_x = target.cam.max_y = 200.f;
    target.grid.cols = 64; target.grid.rows = 48; target.grid.inv_w = 64.f / 200.f; target.grid.inv_h = 48.f / 200.f;
    for (int l = 0; l < FB_MAX_LEVELS; l++) { target.scaleFactors[l] = 1.f + 0.2f * l; target.invLevelSigma2[l] = 1.f; }
    target.logScaleFactor = std::log(1.2f); target.nLevels = 4;
    target.keysUn.assign((size_t)K * S, fb_keypoint());
    for (size_t i = 0; i < target.keysUn.size(); i++) memset(&target.keysUn[i], 0, sizeof(fb_keypoint));
    target.keysUn[(size_t)1 * S + 0].x = 100.f; target.keysUn[(size_t)1 * S + 0].y = 100.f;
    target.keysUn[(size_t)1 * S + 1].x = 150.f; target.keysUn[(size_t)1 * S + 1].y = 100.f;
    const int pts[2] = {pL, pM};
    for (int q = 0; q < 2; q++) {
      const int p = pts[q];
      t.mpXw[(size_t)p * 3] = q ? 2.5f : 0.f; t.mpXw[(size_t)p * 3 + 2] = 5.f; t.mpNormal[(size_t)p * 3 + 2] = 1.f;
      t.mpMinDist[p] = 1.f; t.mpMaxDist[p] = q ? 6.15f : 5.5f;             // 1.1 x the distance: level 1 predicted, octaves 0 and 1 accepted
      for (int b = 0; b < 32; b++) t.mpDesc[(size_t)p * 32 + b] = 0;       // the key frames' descriptors are all zero: distance 0
    }
    const float Scw[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const size_t n1 = map.obsKf.size();
    r = map.SearchAndFuse(g.handle(), t, target, V{1}, std::vector<float>(Scw, Scw + 12), V{pL, pM});
    EXPECT(map.obsKf.size() == n1 + S);
    EXPECT(r.nFused.size() == 1 && r.nFused[0] == 2);
    EXPECT(r.added.size() == 1 && r.added[0].kf == 1 && r.added[0].point == pM && r.added[0].idx == 1 && r.added[0].edge == (int)n1);
    EXPECT(r.replaced.size() == 1 && r.replaced[0].first == pA && r.replaced[0].second == pL);
    EXPECT(map.kfMapPoints[(size_t)1 * S + 0] == pL && map.kfMapPoints[(size_t)1 * S + 1] == pM && map.mpBad[pA] == 1 && t.mpReplaced[pA] == pL);
    for (size_t e = n1 + 1; e < n1 + S; e++) EXPECT(map.obsKf[e] == -1);
    // the set key frame now shares pL and pM with key frame 0: the link that attaches the two sides of the loop
    fishbird::CovisibilityGraph::Updated u = g.UpdateConnections(map, 1);
    EXPECT(u.nCounter >= 1 && g.GetWeight(1, 0) == 2);
    printf("loop_fuse_host_test ok\n");
    return 0;
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 2;
  }
}
