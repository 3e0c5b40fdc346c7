// search_in_neighbors_host_test.cpp -- drives fishbird::CovisibilityMap::FuseTargets / SearchInNeighbors (host/fishbird_host.hpp,
// host pointers throughout) the way LocalMapping::SearchInNeighbors does, on a map whose answers are known by construction:
// every key frame looks down +z from the origin with fx = fy = 100, so a point at (x, 0, 5) projects to (100 + 20 x, 100).
#include <cstdio>
#include <cstdlib>

#include "fishbird_host.hpp"

#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

typedef std::vector<int> V;
typedef fishbird::CovisibilityMap Map;

int main() {
  try {
    const int K = 3, S = 4, cur = 0;
    Map map(K, S);
    for (int s = 0; s < K; s++) map.kfOrder[s] = 0x7000 + 0x100 * s;
    const int pA = map.NewMapPoint(), pB = map.NewMapPoint(), pD = map.NewMapPoint();
    map.AddObservation(pA, cur, 0, 0);                                     // (point, key frame, feature, octave)
    map.AddObservation(pB, 1, 0, 0);
    map.AddObservation(pD, 2, 0, 0);                                       // a second triangulation of pA's location
    map.kfN[cur] = 2; map.kfN[1] = 2;                                      // feature 1 of cur and of key frame 1 is empty
    Map::PointTables t(map, 4);
    for (int l = 0; l < 4; l++) t.scaleFactors[l] = 1.f + 0.2f * l;
    const float x[3] = {0.f, 2.5f, 0.f}, maxd[3] = {5.5f, 6.15f, 5.5f};    // 1.1 x the distance: level 1 predicted, octaves 0 and 1 accepted
    for (int p = 0; p < 3; p++) {
      t.mpXw[(size_t)p * 3] = x[p]; t.mpXw[(size_t)p * 3 + 2] = 5.f; t.mpNormal[(size_t)p * 3 + 2] = 1.f;
      t.mpMinDist[p] = 1.f; t.mpMaxDist[p] = maxd[p];
    }
    t.mpRefKF[pA] = cur; t.mpRefKF[pB] = 1; t.mpRefKF[pD] = 2;
    t.mpFound[pA] = 3; t.mpVisible[pA] = 7; t.mpFound[pD] = 10; t.mpVisible[pD] = 20;
    Map::FuseTarget target;
    memset(&target.cam, 0, sizeof(target.cam)); memset(&target.grid, 0, sizeof(target.grid));
    target.cam.fx = target.cam.fy = 100.f; target.cam.cx = target.cam.cy = 100.f; target.cam.max_x = target.cam.max_y = 200.f;
    target.grid.cols = 64; target.grid.rows = 48; target.grid.inv_w = 64.f / 200.f; target.grid.inv_h = 48.f / 200.f;
    for (int l = 0; l < FB_MAX_LEVELS; l++) { target.scaleFactors[l] = 1.f + 0.2f * l; target.invLevelSigma2[l] = 1.f; }
    target.logScaleFactor = std::log(1.2f); target.nLevels = 4;
    target.keysUn.assign((size_t)K * S, fb_keypoint());
    for (size_t i = 0; i < target.keysUn.size(); i++) memset(&target.keysUn[i], 0, sizeof(fb_keypoint));
    const float px[3][2] = {{100.f, 150.f}, {150.f, 100.f}, {100.f, 0.f}}; // where the features of key frames 0, 1, 2 stand
    for (int k = 0; k < K; k++)
      for (int i = 0; i < map.kfN[k]; i++) { target.keysUn[(size_t)k * S + i].x = px[k][i]; target.keysUn[(size_t)k * S + i].y = 100.f; }

    fishbird::CovisibilityGraph g(K);
    g.AddConnection(cur, 1, 30); g.AddConnection(1, cur, 30); g.AddConnection(cur, 2, 20); g.AddConnection(2, cur, 20);
    g.AddConnection(1, 2, 40); g.AddConnection(2, 1, 40);
    // firsts 1, 2.  1's neighbours: 2 (pushed, not stamped), cur (skipped); 2 then comes as a first, its neighbours 1 (an earlier
    // first) and cur are skipped
    const V targets = map.FuseTargets(g.handle(), t, cur);
    EXPECT(targets == (V{1, 2, 2}));

    // target 1: pA projects onto its empty feature 1 (a new edge).  Target 2: onto feature 0, held by pD with one observation
    // against pA's two: pD->Replace(pA).  Target 2 again: pA is in the key frame.  Candidates: pB, pA.  Fuse(cur): pB projects
    // onto cur's empty feature 1 (a new edge); pA is in cur.
    const size_t n0 = map.obsKf.size();
    Map::Neighbors r = map.SearchInNeighbors(g.handle(), t, target, cur, targets);
    EXPECT(map.obsKf.size() == n0 + 4 * S);
    EXPECT(r.nFused == (V{1, 1, 0, 1}));
    EXPECT(r.candidates == (V{pB, pA}));
    EXPECT(r.added.size() == 2 && r.added[0].kf == 1 && r.added[0].point == pA && r.added[0].idx == 1 && r.added[0].edge == (int)n0);
    EXPECT(r.added[1].kf == cur && r.added[1].point == pB && r.added[1].idx == 1 && r.added[1].edge == (int)n0 + 1);
    EXPECT(r.replaced.size() == 1 && r.replaced[0].first == pD && r.replaced[0].second == pA);
    EXPECT(map.kfMapPoints[(size_t)1 * S + 1] == pA && map.kfMapPoints[(size_t)2 * S + 0] == pA && map.kfMapPoints[(size_t)cur * S + 1] == pB);
    EXPECT(map.mpBad[pD] == 1 && t.mpReplaced[pD] == pA && t.mpFound[pA] == 13 && t.mpVisible[pA] == 27);
    EXPECT(map.obsMp[n0] == pA && map.obsKf[n0] == 1 && map.obsIdx[n0] == 1 && map.obsMp[n0 + 1] == pB && map.obsKf[n0 + 1] == cur);
    for (size_t e = n0 + 2; e < map.obsKf.size(); e++) EXPECT(map.obsKf[e] == -1 && map.obsMp[e] == -1 && map.obsIdx[e] == -1);
    EXPECT(map.obsMp[2] == pA && map.obsKf[2] == 2);                       // pD's edge went over in place
    // step 5: every centre is the origin, level 0 at the reference key frame: max = the distance, the normal is the direction
    EXPECT(t.mpMaxDist[pA] == 5.f && t.mpNormal[(size_t)pA * 3 + 2] == 1.f && t.mpNormal[(size_t)pA * 3] == 0.f);
    EXPECT(t.mpMaxDist[pB] > 5.59f && t.mpMaxDist[pB] < 5.6f && t.mpNormal[(size_t)pB * 3] > 0.44f);
    // step 6: cur shares pA and pB with key frame 1, pA with key frame 2; no weight reaches 15, so the best one is kept
    EXPECT(r.nCounter == 2 && r.front == 1 && g.GetWeight(cur, 1) == 2 && g.GetWeight(cur, 2) == 1 && g.GetWeight(1, cur) == 2);
    printf("search_in_neighbors_host_test ok\n");
    return 0;
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 2;
  }
}
