// map_refresh_host_test.cpp -- drives fishbird::CovisibilityMap::RefreshPoints / ProcessNewKeyFrame / MapPointCulling
// (host/fishbird_host.hpp, host pointers throughout) the way LocalMapping::Run does, on a map whose answers are known by
// construction: the point at the origin, the camera centres on the negative axes, so every unit vector is an axis.
#include <cstdio>
#include <cstdlib>

#include "fishbird_host.hpp"

#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

typedef std::vector<int> V;
typedef fishbird::CovisibilityMap Map;

static void centre(Map::PointTables &t, int kf, float x, float y, float z) {   // R = I: tcw = -Ow
  t.kfTcw[(size_t)kf * 12 + 3] = -x; t.kfTcw[(size_t)kf * 12 + 7] = -y; t.kfTcw[(size_t)kf * 12 + 11] = -z;
}
static void desc(Map::PointTables &t, const Map &m, int kf, int idx, uint8_t byte0) { t.kfDesc[((size_t)kf * m.kpStride + idx) * 32] = byte0; }
static bool desc_is(const Map::PointTables &t, int mp, uint8_t byte0) {
  for (int b = 1; b < 32; b++) if (t.mpDesc[(size_t)mp * 32 + b]) return false;
  return t.mpDesc[(size_t)mp * 32] == byte0;
}

int main() {
  try {
    const int K = 4, S = 8;
    Map map(K, S);
    const uint64_t order[K] = {0x7300, 0x7200, 0x7100, 0x7400};           // std::map order of the slots: 2, 1, 0, 3
    for (int s = 0; s < K; s++) map.kfOrder[s] = order[s];
    const int p0 = map.NewMapPoint(), p1 = map.NewMapPoint();
    map.AddObservation(p0, 0, 1, 2);                                       // (point, key frame, feature, octave)
    map.AddObservation(p0, 1, 0, 1);
    map.AddObservation(p0, 2, 1, 1);
    map.AddObservation(p1, 1, 3, 0);
    map.AddObservation(p1, 3, 2, 0);                                       // p1 observes key frame 3 already
    Map::PointTables t(map, 4);
    for (int l = 0; l < 4; l++) t.scaleFactors[l] = (float)(1 << l);      // 1, 2, 4, 8
    centre(t, 0, -3, 0, 0); centre(t, 1, 0, -4, 0); centre(t, 2, 0, 0, -5); centre(t, 3, 0, 0, -2);
    // distances 0-1 = 4, 0-2 = 4, 1-2 = 8 bits: every median is 4, the first in std::map order wins: key frame 2
    desc(t, map, 0, 1, 0x0f); desc(t, map, 1, 0, 0x00); desc(t, map, 2, 1, 0xff); desc(t, map, 3, 0, 0x0e); desc(t, map, 3, 3, 0x0e);
    t.mpRefKF[p0] = 0; t.mpRefKF[p1] = 1;
    for (int b = 0; b < 32; b++) t.mpDesc[(size_t)p1 * 32 + b] = 0x77;
    fishbird::CovisibilityGraph g(K);

    const V only0{p0, p0};                                                 // listed twice = listed once
    map.RefreshPoints(g.handle(), t, &only0);
    const float third = (float)(1.0 / 3.0);
    EXPECT(t.mpNormal[0] == third && t.mpNormal[1] == third && t.mpNormal[2] == third);
    EXPECT(t.mpMaxDist[p0] == 3.f * 4.f && t.mpMinDist[p0] == 12.f / 8.f);   // reference key frame 0 at feature 1: octave 2
    EXPECT(desc_is(t, p0, 0xff));
    EXPECT(t.mpDesc[(size_t)p1 * 32] == 0x77 && t.mpMaxDist[p1] == 0.f);   // not listed
    t.kfBad[2] = 1;                                                        // left out of the descriptor, not of the normal
    map.RefreshPoints(g.handle(), t, nullptr, FB_REFRESH_DESCRIPTOR);
    EXPECT(desc_is(t, p0, 0x00));                                          // N = 2: median index 0, both 0, key frame 1 first
    EXPECT(t.mpNormal[0] == third);
    t.kfBad[2] = 0;

    // ProcessNewKeyFrame: key frame 3 holds p0 at features 0 and 3, NULL at 1, p1 (which observes it) at 2
    map.kfMapPoints[(size_t)3 * S + 0] = p0; map.kfMapPoints[(size_t)3 * S + 3] = p0; map.kfN[3] = 4;
    const size_t n0 = map.obsKf.size();
    V recent;
    EXPECT(map.ProcessNewKeyFrame(g.handle(), t, 3, recent) == 1);
    EXPECT(map.obsKf.size() == n0 + 4);
    EXPECT(map.obsMp[n0] == p0 && map.obsKf[n0] == 3 && map.obsIdx[n0] == 0);
    for (size_t e = n0 + 1; e < n0 + 4; e++) EXPECT(map.obsKf[e] == -1);
    EXPECT((recent == V{p1, p0}));                                         // ascending feature: 2, then p0's second feature
    // p0 has four observers now: axes x, y, z, z -> (1, 1, 2) / 4
    EXPECT(t.mpNormal[0] == 0.25f && t.mpNormal[1] == 0.25f && t.mpNormal[2] == 0.5f);
    // sorted rows in std::map order: kf2 ff [0 4 5 8], kf1 00 [0 3 4 8], kf0 0f [0 1 4 4], kf3 0e [0 1 3 5]; the median is
    // index (int)(0.5 * 3) = 1: 4, 3, 1, 1 -> key frame 0 is the first with the least
    EXPECT(desc_is(t, p0, 0x0f));
    fishbird::CovisibilityGraph::Updated u = g.UpdateConnections(map, 3);
    EXPECT(u.nCounter == 3 && g.GetWeight(3, 1) == 3);                     // p0 at two features counts twice, p1 once

    // MapPointCulling: p1 was found once in five frames -> SetBadFlag; p0 is young and well found -> kept
    t.mpFound[p1] = 1; t.mpVisible[p1] = 5; t.mpFound[p0] = 1; t.mpVisible[p0] = 4; t.mpFirstKFid[p0] = 9; t.mpFirstKFid[p1] = 9;
    Map::Culled c = map.MapPointCulling(g.handle(), t, 10, 2, recent);
    EXPECT((recent == V{p0}) && (c.points == V{p1}));
    EXPECT(c.erased.size() == 2 && c.erased[0].kf == 1 && c.erased[0].idx == 3 && c.erased[1].kf == 3 && c.erased[1].idx == 2);
    EXPECT(c.erased[0].point == p1 && map.obsKf[c.erased[0].edge] == -1 && map.obsKf[c.erased[1].edge] == -1);
    EXPECT(map.mpBad[p1] == 1 && map.mpBad[p0] == 0);
    EXPECT(map.kfMapPoints[(size_t)1 * S + 3] == -1 && map.kfMapPoints[(size_t)3 * S + 2] == -1 && map.kfMapPoints[(size_t)3 * S + 0] == p0);
    u = g.UpdateConnections(map, 3);                                       // the next UpdateConnections sees the edits
    EXPECT(u.nCounter == 3 && g.GetWeight(3, 1) == 2);
    printf("map_refresh_host_test ok\n");
    return 0;
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 2;
  }
}
