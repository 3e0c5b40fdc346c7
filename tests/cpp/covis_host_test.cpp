// covis_host_test.cpp -- drives fishbird::CovisibilityGraph (host/fishbird_host.hpp) the way LocalMapping drives the reference's
// KeyFrame graph: ProcessNewKeyFrame -> SearchInNeighbors -> KeyFrameCulling, on a map whose answers are known by construction.
#include <cstdio>
#include <cstdlib>

#include "fishbird_host.hpp"

#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

typedef std::vector<int> V;

// n new points seen by every key frame of kfs at the given octaves, each at the key frame's next feature
static std::vector<int> shared(fishbird::CovisibilityMap &m, int n, const V &kfs, const V &octaves) {
  std::vector<int> pts;
  for (int i = 0; i < n; i++) {
    const int p = m.NewMapPoint();
    for (size_t j = 0; j < kfs.size(); j++) m.AddObservation(p, kfs[j], m.kfN[kfs[j]], octaves[j]);
    pts.push_back(p);
  }
  return pts;
}

int main() {
  try {
    const int K = 8, S = 64;
    fishbird::CovisibilityMap map(K, S);
    const uint64_t order[K] = {0x7000, 0x7500, 0x7300, 0x7400, 0x7200, 0x7600, 0x7100, 0x7700};
    for (int s = 0; s < K; s++) map.kfOrder[s] = order[s];
    // key frames 1..5 exist; 1 is redundant (20 points seen by 3, 4, 5 too) and shares two 3-observation points with 2.
    // 3, 4, 5 see everything at octave 0, the others at octave 3: 3, 4, 5 are never redundant themselves
    shared(map, 20, {1, 3, 4, 5}, {3, 0, 0, 0});    // points 0..19
    shared(map, 16, {2, 3, 4, 5}, {3, 0, 0, 0});    // points 20..35
    const std::vector<int> d = shared(map, 2, {1, 2, 3}, {3, 3, 0});
    fishbird::CovisibilityGraph g(K);
    g.UpdateConnections(map, V{1, 2, 3, 4, 5});
    EXPECT(g.GetWeight(3, 4) == 36 && g.GetWeight(1, 2) == 2 && g.GetWeight(1, 3) == 22);
    // ProcessNewKeyFrame: key frame 0 arrives tracking 16 points of key frame 1's and 15 of key frame 2's
    for (int i = 0; i < 16; i++) map.AddObservation(i, 0, i, 3);
    for (int i = 0; i < 15; i++) map.AddObservation(20 + i, 0, 16 + i, 3);
    fishbird::CovisibilityGraph::Updated u = g.UpdateConnections(map, 0);
    EXPECT(u.nCounter == 5 && u.front == 5);                          // 3, 4, 5 share 31 each: the largest pointer leads
    std::vector<int> w;
    EXPECT((g.GetVectorCovisibleKeyFrames(0, &w) == V{5, 3, 4, 1, 2}) && (w == V{31, 31, 31, 16, 15}));
    EXPECT((g.GetBestCovisibilityKeyFrames(0, 2) == V{5, 3}));
    EXPECT((g.GetCovisiblesByWeight(0, 16) == V{5, 3, 4, 1}) && g.GetCovisiblesByWeight(0, 15).empty());
    EXPECT((g.GetConnectedKeyFrames(0) == V{4, 2, 3, 1, 5}));         // ascending pointer
    EXPECT(g.GetWeight(1, 0) == 16 && g.GetWeight(0, 6) == 0);
    // SearchInNeighbors fused one more point of key frame 2 into key frame 0, then UpdateConnections again
    map.AddObservation(35, 0, 31, 3);
    u = g.UpdateConnections(map, 0);
    EXPECT(u.nCounter == 5 && g.GetWeight(0, 2) == 16 && g.GetWeight(2, 0) == 16);
    fishbird::KeyFrameDatabase db(K, 16);
    g.UpdateKeyFrameDatabase(db);
    // KeyFrameCulling around key frame 0; key frame 3 is the first key frame (mnId == 0)
    fishbird::CovisibilityGraph::Culling c = g.KeyFrameCulling(map, 0, 3, {});
    EXPECT((c.slots == V{5, 3, 4, 1, 2}));
    EXPECT(c.culled[3] == 1 && c.nRedundantObservations[3] == 20 && c.nMPs[3] == 22);
    EXPECT(c.culled[4] == 1 && c.nRedundantObservations[4] == 16 && c.nMPs[4] == 16);   // the two shared points went bad with key frame 1
    EXPECT(c.nMPs[1] == 0 && c.culled[0] == 0 && c.culled[2] == 0);
    EXPECT(c.mpBadAfter[d[0]] == 1 && c.mpBadAfter[d[1]] == 1 && c.mpBadAfter[0] == 0);
    EXPECT(g.GetWeight(0, 1) == 16);                                   // the call itself changed nothing
    // the real SetBadFlag of the two culled key frames
    g.SetBadFlag(1);
    g.SetBadFlag(2);
    EXPECT((g.GetVectorCovisibleKeyFrames(0) == V{5, 3, 4}) && g.GetVectorCovisibleKeyFrames(1).empty() && g.GetWeight(3, 1) == 0);
    g.AddConnection(0, 6, 40);
    EXPECT((g.GetVectorCovisibleKeyFrames(0) == V{6, 5, 3, 4}));
    g.EraseConnection(0, 6);
    g.EraseConnection(0, 6);
    EXPECT((g.GetVectorCovisibleKeyFrames(0) == V{5, 3, 4}));
    bool threw = false;
    try { g.GetWeight(0, K); } catch (const std::runtime_error &) { threw = true; }
    EXPECT(threw);
    g.clear();
    EXPECT(g.GetConnectedKeyFrames(0).empty());
    printf("covis_host_test ok\n");
    return 0;
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 2;
  }
}
