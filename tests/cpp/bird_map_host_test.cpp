// The C++ host mirror of the bird side of the key-frame graph and of the local bird map
// (fishbird::CovisibilityGraph::UpdateBirdConnections, GetBirdConnectedBirdKeyFrames and
// fishbird::CovisibilityMap::UpdateLocalBirdMap in host/fishbird_host.hpp) on maps whose answers can be read off by eye.
// Plain g++; links libfishbird_hip.so only.
#include <cstdio>
#include <vector>

#include "fishbird_host.hpp"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } } while (0)

using fishbird::CovisibilityGraph;
using fishbird::CovisibilityMap;
using fishbird::WindowTables;

// pKF->AddMapPointBird(pMPB, idx) and, when edge, pMPB->AddObservation(pKF, idx)
static void hold(WindowTables &t, int kf, int idx, int mpb, bool edge = true) {
  t.kfMapPointsBird[(size_t)kf * t.birdStride + idx] = mpb;
  t.kfNb[kf] = std::max(t.kfNb[kf], idx + 1);
  if (edge) { t.bobsMpb.push_back(mpb); t.bobsKf.push_back(kf); t.bobsIdx.push_back(idx); }
}

static bool same(const std::vector<int> &a, std::initializer_list<int> b) { return a == std::vector<int>(b); }

int main() {
  // ---- UpdateBirdConnections: kf0 holds points 0 1 2 3 and the bad point 4, kf1 holds 0 1 2, kf2 holds 2 3 4; kf3 holds
  // point 5 at two features and kf1 holds it once; kf4 holds nothing.  pKF order: kf1 < kf2 < kf0 < kf3 < kf4.
  const int K = 5, BS = 8;
  CovisibilityMap map(K, 4);
  map.kfOrder = {30, 10, 20, 40, 50};
  WindowTables t(map, 8, BS);
  t.mpbBad.assign(6, 0); t.mpbBad[4] = 1; t.mpbXw.assign(6 * 3, 0.f);
  for (int i = 0; i < 5; i++) hold(t, 0, i, i);
  for (int i = 0; i < 3; i++) hold(t, 1, i, i);
  hold(t, 2, 0, 2); hold(t, 2, 1, 3); hold(t, 2, 2, 4);
  hold(t, 3, 0, 5); hold(t, 3, 1, 5, false); hold(t, 1, 3, 5);
  CovisibilityGraph g(K);
  const std::vector<int32_t> frameId = {3, 6, 9, 12, 15};
  const std::vector<uint8_t> inMap = {1, 1, 1, 1, 1};
  const std::vector<int> all = {0, 1, 2, 3, 4};
  const fb_covis_kf_tables tv = t.view();
  std::vector<CovisibilityGraph::BirdUpdated> r = g.UpdateBirdConnections(map, tv, all, nullptr, 1, 0, frameId, inMap);
  // kf0 {kf1: 3, kf2: 2}; kf1 {kf0: 3, kf2: 1, kf3: 1}; kf2 {kf0: 2, kf1: 1}; kf3 {kf1: 2} (one point, two features); kf4 {}
  CHECK(r[0].nBirdCounter == 2 && r[1].nBirdCounter == 3 && r[2].nBirdCounter == 2 && r[3].nBirdCounter == 1 && r[4].nBirdCounter == 0, "counter sizes");
  CHECK(r[0].front == 1 && r[1].front == 0 && r[2].front == 0 && r[3].front == 1 && r[4].front == -1, "fronts");
  std::vector<int> w;
  CHECK(same(g.GetBirdConnectedBirdKeyFrames(0, &w), {1, 2}) && same(w, {3, 2}), "list of kf0");
  CHECK(same(g.GetBirdConnectedBirdKeyFrames(1, &w), {0}) && same(w, {3}), "list of kf1");
  CHECK(same(g.GetBirdConnectedBirdKeyFrames(3, &w), {1}) && same(w, {2}), "list of kf3: weight 2 from one shared point");
  CHECK(g.GetBirdConnectedBirdKeyFrames(4).empty(), "list of kf4");
  CHECK(g.GetVectorCovisibleKeyFrames(0).empty(), "the front list is untouched");
  std::vector<int32_t> parent(K);
  std::vector<uint8_t> linked(K), first(K);
  fishbird::check(fb_covis_tree_get(g.handle(), parent.data(), linked.data(), first.data()));
  CHECK(parent[0] == -1 && first[0] == 1, "mnId == 0 returns at :516");
  CHECK(parent[1] == 0 && parent[2] == 0 && parent[3] == 1 && linked[3] == 1 && first[3] == 0, "parents from the list's front");
  CHECK(parent[4] == -1 && first[4] == 1, "state 1: an empty counter does nothing");
  // state 3: kf4 (frame id 15) gets the nearest earlier key frame, kf3 (12)
  r = g.UpdateBirdConnections(map, tv, {4}, nullptr, 3, 0, frameId, inMap);
  fishbird::check(fb_covis_tree_get(g.handle(), parent.data(), linked.data(), first.data()));
  CHECK(r[0].nBirdCounter == 0 && parent[4] == 3 && linked[4] == 1 && first[4] == 0, "the search of :453-476");
  // a front counter of 0 and state 1: the key frame does not act
  g.clear();
  std::vector<CovisibilityGraph::Updated> front(1);
  front[0] = {0, -1};
  r = g.UpdateBirdConnections(map, tv, {0}, &front, 1, -1, frameId, inMap);
  CHECK(r[0].nBirdCounter == 0 && r[0].front == -1 && g.GetBirdConnectedBirdKeyFrames(0).empty(), "no front counter, no call");
  int32_t errors = -1;
  fishbird::check(fb_covis_error_count(g.handle(), &errors, nullptr));
  CHECK(errors == 0, "errors %d", errors);

  // ---- UpdateLocalBirdMap: three key frames, 12 fresh points each; kf2 is exactly 5 m from kf0 (3-4-0) and 7.2 m from kf1
  const int K2 = 3;
  CovisibilityMap map2(K2, 4);
  map2.kfOrder = {1, 2, 3};
  WindowTables t2(map2, 8, 16);
  t2.mpbBad.assign(36, 0); t2.mpbXw.assign(36 * 3, 0.f);
  for (int kf = 0; kf < K2; kf++)
    for (int i = 0; i < 12; i++) hold(t2, kf, i, kf * 12 + i, false);
  for (int kf = 0; kf < K2; kf++) { t2.kfTcw[(size_t)kf * 12] = t2.kfTcw[(size_t)kf * 12 + 5] = t2.kfTcw[(size_t)kf * 12 + 10] = 1.f; }
  t2.kfTcw[1 * 12 + 3] = 3.f;                                   // centre (-3, 0, 0)
  t2.kfTcw[2 * 12 + 3] = -3.f; t2.kfTcw[2 * 12 + 7] = -4.f;     // centre (3, 4, 0)
  CovisibilityGraph g2(K2);
  const fb_covis_kf_tables tv2 = t2.view();
  std::vector<int> localKF;
  std::vector<int> pts = map2.UpdateLocalBirdMap(g2.handle(), tv2, 0, localKF);
  CHECK(same(localKF, {0}) && pts.size() == 12 && pts[0] == 0 && pts[11] == 11, "first key frame");
  pts = map2.UpdateLocalBirdMap(g2.handle(), tv2, 1, localKF);
  CHECK(same(localKF, {1, 0}) && pts.size() == 24, "second key frame");
  pts = map2.UpdateLocalBirdMap(g2.handle(), tv2, 2, localKF);
  CHECK(same(localKF, {2, 0}) && pts.size() == 24 && pts[0] == 0 && pts[12] == 24, "kf0 at exactly 5 m stays, kf1 at 7.2 m leaves: %d members", (int)localKF.size());
  std::vector<uint64_t> order(36);
  for (int i = 0; i < 36; i++) order[i] = 1000 - i;             // descending pointers: the set iterates from the last index down
  localKF = {0};
  pts = map2.UpdateLocalBirdMap(g2.handle(), tv2, 1, localKF, &order);
  CHECK(pts.size() == 24 && pts[0] == 23 && pts[23] == 0, "the std::set's order");
  if (g_fail) { std::printf("bird_map_host_test: %d failure(s)\n", g_fail); return 1; }
  std::printf("bird_map_host_test ok\n");
  return 0;
}
