// The C++ host mirror of the loop-closing steps on the covisibility handle (fishbird::CovisibilityMap::DetectLoop,
// LoopMapPoints and LoopConnections in host/fishbird_host.hpp) on a map whose answers can be read off by eye.
// Plain g++; links libfishbird_hip.so only.
#include <cstdio>
#include <vector>

#include "fishbird_host.hpp"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } } while (0)

using fishbird::CovisibilityGraph;
using fishbird::CovisibilityMap;

static bool same(const std::vector<int> &a, std::initializer_list<int> b) { return a == std::vector<int>(b); }

// n new points seen by key frames a and b, at the next free features of both
static void share(CovisibilityMap &m, int a, int b, int n) {
  for (int i = 0; i < n; i++) {
    const int p = m.NewMapPoint();
    m.AddObservation(p, a, m.kfN[a], 0);
    m.AddObservation(p, b, m.kfN[b], 0);
  }
}

int main() {
  // Six key frames, pKF order = slot order.  0 and 1 share 20 points, 0 and 2 share 16, 2 and 5 share 3.
  const int K = 6;
  CovisibilityMap map(K, 64);
  map.kfOrder = {10, 20, 30, 40, 50, 60};
  share(map, 0, 1, 20);
  share(map, 0, 2, 16);
  share(map, 2, 5, 3);
  CovisibilityGraph g(K);
  g.UpdateConnections(map, {0, 1, 2});
  // rows: 0 {1: 20, 2: 16}; 1 {0: 20}; 2 {0: 16, 5: 3 (an entry, not a member)}; 5: nothing (it is no member of row 2)
  CHECK(same(g.GetVectorCovisibleKeyFrames(0), {1, 2}) && same(g.GetVectorCovisibleKeyFrames(2), {0}), "the graph");

  // ---- DetectLoop, th = 3: candidate 2 four times; its group is {0, 2, 5}
  int nGroups = -1;
  bool overflow = true;
  for (int k = 0; k < 3; k++) CHECK(map.DetectLoop(g.handle(), {2}, 3, &nGroups, &overflow).empty() && nGroups == 1 && !overflow, "call %d", k);
  CHECK(same(map.DetectLoop(g.handle(), {2}), {2}), "the fourth consecutive detection is enough");
  // candidate 5 (an empty row) meets that group through the below-threshold entry of row 2: counter 3 + 1
  CHECK(same(map.DetectLoop(g.handle(), {5, 4}, 3, &nGroups), {5}) && nGroups == 2, "through a non-member entry; 4 starts a new group");
  CHECK(map.DetectLoop(g.handle(), {}, 3, &nGroups).empty() && nGroups == 0, "no candidates: the groups are cleared");

  // ---- LoopMapPoints of key frame 0: the list is [1, 2, 0]; 1 holds points 0..19, 2 holds 20..35 and 36..38, 0 adds nothing
  map.mpBad[7] = 1;
  std::vector<int> pts = map.LoopMapPoints(g.handle(), 0);
  CHECK(pts.size() == 38 && pts[0] == 0 && pts[7] == 8 && pts[19] == 20 && pts[37] == 38, "loop points: %zu", pts.size());
  map.mpBad[7] = 0;

  // ---- LoopConnections over [1, 2, 0] after a fusion that makes 1 and 4 share 15 points and 2 and 3 share 2
  share(map, 1, 4, 15);
  share(map, 2, 3, 2);
  std::vector<std::pair<int, int>> up;
  std::vector<std::vector<int>> lc = map.LoopConnections(g.handle(), {1, 2, 0}, &up);
  // 1: {0, 4} - neighbours {0} - the list = {4};  2: {0, 3, 5} - neighbours {0} - the list = {3, 5} (entries below the
  // threshold count: GetConnectedKeyFrames);  0: {1, 2}: both in the list
  CHECK(lc.size() == 3 && same(lc[0], {4}) && same(lc[1], {3, 5}) && lc[2].empty(), "LoopConnections");
  CHECK(up[0] == std::make_pair(2, 0) && up[1] == std::make_pair(3, 0) && up[2] == std::make_pair(2, 1), "counter sizes and fronts");
  CHECK(same(g.GetVectorCovisibleKeyFrames(1), {0, 4}) && same(g.GetVectorCovisibleKeyFrames(4), {1}), "the graph after the pass");
  int32_t errors = -1;
  fishbird::check(fb_covis_error_count(g.handle(), &errors, nullptr));
  CHECK(errors == 0, "errors %d", errors);
  if (g_fail == 0) std::printf("loop_detect_host_test ok\n");
  return g_fail ? 1 : 0;
}
