// local_map_host_test.cpp -- drives the host-pointer variants of the spanning tree and Tracking::UpdateLocalMap
// (fb_covis_tree_get, fb_covis_children, fb_covis_local_map) on fishbird::CovisibilityGraph / CovisibilityMap
// (host/fishbird_host.hpp), on a map whose answers are known by construction.  Every array has exactly the documented size.
#include <cstdio>
#include <cstdlib>

#include "fishbird_host.hpp"

#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

typedef std::vector<int32_t> V;

struct LocalMap {               // the arrays of one fb_covis_local_map call, each of exactly the documented size
  int B, S, capKf, capMp;
  V n, mapPoint, localKf, nLocalKf, localMp, nLocalMp, refKf, nVoters, overflow;
  std::vector<uint8_t> kfBad;
  LocalMap(int B_, int S_, int K, int capKf_, int capMp_)
      : B(B_), S(S_), capKf(capKf_), capMp(capMp_), n(B_, 0), mapPoint((size_t)B_ * S_, -1), localKf((size_t)B_ * capKf_, -5), nLocalKf(B_, 0),
        localMp((size_t)B_ * capMp_, -5), nLocalMp(B_, -5), refKf(B_, -1), nVoters(B_, -5), overflow(B_, -5), kfBad(K, 0) {}
  int run(fishbird::CovisibilityGraph &g, const fishbird::CovisibilityMap &map, const int32_t *gate, int gateMin) {
    fb_local_map_args a;
    memset(&a, 0, sizeof(a));
    a.batch = B; a.kp_stride = S; a.d_n = n.data(); a.d_map_point = mapPoint.data(); a.d_kf_bad = kfBad.data();
    a.cap_kf = capKf; a.d_local_kf = localKf.data(); a.d_n_local_kf = nLocalKf.data();
    a.cap_mp = capMp; a.d_local_mp = localMp.data(); a.d_n_local_mp = nLocalMp.data();
    a.d_ref_kf = refKf.data(); a.d_n_voters = nVoters.data(); a.d_overflow = overflow.data();
    a.d_gate_row = gate; a.gate_min = gateMin;
    const fb_covis_map m = map.view();
    return fb_covis_local_map(g.handle(), &m, &a);
  }
  V kf(int b) const { return V(localKf.begin() + (size_t)b * capKf, localKf.begin() + (size_t)b * capKf + std::min<int>(nLocalKf[b], capKf)); }
  V mp(int b) const { return V(localMp.begin() + (size_t)b * capMp, localMp.begin() + (size_t)b * capMp + std::min<int>(nLocalMp[b], capMp)); }
};

int main() {
  try {
    const int K = 8, S = 16;
    fishbird::CovisibilityMap map(K, S);
    for (int s = 0; s < K; s++) map.kfOrder[s] = 0x7000 + 0x100 * s;
    const int A = map.NewMapPoint(), Bp = map.NewMapPoint(), Cp = map.NewMapPoint(), bad = map.NewMapPoint();
    map.AddObservation(A, 0, 0, 0);            // A is seen by key frame 0, B by 1, C by 4 and 1
    map.AddObservation(Bp, 1, 0, 0);
    map.AddObservation(Cp, 4, 0, 0);
    map.AddObservation(Cp, 1, 1, 0);
    map.AddObservation(bad, 6, 0, 0);
    map.mpBad[bad] = 1;
    fishbird::CovisibilityGraph g(K);
    fb_covis *h = g.handle();
    g.AddConnection(0, 2, 20);
    g.AddConnection(1, 4, 20);
    fishbird::check(fb_covis_change_parent_dev(h, 0, 3, nullptr));
    fishbird::check(fb_covis_change_parent_dev(h, 7, 3, nullptr));
    fishbird::check(fb_covis_change_parent_dev(h, 5, 3, nullptr));
    fishbird::check(fb_covis_erase_child_dev(h, 3, 5, nullptr));
    V parent(K, -7);
    std::vector<uint8_t> linked(K, 9), first(K, 9);
    fishbird::check(fb_covis_tree_get(h, parent.data(), linked.data(), first.data()));
    EXPECT((parent == V{3, -1, -1, -1, -1, 3, -1, 3}));
    EXPECT(linked[0] == 1 && linked[7] == 1 && linked[5] == 0 && linked[3] == 0 && first[0] == 1 && first[7] == 1);
    fishbird::check(fb_covis_tree_get(h, nullptr, linked.data(), nullptr));      // a NULL array is left out
    int32_t nc = -1;
    V kids(K, -7);
    fishbird::check(fb_covis_children(h, 3, &nc, kids.data()));
    EXPECT(nc == 2 && kids[0] == 0 && kids[1] == 7 && kids[2] == -7);            // ascending pointer; the rest is the caller's
    fishbird::check(fb_covis_children(h, 2, &nc, kids.data()));
    EXPECT(nc == 0);
    // sequence 0 holds A and B: voters 0 and 1; 0 takes its neighbour 2 and its parent 3, which ends the loop (1's neighbour 4
    // is never added).  Sequence 1 holds only the bad point: it is cleared, the list that came in stays, its points are collected.
    LocalMap lm(2, 3, K, 6, 4);
    lm.n = {2, 3};
    lm.mapPoint = {A, Bp, -1, -1, bad, -1};
    lm.localKf[6] = 4; lm.localKf[7] = 1; lm.nLocalKf[1] = 2; lm.refKf[1] = 6;
    fishbird::check(lm.run(g, map, nullptr, 0));
    EXPECT((lm.kf(0) == V{0, 1, 2, 3}) && lm.localKf[4] == -5 && lm.refKf[0] == 0 && lm.nVoters[0] == 2 && lm.overflow[0] == 0);
    EXPECT((lm.mp(0) == V{A, Bp, Cp}) && lm.localMp[3] == -5);   // key frame 1 holds B and C
    EXPECT((lm.kf(1) == V{4, 1}) && lm.refKf[1] == 6 && lm.nVoters[1] == 0 && lm.overflow[1] == 0 && (lm.mp(1) == V{Cp, Bp}));
    EXPECT(lm.mapPoint[4] == -1 && lm.mapPoint[0] == A);
    // a gate: sequence 1 is left entirely alone
    LocalMap gated(2, 3, K, 6, 4);
    gated.n = {2, 3};
    gated.mapPoint = {A, Bp, -1, -1, bad, -1};
    const int32_t row[2] = {10, 9};
    fishbird::check(gated.run(g, map, row, 10));
    EXPECT((gated.kf(0) == V{0, 1, 2, 3}) && gated.nLocalMp[1] == -5 && gated.nVoters[1] == -5 && gated.overflow[1] == -5 && gated.mapPoint[4] == bad);
    // capacities one below: the prefix, the full lengths, the flag
    LocalMap small(1, 2, K, 3, 1);
    small.n = {2};
    small.mapPoint = {A, Bp};
    fishbird::check(small.run(g, map, nullptr, 0));
    EXPECT(small.nLocalKf[0] == 4 && (small.kf(0) == V{0, 1, 2}) && small.overflow[0] == 1 && small.nLocalMp[0] == 3 && (small.mp(0) == V{A}));
    fb_local_map_args none;
    memset(&none, 0, sizeof(none));
    const fb_covis_map m = map.view();
    EXPECT(fb_covis_local_map(h, &m, &none) == FB_ERR_ARG && fb_covis_children(h, K, &nc, kids.data()) == FB_ERR_ARG);
    int32_t errors = -1;
    fishbird::check(fb_covis_error_count(h, &errors, nullptr));
    EXPECT(errors == 0);
    g.clear();
    fishbird::check(fb_covis_tree_get(h, parent.data(), linked.data(), first.data()));
    EXPECT((parent == V(K, -1)) && linked[0] == 0 && first[3] == 1);
    printf("local_map_host_test ok\n");
    return 0;
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 2;
  }
}
