// kfdb_host_test.cpp -- drives fishbird::KeyFrameDatabase (host/fishbird_host.hpp) the way Tracking::Relocalization and
// LoopClosing::DetectLoop drive the reference's KeyFrameDatabase, on a database whose answers are known by construction.
#include <cstdio>
#include <cstdlib>

#include "fishbird_host.hpp"

using fishbird::BowVector;

#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// n words starting at `first`, equal weights (L1 norm 1)
static BowVector words(unsigned first, int n) {
  BowVector v;
  for (int i = 0; i < n; i++) v[first + i] = 1.0 / n;
  return v;
}

int main() {
  try {
    // place A: slots 0..2 hold words 0..19 / 0..15 / 4..19; place B: slots 3, 4 hold words 1000..; slot 5 shares one word with A
    fishbird::KeyFrameDatabase db(8, 64);
    db.add(0, words(0, 20));
    db.add(1, words(0, 16));
    db.add(2, words(4, 16));
    db.add(3, words(1000, 20));
    db.add(4, words(1004, 20));
    BowVector stray = words(2000, 9);
    stray[3] = 0.1;
    db.add(5, stray);
    for (int s = 0; s < 3; s++) db.SetBestCovisibilityKeyFrames(s, {(s + 1) % 3, (s + 2) % 3});
    db.SetBestCovisibilityKeyFrames(3, {4});
    db.SetBestCovisibilityKeyFrames(4, {3});
    const BowVector q = words(0, 20);
    EXPECT(fishbird::KeyFrameDatabase::score(q, q) > 1.0 - 1e-12 && fishbird::KeyFrameDatabase::score(q, q) < 1.0 + 1e-12);
    EXPECT(fishbird::KeyFrameDatabase::score(q, words(1000, 20)) == 0.0);
    // slot 0 is the query itself (score 1); 1 and 2 share 16 of 20 words (16 > (int)(20 * 0.8f) = 16 is false: not scored);
    // slot 5 shares one word.  Every retained entry of place A names slot 0 as its best key frame.
    std::vector<int> c = db.DetectRelocalizationCandidates(1, q);
    EXPECT(c.size() == 1 && c[0] == 0);
    EXPECT(db.DetectRelocalizationCandidates(1, q).empty());        // the same mnId again: nothing is listed
    c = db.DetectRelocalizationCandidates(2, words(1002, 20));
    EXPECT(c.size() == 2 && c[0] == 3 && c[1] == 4);                // 18 shared words each: both scored, each its own best
    // DetectLoop: the reference score over the connected key frames, then the query that excludes them
    const float minScore = db.MinScore(q, {1, 2}, {0, 0});
    EXPECT(minScore > 0.7f && minScore < 0.9f);                      // 16 shared words of weight 1/20 vs 1/16: 0.8
    EXPECT(db.MinScore(q, {1, 3}, {0, 1}) == minScore && db.MinScore(q, {3}, {0}) == 0.0f && db.MinScore(q, {}, {}) == 1.0f);
    c = db.DetectLoopCandidates(3, q, {1, 2}, minScore);
    EXPECT(c.size() == 1 && c[0] == 0);
    c = db.DetectLoopCandidates(4, q, {0, 1, 2}, 0.01f);
    EXPECT(c.size() == 1 && c[0] == 5);                             // every key frame of the place is connected: slot 5 alone is listed
    db.erase(0);
    c = db.DetectRelocalizationCandidates(5, q);
    EXPECT(c.size() == 2 && c[0] == 1 && c[1] == 2);                // add order within word 0 / word 4
    bool threw = false;
    try { db.erase(0); } catch (const std::runtime_error &) { threw = true; }
    EXPECT(threw);
    db.clear();
    EXPECT(db.DetectRelocalizationCandidates(6, q).empty());
    printf("kfdb_host_test ok\n");
    return 0;
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 2;
  }
}
