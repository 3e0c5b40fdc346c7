// window_map_ref.cpp -- the window of Optimizer::LocalBundleAdjustmentWithOdom (Optimizer.cc:2139-2227) and its edge loops
// (:2312-2417) restated with the containers the reference uses: KeyFrame / MapPoint objects holding
// std::map<KeyFrame*, size_t> observations and the mnBALocalForKF / mnBAFixedForKF marks.  Stand-alone, plain C++: what one
// host core pays for the walk, and a second model for the lists.
//   window_map_ref map.bin cur with_bird [reps]   ->  one line per list, then "ms <per call>"
// map.bin: int32 K, S, n_mp, n_obs, BS, n_mpb, n_bobs, n_nei; then kf_n[K], kf_mp[K][S], mp_bad[n_mp] (u8), obs_mp, obs_kf,
// obs_idx [n_obs], kf_order[K] (u64), kf_bad[K] (u8), kf_nb[K], kf_mpb[K][BS], mpb_bad[n_mpb] (u8), bobs_mpb, bobs_kf, bobs_idx
// [n_bobs], neighbours[n_nei] (GetVectorCovisibleKeyFrames of cur).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <vector>

struct KeyFrame;
struct MapPoint {
  int index = 0;
  bool bad = false;
  long mnBALocalForKF = -1;
  std::map<KeyFrame *, size_t> mObservations;
  std::map<KeyFrame *, int> mEdge;   // the observation's index in the edge list
};
struct KeyFrame {
  int slot = 0;
  bool bad = false;
  long mnBALocalForKF = -1, mnBAFixedForKF = -1;
  std::vector<MapPoint *> mvpMapPoints, mvpMapPointsBird;
};

template <typename T> static std::vector<T> rd(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short file\n"); exit(2); }
  return v;
}

struct Window {
  std::list<KeyFrame *> lLocalKeyFrames, lFixedCameras;
  std::list<MapPoint *> lLocalMapPoints, lLocalMapPointsBirds;
  std::vector<int> eKf[2], ePt[2], eSrc[2];
};

static void points_of(std::list<KeyFrame *> &kfs, bool bird, long id, std::list<MapPoint *> &out) {
  for (KeyFrame *pKF : kfs) {
    std::vector<MapPoint *> vpMPs = bird ? pKF->mvpMapPointsBird : pKF->mvpMapPoints;   // GetMapPointMatches() copies
    for (MapPoint *pMP : vpMPs)
      if (pMP && !pMP->bad && pMP->mnBALocalForKF != id) { out.push_back(pMP); pMP->mnBALocalForKF = id; }
  }
}

static void fixed_of(std::list<MapPoint *> &pts, long id, std::list<KeyFrame *> &out) {
  for (MapPoint *pMP : pts) {
    std::map<KeyFrame *, size_t> observations = pMP->mObservations;                     // GetObservations() copies
    for (auto &o : observations) {
      KeyFrame *pKFi = o.first;
      if (pKFi->mnBALocalForKF != id && pKFi->mnBAFixedForKF != id) {
        pKFi->mnBAFixedForKF = id;
        if (!pKFi->bad) out.push_back(pKFi);
      }
    }
  }
}

static void window(KeyFrame *pKF, const std::vector<KeyFrame *> &vNeighKFs, bool bHaveBird, long id, Window &w) {
  w.lLocalKeyFrames.push_back(pKF);
  pKF->mnBALocalForKF = id;
  for (KeyFrame *pKFi : vNeighKFs) {
    pKFi->mnBALocalForKF = id;
    if (!pKFi->bad) w.lLocalKeyFrames.push_back(pKFi);
  }
  points_of(w.lLocalKeyFrames, false, id, w.lLocalMapPoints);
  fixed_of(w.lLocalMapPoints, id, w.lFixedCameras);
  if (bHaveBird) {
    points_of(w.lLocalKeyFrames, true, id, w.lLocalMapPointsBirds);
    fixed_of(w.lLocalMapPointsBirds, id, w.lFixedCameras);
  }
  std::map<KeyFrame *, int> vertex;
  int n = 0;
  for (KeyFrame *k : w.lLocalKeyFrames) vertex[k] = n++;
  for (KeyFrame *k : w.lFixedCameras) vertex[k] = n++;
  for (int sd = 0; sd < (bHaveBird ? 2 : 1); sd++) {
    int j = 0;
    for (MapPoint *pMP : sd ? w.lLocalMapPointsBirds : w.lLocalMapPoints) {
      for (auto &o : pMP->mObservations)
        if (!o.first->bad) { w.eKf[sd].push_back(vertex[o.first]); w.ePt[sd].push_back(j); w.eSrc[sd].push_back(pMP->mEdge[o.first]); }
      j++;
    }
  }
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: window_map_ref map.bin cur with_bird [reps]\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  const int cur = atoi(argv[2]), with_bird = atoi(argv[3]), reps = argc > 4 ? atoi(argv[4]) : 1;
  const std::vector<int32_t> h = rd<int32_t>(f, 8);
  const int K = h[0], S = h[1], n_mp = h[2], n_obs = h[3], BS = h[4], n_mpb = h[5], n_bobs = h[6], n_nei = h[7];
  const auto kf_n = rd<int32_t>(f, K), kf_mp = rd<int32_t>(f, (size_t)K * S);
  const auto mp_bad = rd<uint8_t>(f, n_mp);
  const auto obs_mp = rd<int32_t>(f, n_obs), obs_kf = rd<int32_t>(f, n_obs), obs_idx = rd<int32_t>(f, n_obs);
  const auto kf_order = rd<uint64_t>(f, K);
  const auto kf_bad = rd<uint8_t>(f, K);
  const auto kf_nb = rd<int32_t>(f, K), kf_mpb = rd<int32_t>(f, (size_t)K * BS);
  const auto mpb_bad = rd<uint8_t>(f, n_mpb);
  const auto bobs_mpb = rd<int32_t>(f, n_bobs), bobs_kf = rd<int32_t>(f, n_bobs), bobs_idx = rd<int32_t>(f, n_bobs);
  const auto nei = rd<int32_t>(f, n_nei);
  fclose(f);
  // std::map<KeyFrame*, ..> orders by address: the key frames lie in one array in ascending (kf_order, slot)
  std::vector<int> by(K);
  for (int s = 0; s < K; s++) by[s] = s;
  std::sort(by.begin(), by.end(), [&](int a, int b) { return kf_order[a] != kf_order[b] ? kf_order[a] < kf_order[b] : a < b; });
  std::vector<KeyFrame> store(K);
  std::vector<KeyFrame *> kf(K);
  for (int r = 0; r < K; r++) { kf[by[r]] = &store[r]; store[r].slot = by[r]; store[r].bad = kf_bad[by[r]] != 0; }
  std::vector<MapPoint> mp(n_mp), mpb(n_mpb);
  for (int i = 0; i < n_mp; i++) { mp[i].index = i; mp[i].bad = mp_bad[i] != 0; }
  for (int i = 0; i < n_mpb; i++) { mpb[i].index = i; mpb[i].bad = mpb_bad[i] != 0; }
  for (int s = 0; s < K; s++) {
    const int n = std::min(std::max(kf_n[s], 0), S), nb = BS ? std::min(std::max(kf_nb[s], 0), BS) : 0;
    kf[s]->mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n; i++) { const int m = kf_mp[(size_t)s * S + i]; if (m >= 0 && m < n_mp) kf[s]->mvpMapPoints[i] = &mp[m]; }
    kf[s]->mvpMapPointsBird.assign(nb, nullptr);
    for (int i = 0; i < nb; i++) { const int m = kf_mpb[(size_t)s * BS + i]; if (m >= 0 && m < n_mpb) kf[s]->mvpMapPointsBird[i] = &mpb[m]; }
  }
  for (int e = 0; e < n_obs; e++) {
    if (obs_kf[e] < 0 || obs_kf[e] >= K || obs_mp[e] < 0 || obs_mp[e] >= n_mp || obs_idx[e] < 0 || obs_idx[e] >= S) continue;
    mp[obs_mp[e]].mObservations[kf[obs_kf[e]]] = obs_idx[e]; mp[obs_mp[e]].mEdge[kf[obs_kf[e]]] = e;
  }
  for (int e = 0; e < n_bobs; e++) {
    if (bobs_kf[e] < 0 || bobs_kf[e] >= K || bobs_mpb[e] < 0 || bobs_mpb[e] >= n_mpb || bobs_idx[e] < 0 || bobs_idx[e] >= BS) continue;
    mpb[bobs_mpb[e]].mObservations[kf[bobs_kf[e]]] = bobs_idx[e]; mpb[bobs_mpb[e]].mEdge[kf[bobs_kf[e]]] = e;
  }
  std::vector<KeyFrame *> vNeighKFs;
  for (int s : nei) vNeighKFs.push_back(kf[s]);
  Window w;
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < reps; r++) {
    w = Window();
    window(kf[cur], vNeighKFs, with_bird != 0, 1000 + r, w);   // a fresh mnId per call, as every new key frame has
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
  printf("local"); for (KeyFrame *k : w.lLocalKeyFrames) printf(" %d", k->slot); printf("\n");
  printf("fixed"); for (KeyFrame *k : w.lFixedCameras) printf(" %d", k->slot); printf("\n");
  printf("mp"); for (MapPoint *p : w.lLocalMapPoints) printf(" %d", p->index); printf("\n");
  printf("mpb"); for (MapPoint *p : w.lLocalMapPointsBirds) printf(" %d", p->index); printf("\n");
  const char *names[2][3] = {{"obs_kf", "obs_mp", "obs_src"}, {"bobs_kf", "bobs_mpb", "bobs_src"}};
  for (int sd = 0; sd < 2; sd++) {
    const std::vector<int> *l[3] = {&w.eKf[sd], &w.ePt[sd], &w.eSrc[sd]};
    for (int k = 0; k < 3; k++) { printf("%s", names[sd][k]); for (int v : *l[k]) printf(" %d", v); printf("\n"); }
  }
  printf("ms %.4f\n", ms);
  return 0;
}
