// kfdb.hip -- the reference's KeyFrameDatabase and ORBVocabulary::score on gfx950.
//
// Replaces (reference file:line):
//   KeyFrameDatabase::add / erase / clear                       src/KeyFrameDatabase.cc:40-73
//   KeyFrameDatabase::DetectLoopCandidates(pKF, minScore)       :76-197
//   KeyFrameDatabase::DetectRelocalizationCandidates(F)         :199-309
//   the reference-score loop of LoopClosing::DetectLoop         src/LoopClosing.cc:127-141
//   L1Scoring::score                                            Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
//
// Storage: fixed-stride rows [max_keyframes][word_stride] of word ids and values, so add / erase are O(1) row operations.
// The device needs no inverted file.  The reference walks the query's words ascending and each word's list in add order,
// so a key frame enters lKFsSharingWords at (its smallest word shared with the query, its add sequence number): a forward
// scan of every row (k_kfdb_count) plus one sort by that key (k_kfdb_select) yields the same list.  Scores do not depend on
// the list order, so k_kfdb_score runs between the two on every listed key frame above the common-word threshold.
// The double sum of a score is added in ascending word order on one accumulator (the order of the additions is the result).
#include "fb_common.h"
#include "fb_primitives.h"

#include <algorithm>

struct fb_kfdb;

namespace {

constexpr int KF_MAXK = FB_KFDB_MAX_KEYFRAMES;
constexpr int KF_MAXW = FB_KFDB_MAX_WORDS;
constexpr int KF_SEL_T = 1024;
constexpr unsigned long long KEY_NONE = ~0ull;

struct Db {            // device arrays of one handle (mode index: FB_KFDB_RELOC = 0, FB_KFDB_LOOP = 1)
  int K, S;
  uint32_t *ids;       // [K][S] word ids ascending
  double *vals;        // [K][S]
  int32_t *nw;         // [K] words of the row
  uint8_t *occ;        // [K] in the database
  uint32_t *seq;       // [K] add sequence number
  unsigned long long *query[2];  // mnRelocQuery / mnLoopQuery
  int32_t *words[2];   // mnRelocWords / mnLoopWords
  float *score[2];     // mRelocScore / mLoopScore
  // scratch of one query
  unsigned long long *key;  // [K] (smallest shared word, seq) of a listed slot, else KEY_NONE
  int32_t *first;      // [K] first list position naming the slot as pBestKF
  float *tmp;          // [K] scores of fb_kfdb_min_score when the caller wants none
  int32_t *hdr;        // [0] maxCommonWords, [1] lKFsSharingWords.size()
};

__device__ __forceinline__ int find_id(const uint32_t *ids, int n, uint32_t id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (ids[m] < id) lo = m + 1; else hi = m;
  }
  return (lo < n && ids[lo] == id) ? lo : -1;
}

// L1Scoring::score's sum for v1 = q, v2 = k, by one wavefront: 64 consecutive words of k per trip, each lane finds its
// partner in q and forms its term, then the terms are added in ascending lane (= word) order.  Every lane returns the sum.
__device__ __forceinline__ double wave_l1_sum(const uint32_t *q_ids, const double *q_vals, int nq, const uint32_t *k_ids,
                                              const double *k_vals, int nk, int lane) {
  double acc = 0.0;
  for (int base = 0; base < nk; base += 64) {
    const int w = base + lane;
    double term = 0.0;
    bool hit = false;
    if (w < nk) {
      const int j = find_id(q_ids, nq, k_ids[w]);
      if (j >= 0) {
        const double vi = q_vals[j], wi = k_vals[w];
        term = fabs(vi - wi) - fabs(vi) - fabs(wi);
        hit = true;
      }
    }
    unsigned long long m = __ballot(hit);
    while (m) {
      const int b = __ffsll((long long)m) - 1;
      m &= m - 1;
      acc += __shfl(term, b, 64);
    }
  }
  return acc;
}

__device__ __forceinline__ int min_common_words(int maxCommonWords) { return (int)((float)maxCommonWords * 0.8f); }

__global__ __launch_bounds__(256) void k_kfdb_add(Db D, int slot, uint32_t seq, const int32_t *n_words, const uint32_t *ids,
                                                  const double *vals) {
  const int n = min(max(*n_words, 0), D.S);
  const size_t ro = (size_t)slot * D.S;
  for (int i = threadIdx.x; i < n; i += blockDim.x) { D.ids[ro + i] = ids[i]; D.vals[ro + i] = vals[i]; }
  if (threadIdx.x == 0) {
    D.nw[slot] = n; D.occ[slot] = 1; D.seq[slot] = seq;
    for (int m = 0; m < 2; m++) { D.query[m][slot] = 0; D.words[m][slot] = 0; D.score[m][slot] = 0.0f; }
  }
}

// step 1 of both queries: shared words per key frame, the state rule of :86-104 / :207-222, the list key
__global__ __launch_bounds__(256) void k_kfdb_count(Db D, int mode, unsigned long long id, const int32_t *n_words,
                                                    const uint32_t *q_ids, int n_conn, const int32_t *conn) {
  __shared__ uint32_t s_q[KF_MAXW];
  const int nq = min(max(*n_words, 0), KF_MAXW);
  for (int i = threadIdx.x; i < nq; i += blockDim.x) s_q[i] = q_ids[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int kf = blockIdx.x * 4 + (threadIdx.x >> 6); kf < D.K; kf += gridDim.x * 4) {
    unsigned long long key = KEY_NONE;
    if (D.occ[kf]) {
      const int n = D.nw[kf];
      const uint32_t *row = D.ids + (size_t)kf * D.S;
      int c = 0;
      uint32_t mn = 0xffffffffu;
      for (int w = lane; w < n; w += 64) {
        const uint32_t wid = row[w];
        if (find_id(s_q, nq, wid) >= 0) { c++; mn = min(mn, wid); }
      }
      c = fb::wave_sum(c);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
      if (c > 0) {
        const bool fresh = D.query[mode][kf] != id;
        bool connected = false;
        if (fresh && mode == FB_KFDB_LOOP) {
          for (int i = 0; i < n_conn && !connected; i += 64)
            connected = __ballot(i + lane < n_conn && conn[i + lane] == kf) != 0;
        }
        if (lane == 0) {
          if (!fresh) D.words[mode][kf] += c;       // already touched by this id: keeps counting, is not listed again
          else if (connected) D.words[mode][kf] = 1;  // reset on every encounter, then ++ (:95, :102)
          else {
            D.words[mode][kf] = c;
            D.query[mode][kf] = id;
            key = ((unsigned long long)mn << 32) | D.seq[kf];
            atomicMax(&D.hdr[0], c);
            atomicAdd(&D.hdr[1], 1);
          }
        }
      }
    }
    if (lane == 0) D.key[kf] = key;
  }
}

// step 4: si = (float)score(query, slot) for the listed slots with more than minCommonWords common words
__global__ __launch_bounds__(256) void k_kfdb_score(Db D, int mode, const int32_t *n_words, const uint32_t *q_ids,
                                                    const double *q_vals) {
  __shared__ uint32_t s_q[KF_MAXW];
  const int nq = min(max(*n_words, 0), KF_MAXW);
  for (int i = threadIdx.x; i < nq; i += blockDim.x) s_q[i] = q_ids[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int minCommon = min_common_words(D.hdr[0]);
  for (int kf = blockIdx.x * 4 + (threadIdx.x >> 6); kf < D.K; kf += gridDim.x * 4) {
    if (D.key[kf] == KEY_NONE || D.words[mode][kf] <= minCommon) continue;
    const size_t ro = (size_t)kf * D.S;
    const double acc = wave_l1_sum(s_q, q_vals, nq, D.ids + ro, D.vals + ro, D.nw[kf], lane);
    if (lane == 0) D.score[mode][kf] = (float)(-acc / 2.0);
  }
}

// steps 2, 5 and 6: the list order, covisibility accumulation, retention, first-occurrence de-duplication
__global__ __launch_bounds__(KF_SEL_T) void k_kfdb_select(Db D, fb_kfdb_query_args A) {
  __shared__ unsigned long long s_key[KF_MAXK];
  __shared__ int s_val[KF_MAXK];
  __shared__ int s_wv[KF_SEL_T / 64];
  __shared__ float s_mx[KF_SEL_T / 64];
  __shared__ int s_nscored;
  const int tid = threadIdx.x, nt = KF_SEL_T, mode = A.mode, K = D.K;
  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  for (int i = tid; i < n2; i += nt) { s_key[i] = i < K ? D.key[i] : KEY_NONE; s_val[i] = i; }
  if (tid == 0) s_nscored = 0;
  __syncthreads();
  fb::bitonic_sort_kv(s_key, s_val, n2, tid, nt);
  const int L = min(D.hdr[1], K), maxCommon = D.hdr[0], minCommon = min_common_words(maxCommon);
  // the keys are not needed any more: their storage holds accScore and pBestKF per list position
  float *s_acc = reinterpret_cast<float *>(s_key);
  int *s_best = reinterpret_cast<int *>(s_key) + KF_MAXK;
  __syncthreads();
  float lmax = mode == FB_KFDB_LOOP ? A.min_score : 0.0f;  // bestAccScore's start (:145, :259)
  int nsc = 0;
  for (int p = tid; p < L; p += nt) {
    const int slot = s_val[p];
    float acc = 0.0f;
    int best = -1;
    if (D.words[mode][slot] > minCommon) {
      nsc++;
      const float si = D.score[mode][slot];
      if (mode == FB_KFDB_RELOC || si >= A.min_score) {
        float bestScore = si;
        acc = si;
        best = slot;
        for (int c = 0; c < FB_KFDB_COVIS; c++) {
          const int nb = A.covis[(size_t)slot * FB_KFDB_COVIS + c];
          if (nb < 0 || nb >= K) continue;
          if (D.query[mode][nb] != A.query_id) continue;
          if (mode == FB_KFDB_LOOP && !(D.words[mode][nb] > minCommon)) continue;
          const float s2 = D.score[mode][nb];
          acc += s2;
          if (s2 > bestScore) { best = nb; bestScore = s2; }
        }
        if (acc > lmax) lmax = acc;
      }
    }
    s_acc[p] = acc;
    s_best[p] = best;
  }
  for (int i = tid; i < K; i += nt) __hip_atomic_store(&D.first[i], INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  lmax = fb::wave_max(lmax);
  if ((tid & 63) == 0) s_mx[tid >> 6] = lmax;
  if (nsc) atomicAdd(&s_nscored, nsc);
  __syncthreads();
  float bestAcc = s_mx[0];
  for (int w = 1; w < KF_SEL_T / 64; w++) if (s_mx[w] > bestAcc) bestAcc = s_mx[w];
  const float minRetain = 0.75f * bestAcc;
  for (int p = tid; p < L; p += nt)
    if (s_best[p] >= 0 && s_acc[p] > minRetain) atomicMin(&D.first[s_best[p]], p);
  __syncthreads();
  // output in list order: contiguous chunk per thread, block scan of the chunk counts
  const int chunk = (L + nt - 1) / nt;
  const int p0 = min(tid * chunk, L), p1 = min(p0 + chunk, L);
  int cnt = 0;
  for (int p = p0; p < p1; p++)
    if (s_best[p] >= 0 && s_acc[p] > minRetain && __hip_atomic_load(&D.first[s_best[p]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p) cnt++;
  int total;
  int rank = fb::block_excl_scan<KF_SEL_T>(cnt, s_wv, &total);
  for (int p = p0; p < p1; p++)
    if (s_best[p] >= 0 && s_acc[p] > minRetain && __hip_atomic_load(&D.first[s_best[p]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p)
      A.candidates[rank++] = s_best[p];
  if (tid == 0) {
    *A.n_candidates = total;
    if (A.n_sharing) *A.n_sharing = L;
    if (A.max_common_words) *A.max_common_words = maxCommon;
    if (A.n_scored) *A.n_scored = s_nscored;
  }
  if (A.common_words) for (int i = tid; i < K; i += nt) A.common_words[i] = D.words[mode][i];
  if (A.scores) for (int i = tid; i < K; i += nt) A.scores[i] = D.score[mode][i];
}

// scores[i] = (float)score(query, slots[i]); one wavefront per entry
__global__ __launch_bounds__(64) void k_kfdb_list_score(Db D, const int32_t *n_words, const uint32_t *q_ids, const double *q_vals,
                                                        int n_list, const int32_t *slots, float *scores) {
  const int i = blockIdx.x;
  if (i >= n_list) return;
  const int slot = slots[i];
  float s = 0.0f;
  if (slot >= 0 && slot < D.K) {
    const size_t ro = (size_t)slot * D.S;
    const double acc = wave_l1_sum(q_ids, q_vals, max(*n_words, 0), D.ids + ro, D.vals + ro, D.nw[slot], threadIdx.x);
    s = (float)(-acc / 2.0);
  }
  if (threadIdx.x == 0) scores[i] = s;
}

// LoopClosing.cc:129-141 in the list's order (a slot outside the database counts as skipped)
__global__ void k_kfdb_min_score(Db D, int n_list, const int32_t *slots, const uint8_t *skip, const float *scores, float *min_score) {
  if (threadIdx.x || blockIdx.x) return;
  float minScore = 1;
  for (int i = 0; i < n_list; i++) {
    if ((skip && skip[i]) || slots[i] < 0 || slots[i] >= D.K) continue;
    const float score = scores[i];
    if (score < minScore) minScore = score;
  }
  *min_score = minScore;
}

__global__ __launch_bounds__(64) void k_bow_score(int stride, const int32_t *na, const uint32_t *a_ids, const double *a_vals,
                                                  const int32_t *nb, const uint32_t *b_ids, const double *b_vals, double *score) {
  const size_t o = (size_t)blockIdx.x * stride;
  const int n_a = min(max(na[blockIdx.x], 0), stride), n_b = min(max(nb[blockIdx.x], 0), stride);
  const double acc = wave_l1_sum(a_ids + o, a_vals + o, n_a, b_ids + o, b_vals + o, n_b, threadIdx.x);
  if (threadIdx.x == 0) score[blockIdx.x] = -acc / 2.0;
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

struct fb_kfdb {
  fb_kfdb_params p;
  void *block = nullptr;      // one allocation, made by the first call that needs the device
  size_t stateOff = 0, stateBytes = 0;  // the part fb_kfdb_clear zeroes
  Db D;
  std::vector<uint8_t> occ;   // occupancy in the order the calls were made
  uint32_t nextSeq = 0;
  int ensure() {
    FB_TRY(fb::check_device());
    if (block) return FB_OK;
    const size_t K = p.max_keyframes, S = p.word_stride;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += up256(bytes); return o; };
    const size_t oIds = take(K * S * 4), oVals = take(K * S * 8), oSeq = take(K * 4), oKey = take(K * 8), oFirst = take(K * 4),
                 oTmp = take(K * 4), oHdr = take(8);
    stateOff = off;
    const size_t oNw = take(K * 4), oOcc = take(K), oQ0 = take(K * 8), oQ1 = take(K * 8), oW0 = take(K * 4), oW1 = take(K * 4),
                 oS0 = take(K * 4), oS1 = take(K * 4);
    stateBytes = off - stateOff;
    FB_HIP(hipMalloc(&block, off));
    uint8_t *b = static_cast<uint8_t *>(block);
    D.K = (int)K; D.S = (int)S;
    D.ids = (uint32_t *)(b + oIds); D.vals = (double *)(b + oVals); D.seq = (uint32_t *)(b + oSeq);
    D.key = (unsigned long long *)(b + oKey); D.first = (int32_t *)(b + oFirst); D.tmp = (float *)(b + oTmp); D.hdr = (int32_t *)(b + oHdr);
    D.nw = (int32_t *)(b + oNw); D.occ = b + oOcc;
    D.query[0] = (unsigned long long *)(b + oQ0); D.query[1] = (unsigned long long *)(b + oQ1);
    D.words[0] = (int32_t *)(b + oW0); D.words[1] = (int32_t *)(b + oW1);
    D.score[0] = (float *)(b + oS0); D.score[1] = (float *)(b + oS1);
    // rows are read only below nw; everything else starts at 0 (the default stream orders this before any other stream's work
    // only through the synchronisation below: creation is rare)
    FB_HIP(hipMemset(b + oSeq, 0, off - oSeq));
    FB_HIP(hipDeviceSynchronize());
    return FB_OK;
  }
};

extern "C" {

int fb_bow_score_dev(int32_t batch, int32_t stride, const int32_t *na, const uint32_t *a_ids, const double *a_vals,
                     const int32_t *nb, const uint32_t *b_ids, const double *b_vals, double *score, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(batch >= 0 && stride > 0);
  if (batch == 0) return FB_OK;
  FB_ARG(na && a_ids && a_vals && nb && b_ids && b_vals && score);
  k_bow_score<<<batch, 64, 0, fb::as_stream(stream)>>>(stride, na, a_ids, a_vals, nb, b_ids, b_vals, score);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_bow_score(int32_t batch, int32_t stride, const int32_t *na, const uint32_t *a_ids, const double *a_vals,
                 const int32_t *nb, const uint32_t *b_ids, const double *b_vals, double *score) {
  FB_TRY(fb::check_device());
  FB_ARG(batch >= 0 && stride > 0);
  if (batch == 0) return FB_OK;
  FB_ARG(na && a_ids && a_vals && nb && b_ids && b_vals && score);
  const size_t B = batch, n = B * (size_t)stride;
  fb::Stager st;
  st.in(na, B * 4); st.in(a_ids, n * 4); st.in(a_vals, n * 8);
  st.in(nb, B * 4); st.in(b_ids, n * 4); st.in(b_vals, n * 8);
  st.out(score, B * 8, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_bow_score_dev(batch, stride, na, a_ids, a_vals, nb, b_ids, b_vals, score, nullptr));
  return st.fetch(nullptr);
}

int fb_kfdb_create(const fb_kfdb_params *p, fb_kfdb **out) {
  FB_ARG(p && out);
  FB_ARG(p->max_keyframes >= 1 && p->max_keyframes <= KF_MAXK && p->word_stride >= 1 && p->word_stride <= KF_MAXW);
  fb_kfdb *db = new fb_kfdb();
  db->p = *p;
  db->occ.assign(p->max_keyframes, 0);
  *out = db;
  return FB_OK;
}

int fb_kfdb_destroy(fb_kfdb *db) {
  if (!db) return FB_OK;
  if (db->block) { (void)hipDeviceSynchronize(); (void)hipFree(db->block); (void)hipGetLastError(); }
  delete db;
  return FB_OK;
}

int fb_kfdb_clear(fb_kfdb *db, void *stream) {
  FB_ARG(db);
  FB_TRY(db->ensure());
  FB_HIP(hipMemsetAsync(static_cast<uint8_t *>(db->block) + db->stateOff, 0, db->stateBytes, fb::as_stream(stream)));
  std::fill(db->occ.begin(), db->occ.end(), 0);
  return FB_OK;
}

int fb_kfdb_add_dev(fb_kfdb *db, int32_t slot, const int32_t *d_n_words, const uint32_t *d_bow_ids, const double *d_bow_vals,
                    void *stream) {
  FB_ARG(db);
  FB_TRY(db->ensure());
  FB_ARG(slot >= 0 && slot < db->p.max_keyframes);
  FB_ARG(d_n_words && d_bow_ids && d_bow_vals);
  if (db->occ[slot]) { fb::set_error("fb_kfdb_add: slot %d is already in the database", slot); return FB_ERR_ARG; }
  k_kfdb_add<<<1, 256, 0, fb::as_stream(stream)>>>(db->D, slot, db->nextSeq, d_n_words, d_bow_ids, d_bow_vals);
  FB_HIP(hipGetLastError());
  db->nextSeq++;
  db->occ[slot] = 1;
  return FB_OK;
}

int fb_kfdb_add(fb_kfdb *db, int32_t slot, int32_t n_words, const uint32_t *bow_ids, const double *bow_vals) {
  FB_ARG(db);
  FB_TRY(db->ensure());
  FB_ARG(n_words >= 0 && n_words <= db->p.word_stride);
  FB_ARG(n_words == 0 || (bow_ids && bow_vals));
  const int32_t *nw = &n_words;
  const uint32_t dummy_id = 0;
  const double dummy_val = 0.0;
  if (!bow_ids) bow_ids = &dummy_id;
  if (!bow_vals) bow_vals = &dummy_val;
  fb::Stager st;
  st.in(nw, 4); st.in(bow_ids, (size_t)n_words * 4); st.in(bow_vals, (size_t)n_words * 8);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_kfdb_add_dev(db, slot, nw, bow_ids, bow_vals, nullptr));
  return st.fetch(nullptr);
}

int fb_kfdb_add_frame_dev(fb_kfdb *db, int32_t slot, fb_frame *kf, void *stream) {
  FB_ARG(db && kf);
  fb_bow_transform_args v;
  FB_TRY(fb_frame_bow_view_dev(kf, &v));
  FB_ARG(v.f_stride <= db->p.word_stride);
  return fb_kfdb_add_dev(db, slot, v.n_words, v.bow_ids, v.bow_vals, stream);
}

int fb_kfdb_erase(fb_kfdb *db, int32_t slot, void *stream) {
  FB_ARG(db);
  FB_TRY(db->ensure());
  FB_ARG(slot >= 0 && slot < db->p.max_keyframes);
  if (!db->occ[slot]) { fb::set_error("fb_kfdb_erase: slot %d is not in the database", slot); return FB_ERR_ARG; }
  FB_HIP(hipMemsetAsync(db->D.occ + slot, 0, 1, fb::as_stream(stream)));
  db->occ[slot] = 0;
  return FB_OK;
}

int fb_kfdb_query_dev(fb_kfdb *db, const fb_kfdb_query_args *A, void *stream) {
  FB_ARG(db && A);
  FB_TRY(db->ensure());
  FB_ARG(A->mode == FB_KFDB_RELOC || A->mode == FB_KFDB_LOOP);
  FB_ARG(A->n_words && A->bow_ids && A->bow_vals && A->covis && A->n_candidates && A->candidates);
  FB_ARG(A->mode == FB_KFDB_RELOC || (A->n_connected >= 0 && (A->n_connected == 0 || A->connected)));
  hipStream_t s = fb::as_stream(stream);
  fb::ProfScope prof_(fb::P_KFDB, s);
  const int grid = std::min((db->p.max_keyframes + 3) / 4, 1024);
  FB_HIP(hipMemsetAsync(db->D.hdr, 0, 8, s));
  k_kfdb_count<<<grid, 256, 0, s>>>(db->D, A->mode, (unsigned long long)A->query_id, A->n_words, A->bow_ids,
                                    A->mode == FB_KFDB_LOOP ? A->n_connected : 0, A->connected);
  k_kfdb_score<<<grid, 256, 0, s>>>(db->D, A->mode, A->n_words, A->bow_ids, A->bow_vals);
  k_kfdb_select<<<1, KF_SEL_T, 0, s>>>(db->D, *A);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_kfdb_query(fb_kfdb *db, const fb_kfdb_query_args *H) {
  FB_ARG(db && H);
  FB_TRY(db->ensure());
  FB_ARG(H->n_words && H->covis && H->n_candidates && H->candidates);
  const int nq = *H->n_words;
  FB_ARG(nq >= 0 && nq <= KF_MAXW && (nq == 0 || (H->bow_ids && H->bow_vals)));
  FB_ARG(H->mode == FB_KFDB_RELOC || (H->n_connected >= 0 && (H->n_connected == 0 || H->connected)));
  fb_kfdb_query_args D = *H;
  const uint32_t dummy_id = 0;
  const double dummy_val = 0.0;
  if (!D.bow_ids) D.bow_ids = &dummy_id;
  if (!D.bow_vals) D.bow_vals = &dummy_val;
  if (H->mode != FB_KFDB_LOOP || H->n_connected == 0) { D.connected = nullptr; D.n_connected = 0; }
  const size_t K = db->p.max_keyframes;
  fb::Stager st;
  st.in(D.n_words, 4); st.in(D.bow_ids, (size_t)nq * 4); st.in(D.bow_vals, (size_t)nq * 8);
  st.in(D.connected, (size_t)D.n_connected * 4); st.in(D.covis, K * FB_KFDB_COVIS * 4);
  st.out(D.n_candidates, 4, false);
  st.out(D.candidates, K * 4, true);  // copy-in: entries past n_candidates keep the caller's contents
  st.out(D.n_sharing, 4, false); st.out(D.max_common_words, 4, false); st.out(D.n_scored, 4, false);
  st.out(D.common_words, K * 4, false); st.out(D.scores, K * 4, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_kfdb_query_dev(db, &D, nullptr));
  return st.fetch(nullptr);
}

int fb_kfdb_min_score_dev(fb_kfdb *db, const int32_t *d_n_words, const uint32_t *d_bow_ids, const double *d_bow_vals,
                          int32_t n_list, const int32_t *d_slots, const uint8_t *d_skip, float *d_scores, float *d_min_score,
                          void *stream) {
  FB_ARG(db);
  FB_TRY(db->ensure());
  FB_ARG(d_n_words && d_bow_ids && d_bow_vals && d_min_score);
  FB_ARG(n_list >= 0 && n_list <= db->p.max_keyframes && (n_list == 0 || d_slots));
  hipStream_t s = fb::as_stream(stream);
  float *scores = d_scores ? d_scores : db->D.tmp;
  if (n_list) k_kfdb_list_score<<<n_list, 64, 0, s>>>(db->D, d_n_words, d_bow_ids, d_bow_vals, n_list, d_slots, scores);
  k_kfdb_min_score<<<1, 64, 0, s>>>(db->D, n_list, d_slots, d_skip, scores, d_min_score);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_kfdb_min_score(fb_kfdb *db, int32_t n_words, const uint32_t *bow_ids, const double *bow_vals, int32_t n_list,
                      const int32_t *slots, const uint8_t *skip, float *scores, float *min_score) {
  FB_ARG(db);
  FB_TRY(db->ensure());
  FB_ARG(n_words >= 0 && (n_words == 0 || (bow_ids && bow_vals)) && min_score);
  FB_ARG(n_list >= 0 && n_list <= db->p.max_keyframes && (n_list == 0 || slots));
  const int32_t *nw = &n_words;
  const uint32_t dummy_id = 0;
  const double dummy_val = 0.0;
  if (!bow_ids) bow_ids = &dummy_id;
  if (!bow_vals) bow_vals = &dummy_val;
  fb::Stager st;
  st.in(nw, 4); st.in(bow_ids, (size_t)n_words * 4); st.in(bow_vals, (size_t)n_words * 8);
  st.in(slots, (size_t)n_list * 4); st.in(skip, (size_t)n_list);
  st.out(scores, (size_t)n_list * 4, false); st.out(min_score, 4, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_kfdb_min_score_dev(db, nw, bow_ids, bow_vals, n_list, slots, skip, scores, min_score, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
