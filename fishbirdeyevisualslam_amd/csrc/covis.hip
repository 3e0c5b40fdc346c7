// covis.hip -- the reference's covisibility graph and KeyFrameCulling on gfx950.
//
// Replaces (reference file:line):
//   KeyFrame::AddConnection / UpdateBestCovisibles                 src/KeyFrame.cc:179-213
//   KeyFrame::GetConnectedKeyFrames .. GetWeight                   :221-270
//   KeyFrame::UpdateConnections (graph part)                       :564-663
//   KeyFrame::SetBadFlag (graph part) / EraseConnection            :797-798, :807-808, :885-899
//   LocalMapping::KeyFrameCulling                                  src/LocalMapping.cc:656-729
//   MapPoint::EraseObservation (its effect on later key frames)    src/MapPoint.cc:111-137
//   the spanning tree and Tracking::UpdateLocalMap                  covis_tree.inc
//   LoopClosing::CorrectLoop and the map update after the global BA  covis_correct.inc
//   KeyFrame::UpdateBirdConnections and Map::UpdateLocalBirdMap      covis_bird.inc
//   MapPoint::Replace and the loop fusion of CorrectLoop             covis_fuse.inc
//   LocalMapping::SearchInNeighbors                                  covis_neighbors.inc
//
// State: one dense row of uint16 per key frame, W[a][b] = weight (bits 0..14, 0 = no entry) | member of the ordered vector
// (bit 15).  mvpOrderedConnectedKeyFrames is always "descending by (weight, kf_order)" over the members, so it is derived
// on read: one workgroup sorts (weight << 12 | rank of kf_order) keys of a row in LDS.  Everything is integer work and is
// compared bit for bit with tests/covis_ref.py.
#include "fb_common.h"
#include "fb_primitives.h"
#include "covis_plan.h"

#include <algorithm>

struct fb_covis;

namespace {

constexpr int CV_MAXK = FB_KFDB_MAX_KEYFRAMES;
constexpr uint32_t CV_W = 0x7fffu, CV_MEMBER = 0x8000u;
constexpr uint32_t KEY_NONE32 = 0xffffffffu;
static_assert(CV_MAXK <= 4096, "a rank is kept in 12 bits");
enum { LIST_ORDERED = 0, LIST_BY_WEIGHT = 1, LIST_CONNECTED = 2 };

struct Gr {             // device arrays of one handle
  int K;
  uint16_t *W;          // [K][K]
  int32_t *rank;        // [K] position of the slot in ascending (kf_order, slot)
  int32_t *inv;         // [K] the slot at that position
  int32_t *err;         // [1] entries skipped as out of range
  int32_t *parent;      // [K] mpParent, -1 = NULL                                  (the spanning tree: covis_tree.inc)
  uint8_t *linked;      // [K] the slot is in mspChildrens of parent[slot]
  uint8_t *first;       // [K] mbFirstConnection
};

template <typename T> __device__ __forceinline__ T ld(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> __device__ __forceinline__ void st(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the work of one workgroup becomes visible to its own later loads (serial kernels of one workgroup)
__device__ __forceinline__ void group_sync() { __threadfence(); __syncthreads(); }

// maximum of one unsigned per thread over the 1024-thread block (s_wv: [16]); every thread gets it
__device__ __forceinline__ uint32_t block_max_u32(uint32_t v, uint32_t *s_wv) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_wv[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t m = 0;
  for (int w = 0; w < CV_NT / 64; w++) m = max(m, s_wv[w]);
  return m;
}

// 1: live and in range, 0: erased, -1: out of range (never used as an index)
__device__ __forceinline__ int edge_state(const fb_covis_map &M, int e) {
  const int kf = M.obs_kf[e];
  if (kf < 0) return 0;
  const int mp = M.obs_mp[e], idx = M.obs_idx[e];
  if (kf >= M.max_keyframes || mp < 0 || mp >= M.n_mp || idx < 0 || idx >= M.kp_stride) return -1;
  return 1;
}

// ---- the edge list grouped by point: count -> scan -> scatter -------------------------------------------------------
__global__ __launch_bounds__(256) void k_cv_count(fb_covis_map M, int32_t *cnt, int32_t *err) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= M.n_obs) return;
  const int s = edge_state(M, e);
  if (s > 0) atomicAdd(&cnt[M.obs_mp[e]], 1);
  else if (s < 0) atomicAdd(err, 1);
}

// phase 0: bsum[block] = sum of the tile; phase 1: data[i] = bsum[block] + exclusive scan within the tile
__global__ __launch_bounds__(CV_NT) void k_cv_scan_tile(int32_t *data, int n, int32_t *bsum, int phase) {
  __shared__ int s_wv[CV_NT / 64];
  const int base = blockIdx.x * CV_SCAN_TILE + threadIdx.x * CV_SCAN_ITEMS;
  int v[CV_SCAN_ITEMS], sum = 0;
#pragma unroll
  for (int k = 0; k < CV_SCAN_ITEMS; k++) { v[k] = base + k < n ? data[base + k] : 0; sum += v[k]; }
  int total;
  int ex = fb::block_excl_scan<CV_NT>(sum, s_wv, &total);
  if (phase == 0) {
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
    return;
  }
  ex += bsum[blockIdx.x];
#pragma unroll
  for (int k = 0; k < CV_SCAN_ITEMS; k++) { if (base + k < n) data[base + k] = ex; ex += v[k]; }
}

// exclusive scan of the nb tile sums in place, by one workgroup
__global__ __launch_bounds__(CV_NT) void k_cv_scan_sums(int32_t *bsum, int nb) {
  __shared__ int s_wv[CV_NT / 64];
  int carry = 0;
  for (int base = 0; base < nb; base += CV_NT) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? bsum[i] : 0;
    int total;
    const int ex = fb::block_excl_scan<CV_NT>(v, s_wv, &total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_cv_scatter(fb_covis_map M, const int32_t *start, int32_t *fill, int32_t *csr) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= M.n_obs) return;
  if (edge_state(M, e) <= 0) return;
  const int mp = M.obs_mp[e];
  const int pos = start[mp] + atomicAdd(&fill[mp], 1);
  if (pos < M.n_obs) csr[pos] = e;   // (always true: the fills of a point add up to its count)
}

// ---- the std::map order of the slots -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cv_rank(Gr G, const uint64_t *order) {
  __shared__ uint64_t s_o[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const uint64_t mine = i < G.K ? order[i] : 0;
  int r = 0;
  for (int base = 0; base < G.K; base += 256) {
    __syncthreads();
    if (base + threadIdx.x < G.K) s_o[threadIdx.x] = order[base + threadIdx.x];
    __syncthreads();
    const int m = min(256, G.K - base);
    for (int j = 0; j < m; j++) {
      const uint64_t o = s_o[j];
      r += (o < mine || (o == mine && base + j < i)) ? 1 : 0;
    }
  }
  if (i < G.K) { G.rank[i] = r; G.inv[r] = i; }
}

__global__ __launch_bounds__(256) void k_cv_identity(Gr G) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < G.K) { G.rank[i] = i; G.inv[i] = i; }
}

__global__ __launch_bounds__(256) void k_cv_tree_reset(Gr G) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < G.K) { G.parent[i] = -1; G.linked[i] = 0; G.first[i] = 1; }
}

// ---- UpdateConnections -------------------------------------------------------------------------------------------------
// KFcounter of query q (KeyFrame.cc:580-598): one workgroup, the bins in LDS
// (d_n: the list's length on the device, NULL = every row of the launch is a query)
__global__ __launch_bounds__(CV_NT) void k_cv_counter(fb_covis_map M, Gr G, const int32_t *start, const int32_t *csr, const int32_t *slots,
                                                      uint16_t *counter, const int32_t *d_n) {
  __shared__ int s_bin[CV_MAXK];
  const int q = blockIdx.x, K = G.K, S = M.kp_stride;
  if (d_n && q >= *d_n) return;
  for (int b = threadIdx.x; b < K; b += CV_NT) s_bin[b] = 0;
  __syncthreads();
  const int a = slots[q];
  if (a >= 0 && a < K) {
    const int n = min(max(M.kf_n[a], 0), S);
    const int32_t *mps = M.kf_mp + (size_t)a * S;
    for (int i = threadIdx.x; i < n; i += CV_NT) {
      const int mp = mps[i];
      if (mp < 0) continue;
      if (mp >= M.n_mp) { atomicAdd(G.err, 1); continue; }
      if (M.mp_bad[mp]) continue;
      const int p1 = start[mp + 1];
      for (int p = start[mp]; p < p1; p++) {
        const int kf = M.obs_kf[csr[p]];   // in [0, K): the index holds checked edges only
        if (kf != a) atomicAdd(&s_bin[kf], 1);
      }
    }
  } else if (threadIdx.x == 0) {
    atomicAdd(G.err, 1);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < K; b += CV_NT) counter[(size_t)q * K + b] = (uint16_t)min(s_bin[b], (int)CV_W);
}

// key of an ordered-vector entry: larger = earlier
__device__ __forceinline__ uint32_t order_key(uint32_t w, int rank) { return (w << 12) | (uint32_t)rank; }

// What the LoopConnections variant of k_cv_apply adds (covis_loop.inc): the list's length is on the device, and at the turn
// of query q, before its row is replaced, bits[q] = "the row after the update has an entry" and not "member of the ordered
// vector before it" and not "in the list", with the row's size in rowcnt[q].
struct LoopConnOut {
  const int32_t *d_n;
  uint32_t *bits;       // [n_q][(K + 31) / 32], zero when the kernel starts
  int32_t *rowcnt;      // [n_q]
};

// the counters applied to the graph one query after the other (:604-663), by one workgroup
template <bool LC>
__global__ __launch_bounds__(CV_NT) void k_cv_apply(Gr G, int n_q, const int32_t *slots, const uint16_t *counter, int32_t *n_counter,
                                                    int32_t *front, LoopConnOut L) {
  __shared__ int s_wv[CV_NT / 64];
  __shared__ uint32_t s_mx[CV_NT / 64];
  const int tid = threadIdx.x, K = G.K, lane = tid & 63, wave = tid >> 6;
  [[maybe_unused]] uint32_t *s_set = nullptr;   // the members of the list as a bitset, and the words of a bit row:
  [[maybe_unused]] int nw = 0;                  // the LoopConnections instance only; the other one has neither
  if constexpr (LC) {
    __shared__ uint32_t s_members[CV_MAXK / 32];
    s_set = s_members;
    nw = (K + 31) / 32;
    n_q = min(max(*L.d_n, 0), n_q);
    for (int w = tid; w < nw; w += CV_NT) s_set[w] = 0;
    __syncthreads();
    for (int q = tid; q < n_q; q += CV_NT) {
      const int a = slots[q];
      if (a >= 0 && a < K) atomicOr(&s_set[a >> 5], 1u << (a & 31));
    }
    __syncthreads();
  }
  for (int q = 0; q < n_q; q++) {
    const int a = slots[q];
    if (a < 0 || a >= K) {
      if (tid == 0) { n_counter[q] = 0; front[q] = -1; if constexpr (LC) L.rowcnt[q] = 0; }
      continue;
    }
    const uint16_t *C = counter + (size_t)q * K;
    uint16_t *rowA = G.W + (size_t)a * K;
    int cnt = 0;
    uint32_t best15 = 0, bestAny = 0, cur = 0;
    for (int b = tid; b < K; b += CV_NT) {
      const uint32_t w = C[b];
      const int r = G.rank[b];
      if (w) { cnt++; bestAny = max(bestAny, order_key(w, 4095 - r)); }   // strict > in ascending kf_order: the smallest wins
      if (w >= FB_COVIS_TH) best15 = max(best15, order_key(w, r));
      const uint32_t v = rowA[b];
      if ((v & CV_MEMBER) && (v & CV_W)) cur = max(cur, order_key(v & CV_W, r));
    }
    cnt = fb::block_sum<CV_NT>(cnt, s_wv);
    best15 = block_max_u32(best15, s_mx);
    bestAny = block_max_u32(bestAny, s_mx);
    cur = block_max_u32(cur, s_mx);
    if constexpr (LC) {   // LoopClosing.cc:576-588 for this member; with an empty counter the row stays and is what is read
      int mine = 0;
      for (int base = wave * 64; base < nw * 32; base += CV_NT) {
        const int b = base + lane;
        bool bit = false;
        if (b < K) {
          const uint32_t v = rowA[b];
          const uint32_t w = cnt ? (uint32_t)C[b] : (v & CV_W);
          bit = w && !((v & CV_MEMBER) && (v & CV_W)) && !((s_set[b >> 5] >> (b & 31)) & 1u);
        }
        const unsigned long long m = __ballot(bit);
        if (lane == 0) {
          uint32_t *row = L.bits + (size_t)q * nw;
          row[base >> 5] = (uint32_t)m;
          if ((base >> 5) + 1 < nw) row[(base >> 5) + 1] = (uint32_t)(m >> 32);
          mine += __popcll(m);
        }
      }
      mine = fb::block_sum<CV_NT>(mine, s_wv);   // (its barriers also order the reads of rowA before the writes below)
      if (tid == 0) L.rowcnt[q] = mine;
    }
    if (cnt == 0) {   // "This should not happen": the graph stays as it is
      if (tid == 0) { n_counter[q] = 0; front[q] = cur ? G.inv[cur & 4095] : -1; }
      continue;
    }
    const bool has15 = best15 != 0;
    const int pmax = G.inv[4095 - (bestAny & 4095)];
    // AddConnection(a, w) on every member b: one wave per row b
    for (int b = wave; b < K; b += CV_NT / 64) {
      const uint32_t w = C[b];
      const bool member = has15 ? w >= FB_COVIS_TH : b == pmax;
      if (!member) continue;
      uint16_t *rowB = G.W + (size_t)b * K;
      if ((rowB[a] & CV_W) == w) continue;   // the weight is there already: the ordered vector of b is left alone
      for (int j = lane; j < K; j += 64) {
        const uint32_t v = j == a ? w : rowB[j];
        if (v & CV_W) rowB[j] = (uint16_t)(v | CV_MEMBER);
      }
    }
    // mConnectedKeyFrameWeights = KFcounter; the ordered vector = the members (a itself is never a member of its counter)
    for (int b = tid; b < K; b += CV_NT) {
      const uint32_t w = C[b];
      const bool member = has15 ? w >= FB_COVIS_TH : b == pmax;
      rowA[b] = (uint16_t)(w ? (w | (member ? CV_MEMBER : 0u)) : 0u);
    }
    if (tid == 0) { n_counter[q] = cnt; front[q] = has15 ? G.inv[best15 & 4095] : pmax; }
    group_sync();
  }
}

// slot->AddConnection(other, w) (w > 0) or slot->EraseConnection(other) (w == 0)
__global__ __launch_bounds__(CV_NT) void k_cv_set_connection(Gr G, int slot, int other, uint32_t w) {
  uint16_t *row = G.W + (size_t)slot * G.K;
  const uint32_t old = row[other] & CV_W;
  __syncthreads();
  if (old == w) return;   // the same weight / no such entry: nothing is re-sorted
  for (int j = threadIdx.x; j < G.K; j += CV_NT) {
    const uint32_t v = j == other ? w : row[j];
    if (j == other || (v & CV_W)) row[j] = (uint16_t)((v & CV_W) ? (v | CV_MEMBER) : 0u);
  }
}

// SetBadFlag, :797-798: b->EraseConnection(slot) for every b of the row; one wave per b
__global__ __launch_bounds__(256) void k_cv_erase_from_others(Gr G, int slot) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= G.K || b == slot) return;
  if (!(G.W[(size_t)slot * G.K + b] & CV_W)) return;
  uint16_t *row = G.W + (size_t)b * G.K;
  if (!(row[slot] & CV_W)) return;
  for (int j = lane; j < G.K; j += 64) {
    const uint32_t v = j == slot ? 0u : row[j];
    if (j == slot || (v & CV_W)) row[j] = (uint16_t)((v & CV_W) ? (v | CV_MEMBER) : 0u);
  }
}

// ---- reading a row ---------------------------------------------------------------------------------------------------
// s_key[0..n) = the row's entries of the mode in output order (ascending keys), n returned to every thread.
// LIST_CONNECTED: key = rank; otherwise key = ~order_key of a member.
__device__ __forceinline__ int row_sorted(const Gr &G, int slot, int mode, uint32_t *s_key, int *s_wv) {
  const int tid = threadIdx.x, K = G.K;
  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  const uint16_t *row = G.W + (size_t)slot * K;
  int cnt = 0;
  for (int i = tid; i < n2; i += CV_NT) {
    uint32_t key = KEY_NONE32;
    if (i < K) {
      const uint32_t v = row[i], w = v & CV_W;
      if (mode == LIST_CONNECTED) { if (w) { key = (uint32_t)G.rank[i]; cnt++; } }
      else if (w && (v & CV_MEMBER)) { key = ~order_key(w, G.rank[i]); cnt++; }
    }
    s_key[i] = key;
  }
  cnt = fb::block_sum<CV_NT>(cnt, s_wv);
  __syncthreads();
  fb::bitonic_sort(s_key, n2, tid, CV_NT);
  return cnt;
}

__global__ __launch_bounds__(CV_NT) void k_cv_list(Gr G, int slot, int mode, int wmin, int32_t *d_n, int32_t *d_slots, int32_t *d_weights) {
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x;
  int n = row_sorted(G, slot, mode, s_key, s_wv);
  if (mode == LIST_BY_WEIGHT) {
    int m = 0;
    for (int p = tid; p < n; p += CV_NT) m += (int)((~s_key[p]) >> 12) >= wmin ? 1 : 0;
    m = fb::block_sum<CV_NT>(m, s_wv);
    n = m == n ? 0 : m;   // upper_bound == end(): the reference returns an empty vector (:254-255)
  }
  for (int p = tid; p < n; p += CV_NT) {
    const uint32_t k = mode == LIST_CONNECTED ? s_key[p] : ~s_key[p];
    d_slots[p] = G.inv[k & 4095];
    if (d_weights && mode != LIST_CONNECTED) d_weights[p] = (int32_t)(k >> 12);
  }
  if (tid == 0) *d_n = n;
}

__global__ void k_cv_weight(Gr G, int slot, int other, int32_t *d_w) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *d_w = (int32_t)(G.W[(size_t)slot * G.K + other] & CV_W);
}

__global__ __launch_bounds__(CV_NT) void k_cv_rows(Gr G, const int32_t *slots, int32_t *covis) {
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  const int slot = slots ? slots[blockIdx.x] : (int)blockIdx.x;
  if (slot < 0 || slot >= G.K) {
    if (threadIdx.x == 0) atomicAdd(G.err, 1);
    return;
  }
  const int n = row_sorted(G, slot, LIST_ORDERED, s_key, s_wv);
  if (threadIdx.x < FB_KFDB_COVIS)
    covis[(size_t)slot * FB_KFDB_COVIS + threadIdx.x] = (int)threadIdx.x < n ? G.inv[(~s_key[threadIdx.x]) & 4095] : -1;
}

// ---- KeyFrameCulling ---------------------------------------------------------------------------------------------------
// One workgroup walks the list; the overlay of the SetBadFlag() effects: nobs[mp] = Observations(), dead[e] = the edge was
// erased, bad[mp] = isBad() (the caller's mp_bad_after, started as a copy of mp_bad).
__global__ __launch_bounds__(CV_NT) void k_cv_cull(Gr G, fb_covis_map M, const int32_t *start, const int32_t *csr, int32_t *nobs, int32_t *dead,
                                                   int cur_slot, int id0_slot, const uint8_t *not_erase, int32_t *d_n, int32_t *d_slots,
                                                   int32_t *d_nred, int32_t *d_nmps, uint8_t *d_culled, uint8_t *bad) {
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x, S = M.kp_stride;
  const int L = row_sorted(G, cur_slot, LIST_ORDERED, s_key, s_wv);
  int *s_list = reinterpret_cast<int *>(s_key);
  for (int p = tid; p < L; p += CV_NT) {
    const int kf = G.inv[(~s_key[p]) & 4095];
    s_list[p] = kf;
    d_slots[p] = kf; d_nred[p] = 0; d_nmps[p] = 0; d_culled[p] = 0;
  }
  if (tid == 0) *d_n = L;
  __syncthreads();
  for (int p = 0; p < L; p++) {
    const int kf = s_list[p];
    if (kf == id0_slot) continue;                                   // LocalMapping.cc:667
    const int N = min(max(M.kf_n[kf], 0), S);
    const int32_t *mps = M.kf_mp + (size_t)kf * S;
    const uint8_t *oct = M.kf_octave + (size_t)kf * S;
    int my_mps = 0, my_red = 0;
    for (int i = tid; i < N; i += CV_NT) {
      const int mp = mps[i];
      if (mp < 0) continue;
      if (mp >= M.n_mp) { atomicAdd(G.err, 1); continue; }
      if (ld(&bad[mp])) continue;
      my_mps++;
      if (ld(&nobs[mp]) > 3) {                                      // :689
        const int level = oct[i];
        int c = 0;
        const int p1 = start[mp + 1];
        for (int q = start[mp]; q < p1 && c < 3; q++) {
          const int e = csr[q];
          if (ld(&dead[e])) continue;
          const int kfi = M.obs_kf[e];
          if (kfi == kf) continue;
          if ((int)M.kf_octave[(size_t)kfi * S + M.obs_idx[e]] <= level + 1) c++;
        }
        if (c >= 3) my_red++;
      }
    }
    const int nMPs = fb::block_sum<CV_NT>(my_mps, s_wv);
    const int nRed = fb::block_sum<CV_NT>(my_red, s_wv);
    const bool cull = (double)nRed > 0.9 * (double)nMPs;            // :717, in double as written
    if (tid == 0) { d_nred[p] = nRed; d_nmps[p] = nMPs; d_culled[p] = cull ? 1 : 0; }
    if (!cull || (not_erase && not_erase[kf])) continue;            // KeyFrame.cc:790-794
    // KeyFrame.cc:800-802: EraseObservation(pKF) on every point the key frame holds, bad ones included
    for (int i = tid; i < N; i += CV_NT) {
      const int mp = mps[i];
      if (mp < 0 || mp >= M.n_mp) continue;
      const int p1 = start[mp + 1];
      for (int q = start[mp]; q < p1; q++) {
        const int e = csr[q];
        if (M.obs_kf[e] != kf) continue;
        if (atomicExch(&dead[e], 1) == 0) {                         // a point held at two features loses one observation
          if (atomicSub(&nobs[mp], 1) - 1 <= 2) st(&bad[mp], (uint8_t)1);   // MapPoint.cc:129-136
        }
        break;
      }
    }
    group_sync();
  }
}

struct Index {          // scratch of one call that takes a map
  int32_t *start, *fill, *csr, *bsum, *nobs, *dead;
  uint16_t *counter;
};

struct IndexAsk {       // what a call wants of fb_covis::acquire
  size_t n_q = 0;       // queries of an update_connections (the counter rows)
  bool culling = false; // nobs / dead are set up as the culling overlay
  bool ranks = true;    // the ranks of M.kf_order are computed (the window's bird side shares the front side's)
  bool reuse = false;   // the caller's reuse_index
  bool kept = true;     // the index is the one a later reuse_index reads
  size_t head = 0;      // where a new index goes (behind a window head or the window's front index)
  size_t tail = 0;      // bytes the call keeps behind the index
};

}  // namespace

struct fb_covis {
  int K = 0;
  void *block = nullptr;
  Gr G{};
  void *bird_block = nullptr;   // the bird lists (covis_bird.inc), allocated by the first bird call
  uint16_t *WB = nullptr;       // [K][K] mvpBirdConnectedKeyFrames in the format of W: weight | CV_MEMBER, members only
  void *loop_block = nullptr;   // the consistency groups of DetectLoop (covis_loop.inc), allocated by the first such call
  LoopGroupsOff loop_off{};
  int loop_cap = 0;             // groups a buffer holds; 0 = max_keyframes (fb_covis_reserve_loop_groups)
  int loop_cur = 0;             // the buffer the next fb_covis_detect_loop_dev reads as the previous groups
  uint8_t *scr = nullptr;
  ScratchState state{};   // what scr holds; written by the scratch_*() of covis_plan.h only
  int ensure() {
    FB_TRY(fb::check_device());
    if (block) return FB_OK;
    GraphOff o;
    const size_t total = plan_graph(K, &o);
    FB_HIP(hipMalloc(&block, total));
    uint8_t *b = static_cast<uint8_t *>(block);
    G.K = K; G.W = (uint16_t *)(b + o.W); G.rank = (int32_t *)(b + o.rank); G.inv = (int32_t *)(b + o.inv); G.err = (int32_t *)(b + o.err);
    G.parent = (int32_t *)(b + o.parent); G.linked = b + o.linked; G.first = b + o.first;
    FB_HIP(hipMemset(block, 0, total));
    k_cv_identity<<<(K + 255) / 256, 256>>>(G);
    k_cv_tree_reset<<<(K + 255) / 256, 256>>>(G);
    FB_HIP(hipGetLastError());
    FB_HIP(hipDeviceSynchronize());   // creation is rare; orders the default stream's work before every other stream
    return FB_OK;
  }
  int ensure_bird() {
    FB_TRY(ensure());
    if (bird_block) return FB_OK;
    BirdGraphOff o;
    const size_t total = plan_bird_graph(K, &o);
    FB_HIP(hipMalloc(&bird_block, total));
    WB = (uint16_t *)(static_cast<uint8_t *>(bird_block) + o.WB);
    FB_HIP(hipMemset(bird_block, 0, total));
    FB_HIP(hipDeviceSynchronize());   // as ensure(): rare, and ordered before every stream
    return FB_OK;
  }
  // scratch of a call that keeps nothing and builds no index: behind the recorded index, which a later reuse_index still finds
  int behind_index(size_t bytes, uint8_t **p) {
    const size_t at = scratch_behind_index(state);
    FB_TRY(need(at + bytes));
    scratch_build_begins(state, at, false);
    *p = scr + at;
    return FB_OK;
  }
  int need(size_t bytes) {
    if (bytes <= state.capacity) return FB_OK;
    if (scr) { FB_HIP(hipDeviceSynchronize()); FB_HIP(hipFree(scr)); scr = nullptr; scratch_clear(state); }
    FB_HIP(hipMalloc(reinterpret_cast<void **>(&scr), bytes));
    scratch_grown(state, bytes);
    return FB_OK;
  }
  int reserve(const CallPlan &c) {
    FB_TRY(ensure());
    return need(c.total);
  }
  // The index of M for one call, and where the call's tail begins.  Reused when the call asks for it and the state allows;
  // otherwise the scratch is sized once for the whole call (nothing later reallocates), the ranks of M.kf_order and the edge
  // list grouped by point are built at a.head, and the state learns of it once that is enqueued.
  int acquire(const fb_covis_map &M, const IndexAsk &a, Index *ix, uint8_t **tail, hipStream_t s) {
    IndexOff o;
    const size_t bytes = plan_index(M.n_mp, M.n_obs, a.n_q, K, &o);
    const IndexStep st = scratch_decide(state, a.reuse, M, a.head, bytes, a.tail);
    FB_ARG(!st.refused);
    if (!st.reuse) {
      FB_TRY(need(st.total));
      scratch_build_begins(state, st.index_at, a.kept);
    }
    uint8_t *b = scr + st.index_at;
    ix->start = (int32_t *)(b + o.start); ix->fill = (int32_t *)(b + o.fill); ix->nobs = (int32_t *)(b + o.nobs);
    ix->csr = (int32_t *)(b + o.csr); ix->dead = (int32_t *)(b + o.dead); ix->bsum = (int32_t *)(b + o.bsum);
    ix->counter = (uint16_t *)(b + o.counter);
    if (tail) *tail = scr + st.tail_at;
    if (st.reuse) return FB_OK;
    FB_TRY(index_build(M, a.culling, ix, s, a.ranks));
    scratch_build_done(state, st.index_at, st.tail_at, M, a.kept);
    return FB_OK;
  }
  int index_build(const fb_covis_map &M, bool culling, Index *ix, hipStream_t s, bool ranks) {
    const size_t n_mp = M.n_mp, n_obs = M.n_obs, nb = scan_tiles(n_mp);
    if (ranks) k_cv_rank<<<(K + 255) / 256, 256, 0, s>>>(G, M.kf_order);
    // start and fill are adjacent: one memset
    FB_HIP(hipMemsetAsync(ix->start, 0, (size_t)((uint8_t *)ix->nobs - (uint8_t *)ix->start), s));
    if (n_obs) k_cv_count<<<(unsigned)((n_obs + 255) / 256), 256, 0, s>>>(M, ix->start, G.err);
    if (culling) {
      if (n_mp) FB_HIP(hipMemcpyAsync(ix->nobs, ix->start, n_mp * 4, hipMemcpyDeviceToDevice, s));
      if (n_obs) FB_HIP(hipMemsetAsync(ix->dead, 0, n_obs * 4, s));
    }
    k_cv_scan_tile<<<(unsigned)nb, CV_NT, 0, s>>>(ix->start, (int)(n_mp + 1), ix->bsum, 0);
    k_cv_scan_sums<<<1, CV_NT, 0, s>>>(ix->bsum, (int)nb);
    k_cv_scan_tile<<<(unsigned)nb, CV_NT, 0, s>>>(ix->start, (int)(n_mp + 1), ix->bsum, 1);
    if (n_obs) k_cv_scatter<<<(unsigned)((n_obs + 255) / 256), 256, 0, s>>>(M, ix->start, ix->fill, ix->csr);
    FB_HIP(hipGetLastError());
    return FB_OK;
  }
};

namespace {

int check_map(const fb_covis *g, const fb_covis_map *M) {
  FB_ARG(M);
  FB_ARG(M->max_keyframes == g->K);
  FB_ARG(M->kp_stride >= 1 && M->kp_stride <= FB_COVIS_MAX_STRIDE);
  FB_ARG(M->n_mp >= 0 && M->n_mp < INT_MAX && M->n_obs >= 0);
  FB_ARG(M->kf_n && M->kf_mp && M->kf_octave && M->kf_order);
  FB_ARG(M->n_mp == 0 || M->mp_bad);
  FB_ARG(M->n_obs == 0 || (M->obs_mp && M->obs_kf && M->obs_idx));
  return FB_OK;
}

void stage_map(fb::Stager &st, fb_covis_map &M) {
  const size_t K = M.max_keyframes, S = M.kp_stride;
  st.in(M.kf_n, K * 4); st.in(M.kf_mp, K * S * 4); st.in(M.kf_octave, K * S); st.in(M.kf_order, K * 8);
  st.in(M.mp_bad, (size_t)M.n_mp); st.in(M.obs_mp, (size_t)M.n_obs * 4); st.in(M.obs_kf, (size_t)M.n_obs * 4);
  st.in(M.obs_idx, (size_t)M.n_obs * 4);
}

int list_dev(fb_covis *g, int32_t slot, int mode, int32_t w, int32_t *d_n, int32_t *d_slots, int32_t *d_weights, void *stream) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K);
  FB_ARG(d_n && d_slots);
  FB_TRY(g->ensure());
  k_cv_list<<<1, CV_NT, 0, fb::as_stream(stream)>>>(g->G, slot, mode, w, d_n, d_slots, d_weights);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int list_host(fb_covis *g, int32_t slot, int mode, int32_t w, int32_t *n, int32_t *slots, int32_t *weights) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K);
  FB_ARG(n && slots);
  FB_TRY(g->ensure());
  fb::Stager st;
  st.out(n, 4, false);
  st.out(slots, (size_t)g->K * 4, true);   // copy-in: entries past n keep the caller's contents
  st.out(weights, (size_t)g->K * 4, true);
  FB_TRY(st.commit(nullptr));
  FB_TRY(list_dev(g, slot, mode, w, n, slots, weights, nullptr));
  return st.fetch(nullptr);
}

}  // namespace

extern "C" {

int fb_covis_create(int32_t max_keyframes, fb_covis **out) {
  FB_ARG(out);
  FB_ARG(max_keyframes >= 1 && max_keyframes <= CV_MAXK);
  fb_covis *g = new fb_covis();
  g->K = max_keyframes;
  *out = g;
  return FB_OK;
}

int fb_covis_destroy(fb_covis *g) {
  if (!g) return FB_OK;
  if (g->block || g->scr || g->bird_block || g->loop_block) {
    (void)hipDeviceSynchronize();
    if (g->block) (void)hipFree(g->block);
    if (g->bird_block) (void)hipFree(g->bird_block);
    if (g->loop_block) (void)hipFree(g->loop_block);
    if (g->scr) (void)hipFree(g->scr);
    (void)hipGetLastError();
  }
  delete g;
  return FB_OK;
}

int fb_covis_clear(fb_covis *g, void *stream) {
  FB_ARG(g);
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  FB_HIP(hipMemsetAsync(g->G.W, 0, (size_t)g->K * g->K * 2, s));
  FB_HIP(hipMemsetAsync(g->G.err, 0, 4, s));
  if (g->WB) FB_HIP(hipMemsetAsync(g->WB, 0, (size_t)g->K * g->K * 2, s));
  if (g->loop_block) FB_HIP(hipMemsetAsync(static_cast<uint8_t *>(g->loop_block) + g->loop_off.ng, 0, 2 * 4, s));   // mvConsistentGroups.clear()
  k_cv_tree_reset<<<(g->K + 255) / 256, 256, 0, s>>>(g->G);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_reserve(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && n_q >= 0 && n_q <= g->K);
  return g->reserve(plan_map_call(g->K, n_mp, n_obs, n_q, 0));
}

int fb_covis_set_order_dev(fb_covis *g, const uint64_t *d_kf_order, void *stream) {
  FB_ARG(g && d_kf_order);
  FB_TRY(g->ensure());
  k_cv_rank<<<(g->K + 255) / 256, 256, 0, fb::as_stream(stream)>>>(g->G, d_kf_order);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_error_count(fb_covis *g, int32_t *count, void *stream) {
  FB_ARG(g && count);
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  FB_HIP(hipMemcpyAsync(count, g->G.err, 4, hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  return FB_OK;
}

int fb_covis_update_connections_dev(fb_covis *g, const fb_covis_map *M, int32_t n_q, const int32_t *d_slots, int32_t *d_n_counter,
                                    int32_t *d_front, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_ARG(n_q >= 0 && n_q <= g->K);
  FB_ARG(n_q == 0 || (d_slots && d_n_counter && d_front));
  FB_TRY(g->ensure());
  if (n_q == 0) return FB_OK;
  hipStream_t s = fb::as_stream(stream);
  Index ix;
  IndexAsk ask;
  ask.n_q = n_q;
  FB_TRY(g->acquire(*M, ask, &ix, nullptr, s));
  k_cv_counter<<<n_q, CV_NT, 0, s>>>(*M, g->G, ix.start, ix.csr, d_slots, ix.counter, nullptr);
  k_cv_apply<false><<<1, CV_NT, 0, s>>>(g->G, n_q, d_slots, ix.counter, d_n_counter, d_front, LoopConnOut{});
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_update_connections(fb_covis *g, const fb_covis_map *H, int32_t n_q, const int32_t *slots, int32_t *n_counter,
                                int32_t *front) {
  FB_ARG(g);
  FB_TRY(check_map(g, H));
  FB_ARG(n_q >= 0 && n_q <= g->K);
  FB_ARG(n_q == 0 || (slots && n_counter && front));
  FB_TRY(g->ensure());
  if (n_q == 0) return FB_OK;
  fb_covis_map M = *H;
  fb::Stager st;
  stage_map(st, M);
  st.in(slots, (size_t)n_q * 4);
  st.out(n_counter, (size_t)n_q * 4, false); st.out(front, (size_t)n_q * 4, false);
  FB_TRY(st.commit(nullptr));
  IndexDropGuard drop(g->state);   // the index is of staged arrays that go back to the pool: nothing to reuse
  FB_TRY(fb_covis_update_connections_dev(g, &M, n_q, slots, n_counter, front, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_add_connection_dev(fb_covis *g, int32_t slot, int32_t other, int32_t weight, void *stream) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K && other >= 0 && other < g->K && slot != other);
  FB_ARG(weight >= 1 && weight <= FB_COVIS_MAX_STRIDE);
  FB_TRY(g->ensure());
  k_cv_set_connection<<<1, CV_NT, 0, fb::as_stream(stream)>>>(g->G, slot, other, (uint32_t)weight);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_erase_connection_dev(fb_covis *g, int32_t slot, int32_t other, void *stream) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K && other >= 0 && other < g->K && slot != other);
  FB_TRY(g->ensure());
  k_cv_set_connection<<<1, CV_NT, 0, fb::as_stream(stream)>>>(g->G, slot, other, 0u);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_erase_keyframe_dev(fb_covis *g, int32_t slot, void *stream) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K);
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  k_cv_erase_from_others<<<(g->K + 3) / 4, 256, 0, s>>>(g->G, slot);
  FB_HIP(hipGetLastError());
  FB_HIP(hipMemsetAsync(g->G.W + (size_t)slot * g->K, 0, (size_t)g->K * 2, s));
  return FB_OK;
}

int fb_covis_ordered_dev(fb_covis *g, int32_t slot, int32_t *d_n, int32_t *d_slots, int32_t *d_weights, void *stream) {
  return list_dev(g, slot, LIST_ORDERED, 0, d_n, d_slots, d_weights, stream);
}
int fb_covis_ordered(fb_covis *g, int32_t slot, int32_t *n, int32_t *slots, int32_t *weights) {
  return list_host(g, slot, LIST_ORDERED, 0, n, slots, weights);
}
int fb_covis_by_weight_dev(fb_covis *g, int32_t slot, int32_t w, int32_t *d_n, int32_t *d_slots, void *stream) {
  return list_dev(g, slot, LIST_BY_WEIGHT, w, d_n, d_slots, nullptr, stream);
}
int fb_covis_by_weight(fb_covis *g, int32_t slot, int32_t w, int32_t *n, int32_t *slots) {
  return list_host(g, slot, LIST_BY_WEIGHT, w, n, slots, nullptr);
}
int fb_covis_connected_dev(fb_covis *g, int32_t slot, int32_t *d_n, int32_t *d_slots, void *stream) {
  return list_dev(g, slot, LIST_CONNECTED, 0, d_n, d_slots, nullptr, stream);
}
int fb_covis_connected(fb_covis *g, int32_t slot, int32_t *n, int32_t *slots) {
  return list_host(g, slot, LIST_CONNECTED, 0, n, slots, nullptr);
}

int fb_covis_weight_dev(fb_covis *g, int32_t slot, int32_t other, int32_t *d_weight, void *stream) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K && other >= 0 && other < g->K);
  FB_ARG(d_weight);
  FB_TRY(g->ensure());
  k_cv_weight<<<1, 64, 0, fb::as_stream(stream)>>>(g->G, slot, other, d_weight);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_weight(fb_covis *g, int32_t slot, int32_t other, int32_t *weight) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K && other >= 0 && other < g->K);
  FB_ARG(weight);
  FB_TRY(g->ensure());
  fb::Stager st;
  st.out(weight, 4, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_covis_weight_dev(g, slot, other, weight, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_kfdb_rows_dev(fb_covis *g, int32_t n, const int32_t *d_slots, int32_t *d_covis, void *stream) {
  FB_ARG(g);
  FB_ARG(d_covis);
  FB_ARG(!d_slots || (n >= 0 && n <= g->K));
  FB_TRY(g->ensure());
  const int rows = d_slots ? n : g->K;
  if (rows == 0) return FB_OK;
  k_cv_rows<<<rows, CV_NT, 0, fb::as_stream(stream)>>>(g->G, d_slots, d_covis);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_kfdb_rows(fb_covis *g, int32_t n, const int32_t *slots, int32_t *covis) {
  FB_ARG(g);
  FB_ARG(covis);
  FB_ARG(!slots || (n >= 0 && n <= g->K));
  FB_TRY(g->ensure());
  fb::Stager st;
  st.in(slots, (size_t)n * 4);
  st.out(covis, (size_t)g->K * FB_KFDB_COVIS * 4, slots != nullptr);   // listed rows only: the others keep the caller's contents
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_covis_kfdb_rows_dev(g, n, slots, covis, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_keyframe_culling_dev(fb_covis *g, const fb_covis_map *M, int32_t cur_slot, int32_t id0_slot, const uint8_t *d_not_erase,
                                  int32_t *d_n, int32_t *d_slots, int32_t *d_n_redundant, int32_t *d_n_mps, uint8_t *d_culled,
                                  uint8_t *d_mp_bad_after, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_ARG(cur_slot >= 0 && cur_slot < g->K && id0_slot >= -1 && id0_slot < g->K);
  FB_ARG(d_n && d_slots && d_n_redundant && d_n_mps && d_culled);
  FB_ARG(M->n_mp == 0 || d_mp_bad_after);
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  Index ix;
  IndexAsk ask;
  ask.culling = true;
  FB_TRY(g->acquire(*M, ask, &ix, nullptr, s));
  if (M->n_mp) FB_HIP(hipMemcpyAsync(d_mp_bad_after, M->mp_bad, (size_t)M->n_mp, hipMemcpyDeviceToDevice, s));
  k_cv_cull<<<1, CV_NT, 0, s>>>(g->G, *M, ix.start, ix.csr, ix.nobs, ix.dead, cur_slot, id0_slot, d_not_erase, d_n, d_slots,
                                d_n_redundant, d_n_mps, d_culled, d_mp_bad_after);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_keyframe_culling(fb_covis *g, const fb_covis_map *H, int32_t cur_slot, int32_t id0_slot, const uint8_t *not_erase,
                              int32_t *n, int32_t *slots, int32_t *n_redundant, int32_t *n_mps, uint8_t *culled,
                              uint8_t *mp_bad_after) {
  FB_ARG(g);
  FB_TRY(check_map(g, H));
  FB_ARG(cur_slot >= 0 && cur_slot < g->K && id0_slot >= -1 && id0_slot < g->K);
  FB_ARG(n && slots && n_redundant && n_mps && culled);
  FB_ARG(H->n_mp == 0 || mp_bad_after);
  FB_TRY(g->ensure());
  fb_covis_map M = *H;
  const size_t K = g->K;
  fb::Stager st;
  stage_map(st, M);
  st.in(not_erase, K);
  st.out(n, 4, false);
  st.out(slots, K * 4, true); st.out(n_redundant, K * 4, true); st.out(n_mps, K * 4, true); st.out(culled, K, true);
  st.out(mp_bad_after, (size_t)M.n_mp, false);
  FB_TRY(st.commit(nullptr));
  IndexDropGuard drop(g->state);
  FB_TRY(fb_covis_keyframe_culling_dev(g, &M, cur_slot, id0_slot, not_erase, n, slots, n_redundant, n_mps, culled, mp_bad_after,
                                       nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"

#include "covis_window.inc"
#include "covis_tree.inc"
#include "covis_points.inc"
#include "covis_fuse.inc"
#include "covis_correct.inc"
#include "covis_bird.inc"
#include "covis_loop.inc"
#include "covis_neighbors.inc"
