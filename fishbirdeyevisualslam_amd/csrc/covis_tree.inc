// covis_tree.inc -- the key frames' spanning tree and Tracking::UpdateLocalMap on the covisibility graph (included at the
// end of covis.hip, after covis_window.inc: it shares Gr, Index, row_sorted and the window's position-key kernels).
//
// Replaces (reference file:line):
//   KeyFrame::UpdateConnections, the mbFirstConnection block       src/KeyFrame.cc:665-690
//   AddChild / EraseChild / ChangeParent / GetChilds / GetParent    :704-741
//   KeyFrame::SetBadFlag, the tree part                             :810-868
//   Tracking::UpdateLocalMap = UpdateLocalKeyFrames + UpdateLocalPoints   src/Tracking.cc:2085-2229
//
// Tree state per slot: parent, linked (the slot is in mspChildrens of parent[slot]), first (mbFirstConnection).  A
// std::set<KeyFrame*> iterates in ascending kf_order, so "the first child that ..." is a minimum over ranks.  A key
// frame's ordered list is descending in order_key(weight, rank), so "the first member in list order that is a candidate"
// is the candidate member with the largest key: SetBadFlag needs no sorted list, only a maximum per child.
// Everything is integer work and is compared for equality with tests/local_map_ref.py.

namespace {

// LM_EXPAND, LM_NEIGH, LM_HDR: covis_plan.h.  A sequence's header holds the window's WH_* and the ones below.
enum { LH_GATED = WH_COUNT, LH_CARRY, LH_VOTERS, LH_KF_OVER };
constexpr uint32_t TREE_DONE = 0xffffffffu;
static_assert(LM_NEIGH <= 64 && LH_KF_OVER < LM_HDR, "one wave tests the neighbours; the header holds the flags");

__device__ __forceinline__ bool bit_test(const uint32_t *bm, int i) { return (bm[i >> 5] >> (i & 31)) & 1u; }
__device__ __forceinline__ void bit_set(uint32_t *bm, int i) { atomicOr(&bm[i >> 5], 1u << (i & 31)); }

// ---- the tree ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tree_set(Gr G, const int32_t *parent, const uint8_t *linked, const uint8_t *first) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= G.K) return;
  if (parent) {
    int p = parent[i];
    if (p < -1 || p >= G.K) { atomicAdd(G.err, 1); p = -1; }
    G.parent[i] = p;
  }
  if (linked) G.linked[i] = linked[i] ? 1 : 0;
  if (first) G.first[i] = first[i] ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_tree_get(Gr G, int32_t *parent, uint8_t *linked, uint8_t *first) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= G.K) return;
  if (parent) parent[i] = G.parent[i];
  if (linked) linked[i] = G.linked[i];
  if (first) first[i] = G.first[i];
}

// op 0: a->ChangeParent(b); op 1: a->EraseChild(b); op 2: *out = GetParent(a)
__global__ void k_tree_edit(Gr G, int op, int a, int b, int32_t *out) {
  if (threadIdx.x || blockIdx.x) return;
  if (op == 0) { G.parent[a] = b; G.linked[a] = 1; }
  else if (op == 1) { if (G.parent[b] == a) G.linked[b] = 0; }
  else *out = G.parent[a];
}

// s_key[0..n) = the ranks of GetChilds() of `slot`, ascending; n to every thread
__device__ __forceinline__ int children_sorted(const Gr &G, int slot, uint32_t *s_key, int *s_wv) {
  const int tid = threadIdx.x, K = G.K;
  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  int cnt = 0;
  for (int i = tid; i < n2; i += CV_NT) {
    uint32_t key = KEY_NONE32;
    if (i < K && i != slot && G.parent[i] == slot && G.linked[i]) { key = (uint32_t)G.rank[i]; cnt++; }
    s_key[i] = key;
  }
  cnt = fb::block_sum<CV_NT>(cnt, s_wv);
  __syncthreads();
  fb::bitonic_sort(s_key, n2, tid, CV_NT);
  return cnt;
}

__global__ __launch_bounds__(CV_NT) void k_tree_children(Gr G, int slot, int32_t *d_n, int32_t *d_slots) {
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  const int n = children_sorted(G, slot, s_key, s_wv);
  for (int p = threadIdx.x; p < n; p += CV_NT) d_slots[p] = G.inv[s_key[p]];
  if (threadIdx.x == 0) *d_n = n;
}

// The nearest-earlier search of KeyFrame.cc:673-684 (and of UpdateBirdConnections, :453-465, :535-547): the key frame of
// the map with the largest mnFrameId strictly between 0 and `mine`; -1 when nothing qualifies.  Every thread of the
// workgroup calls it and gets the answer.
__device__ __forceinline__ int nearest_earlier(const Gr &G, int mine, const int32_t *fid, const uint8_t *in_map, uint32_t *s_mx) {
  const int tid = threadIdx.x, K = G.K;
  uint32_t best = 0;
  for (int i = tid; i < K; i += CV_NT)
    if (in_map[i] && fid[i] > 0 && fid[i] < mine) best = max(best, (uint32_t)fid[i]);
  best = block_max_u32(best, s_mx);
  if (!best) return -1;
  uint32_t r = 0;                                                   // strict > in set order: the smallest kf_order among equal ids
  for (int i = tid; i < K; i += CV_NT)
    if (in_map[i] && (uint32_t)fid[i] == best) r = max(r, (uint32_t)(4096 - G.rank[i]));
  r = block_max_u32(r, s_mx);
  return G.inv[4096 - r];
}

// KeyFrame.cc:665-690 for the queries of one update_connections batch, one after the other, by one workgroup
__global__ __launch_bounds__(CV_NT) void k_tree_first(Gr G, int n_q, const int32_t *slots, const int32_t *n_counter, const int32_t *front,
                                                      int id0, int state4, const int32_t *fid, const uint8_t *in_map) {
  __shared__ uint32_t s_mx[CV_NT / 64];
  const int tid = threadIdx.x, K = G.K;
  for (int q = 0; q < n_q; q++) {
    const int a = slots[q];
    if (a < 0 || a >= K) continue;                                  // (update_connections gave it an empty answer)
    if (!ld(&G.first[a]) || a == id0 || n_counter[q] == 0) continue;   // :665; an empty counter returned at :604-612
    const int f = front[q];
    if (f < 0 || f >= K) {
      if (tid == 0) atomicAdd(G.err, 1);
      continue;
    }
    int t = f;
    if (state4 && fid[f] > fid[a]) {                                // :669-684
      const int near = nearest_earlier(G, fid[a], fid, in_map, s_mx);
      if (near >= 0) t = near;
    }
    if (tid == 0) { st(&G.parent[a], (int32_t)t); st(&G.linked[a], (uint8_t)1); st(&G.first[a], (uint8_t)0); }
    group_sync();
  }
}

// KeyFrame.cc:810-868 by one workgroup.  s_best[p] of the child at position p: the key of the first member of its ordered
// list that is a parent candidate (0 = none, TREE_DONE = re-parented).  A round adds one candidate, so one entry of each
// remaining child's row updates its key.
__global__ __launch_bounds__(CV_NT) void k_tree_erase(Gr G, int slot, const uint8_t *kf_bad) {
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ uint32_t s_best[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  __shared__ uint32_t s_mx[CV_NT / 64];
  const int tid = threadIdx.x, K = G.K;
  const int P = G.parent[slot];
  if (P < 0) {                                                      // the reference dereferences mpParent
    if (tid == 0) atomicAdd(G.err, 1);
    return;
  }
  const int n = children_sorted(G, slot, s_key, s_wv);
  for (int p = tid; p < n; p += CV_NT) {
    const int c = G.inv[s_key[p]];
    s_key[p] = (uint32_t)c;
    const uint32_t v = G.W[(size_t)c * K + P];
    s_best[p] = (!kf_bad[c] && (v & CV_MEMBER) && (v & CV_W)) ? order_key(v & CV_W, G.rank[P]) : 0u;
  }
  __syncthreads();
  for (;;) {
    uint32_t pick = 0;                                              // the largest weight; among equals the first child
    for (int p = tid; p < n; p += CV_NT) {
      const uint32_t k = s_best[p];
      if (k != 0u && k != TREE_DONE) pick = max(pick, ((k >> 12) << 12) | (uint32_t)(4095 - p));
    }
    pick = block_max_u32(pick, s_mx);
    if (!pick) break;
    const int ps = 4095 - (int)(pick & 4095);
    const int cs = (int)s_key[ps], pP = G.inv[s_best[ps] & 4095];
    __syncthreads();
    if (tid == 0) { G.parent[cs] = pP; G.linked[cs] = 1; }          // pC->ChangeParent(pP)
    for (int p = tid; p < n; p += CV_NT) {
      if (p == ps) { s_best[p] = TREE_DONE; continue; }
      if (s_best[p] == TREE_DONE) continue;
      const int c = (int)s_key[p];
      if (kf_bad[c]) continue;                                      // :827
      const uint32_t v = G.W[(size_t)c * K + cs];
      if ((v & CV_MEMBER) && (v & CV_W)) s_best[p] = max(s_best[p], order_key(v & CV_W, G.rank[cs]));
    }
    __syncthreads();
  }
  for (int p = tid; p < n; p += CV_NT)
    if (s_best[p] != TREE_DONE) { const int c = (int)s_key[p]; G.parent[c] = P; G.linked[c] = 1; }   // :862-866, bad children included
  if (tid == 0) G.linked[slot] = 0;                                 // mpParent->EraseChild(this); mpParent stays
}

// ---- Tracking::UpdateLocalMap ---------------------------------------------------------------------------------------------
struct LmS {            // the scratch of one call, behind the index
  int32_t *hdr;         // [batch][LM_HDR]
  int32_t *voters;      // [batch][LM_EXPAND] the voters when there are at most LM_EXPAND of them
  int32_t *rows;        // [batch][LM_EXPAND][LM_NEIGH] GetBestCovisibilityKeyFrames(10) of each such voter
  int32_t *wslot;       // [batch][list] the local key frames whose points are collected (in-range entries of what fitted)
  int32_t *rowcnt;      // [list]   } one sequence after the other
  int32_t *ptkey;       // [n_mp]   }
  int32_t *plist;       // [n_mp]   }
  int list;
};

void lm_map(uint8_t *b, const LmOff &o, LmS *S) {
  S->list = o.list;
  S->hdr = (int32_t *)(b + o.hdr); S->voters = (int32_t *)(b + o.voters); S->rows = (int32_t *)(b + o.rows); S->wslot = (int32_t *)(b + o.wslot);
  S->rowcnt = (int32_t *)(b + o.rowcnt); S->ptkey = (int32_t *)(b + o.ptkey); S->plist = (int32_t *)(b + o.plist);
}
__host__ __device__ constexpr size_t lm_ints(size_t n) { return ((n * 4 + 255) & ~(size_t)255) / 4; }   // a per-sequence stride
__host__ __device__ __forceinline__ int32_t *lm_hdr(const LmS &S, int b) { return S.hdr + b * lm_ints(LM_HDR); }
__host__ __device__ __forceinline__ int32_t *lm_voters(const LmS &S, int b) { return S.voters + b * lm_ints(LM_EXPAND); }
__host__ __device__ __forceinline__ int32_t *lm_rows(const LmS &S, int b) { return S.rows + b * lm_ints(LM_EXPAND * LM_NEIGH); }
__host__ __device__ __forceinline__ int32_t *lm_wslot(const LmS &S, int b) { return S.wslot + b * lm_ints(S.list); }

// the votes (:2125-2141), the voters in std::map order and pKFmax (:2153-2168); or, with an empty counter, the list that
// came in (:2143-2144).  One workgroup per sequence, the bins in LDS.
__global__ __launch_bounds__(CV_NT) void k_lm_vote(fb_covis_map M, Gr G, const int32_t *start, const int32_t *csr, fb_local_map_args A, LmS S) {
  __shared__ int s_bin[CV_MAXK];
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  __shared__ uint32_t s_mx[CV_NT / 64];
  const int b = blockIdx.x, tid = threadIdx.x, K = G.K;
  int32_t *hdr = lm_hdr(S, b), *wslot = lm_wslot(S, b);
  if (tid < LM_HDR) hdr[tid] = 0;
  if (A.d_gate_row && A.d_gate_row[b] < A.gate_min) {               // if (bOK) bOK = TrackLocalMap(): nothing of this sequence is touched
    __syncthreads();
    if (tid == 0) hdr[LH_GATED] = 1;
    return;
  }
  for (int i = tid; i < K; i += CV_NT) s_bin[i] = 0;
  __syncthreads();
  const int n = min(max(A.d_n[b], 0), A.kp_stride);
  int32_t *mps = A.d_map_point + (size_t)b * A.kp_stride;
  for (int i = tid; i < n; i += CV_NT) {
    const int mp = mps[i];
    if (mp < 0) continue;
    if (mp >= M.n_mp) { atomicAdd(G.err, 1); continue; }
    if (M.mp_bad[mp]) { mps[i] = -1; continue; }                    // :2138
    const int p1 = start[mp + 1];
    for (int p = start[mp]; p < p1; p++) atomicAdd(&s_bin[M.obs_kf[csr[p]]], 1);   // in [0, K): the index holds checked edges only
  }
  __syncthreads();
  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  int any = 0, cnt = 0;
  uint32_t best = 0;
  for (int i = tid; i < n2; i += CV_NT) {
    uint32_t key = KEY_NONE32;
    if (i < K && s_bin[i] > 0) {
      any++;
      if (!A.d_kf_bad[i]) {                                         // :2157
        const int r = G.rank[i];
        key = (uint32_t)r; cnt++;
        best = max(best, order_key((uint32_t)s_bin[i], 4095 - r));  // strict > in ascending kf_order: the smallest among the maxima
      }
    }
    s_key[i] = key;
  }
  any = fb::block_sum<CV_NT>(any, s_wv);
  const int V = fb::block_sum<CV_NT>(cnt, s_wv);
  best = block_max_u32(best, s_mx);
  __syncthreads();
  fb::bitonic_sort(s_key, n2, tid, CV_NT);
  const int cap = min(A.cap_kf, S.list);
  if (tid == 0) A.d_n_voters[b] = any;
  if (any == 0) {                                                   // the list, its length and mpReferenceKF stay; its points are collected
    const int n_in = min(max(A.d_n_local_kf[b], 0), cap);
    const int32_t *in = A.d_local_kf + (size_t)b * A.cap_kf;
    int carry = 0;
    for (int base = 0; base < n_in; base += CV_NT) {
      const int p = base + tid;
      const int kf = p < n_in ? in[p] : -1;
      const bool ok = kf >= 0 && kf < K;
      if (p < n_in && !ok) atomicAdd(G.err, 1);
      int total;
      const int ex = fb::block_excl_scan<CV_NT>(ok ? 1 : 0, s_wv, &total);
      if (ok) wslot[carry + ex] = kf;
      carry += total;
      __syncthreads();
    }
    if (tid == 0) { hdr[LH_CARRY] = 1; hdr[WH_LOCAL] = carry; }
    return;
  }
  int32_t *out = A.d_local_kf + (size_t)b * A.cap_kf, *voters = lm_voters(S, b);
  for (int p = tid; p < V; p += CV_NT) {
    const int kf = G.inv[s_key[p]];
    if (p < cap) { out[p] = kf; wslot[p] = kf; }
    if (V <= LM_EXPAND) voters[p] = kf;
  }
  if (tid == 0) {
    hdr[LH_VOTERS] = V;
    if (V > 0) A.d_ref_kf[b] = G.inv[4095 - (best & 4095)];         // :2224-2228
  }
}

// GetBestCovisibilityKeyFrames(10) of every voter the expansion will visit: one workgroup per (sequence, voter)
__global__ __launch_bounds__(CV_NT) void k_lm_rows(Gr G, LmS S) {
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  const int b = blockIdx.x / LM_EXPAND, p = blockIdx.x % LM_EXPAND;
  const int32_t *hdr = lm_hdr(S, b);
  const int V = hdr[LH_VOTERS];
  if (hdr[LH_GATED] || hdr[LH_CARRY] || V > LM_EXPAND || p >= V) return;
  const int n = row_sorted(G, lm_voters(S, b)[p], LIST_ORDERED, s_key, s_wv);
  if (threadIdx.x < LM_NEIGH)
    lm_rows(S, b)[p * LM_NEIGH + threadIdx.x] = (int)threadIdx.x < n ? G.inv[(~s_key[threadIdx.x]) & 4095] : -1;
}

// the expansion (:2172-2222): serial over the voters, one workgroup per sequence, the marks (mnTrackReferenceForFrame) in LDS
__global__ __launch_bounds__(CV_NT) void k_lm_expand(Gr G, fb_local_map_args A, LmS S) {
  __shared__ uint32_t s_mark[CV_MAXK / 32];
  __shared__ uint32_t s_mx[CV_NT / 64];
  __shared__ int s_pick;
  const int b = blockIdx.x, tid = threadIdx.x, K = G.K;
  int32_t *hdr = lm_hdr(S, b), *wslot = lm_wslot(S, b);
  if (hdr[LH_GATED] || hdr[LH_CARRY]) return;
  const int V = hdr[LH_VOTERS], cap = min(A.cap_kf, S.list);
  int32_t *out = A.d_local_kf + (size_t)b * A.cap_kf;
  const int32_t *voters = lm_voters(S, b), *rows = lm_rows(S, b);
  int size = V;
  auto push = [&](int kf) {                                         // every thread keeps the size; one writes
    if (tid == 0) {
      if (size < cap) { out[size] = kf; wslot[size] = kf; }
      bit_set(s_mark, kf);
    }
    size++;
    __syncthreads();
  };
  if (V <= LM_EXPAND) {                                             // (more voters than that: the loop ends at its first test)
    if (tid < CV_MAXK / 32) s_mark[tid] = 0;
    __syncthreads();
    if (tid < V) bit_set(s_mark, voters[tid]);
    __syncthreads();
    for (int it = 0; it < V; it++) {
      if (size > LM_EXPAND) break;                                  // :2175
      const int kf = voters[it];
      if (tid < 64) {                                               // (a) the first good neighbour of the ten, :2180-2194
        const int c = tid < LM_NEIGH ? rows[it * LM_NEIGH + tid] : -1;
        const bool ok = c >= 0 && !A.d_kf_bad[c] && !bit_test(s_mark, c);
        const unsigned long long m = __ballot(ok);
        const int firstc = __shfl(c, m ? __ffsll((long long)m) - 1 : 0, 64);
        if (tid == 0) s_pick = m ? firstc : -1;
      }
      __syncthreads();
      const int nb = s_pick;
      __syncthreads();
      if (nb >= 0) push(nb);
      uint32_t r = 0;                                               // (b) the first good child in set order, :2196-2209
      for (int i = tid; i < K; i += CV_NT)
        if (G.parent[i] == kf && i != kf && G.linked[i] && !A.d_kf_bad[i] && !bit_test(s_mark, i)) r = max(r, (uint32_t)(4096 - G.rank[i]));
      r = block_max_u32(r, s_mx);
      if (r) push(G.inv[4096 - r]);
      const int par = G.parent[kf];                                 // (c) the parent, no isBad test; the break leaves the outer loop
      if (par >= 0 && !bit_test(s_mark, par)) { push(par); break; }
    }
  }
  if (tid == 0) {
    A.d_n_local_kf[b] = size;
    hdr[WH_LOCAL] = min(size, cap);
    hdr[LH_KF_OVER] = size > A.cap_kf ? 1 : 0;
  }
}

__global__ void k_lm_finish(fb_local_map_args A, LmS S) {
  for (int b = threadIdx.x; b < A.batch; b += blockDim.x) {
    const int32_t *hdr = lm_hdr(S, b);
    if (hdr[LH_GATED]) continue;
    A.d_n_local_mp[b] = hdr[WH_MP];
    A.d_overflow[b] = (hdr[LH_KF_OVER] || hdr[WH_MP] > A.cap_mp) ? 1 : 0;
  }
}

int check_local_map(const fb_local_map_args *a) {
  FB_ARG(a);
  FB_ARG(a->batch >= 1 && a->batch <= 65535 / LM_EXPAND && a->kp_stride >= 1 && a->kp_stride <= (1 << 19));
  FB_ARG(a->d_n && a->d_map_point && a->d_kf_bad);
  FB_ARG(a->cap_kf >= 0 && a->cap_mp >= 0 && (a->cap_kf == 0 || a->d_local_kf) && (a->cap_mp == 0 || a->d_local_mp));
  FB_ARG(a->d_n_local_kf && a->d_n_local_mp && a->d_ref_kf && a->d_n_voters && a->d_overflow);
  FB_ARG(a->reuse_index == 0 || a->reuse_index == 1);
  return FB_OK;
}

int tree_slot(fb_covis *g, int32_t slot) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K);
  return g->ensure();
}

}  // namespace

extern "C" {

int fb_covis_tree_set_dev(fb_covis *g, const int32_t *d_parent, const uint8_t *d_linked, const uint8_t *d_first, void *stream) {
  FB_ARG(g);
  FB_TRY(g->ensure());
  k_tree_set<<<(g->K + 255) / 256, 256, 0, fb::as_stream(stream)>>>(g->G, d_parent, d_linked, d_first);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_tree_get_dev(fb_covis *g, int32_t *d_parent, uint8_t *d_linked, uint8_t *d_first, void *stream) {
  FB_ARG(g);
  FB_TRY(g->ensure());
  k_tree_get<<<(g->K + 255) / 256, 256, 0, fb::as_stream(stream)>>>(g->G, d_parent, d_linked, d_first);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_tree_get(fb_covis *g, int32_t *parent, uint8_t *linked, uint8_t *first) {
  FB_ARG(g);
  FB_TRY(g->ensure());
  fb::Stager st;
  st.out(parent, (size_t)g->K * 4, false); st.out(linked, (size_t)g->K, false); st.out(first, (size_t)g->K, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_covis_tree_get_dev(g, parent, linked, first, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_change_parent_dev(fb_covis *g, int32_t slot, int32_t parent, void *stream) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K && parent >= 0 && parent < g->K && slot != parent);
  FB_TRY(g->ensure());
  k_tree_edit<<<1, 64, 0, fb::as_stream(stream)>>>(g->G, 0, slot, parent, nullptr);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_erase_child_dev(fb_covis *g, int32_t parent, int32_t slot, void *stream) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K && parent >= 0 && parent < g->K);
  FB_TRY(g->ensure());
  k_tree_edit<<<1, 64, 0, fb::as_stream(stream)>>>(g->G, 1, parent, slot, nullptr);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_children_dev(fb_covis *g, int32_t slot, int32_t *d_n, int32_t *d_slots, void *stream) {
  FB_TRY(tree_slot(g, slot));
  FB_ARG(d_n && d_slots);
  k_tree_children<<<1, CV_NT, 0, fb::as_stream(stream)>>>(g->G, slot, d_n, d_slots);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_children(fb_covis *g, int32_t slot, int32_t *n, int32_t *slots) {
  FB_TRY(tree_slot(g, slot));
  FB_ARG(n && slots);
  fb::Stager st;
  st.out(n, 4, false);
  st.out(slots, (size_t)g->K * 4, true);   // copy-in: entries past n keep the caller's contents
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_covis_children_dev(g, slot, n, slots, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_parent_dev(fb_covis *g, int32_t slot, int32_t *d_parent, void *stream) {
  FB_TRY(tree_slot(g, slot));
  FB_ARG(d_parent);
  k_tree_edit<<<1, 64, 0, fb::as_stream(stream)>>>(g->G, 2, slot, 0, d_parent);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_first_connection_dev(fb_covis *g, int32_t n_q, const int32_t *d_slots, const int32_t *d_n_counter, const int32_t *d_front,
                                  int32_t id0_slot, int32_t now_state4, const int32_t *d_kf_frame_id, const uint8_t *d_kf_in_map,
                                  void *stream) {
  FB_ARG(g);
  FB_ARG(n_q >= 0 && n_q <= g->K && id0_slot >= -1 && id0_slot < g->K);
  FB_ARG(n_q == 0 || (d_slots && d_n_counter && d_front));
  FB_ARG(!now_state4 || (d_kf_frame_id && d_kf_in_map));
  FB_TRY(g->ensure());
  if (n_q == 0) return FB_OK;
  k_tree_first<<<1, CV_NT, 0, fb::as_stream(stream)>>>(g->G, n_q, d_slots, d_n_counter, d_front, id0_slot, now_state4 ? 1 : 0, d_kf_frame_id,
                                                       d_kf_in_map);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_tree_erase_keyframe_dev(fb_covis *g, int32_t slot, const uint8_t *d_kf_bad, void *stream) {
  FB_TRY(tree_slot(g, slot));
  FB_ARG(d_kf_bad);
  k_tree_erase<<<1, CV_NT, 0, fb::as_stream(stream)>>>(g->G, slot, d_kf_bad);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_reserve_local_map(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t batch, int32_t with_window) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && n_q >= 0 && n_q <= g->K && batch >= 1);
  return g->reserve(plan_local_map_call(g->K, n_mp, n_obs, n_q, batch, with_window != 0));
}

int fb_covis_local_map_dev(fb_covis *g, const fb_covis_map *M, const fb_local_map_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_local_map(a));
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  const size_t n_mp = M->n_mp;
  LmOff lo;
  IndexAsk ask;
  ask.reuse = a->reuse_index != 0; ask.tail = plan_local_map(a->batch, g->K, n_mp, &lo);
  Index ix;
  uint8_t *tail;
  FB_TRY(g->acquire(*M, ask, &ix, &tail, s));
  LmS S;
  lm_map(tail, lo, &S);
  fb_local_map_args A = *a;
  k_lm_vote<<<A.batch, CV_NT, 0, s>>>(*M, g->G, ix.start, ix.csr, A, S);
  k_lm_rows<<<A.batch * LM_EXPAND, CV_NT, 0, s>>>(g->G, S);
  k_lm_expand<<<A.batch, CV_NT, 0, s>>>(g->G, A, S);
  for (int b = 0; b < A.batch; b++) {                               // UpdateLocalPoints: the window's position keys, a sequence at a time
    WinS W;
    memset(&W, 0, sizeof(W));
    W.hdr = lm_hdr(S, b); W.wslot = lm_wslot(S, b); W.rowcnt = S.rowcnt; W.side[0].ptkey = S.ptkey; W.side[0].plist = S.plist;
    WinOut O;
    memset(&O, 0, sizeof(O));
    O.cap_pt = A.cap_mp; O.pt_index = A.d_local_mp + (size_t)b * A.cap_mp;
    if (n_mp) {
      FB_HIP(hipMemsetAsync(S.ptkey, 0x7f, n_mp * 4, s));
      k_win_mark<<<(unsigned)S.list, WIN_NT, 0, s>>>(*M, W, 0, g->G.err);
      k_win_rowcount<<<(unsigned)S.list, WIN_NT, 0, s>>>(*M, W, 0);
      k_win_rowscan<<<1, CV_NT, 0, s>>>(W, 0);
      k_win_place<<<(unsigned)S.list, WIN_NT, 0, s>>>(*M, W, 0, nullptr, O);
    }
  }
  k_lm_finish<<<1, 64, 0, s>>>(A, S);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_local_map(fb_covis *g, const fb_covis_map *HM, const fb_local_map_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_TRY(check_local_map(ha));
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_local_map_args A = *ha;
  const size_t B = A.batch, K = g->K;
  fb::Stager st;
  stage_map(st, M);
  st.in(A.d_n, B * 4); st.in(A.d_kf_bad, K); st.in(A.d_gate_row, B * 4);
  // copy-in: what a gated sequence, an empty counter or a capacity leaves alone keeps the caller's contents
  st.out(A.d_map_point, B * (size_t)A.kp_stride * 4, true);
  st.out(A.d_local_kf, B * (size_t)A.cap_kf * 4, true); st.out(A.d_n_local_kf, B * 4, true);
  st.out(A.d_local_mp, B * (size_t)A.cap_mp * 4, true); st.out(A.d_n_local_mp, B * 4, true);
  st.out(A.d_ref_kf, B * 4, true); st.out(A.d_n_voters, B * 4, true); st.out(A.d_overflow, B * 4, true);
  FB_TRY(st.commit(nullptr));
  A.reuse_index = 0;   // the staged arrays are new device arrays every call
  IndexDropGuard drop(g->state);
  FB_TRY(fb_covis_local_map_dev(g, &M, &A, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
