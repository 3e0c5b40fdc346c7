// covis_bird.inc -- the bird side of the key-frame graph and the local bird map (included at the end of covis.hip: it
// shares Gr, Index, the edge index kernels, k_cv_list, nearest_earlier and win_bird_map).
//
// Replaces (reference file:line):
//   KeyFrame::UpdateBirdConnections                                 src/KeyFrame.cc:418-562
//   KeyFrame::GetBirdConnectedBirdKeyFrames (and the bird weights)   the getter of mvpBirdConnectedKeyFrames
//   Map::AddKeyFrame, the bird block, and Map::UpdateLocalBirdMap   src/Map.cc:41-46, :97-153
//
// The bird list of key frame a is row a of WB, in the format of W (weight | CV_MEMBER; only members are stored), so the
// ordered list is derived on read by k_cv_list like the front one.  UpdateBirdConnections writes no other key frame's row
// and reads the tree state of its own slot only: the queries of a batch are independent, one workgroup each, and there is
// no serial apply stage.  Everything is integer work except the 5 m test of the local bird map, and is compared for
// equality with tests/bird_map_ref.py.

namespace {

constexpr int LB_NT = 256;
constexpr int LB_NONE = 0x7f7f7f7f;   // pos[] of a point no near member holds (a memset of 0x7f)
enum { LBH_L = 0, LBH_MARKED = 1 };   // header ints: the list's length after the push_front, the number of local points

// ---- UpdateBirdConnections -------------------------------------------------------------------------------------------------
// B: the bird side as a fb_covis_map (win_bird_map).  One workgroup per query, KFcounter in LDS (:424-445).
__global__ __launch_bounds__(CV_NT) void k_bd_update(fb_covis_map B, Gr G, uint16_t *WB, const int32_t *start, const int32_t *csr,
                                                     const int32_t *slots, const int32_t *n_counter, int now_state, int id0,
                                                     const int32_t *fid, const uint8_t *in_map, int32_t *n_bird_counter,
                                                     int32_t *bird_front) {
  __shared__ int s_bin[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  __shared__ uint32_t s_mx[CV_NT / 64];
  __shared__ int s_tree[2];
  const int q = blockIdx.x, tid = threadIdx.x, K = G.K, S = B.kp_stride;
  const int a = slots[q];
  if (a < 0 || a >= K) {
    if (tid == 0) { atomicAdd(G.err, 1); n_bird_counter[q] = 0; bird_front[q] = -1; }
    return;
  }
  uint16_t *rowA = WB + (size_t)a * K;
  const bool acts = (n_counter ? n_counter[q] != 0 : true) || now_state >= 3;   // :701, :608-609
  for (int b = tid; b < K; b += CV_NT) s_bin[b] = 0;
  __syncthreads();
  if (acts) {
    const int n = min(max(B.kf_n[a], 0), S);
    const int32_t *mps = B.kf_mp + (size_t)a * S;
    for (int i = tid; i < n; i += CV_NT) {                            // a point held at two features is walked twice
      const int mp = mps[i];
      if (mp < 0) continue;
      if (mp >= B.n_mp) { atomicAdd(G.err, 1); continue; }
      if (B.mp_bad[mp]) continue;
      const int p1 = start[mp + 1];
      for (int p = start[mp]; p < p1; p++) {
        const int kf = B.obs_kf[csr[p]];   // in [0, K): the index holds checked edges only
        if (kf != a) atomicAdd(&s_bin[kf], 1);
      }
    }
  }
  __syncthreads();
  int cnt = 0;
  uint32_t best = 0, cur = 0;
  for (int b = tid; b < K; b += CV_NT) {
    const uint32_t w = (uint32_t)min(s_bin[b], (int)CV_W);
    const int r = G.rank[b];
    if (w) cnt++;
    if (w >= FB_COVIS_BIRD_TH) best = max(best, order_key(w, r));
    const uint32_t v = rowA[b];
    if ((v & CV_MEMBER) && (v & CV_W)) cur = max(cur, order_key(v & CV_W, r));
  }
  cnt = fb::block_sum<CV_NT>(cnt, s_wv);
  best = block_max_u32(best, s_mx);
  cur = block_max_u32(cur, s_mx);
  if (tid == 0) { s_tree[0] = ld(&G.parent[a]); s_tree[1] = ld(&G.first[a]); }   // one read: the branches below hold barriers
  __syncthreads();
  const int parent = s_tree[0];
  const bool first = s_tree[1] != 0;
  bool search = false;
  int new_parent = -1;
  if (cnt == 0) {                                                     // :447-480 (and a query that does not act): the list stays
    if (tid == 0) { n_bird_counter[q] = 0; bird_front[q] = cur ? G.inv[cur & 4095] : -1; }
    search = acts && now_state >= 3 && parent == -1;
  } else {
    for (int b = tid; b < K; b += CV_NT) {                            // :483-512: the members replace the list, also when there are none
      const uint32_t w = (uint32_t)min(s_bin[b], (int)CV_W);
      rowA[b] = (uint16_t)(w >= FB_COVIS_BIRD_TH ? (w | CV_MEMBER) : 0u);
    }
    if (tid == 0) { n_bird_counter[q] = cnt; bird_front[q] = best ? G.inv[best & 4095] : -1; }
    if ((parent == -1 || first) && a != id0) {                        // :514-517
      if (best) new_parent = G.inv[best & 4095];                      // :519-529
      else search = now_state >= 3;                                   // :533-557
    }
  }
  if (search) {                                                       // (uniform over the workgroup)
    new_parent = nearest_earlier(G, fid[a], fid, in_map, s_mx);
    if (new_parent < 0 && tid == 0) atomicAdd(G.err, 1);              // the reference dereferences an uninitialised pointer
  }
  if (new_parent >= 0 && tid == 0) { st(&G.parent[a], (int32_t)new_parent); st(&G.linked[a], (uint8_t)1); st(&G.first[a], (uint8_t)0); }
}

// ---- Map::AddKeyFrame + UpdateLocalBirdMap -----------------------------------------------------------------------------------
struct LbS {            // the scratch of one call
  int32_t *hdr;         // [64]
  int32_t *wlist;       // [K + 1] localKFbird after the push_front
  uint8_t *wnear;       // [K + 1] !(dis > 5)
  int32_t *cnt;         // [K + 1] pMP_sum
  int32_t *pos;         // [n_mpb] the first holder's position, LB_NONE = none
  int32_t *eoff;        // [n_mpb + 1] 1 = a local point, then its exclusive scan
  int32_t *plist;       // [n_mpb] the local points in ascending index
  int32_t *bsum;
};

void lb_map(uint8_t *b, const LbOff &o, LbS *S) {
  S->hdr = (int32_t *)(b + o.hdr); S->wlist = (int32_t *)(b + o.wlist); S->wnear = b + o.wnear; S->cnt = (int32_t *)(b + o.cnt);
  S->pos = (int32_t *)(b + o.pos); S->eoff = (int32_t *)(b + o.eoff); S->plist = (int32_t *)(b + o.plist); S->bsum = (int32_t *)(b + o.bsum);
}

__device__ __forceinline__ void lb_centre(const fb_covis_kf_tables &T, const float *kf_ow, int slot, float ow[3]) {
  if (kf_ow) { ow[0] = kf_ow[(size_t)slot * 3]; ow[1] = kf_ow[(size_t)slot * 3 + 1]; ow[2] = kf_ow[(size_t)slot * 3 + 2]; }
  else fb::camera_centre(T.kf_Tcw + (size_t)slot * 12, ow);
}

// the list after the push_front (Map.cc:43) and the distance test of every member (:103-106)
__global__ __launch_bounds__(LB_NT) void k_lb_near(Gr G, fb_covis_kf_tables T, fb_local_bird_map_args A, LbS S) {
  const int j = blockIdx.x * LB_NT + threadIdx.x, K = G.K;
  const int n_in = min(max(*A.d_n_local_kf_bird, 0), min(A.cap_kf, K));
  const int L = n_in + 1;
  if (j == 0) { S.hdr[LBH_L] = L; S.hdr[LBH_MARKED] = 0; }
  if (j >= L) return;
  const int slot = j == 0 ? A.new_slot : A.d_local_kf_bird[j - 1];
  S.wlist[j] = slot;
  S.cnt[j] = 0;
  if (slot < 0 || slot >= K) { atomicAdd(G.err, 1); S.wnear[j] = 0; return; }   // never used as an index; it leaves the list
  float cur[3], ref[3];
  lb_centre(T, A.d_kf_ow, A.new_slot, cur);
  lb_centre(T, A.d_kf_ow, slot, ref);
  // cv::norm(refTw - curTw, NORM_L2) of a CV_32F Mat: the difference in float, the squares summed in double
  const double d0 = (double)(float)(ref[0] - cur[0]), d1 = (double)(float)(ref[1] - cur[1]), d2 = (double)(float)(ref[2] - cur[2]);
  const double dis = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  S.wnear[j] = !(dis > 5.0) ? 1 : 0;
}

// the first holder of every point: the smallest position among the near members that hold it (:112-125); one block per member
__global__ __launch_bounds__(LB_NT) void k_lb_first(Gr G, fb_covis_kf_tables T, LbS S) {
  const int j = blockIdx.x;
  if (j >= S.hdr[LBH_L] || !S.wnear[j]) return;
  const int slot = S.wlist[j], BS = T.bird_stride;
  const int n = min(max(T.kf_nb[slot], 0), BS);
  const int32_t *mps = T.kf_mpb + (size_t)slot * BS;
  for (int i = threadIdx.x; i < n; i += LB_NT) {
    const int p = mps[i];
    if (p < 0) continue;                                              // only NULL is skipped: no isBad test (:117)
    if (p >= T.n_mpb) { atomicAdd(G.err, 1); continue; }
    atomicMin(&S.pos[p], j);
  }
}

// pMP_sum of every member and the marks of the local points
__global__ __launch_bounds__(LB_NT) void k_lb_count(int n_mpb, LbS S) {
  const int p = blockIdx.x * LB_NT + threadIdx.x;
  if (p >= n_mpb) return;
  const int j = S.pos[p];
  if (j != LB_NONE) atomicAdd(&S.cnt[j], 1);
  S.eoff[p] = j != LB_NONE ? 1 : 0;
}

// the members that stay (:106-131), in order, by one workgroup
__global__ __launch_bounds__(CV_NT) void k_lb_keep(fb_local_bird_map_args A, LbS S) {
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x, L = S.hdr[LBH_L];
  int carry = 0;
  for (int base = 0; base < L; base += CV_NT) {
    const int j = base + tid;
    const int keep = j < L && S.wnear[j] && S.cnt[j] >= 10 ? 1 : 0;
    int total;
    const int at = carry + fb::block_excl_scan<CV_NT>(keep, s_wv, &total);
    if (keep && at < A.cap_kf) A.d_local_kf_bird[at] = S.wlist[j];
    carry += total;
    __syncthreads();
  }
  if (tid == 0) { *A.d_n_local_kf_bird = min(carry, A.cap_kf); *A.d_overflow = carry > A.cap_kf ? 1 : 0; }
}

__global__ __launch_bounds__(LB_NT) void k_lb_points(int n_mpb, LbS S) {
  const int p = blockIdx.x * LB_NT + threadIdx.x;
  if (p >= n_mpb) return;
  if (S.pos[p] != LB_NONE) S.plist[S.eoff[p]] = p;
}

// localMapPointBirds (:134-143): the marked points in the std::set's order.  Entry i of the index-ordered list goes to its
// rank among the marked points' (order, index) keys; with no order given that is i itself.
__global__ __launch_bounds__(LB_NT) void k_lb_emit(int n_mpb, fb_local_bird_map_args A, LbS S) {
  __shared__ uint64_t s_o[LB_NT];
  const int n = S.eoff[n_mpb];
  if (blockIdx.x != 0 && (int)(blockIdx.x * LB_NT) >= n) return;      // (uniform over the block; block 0 always writes the count)
  const int i = blockIdx.x * LB_NT + threadIdx.x;
  const int mine_p = i < n ? S.plist[i] : 0;
  int r = i;
  if (A.d_mpb_order) {
    const uint64_t mine = i < n ? A.d_mpb_order[mine_p] : 0;
    r = 0;
    for (int base = 0; base < n; base += LB_NT) {
      __syncthreads();
      if (base + (int)threadIdx.x < n) s_o[threadIdx.x] = A.d_mpb_order[S.plist[base + threadIdx.x]];
      __syncthreads();
      const int m = min(LB_NT, n - base);
      for (int k = 0; k < m; k++) {
        const uint64_t o = s_o[k];
        r += (o < mine || (o == mine && base + k < i)) ? 1 : 0;
      }
    }
  }
  if (i < n && r < A.cap_mpb) A.d_local_mpb[r] = mine_p;
  if (i == 0) {
    *A.d_n_local_mpb = min(n, A.cap_mpb);
    if (n > A.cap_mpb) *A.d_overflow = 1;
  }
}

int check_bird(const fb_covis *g, const fb_covis_map *M, const fb_covis_kf_tables *T) {
  FB_ARG(M && T);
  FB_ARG(M->max_keyframes == g->K && M->kf_order);
  FB_ARG(T->bird_stride >= 1 && T->bird_stride <= FB_COVIS_MAX_STRIDE);
  FB_ARG(T->n_mpb >= 0 && T->n_mpb < INT_MAX && T->n_bobs >= 0);
  FB_ARG(T->kf_nb && T->kf_mpb);
  return FB_OK;
}

// what a bird call reads of the caller's host tables, staged; every other pointer is cleared so that none holds a host address
void stage_bird(fb::Stager &st, fb_covis_map &M, fb_covis_kf_tables &T, bool edges, bool poses) {
  const size_t K = M.max_keyframes, BS = T.bird_stride;
  fb_covis_map m{};
  m.max_keyframes = M.max_keyframes; m.kp_stride = M.kp_stride; m.kf_order = M.kf_order;
  fb_covis_kf_tables t{};
  t.bird_stride = T.bird_stride; t.n_mpb = T.n_mpb; t.n_bobs = T.n_bobs; t.n_levels = T.n_levels;
  t.kf_nb = T.kf_nb; t.kf_mpb = T.kf_mpb;
  if (edges) { t.mpb_bad = T.mpb_bad; t.bobs_mpb = T.bobs_mpb; t.bobs_kf = T.bobs_kf; t.bobs_idx = T.bobs_idx; }
  if (poses) t.kf_Tcw = T.kf_Tcw;
  M = m; T = t;
  st.in(M.kf_order, K * 8);
  st.in(T.kf_nb, K * 4); st.in(T.kf_mpb, K * BS * 4);
  if (edges) {
    st.in(T.mpb_bad, (size_t)T.n_mpb); st.in(T.bobs_mpb, (size_t)T.n_bobs * 4); st.in(T.bobs_kf, (size_t)T.n_bobs * 4);
    st.in(T.bobs_idx, (size_t)T.n_bobs * 4);
  }
}

}  // namespace

extern "C" {

int fb_covis_reserve_local_bird_map(fb_covis *g, int32_t n_mpb, int32_t n_bobs) {
  FB_ARG(g);
  FB_ARG(n_mpb >= 0 && n_mpb < INT_MAX && n_bobs >= 0);
  FB_TRY(g->ensure_bird());
  return g->reserve(plan_bird_call(scratch_behind_index(g->state), g->K, n_mpb, n_bobs));
}

int fb_covis_update_bird_connections_dev(fb_covis *g, const fb_covis_map *M, const fb_covis_kf_tables *T, int32_t n_q,
                                         const int32_t *d_slots, const int32_t *d_n_counter, int32_t now_state, int32_t id0_slot,
                                         const int32_t *d_kf_frame_id, const uint8_t *d_kf_in_map, int32_t *d_n_bird_counter,
                                         int32_t *d_bird_front, void *stream) {
  FB_ARG(g);
  FB_TRY(check_bird(g, M, T));
  FB_ARG(T->n_mpb == 0 || T->mpb_bad);
  FB_ARG(T->n_bobs == 0 || (T->bobs_mpb && T->bobs_kf && T->bobs_idx));
  FB_ARG(n_q >= 0 && n_q <= g->K && id0_slot >= -1 && id0_slot < g->K);
  FB_ARG(n_q == 0 || (d_slots && d_n_bird_counter && d_bird_front));
  FB_ARG(now_state < 3 || (d_kf_frame_id && d_kf_in_map));
  FB_TRY(g->ensure_bird());
  if (n_q == 0) return FB_OK;
  hipStream_t s = fb::as_stream(stream);
  const fb_covis_map B = win_bird_map(*M, *T);
  Index ix;
  IndexAsk ask;
  ask.kept = false;                                   // the front index stays the one a later reuse_index reads
  ask.head = scratch_behind_index(g->state);
  FB_TRY(g->acquire(B, ask, &ix, nullptr, s));
  k_bd_update<<<n_q, CV_NT, 0, s>>>(B, g->G, g->WB, ix.start, ix.csr, d_slots, d_n_counter, now_state, id0_slot, d_kf_frame_id,
                                    d_kf_in_map, d_n_bird_counter, d_bird_front);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_update_bird_connections(fb_covis *g, const fb_covis_map *HM, const fb_covis_kf_tables *HT, int32_t n_q,
                                     const int32_t *slots, const int32_t *n_counter, int32_t now_state, int32_t id0_slot,
                                     const int32_t *kf_frame_id, const uint8_t *kf_in_map, int32_t *n_bird_counter,
                                     int32_t *bird_front) {
  FB_ARG(g);
  FB_TRY(check_bird(g, HM, HT));
  FB_ARG(HT->n_mpb == 0 || HT->mpb_bad);
  FB_ARG(HT->n_bobs == 0 || (HT->bobs_mpb && HT->bobs_kf && HT->bobs_idx));
  FB_ARG(n_q >= 0 && n_q <= g->K);
  FB_ARG(n_q == 0 || (slots && n_bird_counter && bird_front));
  FB_TRY(g->ensure_bird());
  if (n_q == 0) return FB_OK;
  fb_covis_map M = *HM;
  fb_covis_kf_tables T = *HT;
  const size_t K = g->K;
  fb::Stager st;
  stage_bird(st, M, T, true, false);
  st.in(slots, (size_t)n_q * 4); st.in(n_counter, (size_t)n_q * 4);
  st.in(kf_frame_id, K * 4); st.in(kf_in_map, K);
  st.out(n_bird_counter, (size_t)n_q * 4, false); st.out(bird_front, (size_t)n_q * 4, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_covis_update_bird_connections_dev(g, &M, &T, n_q, slots, n_counter, now_state, id0_slot, kf_frame_id, kf_in_map,
                                              n_bird_counter, bird_front, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_bird_connected_dev(fb_covis *g, int32_t slot, int32_t *d_n, int32_t *d_slots, int32_t *d_weights, void *stream) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K);
  FB_ARG(d_n && d_slots);
  FB_TRY(g->ensure_bird());
  Gr B = g->G;
  B.W = g->WB;
  k_cv_list<<<1, CV_NT, 0, fb::as_stream(stream)>>>(B, slot, LIST_ORDERED, 0, d_n, d_slots, d_weights);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_bird_connected(fb_covis *g, int32_t slot, int32_t *n, int32_t *slots, int32_t *weights) {
  FB_ARG(g);
  FB_ARG(slot >= 0 && slot < g->K);
  FB_ARG(n && slots);
  FB_TRY(g->ensure_bird());
  fb::Stager st;
  st.out(n, 4, false);
  st.out(slots, (size_t)g->K * 4, true);   // copy-in: entries past n keep the caller's contents
  st.out(weights, (size_t)g->K * 4, true);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_covis_bird_connected_dev(g, slot, n, slots, weights, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_local_bird_map_dev(fb_covis *g, const fb_covis_map *M, const fb_covis_kf_tables *T, const fb_local_bird_map_args *A,
                                void *stream) {
  FB_ARG(g && A);
  FB_TRY(check_bird(g, M, T));
  FB_ARG(A->new_slot >= 0 && A->new_slot < g->K);
  FB_ARG(A->d_kf_ow || T->kf_Tcw);
  FB_ARG(A->cap_kf >= 1 && A->cap_kf <= g->K && A->cap_mpb >= 0);
  FB_ARG(A->d_local_kf_bird && A->d_n_local_kf_bird && A->d_n_local_mpb && A->d_overflow);
  FB_ARG(A->cap_mpb == 0 || A->d_local_mpb);
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  const size_t K = g->K, n_mpb = T->n_mpb, nb = scan_tiles(n_mpb);
  LbOff lo;
  const size_t bytes = plan_local_bird_map(K, n_mpb, &lo);
  uint8_t *base;
  FB_TRY(g->behind_index(bytes, &base));
  LbS S;
  lb_map(base, lo, &S);
  const unsigned members = (unsigned)A->cap_kf + 1, pblocks = (unsigned)((n_mpb + LB_NT - 1) / LB_NT);
  if (n_mpb) FB_HIP(hipMemsetAsync(S.pos, 0x7f, n_mpb * 4, s));
  FB_HIP(hipMemsetAsync(S.eoff, 0, (n_mpb + 1) * 4, s));
  k_lb_near<<<(members + LB_NT - 1) / LB_NT, LB_NT, 0, s>>>(g->G, *T, *A, S);
  k_lb_first<<<members, LB_NT, 0, s>>>(g->G, *T, S);
  if (n_mpb) k_lb_count<<<pblocks, LB_NT, 0, s>>>((int)n_mpb, S);
  k_lb_keep<<<1, CV_NT, 0, s>>>(*A, S);
  k_cv_scan_tile<<<(unsigned)nb, CV_NT, 0, s>>>(S.eoff, (int)(n_mpb + 1), S.bsum, 0);
  k_cv_scan_sums<<<1, CV_NT, 0, s>>>(S.bsum, (int)nb);
  k_cv_scan_tile<<<(unsigned)nb, CV_NT, 0, s>>>(S.eoff, (int)(n_mpb + 1), S.bsum, 1);
  if (n_mpb) k_lb_points<<<pblocks, LB_NT, 0, s>>>((int)n_mpb, S);
  k_lb_emit<<<std::max(pblocks, 1u), LB_NT, 0, s>>>((int)n_mpb, *A, S);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_local_bird_map(fb_covis *g, const fb_covis_map *HM, const fb_covis_kf_tables *HT, const fb_local_bird_map_args *HA) {
  FB_ARG(g && HA);
  FB_TRY(check_bird(g, HM, HT));
  FB_ARG(HA->d_kf_ow || HT->kf_Tcw);
  FB_ARG(HA->cap_kf >= 1 && HA->cap_kf <= g->K && HA->cap_mpb >= 0);
  FB_ARG(HA->d_local_kf_bird && HA->d_n_local_kf_bird && HA->d_n_local_mpb && HA->d_overflow);
  FB_ARG(HA->cap_mpb == 0 || HA->d_local_mpb);
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_covis_kf_tables T = *HT;
  fb_local_bird_map_args A = *HA;
  const size_t K = g->K;
  const float *kf_Tcw = A.d_kf_ow ? nullptr : T.kf_Tcw;
  fb::Stager st;
  stage_bird(st, M, T, false, false);
  st.in(kf_Tcw, K * 48); st.in(A.d_kf_ow, K * 12); st.in(A.d_mpb_order, (size_t)T.n_mpb * 8);
  st.out(A.d_local_kf_bird, (size_t)A.cap_kf * 4, true); st.out(A.d_n_local_kf_bird, 4, true);
  st.out(A.d_local_mpb, (size_t)A.cap_mpb * 4, true);   // copy-in: entries past the count keep the caller's contents
  st.out(A.d_n_local_mpb, 4, false); st.out(A.d_overflow, 4, false);
  FB_TRY(st.commit(nullptr));
  T.kf_Tcw = const_cast<float *>(kf_Tcw);
  FB_TRY(fb_covis_local_bird_map_dev(g, &M, &T, &A, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
