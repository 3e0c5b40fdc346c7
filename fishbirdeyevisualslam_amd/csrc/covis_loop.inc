// covis_loop.inc -- the integer steps of LoopClosing between the device calls that exist (included at the end of covis.hip:
// it shares Gr, Index, row_sorted, the UpdateConnections kernels and the window's point collection).
//
// Replaces (reference file:line):
//   LoopClosing::DetectLoop, the consistency groups                 src/LoopClosing.cc:147-153, :155-228
//   LoopClosing::ComputeSim3, mvpLoopMapPoints                      :355-375
//   LoopClosing::CorrectLoop, LoopConnections                       :571-589
//
// Consistency groups: a group is a bitset over the slots.  The reference's two nested loops (candidate, previous group) have
// one dependence, vbConsistentGroup[g]: the FIRST consistent candidate of g pushes.  That is a minimum over candidate
// positions, which no order of execution changes; everything else of a (candidate, group) pair is independent.  The place
// of a push in the new list is a scan over the candidates plus the rank of g among the groups with the same first
// candidate.  Everything is integer work and is compared for equality with tests/loop_detect_ref.py.

namespace {

constexpr int DL_NT = 256;
constexpr int DL_NONE = 0x7f7f7f7f;   // first[] of a previous group no candidate is consistent with (a memset of 0x7f)

struct LoopS {          // the loop block of one handle as one call sees it
  int cap, nw;
  const uint32_t *pbits;  // [cap][nw] the previous groups
  const int32_t *pcons;   // [cap]
  const int32_t *png;     // [1]
  uint32_t *cbits;        // the current groups, written by this call
  int32_t *ccons;
  int32_t *cng;
  int32_t *first;       // [cap] the first candidate consistent with previous group g
  uint32_t *gbits;      // [K][nw] the group of candidate i
  int32_t *cnt;         // [K] pushes of candidate i, then their exclusive scan
  uint8_t *any, *enough, *valid;   // [K]
};

// One workgroup per candidate: its group from row W[c] (every entry, members or not, and c itself: GetConnectedKeyFrames,
// :167-168) by wave ballots, then the intersection test against every previous group, one wave per group.
__global__ __launch_bounds__(DL_NT) void k_dl_hit(Gr G, const int32_t *d_n, const int32_t *cand, int th, LoopS S) {
  __shared__ uint32_t s_b[CV_MAXK / 32];
  __shared__ int s_flag[2];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = G.K, nw = S.nw;
  if (i >= min(max(*d_n, 0), K)) return;
  const int c = cand[i];
  if (c < 0 || c >= K) {   // never used as an index; it pushes nothing and is not enough
    if (tid == 0) { atomicAdd(G.err, 1); S.valid[i] = 0; S.any[i] = 0; S.enough[i] = 0; }
    return;
  }
  if (tid < 2) s_flag[tid] = 0;
  const uint16_t *row = G.W + (size_t)c * K;
  for (int base = wave * 64; base < nw * 32; base += DL_NT) {
    const int j = base + lane;
    const bool bit = j < K && ((row[j] & CV_W) || j == c);
    const unsigned long long m = __ballot(bit);
    if (lane == 0) {
      s_b[base >> 5] = (uint32_t)m;
      if ((base >> 5) + 1 < nw) s_b[(base >> 5) + 1] = (uint32_t)(m >> 32);
    }
  }
  __syncthreads();
  for (int w = tid; w < nw; w += DL_NT) S.gbits[(size_t)i * nw + w] = s_b[w];
  const int ng = min(max(*S.png, 0), S.cap);
  int any = 0, enough = 0;
  for (int g = wave; g < ng; g += DL_NT / 64) {
    const uint32_t *P = S.pbits + (size_t)g * nw;
    uint32_t acc = 0;
    for (int w = lane; w < nw; w += 64) acc |= s_b[w] & P[w];
    if (__ballot(acc != 0) == 0) continue;                            // sPreviousGroup.count(*sit), :177-185
    any = 1;
    if (S.pcons[g] + 1 >= th) enough = 1;                             // :197, whether or not g was taken already
    if (lane == 0) atomicMin(&S.first[g], i);                         // :191-196: the first consistent candidate pushes
  }
  if (lane == 0) {
    if (any) atomicOr(&s_flag[0], 1);
    if (enough) atomicOr(&s_flag[1], 1);
  }
  __syncthreads();
  if (tid == 0) { S.valid[i] = 1; S.any[i] = (uint8_t)s_flag[0]; S.enough[i] = (uint8_t)s_flag[1]; }
}

// One workgroup: the pushes per candidate and their places (candidate-major), the enough list, the header.
__global__ __launch_bounds__(CV_NT) void k_dl_plan(Gr G, const int32_t *d_n, const int32_t *cand, LoopS S, int32_t *d_n_enough,
                                                   int32_t *d_enough, fb_loop_groups_header *hdr) {
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x, K = G.K;
  const int nc = min(max(*d_n, 0), K), ng = min(max(*S.png, 0), S.cap);
  for (int i = tid; i < nc; i += CV_NT) S.cnt[i] = 0;
  group_sync();
  for (int g = tid; g < ng; g += CV_NT) {
    const int f = ld(&S.first[g]);
    if (f != DL_NONE) atomicAdd(&S.cnt[f], 1);                        // f < nc: only a candidate of this call writes first[]
  }
  group_sync();
  int groups = 0, listed = 0;
  for (int base = 0; base < nc; base += CV_NT) {
    const int i = base + tid;
    int c = 0, e = 0;
    if (i < nc && S.valid[i]) { c = S.any[i] ? ld(&S.cnt[i]) : 1; e = S.enough[i]; }   // :206-210: consistent with none: one push, counter 0
    int tc, te;
    const int xc = fb::block_excl_scan<CV_NT>(c, s_wv, &tc);
    const int xe = fb::block_excl_scan<CV_NT>(e, s_wv, &te);
    if (i < nc) S.cnt[i] = groups + xc;
    if (e) d_enough[listed + xe] = cand[i];                           // listed + xe < nc <= max_keyframes
    groups += tc; listed += te;
    __syncthreads();
  }
  if (tid == 0) {
    *S.cng = min(groups, S.cap);
    *d_n_enough = listed;
    hdr->n_groups = min(groups, S.cap);
    hdr->overflow = groups > S.cap ? 1 : 0;
  }
}

// The pushes take their places.  Blocks [0, gtiles): DL_NT previous groups each; group g goes behind the groups before it
// that have the same first candidate (ranked in LDS tiles, as k_lb_emit ranks).  Blocks behind them: one wave per candidate
// that is consistent with no previous group.
__global__ __launch_bounds__(DL_NT) void k_dl_emit(Gr G, const int32_t *d_n, LoopS S, int gtiles) {
  __shared__ int s_f[DL_NT];
  __shared__ int s_pos[DL_NT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = G.K, nw = S.nw;
  if ((int)blockIdx.x >= gtiles) {
    const int i = ((int)blockIdx.x - gtiles) * (DL_NT / 64) + wave;
    if (i >= min(max(*d_n, 0), K) || !S.valid[i] || S.any[i]) return;
    const int pos = S.cnt[i];
    if (pos >= S.cap) return;
    for (int w = lane; w < nw; w += 64) S.cbits[(size_t)pos * nw + w] = S.gbits[(size_t)i * nw + w];
    if (lane == 0) S.ccons[pos] = 0;
    return;
  }
  const int ng = min(max(*S.png, 0), S.cap);
  const int g0 = blockIdx.x * DL_NT, g = g0 + tid;
  if (g0 >= ng) return;                                               // (uniform over the block)
  const int mine = g < ng ? S.first[g] : DL_NONE;
  int r = 0;
  for (int base = 0; base <= g0; base += DL_NT) {
    __syncthreads();
    s_f[tid] = base + tid < ng ? S.first[base + tid] : DL_NONE;
    __syncthreads();
    const int m = min(DL_NT, g - base);                               // the groups before g only
    for (int k = 0; k < m; k++) r += s_f[k] == mine ? 1 : 0;
  }
  __syncthreads();
  int pos = -1;
  if (mine != DL_NONE) { pos = S.cnt[mine] + r; if (pos >= S.cap) pos = -1; }
  s_f[tid] = mine; s_pos[tid] = pos;
  __syncthreads();
  for (int t = wave; t < DL_NT; t += DL_NT / 64) {
    const int p = s_pos[t];
    if (p < 0) continue;
    const uint32_t *src = S.gbits + (size_t)s_f[t] * nw;
    for (int w = lane; w < nw; w += 64) S.cbits[(size_t)p * nw + w] = src[w];
    if (lane == 0) S.ccons[p] = S.pcons[g0 + t] + 1;                  // :189-190
  }
}

// ---- mvpLoopMapPoints -------------------------------------------------------------------------------------------------------
// the list walked (:356-357): GetVectorCovisibleKeyFrames() of the matched key frame, then the key frame itself
__global__ __launch_bounds__(CV_NT) void k_lp_list(Gr G, int matched, int32_t *hdr, int32_t *wslot) {
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x;
  if (tid < WH_COUNT) hdr[tid] = 0;
  const int n = row_sorted(G, matched, LIST_ORDERED, s_key, s_wv);
  for (int p = tid; p < n; p += CV_NT) wslot[p] = G.inv[(~s_key[p]) & 4095];
  __syncthreads();
  if (tid == 0) { wslot[n] = matched; hdr[WH_LOCAL] = n + 1; }
}

__global__ void k_lp_finish(const int32_t *hdr, int cap, int32_t *d_n_loop, int32_t *d_overflow) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int n = hdr ? hdr[WH_MP] : 0;
    *d_n_loop = min(n, cap);
    *d_overflow = n > cap ? 1 : 0;
  }
}

// ---- LoopConnections --------------------------------------------------------------------------------------------------------
// the offsets of the CSR rows, by one workgroup; rows past the list are empty
__global__ __launch_bounds__(CV_NT) void k_lc_offsets(fb_loop_connections_args A, const int32_t *rowcnt) {
  __shared__ int s_wv[CV_NT / 64];
  const int n = min(max(*A.d_n_set, 0), A.set_cap);
  int carry = 0;
  for (int base = 0; base < A.set_cap; base += CV_NT) {
    const int q = base + threadIdx.x;
    const int v = q < n ? rowcnt[q] : 0;
    int total;
    const int ex = fb::block_excl_scan<CV_NT>(v, s_wv, &total);
    if (q < A.set_cap) A.d_lc_off[q] = carry + ex;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    A.d_lc_off[A.set_cap] = carry;
    A.d_header->total = carry;
    A.d_header->overflow = carry > A.lc_cap ? 1 : 0;
  }
}

// one workgroup per set member: its bit row in ascending kf_order (LoopConnections[pKFi] is a std::set<KeyFrame*>)
__global__ __launch_bounds__(DL_NT) void k_lc_emit(Gr G, fb_loop_connections_args A, const uint32_t *bits) {
  __shared__ int s_wv[DL_NT / 64];
  const int q = blockIdx.x, K = G.K, nw = (K + 31) / 32;
  if (q >= min(max(*A.d_n_set, 0), A.set_cap)) return;
  const int off = A.d_lc_off[q];
  if (A.d_lc_off[q + 1] == off) return;                               // (uniform over the block)
  const uint32_t *row = bits + (size_t)q * nw;
  int carry = off;
  for (int base = 0; base < K; base += DL_NT) {
    const int p = base + threadIdx.x;
    const int slot = p < K ? G.inv[p] : -1;
    const int bit = slot >= 0 && ((row[slot >> 5] >> (slot & 31)) & 1u) ? 1 : 0;
    int total;
    const int ex = fb::block_excl_scan<DL_NT>(bit, s_wv, &total);
    if (bit && carry + ex < A.lc_cap) A.d_lc_slots[carry + ex] = slot;
    carry += total;
    __syncthreads();
  }
}

int check_loop_connections(const fb_covis *g, const fb_loop_connections_args *a) {
  FB_ARG(a);
  FB_ARG(a->set_cap >= 0 && a->set_cap <= g->K && a->lc_cap >= 0);
  FB_ARG(a->d_n_set && a->d_lc_off && a->d_header);
  FB_ARG(a->set_cap == 0 || (a->d_set && a->d_n_counter && a->d_front));
  FB_ARG(a->lc_cap == 0 || a->d_lc_slots);
  return FB_OK;
}

}  // namespace

// the loop block: allocated by the first call that needs it, with the capacity asked for by then
static int loop_ensure(fb_covis *g) {
  FB_TRY(g->ensure());
  if (g->loop_block) return FB_OK;
  if (g->loop_cap == 0) g->loop_cap = g->K;
  const size_t total = plan_loop_groups(g->K, g->loop_cap, &g->loop_off);
  FB_HIP(hipMalloc(&g->loop_block, total));
  FB_HIP(hipMemset(g->loop_block, 0, total));
  FB_HIP(hipDeviceSynchronize());   // as ensure(): rare, and ordered before every stream
  g->loop_cur = 0;
  return FB_OK;
}

extern "C" {

int fb_covis_reserve_loop_groups(fb_covis *g, int32_t cap_groups) {
  FB_ARG(g);
  FB_ARG(cap_groups >= 1);
  if (g->loop_block && cap_groups != g->loop_cap) {   // another capacity: a new block, the groups are gone
    FB_HIP(hipDeviceSynchronize());
    FB_HIP(hipFree(g->loop_block));
    g->loop_block = nullptr;
  }
  g->loop_cap = cap_groups;
  return loop_ensure(g);
}

int fb_covis_detect_loop_dev(fb_covis *g, const int32_t *d_n_candidates, const int32_t *d_candidates, int32_t consistency_th,
                             int32_t *d_n_enough, int32_t *d_enough, fb_loop_groups_header *d_header, void *stream) {
  FB_ARG(g);
  FB_ARG(d_n_candidates && d_candidates && d_n_enough && d_enough && d_header);
  FB_TRY(loop_ensure(g));
  hipStream_t s = fb::as_stream(stream);
  uint8_t *b = static_cast<uint8_t *>(g->loop_block);
  const LoopGroupsOff &o = g->loop_off;
  const int prev = g->loop_cur, cur = 1 - prev, K = g->K;
  LoopS S;
  S.cap = g->loop_cap; S.nw = (int)loop_words(K);
  S.pbits = (const uint32_t *)(b + o.bits[prev]); S.pcons = (const int32_t *)(b + o.cons[prev]); S.png = (const int32_t *)(b + o.ng) + prev;
  S.cbits = (uint32_t *)(b + o.bits[cur]); S.ccons = (int32_t *)(b + o.cons[cur]); S.cng = (int32_t *)(b + o.ng) + cur;
  S.first = (int32_t *)(b + o.first); S.gbits = (uint32_t *)(b + o.cbits); S.cnt = (int32_t *)(b + o.cnt);
  S.any = b + o.any; S.enough = b + o.enough; S.valid = b + o.valid;
  const int gtiles = (S.cap + DL_NT - 1) / DL_NT, ctiles = (K + DL_NT / 64 - 1) / (DL_NT / 64);
  FB_HIP(hipMemsetAsync(S.first, 0x7f, (size_t)S.cap * 4, s));
  k_dl_hit<<<K, DL_NT, 0, s>>>(g->G, d_n_candidates, d_candidates, consistency_th, S);
  k_dl_plan<<<1, CV_NT, 0, s>>>(g->G, d_n_candidates, d_candidates, S, d_n_enough, d_enough, d_header);
  k_dl_emit<<<gtiles + ctiles, DL_NT, 0, s>>>(g->G, d_n_candidates, S, gtiles);
  FB_HIP(hipGetLastError());
  g->loop_cur = cur;   // mvConsistentGroups = vCurrentConsistentGroups (:214): the next call reads what this one wrote
  return FB_OK;
}

int fb_covis_detect_loop(fb_covis *g, const int32_t *n_candidates, const int32_t *candidates, int32_t consistency_th,
                         int32_t *n_enough, int32_t *enough, fb_loop_groups_header *header) {
  FB_ARG(g);
  FB_ARG(n_candidates && candidates && n_enough && enough && header);
  FB_TRY(loop_ensure(g));
  const size_t K = g->K;
  fb::Stager st;
  st.in(n_candidates, 4); st.in(candidates, K * 4);
  st.out(n_enough, 4, false);
  st.out(enough, K * 4, true);   // copy-in: entries past n_enough keep the caller's contents
  st.out(header, sizeof(fb_loop_groups_header), false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_covis_detect_loop_dev(g, n_candidates, candidates, consistency_th, n_enough, enough, header, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_loop_groups(fb_covis *g, int32_t *n, int32_t *consistency, uint32_t *bits, void *stream) {
  FB_ARG(g && n);
  FB_TRY(loop_ensure(g));
  hipStream_t s = fb::as_stream(stream);
  const uint8_t *b = static_cast<const uint8_t *>(g->loop_block);
  const LoopGroupsOff &o = g->loop_off;
  const int cur = g->loop_cur;
  FB_HIP(hipMemcpyAsync(n, b + o.ng + (size_t)cur * 4, 4, hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  const size_t ng = (size_t)std::min(std::max(*n, 0), g->loop_cap);
  if (ng && consistency) FB_HIP(hipMemcpyAsync(consistency, b + o.cons[cur], ng * 4, hipMemcpyDeviceToHost, s));
  if (ng && bits) FB_HIP(hipMemcpyAsync(bits, b + o.bits[cur], ng * loop_words(g->K) * 4, hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  return FB_OK;
}

int fb_covis_reserve_loop_map_points(fb_covis *g, int32_t n_mp) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX);
  LoopPointsOff lo;
  return g->reserve(plan_call(scratch_behind_index(g->state), 0, 0, plan_loop_points(g->K, n_mp, &lo)));
}

int fb_covis_loop_map_points_dev(fb_covis *g, const fb_covis_map *M, int32_t matched_slot, int32_t cap, int32_t *d_n_loop,
                                 int32_t *d_loop_mp, int32_t *d_overflow, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_ARG(matched_slot >= 0 && matched_slot < g->K && cap >= 0);
  FB_ARG(d_n_loop && d_overflow && (cap == 0 || d_loop_mp));
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  const size_t K = g->K, n_mp = M->n_mp;
  if (n_mp == 0) {
    k_lp_finish<<<1, 64, 0, s>>>(nullptr, cap, d_n_loop, d_overflow);
    FB_HIP(hipGetLastError());
    return FB_OK;
  }
  LoopPointsOff lo;
  const size_t bytes = plan_loop_points(K, n_mp, &lo);
  uint8_t *base;
  FB_TRY(g->behind_index(bytes, &base));
  WinS W;
  memset(&W, 0, sizeof(W));
  W.hdr = (int32_t *)(base + lo.hdr); W.wslot = (int32_t *)(base + lo.wslot); W.rowcnt = (int32_t *)(base + lo.rowcnt);
  W.side[0].ptkey = (int32_t *)(base + lo.ptkey); W.side[0].plist = (int32_t *)(base + lo.plist);
  WinOut O;
  memset(&O, 0, sizeof(O));
  O.cap_pt = cap; O.pt_index = d_loop_mp;
  const unsigned list = (unsigned)K + 1;
  k_cv_rank<<<(g->K + 255) / 256, 256, 0, s>>>(g->G, M->kf_order);
  FB_HIP(hipMemsetAsync(W.side[0].ptkey, 0x7f, n_mp * 4, s));
  k_lp_list<<<1, CV_NT, 0, s>>>(g->G, matched_slot, W.hdr, W.wslot);
  k_win_mark<<<list, WIN_NT, 0, s>>>(*M, W, 0, g->G.err);   // the window's first-occurrence collection: mnLoopPointForKF
  k_win_rowcount<<<list, WIN_NT, 0, s>>>(*M, W, 0);
  k_win_rowscan<<<1, CV_NT, 0, s>>>(W, 0);
  k_win_place<<<list, WIN_NT, 0, s>>>(*M, W, 0, nullptr, O);
  k_lp_finish<<<1, 64, 0, s>>>(W.hdr, cap, d_n_loop, d_overflow);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_loop_map_points(fb_covis *g, const fb_covis_map *H, int32_t matched_slot, int32_t cap, int32_t *n_loop,
                             int32_t *loop_mp, int32_t *overflow) {
  FB_ARG(g);
  FB_TRY(check_map(g, H));
  FB_ARG(matched_slot >= 0 && matched_slot < g->K && cap >= 0);
  FB_ARG(n_loop && overflow && (cap == 0 || loop_mp));
  FB_TRY(g->ensure());
  fb_covis_map M = *H;
  M.n_obs = 0; M.obs_mp = M.obs_kf = M.obs_idx = nullptr;   // the edge list is not read
  fb::Stager st;
  stage_map(st, M);
  st.out(n_loop, 4, false);
  st.out(loop_mp, (size_t)cap * 4, true);   // copy-in: entries past n_loop keep the caller's contents
  st.out(overflow, 4, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_covis_loop_map_points_dev(g, &M, matched_slot, cap, n_loop, loop_mp, overflow, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_reserve_loop_connections(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t set_cap) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && set_cap >= 0 && set_cap <= g->K);
  LoopConnOff lo;
  return g->reserve(plan_map_call(g->K, n_mp, n_obs, set_cap, plan_loop_connections(set_cap, g->K, &lo)));
}

int fb_covis_loop_connections_dev(fb_covis *g, const fb_covis_map *M, const fb_loop_connections_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_loop_connections(g, a));
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  const fb_loop_connections_args A = *a;
  LoopConnOff lo;
  Index ix;
  IndexAsk ask;
  ask.n_q = A.set_cap; ask.tail = plan_loop_connections(A.set_cap, g->K, &lo);
  uint8_t *tail;
  FB_TRY(g->acquire(*M, ask, &ix, &tail, s));
  LoopConnOut L;
  L.d_n = A.d_n_set; L.bits = (uint32_t *)(tail + lo.bits); L.rowcnt = (int32_t *)(tail + lo.rowcnt);
  if (A.set_cap) {
    FB_HIP(hipMemsetAsync(L.bits, 0, (size_t)A.set_cap * loop_words(g->K) * 4, s));
    k_cv_counter<<<A.set_cap, CV_NT, 0, s>>>(*M, g->G, ix.start, ix.csr, A.d_set, ix.counter, A.d_n_set);
    k_cv_apply<true><<<1, CV_NT, 0, s>>>(g->G, A.set_cap, A.d_set, ix.counter, A.d_n_counter, A.d_front, L);
  }
  k_lc_offsets<<<1, CV_NT, 0, s>>>(A, L.rowcnt);
  if (A.set_cap) k_lc_emit<<<A.set_cap, DL_NT, 0, s>>>(g->G, A, L.bits);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_loop_connections(fb_covis *g, const fb_covis_map *H, const fb_loop_connections_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, H));
  FB_TRY(check_loop_connections(g, ha));
  FB_TRY(g->ensure());
  fb_covis_map M = *H;
  fb_loop_connections_args A = *ha;
  const size_t n = A.set_cap;
  fb::Stager st;
  stage_map(st, M);
  st.in(A.d_n_set, 4); st.in(A.d_set, n * 4);
  // copy-in: rows past the list and entries past the total keep the caller's contents
  st.out(A.d_n_counter, n * 4, true); st.out(A.d_front, n * 4, true);
  st.out(A.d_lc_off, (n + 1) * 4, false); st.out(A.d_lc_slots, (size_t)A.lc_cap * 4, true);
  st.out(A.d_header, sizeof(fb_loop_connections_header), false);
  FB_TRY(st.commit(nullptr));
  IndexDropGuard drop(g->state);   // the index is of staged arrays that go back to the pool: nothing to reuse
  FB_TRY(fb_covis_loop_connections_dev(g, &M, &A, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
