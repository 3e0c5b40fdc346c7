// covis_neighbors.inc -- LocalMapping::SearchInNeighbors on the device-resident map (included from covis.hip after
// covis_fuse.inc and covis_loop.inc: it shares FzRun / fz_replace, the window's first-occurrence collection, the refresh
// and the batched UpdateConnections).
//
// Replaces (reference file:line):
//   LocalMapping::SearchInNeighbors                                        src/LocalMapping.cc:478-558
//   ORBmatcher::Fuse(pKF, vpMapPoints, th), its skip rule and its commit   src/ORBmatcher.cc:843-851, :952-972
//   MapPoint::AddObservation (monocular)                                   src/MapPoint.cc:98-109
//
// One Fuse call is prepare -> grid -> search -> commit, as in SearchAndFuse; the search of a call runs as a batch before its
// commit (DESIGN 7l says why that is exact), the calls follow each other on the stream because the commit of one changes
// the descriptors and bad flags the next one's search reads.

namespace {

enum { SH_OK = 16, SH_NT, SH_NC, SH_CUR, SH_ONE, SH_SCALE = 32 };      // ints of SinS.hdr behind the window's header
static_assert(WH_COUNT <= SH_OK && SH_SCALE + FB_MAX_LEVELS <= 64, "the header region holds 64 ints");

struct SinS {           // the scratch of one call, behind the log
  int32_t *hdr;         // [64] the window's header; ok, the clamped counts, cur as a query, ok as a count; the scale factors
  int32_t *snap;        // [S] vpMapPointMatches
  int32_t *wslot, *rowcnt, *ptkey, *plist;                                 // the first-occurrence collection
  fb_keypoint *kps; uint8_t *kdesc; int32_t *n_kf, *n_list; float *pose, *ow;   // the key frame as the search's batch of one
  int32_t *cell_start, *cell_items;
  uint8_t *valid; float *xw, *normal, *mind, *maxd; uint8_t *desc;         // the points as the search's list
  int32_t *best;
};
void sin_map(uint8_t *b, const SinOff &o, SinS *S) {
  S->hdr = (int32_t *)(b + o.hdr); S->snap = (int32_t *)(b + o.snap); S->wslot = (int32_t *)(b + o.wslot); S->rowcnt = (int32_t *)(b + o.rowcnt);
  S->ptkey = (int32_t *)(b + o.ptkey); S->plist = (int32_t *)(b + o.plist); S->kps = (fb_keypoint *)(b + o.kps); S->kdesc = b + o.kdesc;
  S->n_kf = (int32_t *)(b + o.n_kf); S->n_list = (int32_t *)(b + o.n_list); S->pose = (float *)(b + o.pose); S->ow = (float *)(b + o.ow);
  S->cell_start = (int32_t *)(b + o.cell_start); S->cell_items = (int32_t *)(b + o.cell_items); S->valid = b + o.valid;
  S->xw = (float *)(b + o.xw); S->normal = (float *)(b + o.normal); S->mind = (float *)(b + o.mind); S->maxd = (float *)(b + o.maxd);
  S->desc = b + o.desc; S->best = (int32_t *)(b + o.best);
}

// ---- the target list (LocalMapping.cc:481-503) ---------------------------------------------------------------------------------
// One workgroup.  The ordered vectors come from row_sorted; the pushes are serial and few, thread 0 makes them.
__global__ __launch_bounds__(CV_NT) void k_sin_targets(Gr G, int cur, int nn, int nn2, const uint8_t *kf_bad, int cap, int32_t *d_n,
                                                       int32_t *d_targets) {
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ int s_first[CV_MAXK];
  __shared__ uint32_t s_stamp[CV_MAXK / 32];                            // mnFuseTargetForKF == cur's id
  __shared__ int s_wv[CV_NT / 64];
  __shared__ int s_pos;
  const int tid = threadIdx.x;
  for (int w = tid; w < CV_MAXK / 32; w += CV_NT) s_stamp[w] = 0u;
  if (tid == 0) s_pos = 0;
  const int n1 = min(row_sorted(G, cur, LIST_ORDERED, s_key, s_wv), max(nn, 0));   // :484
  for (int p = tid; p < n1; p += CV_NT) s_first[p] = G.inv[(~s_key[p]) & 4095];
  __syncthreads();
  for (int a = 0; a < n1; a++) {
    const int f = s_first[a];
    if (kf_bad[f] || ((s_stamp[f >> 5] >> (f & 31)) & 1u)) continue;    // :489
    const int n2 = min(row_sorted(G, f, LIST_ORDERED, s_key, s_wv), max(nn2, 0));   // :495
    if (tid == 0) {
      int pos = s_pos;
      if (pos < cap) d_targets[pos] = f;                                // :491
      pos++;
      s_stamp[f >> 5] |= 1u << (f & 31);                                // :492
      for (int p = 0; p < n2; p++) {
        const int s2 = G.inv[(~s_key[p]) & 4095];
        if (kf_bad[s2] || ((s_stamp[s2 >> 5] >> (s2 & 31)) & 1u) || s2 == cur) continue;   // :499
        if (pos < cap) d_targets[pos] = s2;                             // :501, not stamped
        pos++;
      }
      s_pos = pos;
    }
    __syncthreads();
  }
  if (tid == 0) {
    *d_n = s_pos;
    if (s_pos > cap) atomicAdd(G.err, 1);
  }
}

// ---- one call ------------------------------------------------------------------------------------------------------------------
// the flags of the call, the snapshot of cur's row (:508), and the counts at zero
__global__ __launch_bounds__(CV_NT) void k_sin_begin(fb_covis_map M, fb_search_in_neighbors_args P, SinS S, int32_t *err) {
  const int tid = threadIdx.x, cur = P.cur_slot, NF = P.n_features;
  const bool ok = M.kf_n[cur] == NF;                                    // the host's N is the table's, or nothing is done
  for (int i = tid; i < M.kp_stride; i += CV_NT) S.snap[i] = (ok && i < NF) ? M.kf_mp[(size_t)cur * M.kp_stride + i] : -1;
  for (int k = tid; k <= P.n_targets; k += CV_NT) P.d_n_fused[k] = 0;
  if (tid < P.n_levels) reinterpret_cast<float *>(S.hdr + SH_SCALE)[tid] = P.scale_factors[tid];
  if (tid == 0) {
    if (!ok) atomicAdd(err, 1);
    S.hdr[SH_OK] = ok ? 1 : 0; S.hdr[SH_ONE] = ok ? 1 : 0; S.hdr[SH_CUR] = ok ? cur : -1; S.hdr[SH_NC] = 0;
    S.hdr[SH_NT] = ok ? min(max(*P.d_n_targets, 0), P.n_targets) : 0;
    *P.d_n_added = 0; *P.map.d_n_replaced = 0; *P.d_n_candidates = 0;
  }
}

struct SinTurn { int kf, n; const int32_t *list; };                    // one Fuse call: the key frame (-1: idle), the list
__device__ __forceinline__ SinTurn sin_turn(const fb_search_in_neighbors_args &P, const SinS &S, int k, int phase) {
  SinTurn t;
  t.kf = -1; t.n = 0; t.list = nullptr;
  if (phase == 0) {                                                     // :513, target k and the snapshot
    if (k >= S.hdr[SH_NT]) return t;
    t.kf = P.d_targets[k]; t.n = P.n_features; t.list = S.snap;
  } else if (S.hdr[SH_OK]) {                                            // :538, cur and the candidates
    t.kf = P.cur_slot; t.n = S.hdr[SH_NC]; t.list = P.d_candidates;
  }
  return t;
}

// IsInKeyFrame(kf) of mp on the map as it stands: the index's row of the point, then the edges it gained in this call
__device__ __forceinline__ bool sin_in_keyframe(const FzRun &R, int mp, int kf) {
  const int p1 = R.start[mp + 1];
  for (int p = R.start[mp]; p < p1; p++) {
    const int e = R.csr[p];
    if (R.A.obs_mp[e] == mp && R.A.obs_kf[e] == kf) return true;
  }
  int steps = 0;
  for (int e = R.head[mp]; e >= 0 && steps <= R.cap; e = R.next[e], steps++)
    if (R.A.obs_kf[e] == kf) return true;
  return false;
}

// The key frame of the turn as the search reads it and the listed points with the skip rule of :843-851, from the map as it
// stands.  One workgroup.
__global__ __launch_bounds__(CV_NT) void k_sin_prepare(FzRun R, fb_search_in_neighbors_args P, int k, int phase, SinS S) {
  const fb_covis_map &M = R.M;
  const int tid = threadIdx.x, St = M.kp_stride;
  const SinTurn t = sin_turn(P, S, k, phase);
  if (t.kf < 0 || t.kf >= M.max_keyframes) {
    if (tid == 0) { if (t.list) atomicAdd(R.G.err, 1); *S.n_kf = 0; *S.n_list = 0; }   // (an idle launch is no error)
    return;
  }
  for (int i = tid; i < St; i += CV_NT) fz_stage_feature(S, P.kf_keys_un, P.map.kf_desc, t.kf, St, i);
  if (tid < 12) S.pose[tid] = P.kf_Tcw[(size_t)t.kf * 12 + tid];
  if (tid == 64) fb::camera_centre(P.kf_Tcw + (size_t)t.kf * 12, S.ow);
  if (tid == 0) { *S.n_kf = min(max(M.kf_n[t.kf], 0), St); *S.n_list = t.n; }
  for (int i = tid; i < t.n; i += CV_NT) {
    const int mp = t.list[i];
    S.best[i] = -1;
    if (mp < 0) { S.valid[i] = 0; continue; }                           // :845
    if (mp >= M.n_mp) { atomicAdd(R.G.err, 1); S.valid[i] = 0; continue; }
    S.valid[i] = (!M.mp_bad[mp] && !sin_in_keyframe(R, mp, t.kf)) ? 1 : 0;   // :848
    fz_stage_point(S, P, mp, i);
  }
}

// The commit of Fuse (:952-972) serial in i; one wave, parallel over the edges of the two points of a step.
__global__ __launch_bounds__(64) void k_sin_commit(FzRun R, fb_search_in_neighbors_args P, int k, int phase, SinS Sc, int e0, int key_cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pt_smem[];
  const FzLds L = fz_lds(pt_smem, R.cap, key_cap);
  const int lane = threadIdx.x, S = R.M.kp_stride;
  const SinTurn t = sin_turn(P, Sc, k, phase);
  if (t.kf < 0 || t.kf >= R.M.max_keyframes) return;                    // d_n_fused is 0 since k_sin_begin
  const int N = *Sc.n_kf;
  const uint32_t r = (uint32_t)R.G.rank[t.kf];
  int n_rep = *R.A.d_n_replaced, n_add = *P.d_n_added, n_fused = 0;
  for (int base = 0; base < t.n; base += 64) {
    const int i_l = base + lane;
    int b_l = -1;
    if (i_l < t.n && Sc.valid[i_l]) b_l = Sc.best[i_l];
    if (b_l >= N) b_l = -1;
    unsigned long long todo = __ballot(b_l >= 0);                       // bestDist <= TH_LOW
    while (todo) {
      const int b = __ffsll((long long)todo) - 1, i = base + b;
      todo &= todo - 1;
      const int best = __shfl(b_l, b, 64), pMP = t.list[i];
      group_sync();
      if (ld(&R.A.mp_bad[pMP])) continue;                               // :848 on the live map: an earlier step replaced it
      const int nP = fz_keys(R, L, pMP, lane);                          // Observations(pMP) and its key frames
      if ((L.has[r >> 5] >> (r & 31)) & 1u) continue;                   // IsInKeyFrame(pKF): cur holds the point at two features
      const int have = ld(&R.A.kf_mp[(size_t)t.kf * S + best]);         // pKF->GetMapPoint(bestIdx), as it stands now
      if (have >= R.M.n_mp) { if (lane == 0) atomicAdd(R.G.err, 1); continue; }
      if (have >= 0) {
        n_fused++;                                                      // :970
        if (ld(&R.A.mp_bad[have])) continue;                            // :958
        const int nK = fz_edges(R, L, have, lane, [](int, int) {});     // Observations(pMPinKF)
        if (nK > nP) fz_replace(R, L, pMP, have, lane, &n_rep);         // :960-961
        else fz_replace(R, L, have, pMP, lane, &n_rep);                 // :962-963
        continue;
      }
      if (nP > R.cap) {                                                 // the overflow contract: AddObservation's early return
        if (lane == 0) { atomicAdd(R.G.err, 1); st(&R.A.kf_mp[(size_t)t.kf * S + best], pMP); }
        n_fused++;
        continue;
      }
      if (n_add >= P.new_edge_cap) { if (lane == 0) atomicAdd(R.G.err, 1); continue; }   // the block is full: the add is not made
      const int e = e0 + n_add;
      if (lane == 0) {
        st(&R.A.obs_mp[e], pMP); st(&R.A.obs_kf[e], t.kf); st(&R.obs_idx[e], best);       // :967 AddObservation
        fz_link(R, pMP, e);
        st(&R.A.kf_mp[(size_t)t.kf * S + best], pMP);                   // :968 AddMapPoint
        if (n_add < P.added_cap) { int32_t *row = P.d_added + (size_t)n_add * 4; row[0] = t.kf; row[1] = pMP; row[2] = best; row[3] = e; }
      }
      n_add++; n_fused++;
    }
  }
  if (lane == 0) { P.d_n_fused[phase ? P.n_targets : k] = n_fused; *P.d_n_added = n_add; *R.A.d_n_replaced = n_rep; }
}

// the list the first-occurrence collection walks: the targets in list order (:520), slots out of range dropped
__global__ __launch_bounds__(CV_NT) void k_sin_wlist(fb_search_in_neighbors_args P, SinS S, int K) {
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x, n = S.hdr[SH_NT];
  if (tid < WH_COUNT) S.hdr[tid] = 0;
  int carry = 0;
  for (int base = 0; base < n; base += CV_NT) {
    const int p = base + tid;
    const int kf = p < n ? P.d_targets[p] : -1;
    const int take = (kf >= 0 && kf < K) ? 1 : 0;                       // (counted by its k_sin_prepare)
    int total;
    const int ex = fb::block_excl_scan<CV_NT>(take, s_wv, &total);
    if (take) S.wslot[carry + ex] = kf;
    carry += total;
    __syncthreads();
  }
  group_sync();
  if (tid == 0) S.hdr[WH_LOCAL] = carry;
}

__global__ void k_sin_candidates(fb_search_in_neighbors_args P, SinS S, int32_t *err) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int n = S.hdr[WH_MP];
    *P.d_n_candidates = n;
    S.hdr[SH_NC] = min(n, P.cand_cap);
    if (n > P.cand_cap) atomicAdd(err, 1);
  }
}

// the list of one, cur (:542): its live points are collected like the candidates
__global__ void k_sin_curlist(fb_search_in_neighbors_args P, SinS S) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    for (int i = 0; i < WH_COUNT; i++) S.hdr[i] = 0;
    S.wslot[0] = P.cur_slot;
    S.hdr[WH_LOCAL] = S.hdr[SH_OK];
  }
}

int check_fuse_targets(const fb_covis *g, int32_t cur_slot, int32_t nn, int32_t nn2, const uint8_t *kf_bad, int32_t target_cap,
                       const int32_t *n_targets, const int32_t *targets) {
  FB_ARG(g);
  FB_ARG(cur_slot >= 0 && cur_slot < g->K);
  FB_ARG(nn >= 0 && nn2 >= 0 && kf_bad && target_cap >= 0 && n_targets && (target_cap == 0 || targets));
  return FB_OK;
}

int check_search_in_neighbors(const fb_covis *g, const fb_covis_map *M, const fb_search_in_neighbors_args *a) {
  FB_ARG(a);
  FB_ARG(a->cur_slot >= 0 && a->cur_slot < g->K);
  FB_ARG(a->n_features >= 0 && a->n_features <= M->kp_stride);
  FB_ARG(a->n_targets >= 0 && a->n_targets <= FB_FUSE_TARGETS_MAX && a->d_n_targets && (a->n_targets == 0 || a->d_targets));
  FB_ARG(a->n_levels >= 1 && a->n_levels <= FB_MAX_LEVELS && a->grid.cols > 0 && a->grid.rows > 0 && a->kf_keys_un && a->kf_Tcw);
  FB_ARG(M->n_mp == 0 || (a->mp_xw && a->mp_normal && a->mp_min_dist && a->mp_max_dist && a->mp_ref_kf));
  FB_ARG(a->d_n_fused && a->cand_cap >= 0 && a->d_n_candidates && (a->cand_cap == 0 || a->d_candidates));
  FB_ARG(a->d_n_added && a->added_cap >= 0 && (a->added_cap == 0 || a->d_added) && a->d_n_counter && a->d_front);
  FB_ARG(a->obs_cap >= 0 && a->new_edge_cap >= 0);
  if ((int64_t)M->n_obs + a->new_edge_cap > (int64_t)a->obs_cap) {
    fb::set_error("fb_covis_search_in_neighbors: %d edges and %d new ones do not fit obs_cap = %d", M->n_obs, a->new_edge_cap, a->obs_cap);
    return FB_ERR_CAPACITY;
  }
  FB_ARG(a->obs_cap == 0 || (a->obs_idx && a->map.obs_mp && a->map.obs_kf));
  return check_point_fuse(M, &a->map);
}

}  // namespace

extern "C" {

int fb_covis_fuse_targets_dev(fb_covis *g, int32_t cur_slot, int32_t nn, int32_t nn2, const uint8_t *d_kf_bad, int32_t target_cap,
                              int32_t *d_n_targets, int32_t *d_targets, void *stream) {
  FB_TRY(check_fuse_targets(g, cur_slot, nn, nn2, d_kf_bad, target_cap, d_n_targets, d_targets));
  FB_TRY(g->ensure());
  k_sin_targets<<<1, CV_NT, 0, fb::as_stream(stream)>>>(g->G, cur_slot, nn, nn2, d_kf_bad, target_cap, d_n_targets, d_targets);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_fuse_targets(fb_covis *g, int32_t cur_slot, int32_t nn, int32_t nn2, const uint8_t *kf_bad, int32_t target_cap,
                          int32_t *n_targets, int32_t *targets) {
  FB_TRY(check_fuse_targets(g, cur_slot, nn, nn2, kf_bad, target_cap, n_targets, targets));
  FB_TRY(g->ensure());
  fb::Stager st;
  st.in(kf_bad, (size_t)g->K);
  st.out(n_targets, 4, false);
  st.out(targets, (size_t)target_cap * 4, true);   // copy-in: entries past the count keep the caller's contents
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_covis_fuse_targets_dev(g, cur_slot, nn, nn2, kf_bad, target_cap, n_targets, targets, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_reserve_search_in_neighbors(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t new_edge_cap, int32_t kp_stride,
                                         int32_t n_targets, int32_t cand_cap, int32_t grid_cells) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && new_edge_cap >= 0 && (int64_t)n_obs + new_edge_cap <= INT_MAX);
  FB_ARG(kp_stride >= 1 && kp_stride <= FB_COVIS_MAX_STRIDE && n_targets >= 0 && n_targets <= FB_FUSE_TARGETS_MAX && cand_cap >= 0 &&
         grid_cells >= 0);
  FzOff fo;
  SinOff so;
  const size_t S = kp_stride, edges = (size_t)n_obs + (size_t)new_edge_cap;
  return g->reserve(plan_map_call(g->K, n_mp, edges, 1, plan_point_fuse(n_mp, edges, 0, &fo) +
                                                            plan_search_in_neighbors(n_mp, S, n_targets, std::max(S, (size_t)cand_cap), grid_cells, &so)));
}

int fb_covis_search_in_neighbors_dev(fb_covis *g, const fb_covis_map *M, const fb_search_in_neighbors_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_search_in_neighbors(g, M, a));
  FB_TRY(check_point_fuse_own(M, &a->map, a->obs_cap != 0));
  FB_ARG(a->obs_cap == 0 || a->obs_idx == M->obs_idx);
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  const size_t S = M->kp_stride, n_mp = M->n_mp, cells = (size_t)a->grid.cols * a->grid.rows, list = std::max(S, (size_t)a->cand_cap);
  // The block the call owns is preset to tombstones and the walk runs on the grown map: its index is the one of the map as it
  // came in (a tombstone is no edge), and the index built again for steps 5-6 lies where this one lay.
  fb_covis_map G2 = *M;
  G2.n_obs = M->n_obs + a->new_edge_cap;
  if (a->new_edge_cap) {
    int32_t *arr[3] = {a->map.obs_mp, a->map.obs_kf, a->obs_idx};
    for (int32_t *p : arr) FB_HIP(hipMemsetAsync(p + M->n_obs, 0xff, (size_t)a->new_edge_cap * 4, s));
  }
  SinOff so;
  FzOff fo;
  const size_t more = plan_search_in_neighbors(n_mp, S, a->n_targets, list, cells, &so);
  FzRun R;
  uint8_t *b;
  FB_TRY(fz_begin(g, &G2, a->map, 0, &R, s, more, &b, 1));
  R.obs_idx = a->obs_idx;
  SinS Sc;
  sin_map(b, so, &Sc);
  k_sin_begin<<<1, CV_NT, 0, s>>>(*M, *a, Sc, g->G.err);
  FB_HIP(hipGetLastError());
  fb_fuse_args F;
  memset(&F, 0, sizeof(F));
  F.batch = 1; F.th = a->th; F.pose = Sc.pose; F.Ow = Sc.ow; F.best_idx = Sc.best;
  F.kf.kf_stride = (int32_t)S; F.kf.n_kf = Sc.n_kf; F.kf.kf_kps = Sc.kps; F.kf.kf_desc = Sc.kdesc; F.kf.kf_cell_start = Sc.cell_start;
  F.kf.kf_cell_items = Sc.cell_items; F.kf.cam = a->cam; F.kf.grid = a->grid; F.kf.log_scale_factor = a->log_scale_factor;
  F.kf.n_levels = a->n_levels;
  memcpy(F.kf.scale_factors, a->scale_factors, sizeof(F.kf.scale_factors));
  memcpy(F.kf.inv_level_sigma2, a->inv_level_sigma2, sizeof(F.kf.inv_level_sigma2));
  F.mp.mp_stride = (int32_t)list; F.mp.n_mp = Sc.n_list; F.mp.mp_valid = Sc.valid; F.mp.mp_xw = Sc.xw; F.mp.mp_normal = Sc.normal;
  F.mp.mp_max_dist = Sc.maxd; F.mp.mp_min_dist = Sc.mind; F.mp.mp_desc = Sc.desc;
  auto fuse = [&](int k, int phase) -> int {                            // four launches, no host wait
    k_sin_prepare<<<1, CV_NT, 0, s>>>(R, *a, k, phase, Sc);
    FB_HIP(hipGetLastError());
    FB_TRY(fb_grid_build_batch_dev(Sc.kps, Sc.n_kf, 1, (int)S, &a->grid, Sc.cell_start, Sc.cell_items, stream));
    FB_TRY(fb_fuse_search_dev(&F, stream));
    k_sin_commit<<<1, 64, fz_lds_bytes(g->K), s>>>(R, *a, k, phase, Sc, M->n_obs, fz_key_cap(g->K));
    FB_HIP(hipGetLastError());
    return FB_OK;
  };
  for (int k = 0; k < a->n_targets; k++) FB_TRY(fuse(k, 0));            // :509-514
  // :517-536, the window's first-occurrence collection over the targets (mnFuseCandidateForKF)
  WinS W;
  memset(&W, 0, sizeof(W));
  W.hdr = Sc.hdr; W.wslot = Sc.wslot; W.rowcnt = Sc.rowcnt; W.side[0].ptkey = Sc.ptkey; W.side[0].plist = Sc.plist;
  WinOut O;
  memset(&O, 0, sizeof(O));
  O.cap_pt = a->cand_cap; O.pt_index = a->d_candidates;
  auto collect = [&](unsigned rows) -> int {
    if (n_mp) FB_HIP(hipMemsetAsync(Sc.ptkey, 0x7f, n_mp * 4, s));
    k_win_mark<<<rows, WIN_NT, 0, s>>>(G2, W, 0, g->G.err);
    k_win_rowcount<<<rows, WIN_NT, 0, s>>>(G2, W, 0);
    k_win_rowscan<<<1, CV_NT, 0, s>>>(W, 0);
    k_win_place<<<rows, WIN_NT, 0, s>>>(G2, W, 0, nullptr, O);
    FB_HIP(hipGetLastError());
    return FB_OK;
  };
  k_sin_wlist<<<1, CV_NT, 0, s>>>(*a, Sc, g->K);
  FB_TRY(collect((unsigned)std::max(a->n_targets, 1)));
  k_sin_candidates<<<1, 64, 0, s>>>(*a, Sc, g->G.err);
  FB_HIP(hipGetLastError());
  FB_TRY(fuse(0, 1));                                                   // :538
  // :542-557 on the grown map: cur's live points, both parts of the refresh, UpdateConnections
  O.cap_pt = 0; O.pt_index = nullptr;
  k_sin_curlist<<<1, 64, 0, s>>>(*a, Sc);
  FB_TRY(collect(1));
  Index ix;
  IndexAsk ask;
  ask.n_q = 1;
  ask.tail = plan_point_fuse(n_mp, (size_t)G2.n_obs, 0, &fo) + more;
  FB_TRY(g->acquire(G2, ask, &ix, nullptr, s));                        // where the first one lay: the tail stays
  PtRun Rf;
  memset(&Rf, 0, sizeof(Rf));
  fb_point_refresh_args &A = Rf.A;
  A.what = FB_REFRESH_NORMAL_DEPTH | FB_REFRESH_DESCRIPTOR; A.n_levels = a->n_levels; A.kf_Tcw = a->kf_Tcw; A.kf_bad = a->map.kf_bad;
  A.kf_desc = a->map.kf_desc; A.scale_factors = reinterpret_cast<const float *>(Sc.hdr + SH_SCALE); A.mp_xw = a->mp_xw; A.mp_ref_kf = a->mp_ref_kf;
  A.mp_normal = a->mp_normal; A.mp_min_dist = a->mp_min_dist; A.mp_max_dist = a->mp_max_dist; A.mp_desc = a->map.mp_desc;
  Rf.list = Sc.plist; Rf.d_n = Sc.hdr + WH_MP; Rf.n_list = (int)std::min((size_t)a->n_features, n_mp); Rf.cap = g->K;
  FB_TRY(launch_refresh(g, &G2, ix, Rf, s));
  k_cv_counter<<<1, CV_NT, 0, s>>>(G2, g->G, ix.start, ix.csr, Sc.hdr + SH_CUR, ix.counter, Sc.hdr + SH_ONE);
  k_cv_apply<false><<<1, CV_NT, 0, s>>>(g->G, 1, Sc.hdr + SH_CUR, ix.counter, a->d_n_counter, a->d_front, LoopConnOut{});
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_search_in_neighbors(fb_covis *g, const fb_covis_map *HM, const fb_search_in_neighbors_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_TRY(check_search_in_neighbors(g, HM, ha));
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_search_in_neighbors_args A = *ha;
  const size_t K = g->K, S = M.kp_stride, n_mp = M.n_mp, n_edges = (size_t)M.n_obs + (size_t)A.new_edge_cap;
  fb::Stager st;
  st.in(A.d_n_targets, 4); st.in(A.d_targets, (size_t)A.n_targets * 4);
  st.in(A.kf_keys_un, K * S * sizeof(fb_keypoint)); st.in(A.kf_Tcw, K * 48);
  st.in(A.mp_xw, n_mp * 12); st.in(A.mp_ref_kf, n_mp * 4);
  // copy-in: what the call leaves alone keeps the caller's contents
  st.out(A.mp_normal, n_mp * 12, true); st.out(A.mp_min_dist, n_mp * 4, true); st.out(A.mp_max_dist, n_mp * 4, true);
  stage_point_fuse(st, M, A.map, n_edges);
  st.out(A.obs_idx, n_edges * 4, true);
  st.out(A.d_n_fused, ((size_t)A.n_targets + 1) * 4, false);
  st.out(A.d_n_candidates, 4, false); st.out(A.d_candidates, (size_t)A.cand_cap * 4, true);
  st.out(A.d_n_added, 4, false); st.out(A.d_added, (size_t)A.added_cap * 16, true);
  st.out(A.d_n_counter, 4, false); st.out(A.d_front, 4, false);
  FB_TRY(st.commit(nullptr));
  M.kf_mp = A.map.kf_mp; M.mp_bad = A.map.mp_bad; M.obs_mp = A.map.obs_mp; M.obs_kf = A.map.obs_kf; M.obs_idx = A.obs_idx;
  IndexDropGuard drop(g->state);
  FB_TRY(fb_covis_search_in_neighbors_dev(g, &M, &A, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
