// covis_fuse.inc -- MapPoint::Replace, the loop fusion and SearchAndFuse on the device-resident map (included from covis.hip after
// covis_points.inc: it shares pt_sort, pt_descriptor, Gr, Index).
//
// Replaces (reference file:line):
//   MapPoint::Replace                                                      src/MapPoint.cc:177-215
//   MapPoint::AddObservation (monocular), with its early return            src/MapPoint.cc:98-109
//   LoopClosing::CorrectLoop, the loop fusion                              src/LoopClosing.cc:545-560
//   LoopClosing::SearchAndFuse                                             src/LoopClosing.cc:616-642
//   ORBmatcher::Fuse(pKF, Scw, ..), its skip rule and its commit           src/ORBmatcher.cc:994, :1006, :1083-1097
//
// Pairs that share a point depend on each other, so the list is walked serially by one wave; within an operation the wave
// is parallel over the edges of the two points.  The edges of a point as they stand in the middle of the walk are
//   { e in the index's row of the point : obs_mp[e] is still the point and obs_kf[e] >= 0 }  +  the point's list,
// where the list (head / next) holds the edges the point gained in this call whose row in the index is another point's (or
// none's: a new edge).  A Replace takes every edge of `from`, so its list is dropped whole and next[e] is free to be written
// again when e moves on.  The cost of an operation is the edges of its two points, whatever the length of the walk.
// Arrays the walk both reads and writes go through ld / st; group_sync() separates the operations.

namespace {

struct FzRun {
  fb_covis_map M;
  Gr G;
  const int32_t *start, *csr;
  int32_t *head, *next;         // the lists, see above
  const int32_t *home;          // [M.n_obs] obs_mp as it came in
  fb_point_fuse_arrays A;
  int32_t *obs_idx;             // writable (loop fusion), or NULL
  int cap;                      // K: more live edges than key frames is a repeated (mp, kf) edge
};

struct FzLds {
  uint4 *D;                     // [PT_STAGE][2]
  uint32_t *key;                // [pow2 >= 2 * cap] the keys (rank << 15 | feature) of `to`
  int32_t *edge;                // [cap] the edges of `from`
  uint32_t *has;                // [(cap + 31) / 32] the ranks `to` has an edge to
  int32_t *n;                   // [1]
};

__device__ __forceinline__ FzLds fz_lds(uint8_t *smem, int cap, int key_cap) {
  FzLds L;
  L.D = reinterpret_cast<uint4 *>(smem);
  L.key = reinterpret_cast<uint32_t *>(smem + (size_t)PT_STAGE * 32);
  L.edge = reinterpret_cast<int32_t *>(L.key + key_cap);
  L.has = reinterpret_cast<uint32_t *>(L.edge + cap);
  L.n = reinterpret_cast<int32_t *>(L.has + (cap + 31) / 32);
  return L;
}

// The live edges of mp as they stand, handed to put(position, edge) for the first `cap` of them; -> their number (every lane).
template <typename Put>
__device__ __forceinline__ int fz_edges(const FzRun &R, const FzLds &L, int mp, int lane, Put put) {
  const int p0 = R.start[mp], cnt = R.start[mp + 1] - p0;
  int n = 0;
  for (int base = 0; base < cnt; base += 64) {
    const int q = base + lane;
    int e = -1;
    bool live = false;
    if (q < cnt) {
      e = R.csr[p0 + q];
      live = ld(&R.A.obs_mp[e]) == mp && ld(&R.A.obs_kf[e]) >= 0;
    }
    const unsigned long long mask = __ballot(live);
    const int pos = n + __popcll(mask & ((1ull << lane) - 1ull));
    if (live && pos < R.cap) put(pos, e);
    n += __popcll(mask);
  }
  __syncthreads();
  if (lane == 0) {                                                      // the list: short, and one lane follows it
    int steps = 0;
    for (int e = ld(&R.head[mp]); e >= 0 && steps <= R.cap; e = ld(&R.next[e]), steps++) {
      if (n < R.cap) put(n, e);
      n++;
    }
    *L.n = n;
  }
  __syncthreads();
  return *L.n;
}

// the edges of `to` as keys in L.key and as bits of L.has
__device__ __forceinline__ int fz_keys(const FzRun &R, const FzLds &L, int mp, int lane) {
  for (int w = lane; w < (R.cap + 31) / 32; w += 64) L.has[w] = 0u;
  __syncthreads();
  return fz_edges(R, L, mp, lane, [&](int pos, int e) {
    const uint32_t r = (uint32_t)R.G.rank[ld(&R.A.obs_kf[e])];
    L.key[pos] = (r << 15) | (uint32_t)ld(&R.M.obs_idx[e]);
    atomicOr(&L.has[r >> 5], 1u << (r & 31));
  });
}

// e becomes an edge of mp that the index does not list under mp
__device__ __forceinline__ void fz_link(const FzRun &R, int mp, int e) {
  const int old = atomicExch(&R.head[mp], e);
  st(&R.next[e], old);
}

// ComputeDistinctiveDescriptors(mp) from its n keys in L.key
__device__ __forceinline__ void fz_refresh(const FzRun &R, const FzLds &L, int mp, int n, int lane) {
  group_sync();
  if (ld(&R.A.mp_bad[mp]) || n == 0) return;                            // :251, observations.empty()
  if (n > R.cap) { if (lane == 0) atomicAdd(R.G.err, 1); return; }
  pt_sort(L.key, n, lane);
  pt_descriptor(R.A.kf_bad, R.A.kf_desc, R.A.mp_desc + (size_t)mp * 32, R.G, R.M.kp_stride, L.key, L.D, n, lane);
}

// from->Replace(to), MapPoint.cc:177-215; n_rep counts the pairs that took effect
__device__ __forceinline__ void fz_replace(const FzRun &R, const FzLds &L, int from, int to, int lane, int *n_rep) {
  if (from == to) return;                                               // :179
  group_sync();
  const int S = R.M.kp_stride;
  const int nf = fz_edges(R, L, from, lane, [&](int pos, int e) { L.edge[pos] = e; });   // obs = mObservations
  int nt = fz_keys(R, L, to, lane);
  if (nf > R.cap || nt > R.cap) { if (lane == 0) atomicAdd(R.G.err, 1); return; }
  if (lane == 0) {
    st(&R.A.mp_bad[from], (uint8_t)1);                                  // :189
    st(&R.A.mp_replaced[from], to);                                     // :192
    st(&R.head[from], -1);                                              // mObservations.clear()
  }
  for (int base = 0; base < nf; base += 64) {                           // :195
    const int j = base + lane;
    bool move = false;
    uint32_t key = 0;
    if (j < nf) {
      const int e = L.edge[j], kf = ld(&R.A.obs_kf[e]), idx = ld(&R.M.obs_idx[e]);
      const uint32_t r = (uint32_t)R.G.rank[kf];
      move = !((L.has[r >> 5] >> (r & 31)) & 1u);                       // !pMP->IsInKeyFrame(pKF)
      if (move) {
        st(&R.A.kf_mp[(size_t)kf * S + idx], to);                       // ReplaceMapPointMatch
        st(&R.A.obs_mp[e], to);                                         // pMP->AddObservation(pKF, idx)
        if (e >= R.M.n_obs || R.home[e] != to) fz_link(R, to, e);
        key = (r << 15) | (uint32_t)idx;
      } else {
        st(&R.A.kf_mp[(size_t)kf * S + idx], -1);                       // EraseMapPointMatch
        st(&R.A.obs_kf[e], -1);
      }
    }
    const unsigned long long mask = __ballot(move);
    if (move) L.key[nt + __popcll(mask & ((1ull << lane) - 1ull))] = key;   // nt + nf <= 2 * cap
    nt += __popcll(mask);
  }
  if (lane == 0) {                                                      // :210-211
    st(&R.A.mp_found[to], (int32_t)((uint32_t)ld(&R.A.mp_found[to]) + (uint32_t)ld(&R.A.mp_found[from])));
    st(&R.A.mp_visible[to], (int32_t)((uint32_t)ld(&R.A.mp_visible[to]) + (uint32_t)ld(&R.A.mp_visible[from])));
    if (*n_rep < R.A.replaced_cap) { R.A.d_replaced[(size_t)*n_rep * 2] = from; R.A.d_replaced[(size_t)*n_rep * 2 + 1] = to; }
  }
  *n_rep += 1;
  fz_refresh(R, L, to, nt, lane);                                       // :212
}

__global__ __launch_bounds__(64) void k_fz_replace(FzRun R, fb_replace_points_args P, int key_cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pt_smem[];
  const FzLds L = fz_lds(pt_smem, R.cap, key_cap);
  const int lane = threadIdx.x;
  int n = P.n_pairs, n_rep = 0;
  if (P.d_n_pairs) n = min(max(*P.d_n_pairs, 0), n);
  for (int base = 0; base < n; base += 64) {
    const int from_l = base + lane < n ? P.d_from[base + lane] : -1;
    unsigned long long todo = __ballot(from_l >= 0);                    // from < 0: the NULL of vpReplacePoints
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int from = __shfl(from_l, b, 64), to = P.d_to[base + b];
      if (from >= R.M.n_mp || to < 0 || to >= R.M.n_mp) { if (lane == 0) atomicAdd(R.G.err, 1); continue; }
      fz_replace(R, L, from, to, lane, &n_rep);
    }
  }
  if (lane == 0) *R.A.d_n_replaced = n_rep;
}

// LoopClosing.cc:545-560.  The new edges go to [M.n_obs, M.n_obs + n_features) in the order they are made.
__global__ __launch_bounds__(64) void k_fz_loop_fuse(FzRun R, fb_loop_fuse_args P, int key_cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pt_smem[];
  const FzLds L = fz_lds(pt_smem, R.cap, key_cap);
  const int lane = threadIdx.x, cur = P.cur_slot, NF = P.n_features, S = R.M.kp_stride, e0 = R.M.n_obs;
  int n_rep = 0, n_new = 0;
  const bool ok = R.M.kf_n[cur] == NF;                                  // the host's N is the table's, or nothing is done
  if (!ok && lane == 0) atomicAdd(R.G.err, 1);
  for (int base = 0; ok && base < NF; base += 64) {
    const int m_l = base + lane < NF ? P.d_matched[base + lane] : -1;
    unsigned long long todo = __ballot(m_l >= 0);                       // :547
    while (todo) {
      const int b = __ffsll((long long)todo) - 1, i = base + b;
      todo &= todo - 1;
      const int loop = __shfl(m_l, b, 64);
      group_sync();
      const int have = ld(&R.A.kf_mp[(size_t)cur * S + i]);             // GetMapPoint(i), as it stands now
      if (loop >= R.M.n_mp || have >= R.M.n_mp) { if (lane == 0) atomicAdd(R.G.err, 1); continue; }
      if (have >= 0) { fz_replace(R, L, have, loop, lane, &n_rep); continue; }   // :552
      if (lane == 0) st(&R.A.kf_mp[(size_t)cur * S + i], loop);         // :555
      int nt = fz_keys(R, L, loop, lane);
      if (nt > R.cap) { if (lane == 0) atomicAdd(R.G.err, 1); continue; }
      const uint32_t r = (uint32_t)R.G.rank[cur];
      if (!((L.has[r >> 5] >> (r & 31)) & 1u)) {                        // MapPoint.cc:101
        const int e = e0 + n_new;
        if (lane == 0) {
          st(&R.A.obs_mp[e], loop); st(&R.A.obs_kf[e], cur); st(&R.obs_idx[e], i);
          fz_link(R, loop, e);
          L.key[nt] = (r << 15) | (uint32_t)i;
          if (n_new < P.added_cap) { int32_t *row = P.d_added + (size_t)n_new * 4; row[0] = cur; row[1] = loop; row[2] = i; row[3] = e; }
        }
        nt++; n_new++;
      }
      fz_refresh(R, L, loop, nt, lane);                                 // :557
    }
  }
  group_sync();
  for (int e = e0 + n_new + lane; e < e0 + NF; e += 64) { R.A.obs_mp[e] = -1; R.A.obs_kf[e] = -1; R.obs_idx[e] = -1; }
  if (lane == 0) { *P.d_n_added = n_new; *R.A.d_n_replaced = n_rep; }
}

// ---- SearchAndFuse (LoopClosing.cc:616-642) ----------------------------------------------------------------------------------
struct SafS {           // the scratch of one call, behind the log; one key frame's at a time
  int32_t *mark;        // [n_mp] k + 1: the point is in spAlreadyFound of key frame k
  fb_keypoint *kps; uint8_t *kdesc; int32_t *n_kf, *n_list; float *pose;   // the key frame as the search's batch of one
  int32_t *cell_start, *cell_items;
  uint8_t *valid; float *xw, *normal, *mind, *maxd; uint8_t *desc;         // the loop points as the search's lists
  int32_t *best, *rep;
};
void saf_map(uint8_t *b, const SafOff &o, SafS *S) {
  S->mark = (int32_t *)(b + o.mark); S->kps = (fb_keypoint *)(b + o.kps); S->kdesc = b + o.kdesc; S->n_kf = (int32_t *)(b + o.n_kf);
  S->n_list = (int32_t *)(b + o.n_list); S->pose = (float *)(b + o.pose); S->cell_start = (int32_t *)(b + o.cell_start);
  S->cell_items = (int32_t *)(b + o.cell_items); S->valid = b + o.valid; S->xw = (float *)(b + o.xw); S->normal = (float *)(b + o.normal);
  S->mind = (float *)(b + o.mind); S->maxd = (float *)(b + o.maxd); S->desc = b + o.desc; S->best = (int32_t *)(b + o.best);
  S->rep = (int32_t *)(b + o.rep);
}

// What the prepare kernels of SearchAndFuse and SearchInNeighbors (covis_neighbors.inc) share.  S: the scratch of the call
// (kps, kdesc; xw, normal, mind, maxd, desc, best), P: its arguments (the point getters and map.mp_desc).
// feature i of key frame `slot` as the search's batch of one reads it
template <typename Scr>
__device__ __forceinline__ void fz_stage_feature(const Scr &S, const fb_keypoint *kf_keys_un, const uint8_t *kf_desc, int slot, int St, int i) {
  S.kps[i] = kf_keys_un[(size_t)slot * St + i];
  const uint4 *src = reinterpret_cast<const uint4 *>(kf_desc + ((size_t)slot * St + i) * 32);
  uint4 *dst = reinterpret_cast<uint4 *>(S.kdesc + (size_t)i * 32);
  dst[0] = src[0]; dst[1] = src[1];
}
// point mp as entry i of the search's list: its getters and its descriptor as they stand
template <typename Scr, typename Args>
__device__ __forceinline__ void fz_stage_point(const Scr &S, const Args &P, int mp, int i) {
  for (int c = 0; c < 3; c++) { S.xw[i * 3 + c] = P.mp_xw[(size_t)mp * 3 + c]; S.normal[i * 3 + c] = P.mp_normal[(size_t)mp * 3 + c]; }
  S.mind[i] = P.mp_min_dist[mp]; S.maxd[i] = P.mp_max_dist[mp];
  const uint4 *src = reinterpret_cast<const uint4 *>(P.map.mp_desc + (size_t)mp * 32);
  uint4 *dst = reinterpret_cast<uint4 *>(S.desc + (size_t)i * 32);
  dst[0] = src[0]; dst[1] = src[1];
  S.best[i] = -1;
}

// Key frame k of the set as the search reads it, spAlreadyFound (:994) and the loop points with their skip rule (:1006), from
// the map as it stands.  One workgroup.
__global__ __launch_bounds__(CV_NT) void k_saf_prepare(fb_covis_map M, fb_search_and_fuse_args P, int k, SafS S, int32_t *err) {
  const int tid = threadIdx.x, St = M.kp_stride, slot = P.d_set_slots[k];
  if (slot < 0 || slot >= M.max_keyframes) {
    if (tid == 0) { atomicAdd(err, 1); *S.n_kf = 0; *S.n_list = 0; }
    return;
  }
  const int N = min(max(M.kf_n[slot], 0), St);
  for (int i = tid; i < St; i += CV_NT) {
    fz_stage_feature(S, P.kf_keys_un, P.map.kf_desc, slot, St, i);
    if (i < N) {
      const int p = M.kf_mp[(size_t)slot * St + i];
      if (p >= M.n_mp) atomicAdd(err, 1);
      else if (p >= 0 && !M.mp_bad[p]) st(&S.mark[p], k + 1);           // GetMapPoints(): the non-bad entries
    }
  }
  if (tid < 12) S.pose[tid] = P.d_set_Scw[(size_t)k * 12 + tid];
  if (tid == 0) { *S.n_kf = N; *S.n_list = P.n_loop; }
  group_sync();
  for (int i = tid; i < P.n_loop; i += CV_NT) {
    const int mp = P.d_loop_mp[i];
    if (mp < 0 || mp >= M.n_mp) { atomicAdd(err, 1); S.valid[i] = 0; continue; }
    S.valid[i] = (!M.mp_bad[mp] && ld(&S.mark[mp]) != k + 1) ? 1 : 0;
    fz_stage_point(S, P, mp, i);
  }
}

// The commit of Fuse (:1083-1097) serial in i, then the Replace loop (:633-640), for key frame k; one wave.
__global__ __launch_bounds__(64) void k_saf_commit(FzRun R, fb_search_and_fuse_args P, int k, SafS Sc, int key_cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pt_smem[];
  const FzLds L = fz_lds(pt_smem, R.cap, key_cap);
  const int lane = threadIdx.x, S = R.M.kp_stride, slot = P.d_set_slots[k], e0 = R.M.n_obs + k * S;
  int n_rep = k ? *R.A.d_n_replaced : 0, n_add = k ? *P.d_n_added : 0, n_new = 0, n_fused = 0;
  if (slot >= 0 && slot < R.M.max_keyframes) {
    const int N = *Sc.n_kf;
    const uint32_t r = (uint32_t)R.G.rank[slot];
    for (int base = 0; base < P.n_loop; base += 64) {
      const int i_l = base + lane;
      int b_l = -1;
      if (i_l < P.n_loop) {
        if (Sc.valid[i_l]) b_l = Sc.best[i_l];
        if (b_l >= N) b_l = -1;
        st(&Sc.rep[i_l], -1);
      }
      unsigned long long todo = __ballot(b_l >= 0);                     // bestDist <= TH_LOW
      while (todo) {
        const int b = __ffsll((long long)todo) - 1, i = base + b;
        todo &= todo - 1;
        const int best = __shfl(b_l, b, 64), loop = P.d_loop_mp[i];
        group_sync();
        const int have = ld(&R.A.kf_mp[(size_t)slot * S + best]);       // pKF->GetMapPoint(bestIdx), as it stands now
        if (have >= R.M.n_mp) { if (lane == 0) atomicAdd(R.G.err, 1); continue; }
        n_fused++;                                                      // :1096
        if (have >= 0) {
          if (lane == 0 && !ld(&R.A.mp_bad[have])) st(&Sc.rep[i], have);   // :1088-1089
          continue;
        }
        const int nt = fz_keys(R, L, loop, lane);
        if (nt <= R.cap && !((L.has[r >> 5] >> (r & 31)) & 1u) && n_new < S) {   // AddObservation, MapPoint.cc:101
          const int e = e0 + n_new;
          if (lane == 0) {
            st(&R.A.obs_mp[e], loop); st(&R.A.obs_kf[e], slot); st(&R.obs_idx[e], best);
            fz_link(R, loop, e);
            if (n_add < P.added_cap) { int32_t *row = P.d_added + (size_t)n_add * 4; row[0] = slot; row[1] = loop; row[2] = best; row[3] = e; }
          }
          n_new++; n_add++;
        } else if ((nt > R.cap || n_new >= S) && lane == 0) {           // (S adds fill the block: S distinct empty features at most)
          atomicAdd(R.G.err, 1);
        }
        if (lane == 0) st(&R.A.kf_mp[(size_t)slot * S + best], loop);   // AddMapPoint
      }
    }
    group_sync();
    for (int base = 0; base < P.n_loop; base += 64) {                   // LoopClosing.cc:633
      const int r_l = base + lane < P.n_loop ? ld(&Sc.rep[base + lane]) : -1;
      unsigned long long todo = __ballot(r_l >= 0);
      while (todo) {
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        fz_replace(R, L, __shfl(r_l, b, 64), P.d_loop_mp[base + b], lane, &n_rep);
      }
    }
  }
  group_sync();
  for (int e = e0 + n_new + lane; e < e0 + S; e += 64) { R.A.obs_mp[e] = -1; R.A.obs_kf[e] = -1; R.obs_idx[e] = -1; }
  if (lane == 0) { P.d_n_fused[k] = n_fused; *P.d_n_added = n_add; *R.A.d_n_replaced = n_rep; }
}

int fz_key_cap(int K) { return pow2_at_least(2 * K); }
size_t fz_lds_bytes(int K) { return (size_t)PT_STAGE * 32 + (size_t)fz_key_cap(K) * 4 + (size_t)K * 4 + (size_t)((K + 31) / 32) * 4 + 16; }

int check_point_fuse(const fb_covis_map *M, const fb_point_fuse_arrays *a) {
  FB_ARG(a->kf_mp && a->kf_bad && a->kf_desc && a->d_n_replaced);
  FB_ARG(M->n_mp == 0 || (a->mp_bad && a->mp_found && a->mp_visible && a->mp_replaced && a->mp_desc));
  FB_ARG(M->n_obs == 0 || (a->obs_mp && a->obs_kf));
  FB_ARG(a->replaced_cap >= 0 && (a->replaced_cap == 0 || a->d_replaced));
  FB_ARG((size_t)M->max_keyframes * (size_t)M->kp_stride < (size_t)UINT32_MAX);   // a row of kf_desc is kept in 32 bits
  return FB_OK;
}
// the arrays the call edits are the map's own: the caller goes on with the map's pointers
int check_point_fuse_own(const fb_covis_map *M, const fb_point_fuse_arrays *a, bool edges) {
  FB_ARG(a->kf_mp == M->kf_mp && (M->n_mp == 0 || a->mp_bad == M->mp_bad));
  FB_ARG(!edges || (a->obs_mp == M->obs_mp && a->obs_kf == M->obs_kf));
  FB_ARG(((uintptr_t)a->kf_desc & 15) == 0 && ((uintptr_t)a->mp_desc & 15) == 0);
  return FB_OK;
}

int check_replace(const fb_covis_map *M, const fb_replace_points_args *a) {
  FB_ARG(a);
  FB_ARG(a->n_pairs >= 0 && (a->n_pairs == 0 || (a->d_from && a->d_to)));
  return check_point_fuse(M, &a->map);
}

int check_loop_fuse(const fb_covis *g, const fb_covis_map *M, const fb_loop_fuse_args *a) {
  FB_ARG(a);
  FB_ARG(a->cur_slot >= 0 && a->cur_slot < g->K);
  FB_ARG(a->n_features >= 0 && a->n_features <= M->kp_stride && (a->n_features == 0 || a->d_matched));
  FB_ARG(a->obs_cap >= 0 && a->d_n_added && a->added_cap >= 0 && (a->added_cap == 0 || a->d_added));
  if ((int64_t)M->n_obs + a->n_features > (int64_t)a->obs_cap) {
    fb::set_error("fb_covis_loop_fuse: %d edges and %d features do not fit obs_cap = %d", M->n_obs, a->n_features, a->obs_cap);
    return FB_ERR_CAPACITY;
  }
  FB_ARG(a->obs_cap == 0 || (a->obs_idx && a->map.obs_mp && a->map.obs_kf));
  return check_point_fuse(M, &a->map);
}

int check_search_and_fuse(const fb_covis *g, const fb_covis_map *M, const fb_search_and_fuse_args *a) {
  FB_ARG(a);
  FB_ARG(a->n_set >= 0 && a->n_set <= g->K && (a->n_set == 0 || (a->d_set_slots && a->d_set_Scw && a->d_n_fused)));
  FB_ARG(a->n_loop >= 0 && (a->n_loop == 0 || a->d_loop_mp));
  FB_ARG(a->n_levels >= 1 && a->n_levels <= FB_MAX_LEVELS && a->grid.cols > 0 && a->grid.rows > 0 && a->kf_keys_un);
  FB_ARG(M->n_mp == 0 || (a->mp_xw && a->mp_normal && a->mp_min_dist && a->mp_max_dist));
  FB_ARG(a->obs_cap >= 0 && a->d_n_added && a->added_cap >= 0 && (a->added_cap == 0 || a->d_added));
  if ((int64_t)M->n_obs + (int64_t)a->n_set * M->kp_stride > (int64_t)a->obs_cap) {
    fb::set_error("fb_covis_search_and_fuse: %d edges and %d key frames of %d features do not fit obs_cap = %d", M->n_obs, a->n_set,
                  M->kp_stride, a->obs_cap);
    return FB_ERR_CAPACITY;
  }
  FB_ARG(a->obs_cap == 0 || (a->obs_idx && a->map.obs_mp && a->map.obs_kf));
  return check_point_fuse(M, &a->map);
}

// the index of M, the log behind it, and the walk's arguments
// (n_q: counter rows the index is sized with, for a call that builds it again at the same place for an UpdateConnections)
int fz_begin(fb_covis *g, const fb_covis_map *M, const fb_point_fuse_arrays &A, size_t n_new, FzRun *R, hipStream_t s, size_t more = 0,
             uint8_t **more_at = nullptr, size_t n_q = 0) {
  FzOff fo;
  IndexAsk ask;
  ask.n_q = n_q;
  const size_t log_bytes = plan_point_fuse(M->n_mp, M->n_obs, n_new, &fo);
  ask.tail = log_bytes + more;
  Index ix;
  uint8_t *b;
  FB_TRY(g->acquire(*M, ask, &ix, &b, s));
  scratch_drop_index(g->state);                                         // edges change owner: a later reuse_index rebuilds
  R->M = *M; R->G = g->G; R->start = ix.start; R->csr = ix.csr;
  R->head = (int32_t *)(b + fo.head); R->next = (int32_t *)(b + fo.next); R->home = (const int32_t *)(b + fo.home);
  R->A = A; R->obs_idx = nullptr; R->cap = g->K;
  if (more_at) *more_at = b + log_bytes;
  if (M->n_mp) FB_HIP(hipMemsetAsync(R->head, 0xff, (size_t)M->n_mp * 4, s));
  if (M->n_obs) FB_HIP(hipMemcpyAsync(b + fo.home, M->obs_mp, (size_t)M->n_obs * 4, hipMemcpyDeviceToDevice, s));
  return FB_OK;
}

void stage_point_fuse(fb::Stager &st, fb_covis_map &M, fb_point_fuse_arrays &A, size_t n_edges) {
  const size_t K = M.max_keyframes, S = M.kp_stride, n_mp = M.n_mp;
  st.in(M.kf_n, K * 4); st.in(M.kf_octave, K * S); st.in(M.kf_order, K * 8);
  st.in(A.kf_bad, K); st.in(A.kf_desc, K * S * 32);
  // the arrays the call edits are the map's: staged once
  st.out(A.kf_mp, K * S * 4, true); st.out(A.mp_bad, n_mp, true); st.out(A.obs_mp, n_edges * 4, true); st.out(A.obs_kf, n_edges * 4, true);
  st.out(A.mp_found, n_mp * 4, true); st.out(A.mp_visible, n_mp * 4, true); st.out(A.mp_replaced, n_mp * 4, true);
  st.out(A.mp_desc, n_mp * 32, true);
  st.out(A.d_n_replaced, 4, false); st.out(A.d_replaced, (size_t)A.replaced_cap * 8, true);
}

}  // namespace

extern "C" {

int fb_covis_reserve_replace_points(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && n_q >= 0 && n_q <= g->K);
  FzOff fo;
  return g->reserve(plan_map_call(g->K, n_mp, n_obs, n_q, plan_point_fuse(n_mp, n_obs, 0, &fo)));
}

int fb_covis_replace_points_dev(fb_covis *g, const fb_covis_map *M, const fb_replace_points_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_replace(M, a));
  FB_TRY(check_point_fuse_own(M, &a->map, M->n_obs != 0));
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  FzRun R;
  FB_TRY(fz_begin(g, M, a->map, 0, &R, s));
  k_fz_replace<<<1, 64, fz_lds_bytes(g->K), s>>>(R, *a, fz_key_cap(g->K));
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_replace_points(fb_covis *g, const fb_covis_map *HM, const fb_replace_points_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_TRY(check_replace(HM, ha));
  FB_ARG(!ha->d_n_pairs);
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_replace_points_args A = *ha;
  fb::Stager st;
  st.in(M.obs_idx, (size_t)M.n_obs * 4);
  st.in(A.d_from, (size_t)A.n_pairs * 4); st.in(A.d_to, (size_t)A.n_pairs * 4);
  stage_point_fuse(st, M, A.map, (size_t)M.n_obs);
  FB_TRY(st.commit(nullptr));
  M.kf_mp = A.map.kf_mp; M.mp_bad = A.map.mp_bad; M.obs_mp = A.map.obs_mp; M.obs_kf = A.map.obs_kf;
  IndexDropGuard drop(g->state);
  FB_TRY(fb_covis_replace_points_dev(g, &M, &A, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_reserve_loop_fuse(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t n_features) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && n_q >= 0 && n_q <= g->K && n_features >= 0);
  FzOff fo;
  return g->reserve(plan_map_call(g->K, n_mp, n_obs, n_q, plan_point_fuse(n_mp, n_obs, n_features, &fo)));
}

int fb_covis_loop_fuse_dev(fb_covis *g, const fb_covis_map *M, const fb_loop_fuse_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_loop_fuse(g, M, a));
  // the block is written through a->..., and the caller goes on with the map's own pointers: they must be the same arrays
  FB_TRY(check_point_fuse_own(M, &a->map, a->obs_cap != 0));
  FB_ARG(a->obs_cap == 0 || a->obs_idx == M->obs_idx);
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  FzRun R;
  FB_TRY(fz_begin(g, M, a->map, (size_t)a->n_features, &R, s));
  R.obs_idx = a->obs_idx;
  k_fz_loop_fuse<<<1, 64, fz_lds_bytes(g->K), s>>>(R, *a, fz_key_cap(g->K));
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_loop_fuse(fb_covis *g, const fb_covis_map *HM, const fb_loop_fuse_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_TRY(check_loop_fuse(g, HM, ha));
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_loop_fuse_args A = *ha;
  const size_t n_edges = (size_t)M.n_obs + (size_t)A.n_features;
  fb::Stager st;
  st.in(A.d_matched, (size_t)A.n_features * 4);
  stage_point_fuse(st, M, A.map, n_edges);
  st.out(A.obs_idx, n_edges * 4, true);
  st.out(A.d_n_added, 4, false); st.out(A.d_added, (size_t)A.added_cap * 16, true);
  FB_TRY(st.commit(nullptr));
  M.kf_mp = A.map.kf_mp; M.mp_bad = A.map.mp_bad; M.obs_mp = A.map.obs_mp; M.obs_kf = A.map.obs_kf; M.obs_idx = A.obs_idx;
  IndexDropGuard drop(g->state);
  FB_TRY(fb_covis_loop_fuse_dev(g, &M, &A, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_reserve_search_and_fuse(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t kp_stride, int32_t n_set, int32_t n_loop,
                                     int32_t grid_cells) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && n_q >= 0 && n_q <= g->K && n_set >= 0 && n_set <= g->K && n_loop >= 0 && grid_cells >= 0);
  FB_ARG(kp_stride >= 1 && kp_stride <= FB_COVIS_MAX_STRIDE);
  FzOff fo;
  SafOff so;
  const size_t S = kp_stride;
  return g->reserve(plan_map_call(g->K, n_mp, n_obs, n_q, plan_point_fuse(n_mp, n_obs, (size_t)n_set * S, &fo) +
                                                              plan_search_and_fuse(n_mp, S, n_loop, grid_cells, &so)));
}

int fb_covis_search_and_fuse_dev(fb_covis *g, const fb_covis_map *M, const fb_search_and_fuse_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_search_and_fuse(g, M, a));
  FB_TRY(check_point_fuse_own(M, &a->map, a->obs_cap != 0));
  FB_ARG(a->obs_cap == 0 || a->obs_idx == M->obs_idx);
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  FB_HIP(hipMemsetAsync(a->d_n_added, 0, 4, s));
  FB_HIP(hipMemsetAsync(a->map.d_n_replaced, 0, 4, s));
  if (a->n_set == 0) return FB_OK;
  const size_t S = M->kp_stride, cells = (size_t)a->grid.cols * a->grid.rows;
  SafOff so;
  const size_t more = plan_search_and_fuse(M->n_mp, S, a->n_loop, cells, &so);
  FzRun R;
  uint8_t *b;
  FB_TRY(fz_begin(g, M, a->map, (size_t)a->n_set * S, &R, s, more, &b));
  R.obs_idx = a->obs_idx;
  SafS Sc;
  saf_map(b, so, &Sc);
  if (M->n_mp) FB_HIP(hipMemsetAsync(Sc.mark, 0, (size_t)M->n_mp * 4, s));
  fb_fuse_args F;
  memset(&F, 0, sizeof(F));
  F.batch = 1; F.th = a->th; F.pose = Sc.pose; F.best_idx = Sc.best;
  F.kf.kf_stride = (int32_t)S; F.kf.n_kf = Sc.n_kf; F.kf.kf_kps = Sc.kps; F.kf.kf_desc = Sc.kdesc; F.kf.kf_cell_start = Sc.cell_start;
  F.kf.kf_cell_items = Sc.cell_items; F.kf.cam = a->cam; F.kf.grid = a->grid; F.kf.log_scale_factor = a->log_scale_factor;
  F.kf.n_levels = a->n_levels;
  memcpy(F.kf.scale_factors, a->scale_factors, sizeof(F.kf.scale_factors));
  memcpy(F.kf.inv_level_sigma2, a->inv_level_sigma2, sizeof(F.kf.inv_level_sigma2));
  F.mp.mp_stride = a->n_loop; F.mp.n_mp = Sc.n_list; F.mp.mp_valid = Sc.valid; F.mp.mp_xw = Sc.xw; F.mp.mp_normal = Sc.normal;
  F.mp.mp_max_dist = Sc.maxd; F.mp.mp_min_dist = Sc.mind; F.mp.mp_desc = Sc.desc;
  for (int k = 0; k < a->n_set; k++) {                                  // four launches per key frame, no host wait
    if (a->n_loop) {                                                    // no loop point: the commit alone leaves nFused = 0 and tombstones
      k_saf_prepare<<<1, CV_NT, 0, s>>>(*M, *a, k, Sc, g->G.err);
      FB_HIP(hipGetLastError());
      FB_TRY(fb_grid_build_batch_dev(Sc.kps, Sc.n_kf, 1, (int)S, &a->grid, Sc.cell_start, Sc.cell_items, stream));
      FB_TRY(fb_fuse_sim3_search_dev(&F, stream));
    }
    k_saf_commit<<<1, 64, fz_lds_bytes(g->K), s>>>(R, *a, k, Sc, fz_key_cap(g->K));
    FB_HIP(hipGetLastError());
  }
  return FB_OK;
}

int fb_covis_search_and_fuse(fb_covis *g, const fb_covis_map *HM, const fb_search_and_fuse_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_TRY(check_search_and_fuse(g, HM, ha));
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_search_and_fuse_args A = *ha;
  const size_t K = g->K, S = M.kp_stride, n_mp = M.n_mp, n_edges = (size_t)M.n_obs + (size_t)A.n_set * S;
  fb::Stager st;
  st.in(A.d_set_slots, (size_t)A.n_set * 4); st.in(A.d_set_Scw, (size_t)A.n_set * 48); st.in(A.d_loop_mp, (size_t)A.n_loop * 4);
  st.in(A.kf_keys_un, K * S * sizeof(fb_keypoint));
  st.in(A.mp_xw, n_mp * 12); st.in(A.mp_normal, n_mp * 12); st.in(A.mp_min_dist, n_mp * 4); st.in(A.mp_max_dist, n_mp * 4);
  stage_point_fuse(st, M, A.map, n_edges);
  st.out(A.obs_idx, n_edges * 4, true);
  st.out(A.d_n_fused, (size_t)A.n_set * 4, false);
  st.out(A.d_n_added, 4, false); st.out(A.d_added, (size_t)A.added_cap * 16, true);
  FB_TRY(st.commit(nullptr));
  M.kf_mp = A.map.kf_mp; M.mp_bad = A.map.mp_bad; M.obs_mp = A.map.obs_mp; M.obs_kf = A.map.obs_kf; M.obs_idx = A.obs_idx;
  IndexDropGuard drop(g->state);
  FB_TRY(fb_covis_search_and_fuse_dev(g, &M, &A, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
