// covis_window.inc -- the local-BA window collected from the covisibility graph (included at the end of covis.hip: it
// shares Gr, Index and the CSR build).
//
// Replaces (reference file:line):
//   Optimizer::LocalBundleAdjustment[WithOdom], the window          src/Optimizer.cc:838-889, :2139-2227
//   the vertex and edge loops (what they read of the map)            :2245-2284, :2312-2417
//   the write-back and the erase lists                               :2574-2669
//
// The reference's three serial walks mark what they have seen (mnBALocalForKF / mnBAFixedForKF); here each "first
// occurrence" is a minimum over position keys, which no order of execution changes:
//   local points   atomicMin over (position of the key frame in the local list) * stride + feature, per point;
//   fixed cameras  64-bit atomicMin over (side << 44 | position of the point << 12 | rank of kf_order), per key frame;
//   edges          per point, the rank of an edge among the point's edges of non-bad key frames.
// Everything is integer work plus copied floats and is compared for equality with tests/local_window_ref.py.

namespace {

constexpr int WIN_NT = 256;
constexpr int32_t WIN_NOKEY = 0x7f7f7f7f;                 // what hipMemset(0x7f) leaves: above every position key (< 2^27)
constexpr uint64_t WIN_NOFIX = ~0ull;
enum { WH_LOCAL = 0, WH_FIXED, WH_MP, WH_OBS, WH_MPB, WH_BOBS, WH_OVERFLOW, WH_COUNT };
enum { LP_NONE = -1, LP_BAD_NEIGHBOUR = -2 };

struct WinSide {        // the scratch of one side (front: MapPoint, bird: MapPointBird)
  int32_t *ptkey;       // [n_pt] the smallest position key of the point among the local key frames' features
  int32_t *plist;       // [n_pt] the local points in list order
  int32_t *eoff;        // [n_pt + 1] edges per local point, then their exclusive scan
  int32_t *bsum;
};

struct WinS {           // the scratch of one window
  int32_t *hdr;         // [WH_COUNT]
  int32_t *lpos;        // [K] position in the local list, LP_NONE, LP_BAD_NEIGHBOUR
  int32_t *widx;        // [K] index in the window's key frame list, -1 = not in it
  int32_t *wslot;       // [K] that list
  uint8_t *wfixed;      // [K]
  uint64_t *fixkey;     // [K]
  int32_t *rowcnt;      // [K] new local points per local key frame, then their exclusive scan
  WinSide side[2];
};

struct WinOut {         // one side of fb_covis_window
  int cap_pt, cap_e;
  int32_t *pt_index; float *pt_xw;
  int32_t *e_kf, *e_pt, *e_src;
  float *e_meas, *e_inv_sigma2;
};

__global__ __launch_bounds__(CV_NT) void k_win_local(Gr G, int cur, const uint8_t *kf_bad, WinS W) {
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x, K = G.K;
  for (int b = tid; b < K; b += CV_NT) { W.lpos[b] = LP_NONE; W.widx[b] = -1; W.wslot[b] = -1; W.wfixed[b] = 0; W.fixkey[b] = WIN_NOFIX; }
  if (tid < WH_COUNT) W.hdr[tid] = 0;
  group_sync();
  const int n = row_sorted(G, cur, LIST_ORDERED, s_key, s_wv);
  if (tid == 0) { W.lpos[cur] = 0; W.wslot[0] = cur; }
  int carry = 1;
  for (int base = 0; base < n; base += CV_NT) {
    const int p = base + tid;
    const int kf = p < n ? G.inv[(~s_key[p]) & 4095] : cur;
    const int take = (kf != cur && !kf_bad[kf]) ? 1 : 0;            // :2150
    int total;
    const int ex = fb::block_excl_scan<CV_NT>(take, s_wv, &total);
    if (take) { W.lpos[kf] = carry + ex; W.wslot[carry + ex] = kf; }
    else if (kf != cur) W.lpos[kf] = LP_BAD_NEIGHBOUR;              // marked at :2149, so never a fixed camera
    carry += total;
    __syncthreads();
  }
  if (tid == 0) W.hdr[WH_LOCAL] = carry;
}

// the first occurrence of every point: the smallest (local position, feature)
__global__ __launch_bounds__(WIN_NT) void k_win_mark(fb_covis_map M, WinS W, int sd, int32_t *err) {
  const int p = blockIdx.x;
  if (p >= W.hdr[WH_LOCAL]) return;
  const int kf = W.wslot[p], S = M.kp_stride, n = min(max(M.kf_n[kf], 0), S);
  const int32_t *mps = M.kf_mp + (size_t)kf * S;
  for (int i = threadIdx.x; i < n; i += WIN_NT) {
    const int mp = mps[i];
    if (mp < 0) continue;
    if (mp >= M.n_mp) { atomicAdd(err, 1); continue; }
    if (M.mp_bad[mp]) continue;
    atomicMin(&W.side[sd].ptkey[mp], p * S + i);
  }
}

__device__ __forceinline__ bool win_first(const fb_covis_map &M, const int32_t *ptkey, const int32_t *mps, int p, int i, int n) {
  if (i >= n) return false;
  const int mp = mps[i];
  return mp >= 0 && mp < M.n_mp && !M.mp_bad[mp] && ptkey[mp] == p * M.kp_stride + i;
}

__global__ __launch_bounds__(WIN_NT) void k_win_rowcount(fb_covis_map M, WinS W, int sd) {
  __shared__ int s_wv[WIN_NT / 64];
  const int p = blockIdx.x;
  if (p >= W.hdr[WH_LOCAL]) return;
  const int kf = W.wslot[p], S = M.kp_stride, n = min(max(M.kf_n[kf], 0), S);
  const int32_t *mps = M.kf_mp + (size_t)kf * S;
  int c = 0;
  for (int i = threadIdx.x; i < n; i += WIN_NT) c += win_first(M, W.side[sd].ptkey, mps, p, i, n) ? 1 : 0;
  c = fb::block_sum<WIN_NT>(c, s_wv);
  if (threadIdx.x == 0) W.rowcnt[p] = c;
}

__global__ __launch_bounds__(CV_NT) void k_win_rowscan(WinS W, int sd) {
  __shared__ int s_wv[CV_NT / 64];
  const int n = W.hdr[WH_LOCAL];
  int carry = 0;
  for (int base = 0; base < n; base += CV_NT) {
    const int i = base + threadIdx.x;
    const int v = i < n ? W.rowcnt[i] : 0;
    int total;
    const int ex = fb::block_excl_scan<CV_NT>(v, s_wv, &total);
    if (i < n) W.rowcnt[i] = carry + ex;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) W.hdr[sd ? WH_MPB : WH_MP] = carry;
}

// the local points take their places; their indices and positions go out
__global__ __launch_bounds__(WIN_NT) void k_win_place(fb_covis_map M, WinS W, int sd, const float *xw, WinOut O) {
  __shared__ int s_wv[WIN_NT / 64];
  const int p = blockIdx.x;
  if (p >= W.hdr[WH_LOCAL]) return;
  const int kf = W.wslot[p], S = M.kp_stride, n = min(max(M.kf_n[kf], 0), S);
  const int32_t *mps = M.kf_mp + (size_t)kf * S;
  int carry = W.rowcnt[p];
  for (int base = 0; base < n; base += WIN_NT) {
    const int i = base + threadIdx.x;
    const bool first = win_first(M, W.side[sd].ptkey, mps, p, i, n);
    int total;
    const int ex = fb::block_excl_scan<WIN_NT>(first ? 1 : 0, s_wv, &total);
    if (first) {
      const int mp = mps[i], pos = carry + ex;          // pos < the number of points: every point is first at one feature
      W.side[sd].plist[pos] = mp;
      if (pos < O.cap_pt) {
        O.pt_index[pos] = mp;
        if (O.pt_xw) for (int c = 0; c < 3; c++) O.pt_xw[(size_t)pos * 3 + c] = xw[(size_t)mp * 3 + c];   // (the local map lists indices only)
      }
    }
    carry += total;
    __syncthreads();
  }
}

// one wave per local point: its edges of non-bad key frames are counted, its non-local observers bid for a place among
// the fixed cameras
__global__ __launch_bounds__(WIN_NT) void k_win_observers(fb_covis_map M, Gr G, const int32_t *start, const int32_t *csr, const uint8_t *kf_bad,
                                                          WinS W, int sd) {
  const int j = blockIdx.x * (WIN_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= W.hdr[sd ? WH_MPB : WH_MP]) return;
  const int mp = W.side[sd].plist[j], s1 = start[mp + 1];
  int c = 0;
  for (int q = start[mp] + lane; q < s1; q += 64) {
    const int kf = M.obs_kf[csr[q]];                     // in [0, K): the index holds checked edges only
    if (kf_bad[kf]) continue;                            // :2184, :2332
    c++;
    if (W.lpos[kf] == LP_NONE)
      atomicMin((unsigned long long *)&W.fixkey[kf], ((unsigned long long)sd << 44) | ((unsigned long long)j << 12) | (unsigned long long)G.rank[kf]);
  }
  c = fb::wave_sum(c);
  if (lane == 0) W.side[sd].eoff[j] = c;
}

// lFixedCameras = the bids in ascending order; the slot -> window index table; the key frame arrays go out
__global__ __launch_bounds__(CV_NT) void k_win_fixed(Gr G, WinS W, fb_covis_kf_tables T, fb_covis_window O) {
  __shared__ uint64_t s_key[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x, K = G.K, n_local = W.hdr[WH_LOCAL];
  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  int cnt = 0;
  for (int i = tid; i < n2; i += CV_NT) {
    const uint64_t k = i < K ? W.fixkey[i] : WIN_NOFIX;
    s_key[i] = k;
    cnt += k != WIN_NOFIX ? 1 : 0;
    if (i < K) {
      const int lp = W.lpos[i];
      W.widx[i] = lp >= 0 ? lp : -1;
      if (lp >= 0) W.wfixed[lp] = T.kf_init[i] ? 1 : 0;             // :2260
    }
  }
  const int n_fixed = fb::block_sum<CV_NT>(cnt, s_wv);
  __syncthreads();
  fb::bitonic_sort(s_key, n2, tid, CV_NT);
  for (int f = tid; f < n_fixed; f += CV_NT) {
    const int kf = G.inv[s_key[f] & 4095];
    W.widx[kf] = n_local + f; W.wslot[n_local + f] = kf; W.wfixed[n_local + f] = 1;   // n_local + n_fixed <= K: disjoint sets of slots
  }
  if (tid == 0) W.hdr[WH_FIXED] = n_fixed;
  group_sync();
  const int n_out = min(n_local + n_fixed, (int)O.cap_kf);
  for (int w = tid; w < n_out; w += CV_NT) { O.kf_slot[w] = W.wslot[w]; O.kf_fixed[w] = W.wfixed[w]; }
  for (int t = tid; t < n_out * 12; t += CV_NT) O.kf_Tcw[t] = T.kf_Tcw[(size_t)W.wslot[t / 12] * 12 + t % 12];
}

__device__ __forceinline__ uint64_t win_edge_key(const fb_covis_map &M, const Gr &G, const int32_t *csr, const uint8_t *kf_bad, int q, int s1) {
  if (q >= s1) return ~0ull;
  const int e = csr[q], kf = M.obs_kf[e];
  return kf_bad[kf] ? ~0ull : ((uint64_t)G.rank[kf] << 32) | (uint32_t)e;
}

// one wave per local point: each edge's place is the number of the point's edges before it in std::map order, found
// against tiles of 64 edges held one per lane -- no bound on a point's degree
__global__ __launch_bounds__(WIN_NT) void k_win_edges(fb_covis_map M, Gr G, const int32_t *start, const int32_t *csr, fb_covis_kf_tables T, WinS W,
                                                      int sd, WinOut O, int32_t *err) {
  const int j = blockIdx.x * (WIN_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= W.hdr[sd ? WH_MPB : WH_MP]) return;
  const int mp = W.side[sd].plist[j], s0 = start[mp], s1 = start[mp + 1], o0 = W.side[sd].eoff[j], S = M.kp_stride;
  for (int c0 = s0; c0 < s1; c0 += 64) {
    const uint64_t mine = win_edge_key(M, G, csr, T.kf_bad, c0 + lane, s1);
    int pos = 0;
    for (int t0 = s0; t0 < s1; t0 += 64) {
      const uint64_t theirs = win_edge_key(M, G, csr, T.kf_bad, t0 + lane, s1);
      const int m = min(64, s1 - t0);
      for (int l = 0; l < m; l++) pos += (uint64_t)__shfl((unsigned long long)theirs, l, 64) < mine ? 1 : 0;
    }
    if (mine == ~0ull) continue;
    const int o = o0 + pos;                                // < o0 + the point's count: the keys of a point are distinct
    if (o >= O.cap_e) continue;
    const int e = (int)(uint32_t)mine, kf = M.obs_kf[e];
    const size_t f = (size_t)kf * S + M.obs_idx[e];
    O.e_kf[o] = W.widx[kf]; O.e_pt[o] = j; O.e_src[o] = e;
    int oct;
    if (sd == 0) {
      const fb_keypoint kp = T.kf_keys_un[f];
      O.e_meas[(size_t)o * 2] = kp.x; O.e_meas[(size_t)o * 2 + 1] = kp.y;
      oct = kp.octave;
    } else {
      for (int c = 0; c < 3; c++) O.e_meas[(size_t)o * 3 + c] = T.kf_bird_xc[f * 3 + c];
      oct = M.kf_octave[f];
    }
    if (oct < 0 || oct >= T.n_levels) { atomicAdd(err, 1); oct = min(max(oct, 0), T.n_levels - 1); }
    O.e_inv_sigma2[o] = T.inv_level_sigma2[oct];
  }
}

__global__ void k_win_header(WinS W, const int32_t *total_obs, const int32_t *total_bobs, fb_covis_window O) {
  if (threadIdx.x || blockIdx.x) return;
  int32_t *h = W.hdr;
  h[WH_OBS] = *total_obs;
  h[WH_BOBS] = total_bobs ? *total_bobs : 0;
  h[WH_OVERFLOW] = (h[WH_LOCAL] + h[WH_FIXED] > O.cap_kf || h[WH_MP] > O.cap_mp || h[WH_OBS] > O.cap_obs || h[WH_MPB] > O.cap_mpb ||
                    h[WH_BOBS] > O.cap_bobs) ? 1 : 0;
  int32_t *out = reinterpret_cast<int32_t *>(O.header);
  for (int i = 0; i < WH_COUNT; i++) out[i] = h[i];
}

// ---- after the optimisation -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WIN_NT) void k_win_scatter(fb_covis_map M, fb_covis_kf_tables T, fb_covis_window O, int K) {
  const fb_covis_window_header h = *O.header;
  if (h.overflow) return;
  const int t = blockIdx.x * WIN_NT + threadIdx.x;
  if (t < h.n_local * 12) {
    const int kf = O.kf_slot[t / 12];
    if (kf >= 0 && kf < K) T.kf_Tcw[(size_t)kf * 12 + t % 12] = O.kf_Tcw[t];
  }
  if (t < h.n_mp * 3) {
    const int mp = O.mp_index[t / 3];
    if (mp >= 0 && mp < M.n_mp) T.mp_xw[(size_t)mp * 3 + t % 3] = O.mp_xw[t];
  }
  if (t < h.n_mpb * 3) {
    const int mp = O.mpb_index[t / 3];
    if (mp >= 0 && mp < T.n_mpb) T.mpb_xw[(size_t)mp * 3 + t % 3] = O.mpb_xw[t];
  }
}

// vToErase / vToEraseBird in edge order: block 0 the front edges, block 1 the bird edges
__global__ __launch_bounds__(CV_NT) void k_win_erase(fb_covis_map M, fb_covis_kf_tables T, fb_covis_window O, int K, const uint8_t *outl,
                                                     const uint8_t *boutl, int32_t *n_erase, int32_t *erase, int32_t *berase) {
  __shared__ int s_wv[CV_NT / 64];
  const fb_covis_window_header h = *O.header;
  const int sd = blockIdx.x, n_kf = h.n_local + h.n_fixed;
  const uint8_t *flag = sd ? boutl : outl;
  const int n = (h.overflow || !flag) ? 0 : (sd ? h.n_bobs : h.n_obs);
  const int32_t *e_kf = sd ? O.bobs_kf : O.obs_kf, *e_pt = sd ? O.bobs_mpb : O.obs_mp, *e_src = sd ? O.bobs_src : O.obs_src;
  const int32_t *pt_index = sd ? O.mpb_index : O.mp_index, *src_idx = sd ? T.bobs_idx : M.obs_idx;
  const int n_pt = sd ? h.n_mpb : h.n_mp, n_src = sd ? T.n_bobs : M.n_obs;
  int32_t *rows = sd ? berase : erase;
  int carry = 0;
  for (int base = 0; base < n; base += CV_NT) {
    const int o = base + threadIdx.x;
    const bool out = o < n && flag[o];
    int total;
    const int ex = fb::block_excl_scan<CV_NT>(out ? 1 : 0, s_wv, &total);
    if (out) {
      const int w = e_kf[o], j = e_pt[o], e = e_src[o];
      int32_t *r = rows + (size_t)(carry + ex) * 4;      // carry + ex <= o < the capacity of the edge arrays
      r[0] = w >= 0 && w < n_kf ? O.kf_slot[w] : -1;
      r[1] = j >= 0 && j < n_pt ? pt_index[j] : -1;
      r[2] = e >= 0 && e < n_src ? src_idx[e] : -1;
      r[3] = e;
    }
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) n_erase[sd] = carry;
}

void win_map(uint8_t *b, const WinOff &o, WinS *W) {
  W->hdr = (int32_t *)(b + o.hdr);
  W->lpos = (int32_t *)(b + o.lpos); W->widx = (int32_t *)(b + o.widx); W->wslot = (int32_t *)(b + o.wslot);
  W->rowcnt = (int32_t *)(b + o.rowcnt); W->wfixed = b + o.wfixed; W->fixkey = (uint64_t *)(b + o.fixkey);
  for (int sd = 0; sd < 2; sd++) {
    W->side[sd].ptkey = (int32_t *)(b + o.side[sd].ptkey); W->side[sd].plist = (int32_t *)(b + o.side[sd].plist);
    W->side[sd].eoff = (int32_t *)(b + o.side[sd].eoff); W->side[sd].bsum = (int32_t *)(b + o.side[sd].bsum);
  }
}

bool win_has_bird(const fb_covis_kf_tables *T, int with_bird) { return with_bird && T->bobs_kf; }

// the bird side as a fb_covis_map: MapPointBird in the place of MapPoint
fb_covis_map win_bird_map(const fb_covis_map &M, const fb_covis_kf_tables &T) {
  fb_covis_map B = M;
  B.kp_stride = T.bird_stride; B.kf_n = T.kf_nb; B.kf_mp = T.kf_mpb; B.kf_octave = T.kf_bird_octave;
  B.n_mp = T.n_mpb; B.mp_bad = T.mpb_bad; B.n_obs = T.n_bobs; B.obs_mp = T.bobs_mpb; B.obs_kf = T.bobs_kf; B.obs_idx = T.bobs_idx;
  return B;
}

int check_tables(const fb_covis_map *M, const fb_covis_kf_tables *T, bool bird) {
  FB_ARG(T);
  FB_ARG(T->kf_Tcw && T->kf_bad && T->kf_init && T->kf_keys_un && T->inv_level_sigma2);
  FB_ARG(T->n_levels >= 1 && T->n_levels <= FB_MAX_LEVELS);
  FB_ARG(M->n_mp == 0 || T->mp_xw);
  if (bird) {
    FB_ARG(T->bird_stride >= 1 && T->bird_stride <= FB_COVIS_MAX_STRIDE);
    FB_ARG(T->n_mpb >= 0 && T->n_mpb < INT_MAX && T->n_bobs >= 0);
    FB_ARG(T->kf_nb && T->kf_mpb && T->kf_bird_octave && T->kf_bird_xc);
    FB_ARG(T->n_mpb == 0 || (T->mpb_bad && T->mpb_xw));
    FB_ARG(T->n_bobs == 0 || (T->bobs_mpb && T->bobs_idx));
  }
  return FB_OK;
}

int check_window(const fb_covis_window *O, bool bird) {
  FB_ARG(O && O->header);
  FB_ARG(O->cap_kf >= 0 && O->cap_mp >= 0 && O->cap_obs >= 0 && O->cap_mpb >= 0 && O->cap_bobs >= 0);
  FB_ARG(O->cap_kf == 0 || (O->kf_slot && O->kf_fixed && O->kf_Tcw));
  FB_ARG(O->cap_mp == 0 || (O->mp_index && O->mp_xw));
  FB_ARG(O->cap_obs == 0 || (O->obs_kf && O->obs_mp && O->obs_src && O->obs_uv && O->obs_inv_sigma2));
  if (bird) {
    FB_ARG(O->cap_mpb == 0 || (O->mpb_index && O->mpb_xw));
    FB_ARG(O->cap_bobs == 0 || (O->bobs_kf && O->bobs_mpb && O->bobs_src && O->bobs_xc && O->bobs_inv_sigma2));
  }
  return FB_OK;
}

WinOut win_out(const fb_covis_window &O, int sd) {
  if (sd) return {O.cap_mpb, O.cap_bobs, O.mpb_index, O.mpb_xw, O.bobs_kf, O.bobs_mpb, O.bobs_src, O.bobs_xc, O.bobs_inv_sigma2};
  return {O.cap_mp, O.cap_obs, O.mp_index, O.mp_xw, O.obs_kf, O.obs_mp, O.obs_src, O.obs_uv, O.obs_inv_sigma2};
}

}  // namespace

extern "C" {

int fb_covis_reserve_window(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_mpb, int32_t n_bobs) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && n_mpb >= 0 && n_mpb < INT_MAX && n_bobs >= 0);
  return g->reserve(plan_window_call(g->K, n_mp, n_obs, n_mpb, n_bobs));
}

int fb_covis_local_window_dev(fb_covis *g, const fb_covis_map *M, const fb_covis_kf_tables *T, int32_t cur_slot, int32_t with_bird,
                              const fb_covis_window *O, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_ARG(T);
  const bool bird = win_has_bird(T, with_bird);
  FB_TRY(check_tables(M, T, bird));
  FB_TRY(check_window(O, bird));
  FB_ARG(cur_slot >= 0 && cur_slot < g->K);
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  const size_t K = g->K, n_pt[2] = {(size_t)M->n_mp, bird ? (size_t)T->n_mpb : 0}, n_e[2] = {(size_t)M->n_obs, bird ? (size_t)T->n_bobs : 0};
  const CallPlan plan = plan_window_call(K, n_pt[0], n_e[0], n_pt[1], n_e[1]);
  WinOff wo;
  plan_window(K, n_pt[0], n_pt[1], &wo);
  scratch_window_begins(g->state);
  fb_covis_window out = *O;
  if (!bird) { out.cap_mpb = 0; out.cap_bobs = 0; }
  const fb_covis_map maps[2] = {*M, bird ? win_bird_map(*M, *T) : *M};
  Index ix[2];
  IndexAsk front, back;
  front.head = plan.front; front.tail = plan.total - plan.bird;   // the whole call is sized here: nothing below reallocates
  back.head = plan.bird; back.ranks = false; back.kept = false;   // the front side's index is the one a later reuse_index reads
  FB_TRY(g->acquire(maps[0], front, &ix[0], nullptr, s));
  if (bird) FB_TRY(g->acquire(maps[1], back, &ix[1], nullptr, s));
  WinS W;
  win_map(g->scr, wo, &W);
  k_win_local<<<1, CV_NT, 0, s>>>(g->G, cur_slot, T->kf_bad, W);
  const int n_sides = bird ? 2 : 1;
  for (int sd = 0; sd < n_sides; sd++) {
    const fb_covis_map &Ms = maps[sd];
    const WinSide &ws = W.side[sd];
    if (n_pt[sd] == 0) { FB_HIP(hipMemsetAsync(ws.eoff, 0, 4, s)); continue; }
    const unsigned waves = (unsigned)((n_pt[sd] + WIN_NT / 64 - 1) / (WIN_NT / 64)), nb = (unsigned)((n_pt[sd] + 1 + CV_SCAN_TILE - 1) / CV_SCAN_TILE);
    FB_HIP(hipMemsetAsync(ws.ptkey, 0x7f, n_pt[sd] * 4, s));
    FB_HIP(hipMemsetAsync(ws.eoff, 0, (n_pt[sd] + 1) * 4, s));
    k_win_mark<<<(unsigned)K, WIN_NT, 0, s>>>(Ms, W, sd, g->G.err);
    k_win_rowcount<<<(unsigned)K, WIN_NT, 0, s>>>(Ms, W, sd);
    k_win_rowscan<<<1, CV_NT, 0, s>>>(W, sd);
    k_win_place<<<(unsigned)K, WIN_NT, 0, s>>>(Ms, W, sd, sd ? T->mpb_xw : T->mp_xw, win_out(out, sd));
    k_win_observers<<<waves, WIN_NT, 0, s>>>(Ms, g->G, ix[sd].start, ix[sd].csr, T->kf_bad, W, sd);
    k_cv_scan_tile<<<nb, CV_NT, 0, s>>>(ws.eoff, (int)(n_pt[sd] + 1), ws.bsum, 0);
    k_cv_scan_sums<<<1, CV_NT, 0, s>>>(ws.bsum, (int)nb);
    k_cv_scan_tile<<<nb, CV_NT, 0, s>>>(ws.eoff, (int)(n_pt[sd] + 1), ws.bsum, 1);
  }
  k_win_fixed<<<1, CV_NT, 0, s>>>(g->G, W, *T, out);
  for (int sd = 0; sd < n_sides; sd++) {
    if (n_pt[sd] == 0) continue;
    const unsigned waves = (unsigned)((n_pt[sd] + WIN_NT / 64 - 1) / (WIN_NT / 64));
    k_win_edges<<<waves, WIN_NT, 0, s>>>(maps[sd], g->G, ix[sd].start, ix[sd].csr, *T, W, sd, win_out(out, sd), g->G.err);
  }
  k_win_header<<<1, 64, 0, s>>>(W, W.side[0].eoff + n_pt[0], bird ? W.side[1].eoff + n_pt[1] : nullptr, out);
  FB_HIP(hipGetLastError());
  scratch_window_done(g->state, plan.front, out.cap_kf);
  return FB_OK;
}

int fb_covis_local_window_header(fb_covis *g, fb_covis_window_header *header, int32_t *kf_slot, uint8_t *kf_fixed, void *stream) {
  FB_ARG(g && header);
  FB_ARG(g->state.win_valid);
  hipStream_t s = fb::as_stream(stream);
  Regions r;
  WinOff wo;
  win_kf_regions(r, g->K, &wo);
  const size_t n = (size_t)std::min(g->state.win_cap_kf, g->K);
  FB_HIP(hipMemcpyAsync(header, g->scr + wo.hdr, sizeof(*header), hipMemcpyDeviceToHost, s));
  if (kf_slot && n) FB_HIP(hipMemcpyAsync(kf_slot, g->scr + wo.wslot, n * 4, hipMemcpyDeviceToHost, s));
  if (kf_fixed && n) FB_HIP(hipMemcpyAsync(kf_fixed, g->scr + wo.wfixed, n, hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  if (header->overflow) { fb::set_error("fb_covis_local_window: a list is longer than its capacity"); return FB_ERR_CAPACITY; }
  return FB_OK;
}

int fb_covis_local_window(fb_covis *g, const fb_covis_map *HM, const fb_covis_kf_tables *HT, int32_t cur_slot, int32_t with_bird,
                          const fb_covis_window *HO) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_ARG(HT);
  const bool bird = win_has_bird(HT, with_bird);
  FB_TRY(check_tables(HM, HT, bird));
  FB_TRY(check_window(HO, bird));
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_covis_kf_tables T = *HT;
  fb_covis_window O = *HO;
  const size_t K = M.max_keyframes, S = M.kp_stride, BS = T.bird_stride;
  const float *kf_Tcw = T.kf_Tcw, *mp_xw = T.mp_xw, *mpb_xw = bird ? T.mpb_xw : nullptr;
  fb::Stager st;
  stage_map(st, M);
  st.in(kf_Tcw, K * 48); st.in(T.kf_bad, K); st.in(T.kf_init, K); st.in(T.kf_keys_un, K * S * sizeof(fb_keypoint));
  st.in(T.inv_level_sigma2, (size_t)T.n_levels * 4); st.in(mp_xw, (size_t)M.n_mp * 12);
  if (bird) {
    st.in(T.kf_nb, K * 4); st.in(T.kf_mpb, K * BS * 4); st.in(T.kf_bird_octave, K * BS); st.in(T.kf_bird_xc, K * BS * 12);
    st.in(T.mpb_bad, (size_t)T.n_mpb); st.in(mpb_xw, (size_t)T.n_mpb * 12);
    st.in(T.bobs_mpb, (size_t)T.n_bobs * 4); st.in(T.bobs_kf, (size_t)T.n_bobs * 4); st.in(T.bobs_idx, (size_t)T.n_bobs * 4);
  } else {
    T.kf_nb = nullptr; T.kf_mpb = nullptr; T.kf_bird_octave = nullptr; T.kf_bird_xc = nullptr; T.mpb_bad = nullptr;
    T.bobs_mpb = nullptr; T.bobs_kf = nullptr; T.bobs_idx = nullptr;
    O.mpb_index = nullptr; O.mpb_xw = nullptr; O.bobs_kf = nullptr; O.bobs_mpb = nullptr; O.bobs_src = nullptr; O.bobs_xc = nullptr;
    O.bobs_inv_sigma2 = nullptr; O.cap_mpb = 0; O.cap_bobs = 0;
  }
  // copy-in: entries past the counts keep the caller's contents
  st.out(O.kf_slot, (size_t)O.cap_kf * 4, true); st.out(O.kf_fixed, (size_t)O.cap_kf, true); st.out(O.kf_Tcw, (size_t)O.cap_kf * 48, true);
  st.out(O.mp_index, (size_t)O.cap_mp * 4, true); st.out(O.mp_xw, (size_t)O.cap_mp * 12, true);
  st.out(O.obs_kf, (size_t)O.cap_obs * 4, true); st.out(O.obs_mp, (size_t)O.cap_obs * 4, true); st.out(O.obs_src, (size_t)O.cap_obs * 4, true);
  st.out(O.obs_uv, (size_t)O.cap_obs * 8, true); st.out(O.obs_inv_sigma2, (size_t)O.cap_obs * 4, true);
  st.out(O.mpb_index, (size_t)O.cap_mpb * 4, true); st.out(O.mpb_xw, (size_t)O.cap_mpb * 12, true);
  st.out(O.bobs_kf, (size_t)O.cap_bobs * 4, true); st.out(O.bobs_mpb, (size_t)O.cap_bobs * 4, true); st.out(O.bobs_src, (size_t)O.cap_bobs * 4, true);
  st.out(O.bobs_xc, (size_t)O.cap_bobs * 12, true); st.out(O.bobs_inv_sigma2, (size_t)O.cap_bobs * 4, true);
  st.out(O.header, sizeof(fb_covis_window_header), false);
  FB_TRY(st.commit(nullptr));
  T.kf_Tcw = const_cast<float *>(kf_Tcw); T.mp_xw = const_cast<float *>(mp_xw); T.mpb_xw = const_cast<float *>(mpb_xw);
  IndexDropGuard drop(g->state);   // the index is of staged arrays
  FB_TRY(fb_covis_local_window_dev(g, &M, &T, cur_slot, with_bird, &O, nullptr));
  FB_TRY(st.fetch(nullptr));
  if (HO->header->overflow) { fb::set_error("fb_covis_local_window: a list is longer than its capacity"); return FB_ERR_CAPACITY; }
  return FB_OK;
}

int fb_covis_window_scatter_dev(fb_covis *g, const fb_covis_map *M, const fb_covis_kf_tables *T, const fb_covis_window *O,
                                const uint8_t *d_obs_outlier, const uint8_t *d_bobs_outlier, int32_t *d_n_erase, int32_t *d_erase,
                                int32_t *d_berase, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_ARG(T && O);
  const bool bird = O->cap_mpb > 0 || O->cap_bobs > 0;
  FB_TRY(check_tables(M, T, bird));
  FB_TRY(check_window(O, bird));
  FB_ARG(d_n_erase);
  FB_ARG(!d_obs_outlier || O->cap_obs == 0 || d_erase);
  FB_ARG(!d_bobs_outlier || O->cap_bobs == 0 || d_berase);
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  fb_covis_window out = *O;
  const size_t n = std::max({(size_t)out.cap_kf * 12, (size_t)out.cap_mp * 3, (size_t)out.cap_mpb * 3});
  if (n) k_win_scatter<<<(unsigned)((n + WIN_NT - 1) / WIN_NT), WIN_NT, 0, s>>>(*M, *T, out, g->K);
  k_win_erase<<<2, CV_NT, 0, s>>>(*M, *T, out, g->K, d_obs_outlier, bird ? d_bobs_outlier : nullptr, d_n_erase, d_erase, d_berase);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

}  // extern "C"
