// covis_points.inc -- the per-point side of LocalMapping on the device-resident map (included from covis.hip after
// covis_tree.inc: it shares Gr, Index, same_map; covis_correct.inc, included after it, shares nd_unit / nd_finish).
//
// Replaces (reference file:line):
//   MapPoint::UpdateNormalAndDepth                                         src/MapPoint.cc:330-371
//   MapPoint::ComputeDistinctiveDescriptors                                src/MapPoint.cc:242-307
//   LocalMapping::ProcessNewKeyFrame, the point loop                       src/LocalMapping.cc:158-179
//   MapPoint::AddObservation (monocular)                                   src/MapPoint.cc:98-109
//   LocalMapping::MapPointCulling                                          src/LocalMapping.cc:207-228
//   MapPoint::SetBadFlag (its edits of the map arrays)                     src/MapPoint.cc:151-168
//
// Every point's outcome depends only on its own edges, so the two serial loops become a per-entry classification and
// ordered compactions.  The only float decision is found / visible < 0.25f, repeated as written.
#include "fb_distinctive.h"
#include "fb_frame_geom.h"

namespace {

constexpr int PT_STAGE = FB_REFRESH_STAGE;
constexpr uint32_t PT_IDX = 0x7fffu;                   // a sort key is rank << 15 | feature index (kp_stride <= 32767)
static_assert(FB_COVIS_MAX_STRIDE <= 0x7fff, "a feature index is kept in 15 bits");
enum { MPC_NONE = -1, MPC_DROP = 0, MPC_CULL = 1, MPC_KEEP = 2 };

// normali / cv::norm(normali) of one observer (MapPoint.cc:354-355): a CV_32F difference, the norm in double, Mat / double
// as a product with the float reciprocal
__device__ __forceinline__ void nd_unit(const float X[3], const float *Ow, float u[3]) {
  const float d0 = X[0] - Ow[0], d1 = X[1] - Ow[1], d2 = X[2] - Ow[2];
  const float inv = (float)(1.0 / sqrt((double)d0 * (double)d0 + (double)d1 * (double)d1 + (double)d2 * (double)d2));
  u[0] = d0 * inv; u[1] = d1 * inv; u[2] = d2 * inv;
}
// :359-369 from the sum of the n unit vectors, the centre of the reference key frame and the two scale factors
__device__ __forceinline__ void nd_finish(const float X[3], const float *Or, float scale_level, float scale_last, const float sum[3], int n,
                                          float *normal, float *min_dist, float *max_dist) {
  const float dist = fb::norm3(X[0] - Or[0], X[1] - Or[1], X[2] - Or[2]);
  const float maxd = dist * scale_level;                                // :367-369
  *max_dist = maxd;
  *min_dist = maxd / scale_last;
  const float in = (float)(1.0 / (double)n);
  normal[0] = sum[0] * in; normal[1] = sum[1] * in; normal[2] = sum[2] * in;
}

// ascending sort of s_key[0..n) by one wave (the block is that wave).  Up to 64 keys: every lane ranks its own key against
// the others; more: the bitonic network over the next power of two (s_key holds that many).  Ends with a barrier.
template <typename KT>
__device__ __forceinline__ void pt_sort(KT *s_key, int n, int lane) {
  if (n <= 64) {
    const KT key = lane < n ? s_key[lane] : ~(KT)0;
    int pos = 0;
    for (int j = 0; j < n; j++) {
      const KT o = s_key[j];
      pos += (o < key || (o == key && j < lane)) ? 1 : 0;
    }
    __syncthreads();
    if (lane < n) s_key[pos] = key;
    __syncthreads();
    return;
  }
  int n2 = 128;
  while (n2 < n) n2 <<= 1;
  for (int q = n + lane; q < n2; q += 64) s_key[q] = ~(KT)0;
  __syncthreads();
  fb::bitonic_sort(s_key, n2, lane, 64);
}

// ComputeDistinctiveDescriptors (:261-307) of one point by one wave, from its n observers as sorted keys (rank << 15 | feature)
// in s_key: the observers of key frames that are not bad (:265) are compacted in place in observer order as rows of kf_desc,
// and the pick gives its 32 bytes to dst.  D: [PT_STAGE][32] of LDS.
__device__ __forceinline__ void pt_descriptor(const uint8_t *kf_bad, const uint8_t *kf_desc, uint8_t *dst_row, const Gr &G, int S, uint32_t *s_key,
                                              uint4 *D, int n, int lane) {
  int N = 0;
  for (int base = 0; base < n; base += 64) {
    const int j = base + lane;
    bool keep = false;
    uint32_t row = 0;
    if (j < n) {
      const uint32_t key = s_key[j];
      const int kf = G.inv[key >> 15];
      keep = !kf_bad[kf];
      row = (uint32_t)kf * (uint32_t)S + (key & PT_IDX);
    }
    const unsigned long long mask = __ballot(keep);
    __syncthreads();                                                    // the chunk is read: the writes land at or before it
    if (keep) s_key[N + __popcll(mask & ((1ull << lane) - 1ull))] = row;
    N += __popcll(mask);
  }
  __syncthreads();
  if (N == 0) return;                                                   // vDescriptors.empty()
  uint4 *dst = reinterpret_cast<uint4 *>(dst_row);
  if (N <= PT_STAGE) {
    for (int t = lane; t < N * 2; t += 64) D[t] = reinterpret_cast<const uint4 *>(kf_desc + (size_t)s_key[t >> 1] * 32)[t & 1];
    __syncthreads();
    const int best = fb::distinctive_pick(lane, N, [&](int j) { return (const uint4 *)(D + j * 2); });
    if (lane < 2) dst[lane] = D[best * 2 + lane];
  } else {
    auto at = [&](int j) { return reinterpret_cast<const uint4 *>(kf_desc + (size_t)s_key[j] * 32); };
    const int best = fb::distinctive_pick(lane, N, at);
    if (lane < 2) dst[lane] = at(best)[lane];
  }
}

struct PtRun {
  fb_point_refresh_args A;
  const int32_t *list, *d_n;   // list == NULL: every point
  int n_list;
  int cap;                     // s_key holds the next power of two >= cap keys; a point with more observers is counted and skipped
  int extra_slot;              // with extra_idx: every listed point has one more edge, (mp, extra_slot, extra_idx[i]), that the
  const int32_t *extra_idx;    // index does not know yet (ProcessNewKeyFrame)
};

// One wave per listed point.  LDS: [PT_STAGE][32] descriptors, then the keys.
__global__ __launch_bounds__(64) void k_pt_refresh(fb_covis_map M, Gr G, const int32_t *start, const int32_t *csr, PtRun R) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pt_smem[];
  uint4 *D = reinterpret_cast<uint4 *>(pt_smem);
  uint32_t *s_key = reinterpret_cast<uint32_t *>(pt_smem + (size_t)PT_STAGE * 32);
  const int lane = threadIdx.x, i = blockIdx.x, S = M.kp_stride;
  const fb_point_refresh_args &A = R.A;
  int mp = i;
  if (R.list) {
    int nl = R.n_list;
    if (R.d_n) nl = min(max(*R.d_n, 0), nl);
    if (i >= nl) return;
    mp = R.list[i];
    if (mp < 0 || mp >= M.n_mp) { if (lane == 0) atomicAdd(G.err, 1); return; }
  }
  if (M.mp_bad[mp]) return;                                             // :251, :338
  const int p0 = start[mp], cnt = start[mp + 1] - p0, n = cnt + (R.extra_idx ? 1 : 0);
  if (n == 0) return;                                                   // observations.empty()
  if (n > R.cap) { if (lane == 0) atomicAdd(G.err, 1); return; }        // more observers than slots: a repeated (mp, kf) edge
  for (int q = lane; q < cnt; q += 64) {
    const int e = csr[p0 + q];                                          // a checked, live edge
    s_key[q] = ((uint32_t)G.rank[M.obs_kf[e]] << 15) | (uint32_t)M.obs_idx[e];
  }
  if (R.extra_idx && lane == 0) s_key[cnt] = ((uint32_t)G.rank[R.extra_slot] << 15) | (uint32_t)R.extra_idx[i];
  __syncthreads();
  pt_sort(s_key, n, lane);

  if (A.what & FB_REFRESH_NORMAL_DEPTH) {
    const int ref = A.mp_ref_kf[mp];
    if (ref < 0 || ref >= G.K) {                                        // the reference dereferences pRefKF
      if (lane == 0) atomicAdd(G.err, 1);
    } else {
      const float X[3] = {A.mp_xw[(size_t)mp * 3], A.mp_xw[(size_t)mp * 3 + 1], A.mp_xw[(size_t)mp * 3 + 2]};
      float sum[3] = {0.0f, 0.0f, 0.0f};
      int ref_idx = -1;
      for (int base = 0; base < n; base += 64) {                        // the unit vectors 64 at a time, their sum in observer order
        const int j = base + lane;
        float u[3] = {0.0f, 0.0f, 0.0f};
        if (j < n) {
          const uint32_t key = s_key[j];
          const int kf = G.inv[key >> 15];
          float Ow[3];
          fb::camera_centre(A.kf_Tcw + (size_t)kf * 12, Ow);
          nd_unit(X, Ow, u);
          if (kf == ref) ref_idx = (int)(key & PT_IDX);
        }
        const int m = min(64, n - base);
        for (int t = 0; t < m; t++) {
          sum[0] = sum[0] + __shfl(u[0], t, 64); sum[1] = sum[1] + __shfl(u[1], t, 64); sum[2] = sum[2] + __shfl(u[2], t, 64);   // :355
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ref_idx = max(ref_idx, __shfl_xor(ref_idx, o, 64));
      if (ref_idx < 0) ref_idx = 0;                                     // observations[pRefKF] inserts 0 when it is not there
      const int level = M.kf_octave[(size_t)ref * S + ref_idx];         // :361
      if (level >= A.n_levels) {
        if (lane == 0) atomicAdd(G.err, 1);
      } else if (lane == 0) {
        float Or[3];
        fb::camera_centre(A.kf_Tcw + (size_t)ref * 12, Or);
        nd_finish(X, Or, A.scale_factors[level], A.scale_factors[A.n_levels - 1], sum, n, A.mp_normal + (size_t)mp * 3, A.mp_min_dist + mp,
                  A.mp_max_dist + mp);
      }
    }
  }
  if (!(A.what & FB_REFRESH_DESCRIPTOR)) return;

  pt_descriptor(A.kf_bad, A.kf_desc, A.mp_desc + (size_t)mp * 32, G, S, s_key, D, n, lane);
}

// ---- ProcessNewKeyFrame ---------------------------------------------------------------------------------------------------
// One workgroup: the features of the key frame classified (0: nothing, 1: new edge, 2: recent list), both classes compacted
// in ascending i.  first[mp] (0x7f filled) becomes the first feature that holds a live point.
__global__ __launch_bounds__(CV_NT) void k_pnk(fb_covis_map M, Gr G, const int32_t *start, const int32_t *csr, int32_t *first,
                                               fb_new_keyframe_args A, int32_t *gain, int32_t *gain_idx, int32_t *n_gain) {
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x, slot = A.slot, NF = A.n_features, S = M.kp_stride, base = M.n_obs;
  if (M.kf_n[slot] != NF) {                                             // the host's N is not the table's: nothing is done
    for (int e = base + tid; e < base + NF; e += CV_NT) { A.obs_mp[e] = -1; A.obs_kf[e] = -1; A.obs_idx[e] = -1; }
    if (tid == 0) { atomicAdd(G.err, 1); *A.d_n_added = 0; *n_gain = 0; }
    return;
  }
  const int32_t *mps = M.kf_mp + (size_t)slot * S;
  for (int i = tid; i < NF; i += CV_NT) {
    const int mp = mps[i];
    if (mp >= 0 && mp < M.n_mp && !M.mp_bad[mp]) atomicMin(&first[mp], i);
  }
  group_sync();
  const int nrec0 = min(max(*A.d_n_recent, 0), A.recent_cap);
  int cadd = 0, crec = 0;
  for (int tile = 0; tile < NF; tile += CV_NT) {
    const int i = tile + tid;
    int cls = 0, mp = -1;
    if (i < NF) {
      mp = mps[i];
      if (mp < 0) {                                                     // :163
      } else if (mp >= M.n_mp) {
        atomicAdd(G.err, 1);
      } else if (!M.mp_bad[mp]) {                                       // :165
        bool has = false;                                               // IsInKeyFrame before this loop began
        const int p1 = start[mp + 1];
        for (int p = start[mp]; p < p1; p++) has = has || M.obs_kf[csr[p]] == slot;
        cls = (!has && ld(&first[mp]) == i) ? 1 : 2;                    // a later feature finds the edge of the first
      }
    }
    int tadd, trec;
    const int eadd = fb::block_excl_scan<CV_NT>(cls == 1 ? 1 : 0, s_wv, &tadd);
    const int erec = fb::block_excl_scan<CV_NT>(cls == 2 ? 1 : 0, s_wv, &trec);
    if (cls == 1) {                                                     // AddObservation(pKF, i)
      const int k = cadd + eadd, e = base + k;
      A.obs_mp[e] = mp; A.obs_kf[e] = slot; A.obs_idx[e] = i;
      gain[k] = mp; gain_idx[k] = i;
    } else if (cls == 2) {                                              // mlpRecentAddedMapPoints.push_back
      const int pos = nrec0 + crec + erec;
      if (pos < A.recent_cap) A.d_recent[pos] = mp; else atomicAdd(G.err, 1);
    }
    cadd += tadd; crec += trec;
    __syncthreads();
  }
  for (int e = base + cadd + tid; e < base + NF; e += CV_NT) { A.obs_mp[e] = -1; A.obs_kf[e] = -1; A.obs_idx[e] = -1; }
  if (tid == 0) { *A.d_n_added = cadd; *n_gain = cadd; *A.d_n_recent = min(nrec0 + crec, A.recent_cap); }
}

// ---- MapPointCulling -------------------------------------------------------------------------------------------------------
struct MpcS {           // the scratch of one call, behind the index
  int32_t *first;       // [n_mp] the first list entry that gives the point SetBadFlag
  int32_t *val, *dec, *rowbase;   // [cap] the list as it came in, the branch of each entry, where its erased rows begin
  int32_t *bcnt;        // [blocks][3] kept, culled, erased rows of a block of PT_NT entries
};
void mpc_map(uint8_t *b, const MpcOff &o, MpcS *S) {
  S->first = (int32_t *)(b + o.first); S->val = (int32_t *)(b + o.val); S->dec = (int32_t *)(b + o.dec);
  S->rowbase = (int32_t *)(b + o.rowbase); S->bcnt = (int32_t *)(b + o.bcnt);
}

// the branch of every entry from the map as it came in (:209-227); nothing of the map is written yet
__global__ __launch_bounds__(PT_NT) void k_mpc_decide(fb_covis_map M, const int32_t *start, fb_map_point_culling_args A, MpcS S, int32_t *err) {
  const int i = blockIdx.x * PT_NT + threadIdx.x;
  if (i >= A.recent_cap) return;
  const int n = min(max(*A.d_n_recent, 0), A.recent_cap);
  if (i >= n) { S.dec[i] = MPC_NONE; return; }
  const int mp = A.d_recent[i];
  S.val[i] = mp;
  int dec = MPC_DROP;
  if (mp < 0 || mp >= M.n_mp) {
    atomicAdd(err, 1);
  } else if (!M.mp_bad[mp]) {                                           // :210
    const float ratio = (float)A.mp_found[mp] / (float)A.mp_visible[mp];   // static_cast<float>(mnFound)/mnVisible
    const int age = A.cur_kf_id - A.mp_first_kf_id[mp], nobs = start[mp + 1] - start[mp];
    if (ratio < 0.25f) dec = MPC_CULL;                                  // :214
    else if (age >= 2 && nobs <= A.n_th_obs) dec = MPC_CULL;            // :219
    else if (age >= 3) dec = MPC_DROP;                                  // :224
    else dec = MPC_KEEP;
    if (dec == MPC_CULL) atomicMin(&S.first[mp], i);
  }
  S.dec[i] = dec;
}

// a point listed twice is bad by its second entry; then the counts of each block
__global__ __launch_bounds__(PT_NT) void k_mpc_count(const int32_t *start, int cap, MpcS S) {
  __shared__ int s_wv[PT_NT / 64];
  const int i = blockIdx.x * PT_NT + threadIdx.x;
  int dec = i < cap ? S.dec[i] : MPC_NONE, rows = 0;
  if (dec == MPC_CULL) {
    const int mp = S.val[i];
    if (S.first[mp] != i) { dec = MPC_DROP; S.dec[i] = dec; }
    else rows = start[mp + 1] - start[mp];
  }
  const int k = fb::block_sum<PT_NT>(dec == MPC_KEEP ? 1 : 0, s_wv), c = fb::block_sum<PT_NT>(dec == MPC_CULL ? 1 : 0, s_wv),
            r = fb::block_sum<PT_NT>(rows, s_wv);
  if (threadIdx.x == 0) { S.bcnt[blockIdx.x * 3] = k; S.bcnt[blockIdx.x * 3 + 1] = c; S.bcnt[blockIdx.x * 3 + 2] = r; }
}

// the kept list and the culled list in list order; the last block leaves the three counts
__global__ __launch_bounds__(PT_NT) void k_mpc_place(const int32_t *start, fb_map_point_culling_args A, MpcS S) {
  __shared__ int s_wv[PT_NT / 64];
  const int i = blockIdx.x * PT_NT + threadIdx.x;
  int pk = 0, pc = 0, pr = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += PT_NT) { pk += S.bcnt[b * 3]; pc += S.bcnt[b * 3 + 1]; pr += S.bcnt[b * 3 + 2]; }
  pk = fb::block_sum<PT_NT>(pk, s_wv); pc = fb::block_sum<PT_NT>(pc, s_wv); pr = fb::block_sum<PT_NT>(pr, s_wv);
  const int dec = i < A.recent_cap ? S.dec[i] : MPC_NONE, mp = dec == MPC_KEEP || dec == MPC_CULL ? S.val[i] : 0;
  const int rows = dec == MPC_CULL ? start[mp + 1] - start[mp] : 0;
  int tk, tc, tr;
  const int ek = fb::block_excl_scan<PT_NT>(dec == MPC_KEEP ? 1 : 0, s_wv, &tk);
  const int ec = fb::block_excl_scan<PT_NT>(dec == MPC_CULL ? 1 : 0, s_wv, &tc);
  const int er = fb::block_excl_scan<PT_NT>(rows, s_wv, &tr);
  if (dec == MPC_KEEP) A.d_recent[pk + ek] = mp;
  if (dec == MPC_CULL) { A.d_culled[pc + ec] = mp; S.rowbase[i] = pr + er; }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) { *A.d_n_recent = pk + tk; *A.d_n_culled = pc + tc; *A.d_n_erased = pr + tr; }
}

// SetBadFlag of the culled entries, one wave each: the point's live edges in ascending kf_order (key = rank, feature, edge)
__global__ __launch_bounds__(64) void k_mpc_erase(fb_covis_map M, Gr G, const int32_t *start, const int32_t *csr, fb_map_point_culling_args A,
                                                  MpcS S, int cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pt_smem[];
  unsigned long long *s_key = reinterpret_cast<unsigned long long *>(pt_smem);
  const int lane = threadIdx.x, i = blockIdx.x;
  if (S.dec[i] != MPC_CULL) return;
  const int mp = S.val[i], p0 = start[mp], n = start[mp + 1] - p0;
  if (lane == 0) A.mp_bad[mp] = 1;                                      // MapPoint.cc:157
  if (n == 0) return;
  if (n > cap) { if (lane == 0) atomicAdd(G.err, 1); return; }
  for (int q = lane; q < n; q += 64) {
    const int e = csr[p0 + q];
    s_key[q] = ((unsigned long long)(((uint32_t)G.rank[M.obs_kf[e]] << 15) | (uint32_t)M.obs_idx[e]) << 32) | (uint32_t)e;
  }
  __syncthreads();
  pt_sort(s_key, n, lane);
  const int r0 = S.rowbase[i];
  for (int j = lane; j < n; j += 64) {
    const unsigned long long key = s_key[j];
    const int e = (int)(uint32_t)key, idx = (int)((key >> 32) & PT_IDX), kf = G.inv[(uint32_t)(key >> 47)];
    A.obs_kf[e] = -1;                                                   // mObservations.clear()
    A.kf_mp[(size_t)kf * M.kp_stride + idx] = -1;                       // EraseMapPointMatch(idx)
    const int r = r0 + j;
    if (r < A.erased_cap) { A.d_erased[(size_t)r * 4] = kf; A.d_erased[(size_t)r * 4 + 1] = mp; A.d_erased[(size_t)r * 4 + 2] = idx; A.d_erased[(size_t)r * 4 + 3] = e; }
  }
}

int pow2_at_least(int v) {
  int n2 = 128;
  while (n2 < v) n2 <<= 1;
  return n2;
}

int check_refresh_arrays(const fb_covis_map *M, const fb_point_refresh_args *a) {
  FB_ARG(a->n_levels >= 1 && a->n_levels <= FB_MAX_LEVELS);
  FB_ARG(a->kf_Tcw && a->kf_bad && a->kf_desc && a->scale_factors);
  FB_ARG(M->n_mp == 0 || (a->mp_xw && a->mp_ref_kf && a->mp_normal && a->mp_min_dist && a->mp_max_dist && a->mp_desc));
  FB_ARG((size_t)M->max_keyframes * (size_t)M->kp_stride < (size_t)UINT32_MAX);   // a row of kf_desc is kept in 32 bits
  return FB_OK;
}

// the device arrays the wave reads and stores as uint4
int check_desc_aligned(const fb_point_refresh_args *a) {
  FB_ARG(((uintptr_t)a->kf_desc & 15) == 0 && ((uintptr_t)a->mp_desc & 15) == 0);
  return FB_OK;
}

int check_refresh(const fb_covis_map *M, const fb_point_refresh_args *a) {
  FB_ARG(a);
  FB_ARG(a->what != 0 && (a->what & ~(FB_REFRESH_NORMAL_DEPTH | FB_REFRESH_DESCRIPTOR)) == 0);
  FB_ARG(a->reuse_index == 0 || a->reuse_index == 1);
  FB_ARG(!a->d_list || a->n_list >= 0);
  FB_ARG(a->d_list || !a->d_n_list);
  return check_refresh_arrays(M, a);
}

int launch_refresh(fb_covis *g, const fb_covis_map *M, const Index &ix, const PtRun &R, hipStream_t s) {
  const int blocks = R.list ? R.n_list : M->n_mp;
  if (blocks == 0) return FB_OK;
  const size_t lds = (size_t)PT_STAGE * 32 + (size_t)pow2_at_least(g->K) * 4;
  k_pt_refresh<<<(unsigned)blocks, 64, lds, s>>>(*M, g->G, ix.start, ix.csr, R);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int check_new_keyframe(const fb_covis *g, const fb_covis_map *M, const fb_new_keyframe_args *a) {
  FB_ARG(a);
  FB_ARG(a->slot >= 0 && a->slot < g->K);
  FB_ARG(a->n_features >= 0 && a->n_features <= M->kp_stride);
  FB_ARG(a->obs_cap >= 0 && (int64_t)M->n_obs + a->n_features <= (int64_t)a->obs_cap);
  FB_ARG(a->obs_cap == 0 || (a->obs_mp && a->obs_kf && a->obs_idx));
  FB_ARG(a->d_n_added && a->d_n_recent && a->recent_cap >= 0 && (a->recent_cap == 0 || a->d_recent));
  // the block is written through a->obs_*, and the caller goes on with the map's own pointers: they must be the same arrays
  FB_ARG(a->n_features == 0 || (a->obs_mp == M->obs_mp && a->obs_kf == M->obs_kf && a->obs_idx == M->obs_idx));
  return check_refresh_arrays(M, &a->refresh);
}

int check_culling(const fb_covis_map *M, const fb_map_point_culling_args *a) {
  FB_ARG(a);
  FB_ARG(a->recent_cap >= 0 && (a->recent_cap == 0 || a->d_recent) && a->d_n_recent);
  FB_ARG(M->n_mp == 0 || (a->mp_first_kf_id && a->mp_found && a->mp_visible && a->mp_bad));
  FB_ARG(a->kf_mp && (M->n_obs == 0 || a->obs_kf));
  FB_ARG(a->d_n_culled && a->d_n_erased && (a->recent_cap == 0 || a->d_culled) && a->erased_cap >= 0 && (a->erased_cap == 0 || a->d_erased));
  return FB_OK;
}

}  // namespace

extern "C" {

int fb_covis_reserve_refresh_points(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && n_q >= 0 && n_q <= g->K);
  return g->reserve(plan_map_call(g->K, n_mp, n_obs, n_q, 0));
}

int fb_covis_refresh_points_dev(fb_covis *g, const fb_covis_map *M, const fb_point_refresh_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_refresh(M, a));
  FB_TRY(check_desc_aligned(a));
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  Index ix;
  IndexAsk ask;
  ask.reuse = a->reuse_index != 0;
  FB_TRY(g->acquire(*M, ask, &ix, nullptr, s));
  PtRun R;
  memset(&R, 0, sizeof(R));
  R.A = *a; R.list = a->d_list; R.d_n = a->d_n_list; R.n_list = a->d_list ? a->n_list : 0; R.cap = g->K;
  return launch_refresh(g, M, ix, R, s);
}

int fb_covis_refresh_points(fb_covis *g, const fb_covis_map *HM, const fb_point_refresh_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_TRY(check_refresh(HM, ha));
  FB_ARG(!ha->d_n_list);
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_point_refresh_args A = *ha;
  const size_t K = g->K, S = M.kp_stride, n_mp = M.n_mp;
  fb::Stager st;
  stage_map(st, M);
  st.in(A.d_list, (size_t)A.n_list * 4);
  st.in(A.kf_Tcw, K * 48); st.in(A.kf_bad, K); st.in(A.kf_desc, K * S * 32); st.in(A.scale_factors, (size_t)A.n_levels * 4);
  st.in(A.mp_xw, n_mp * 12); st.in(A.mp_ref_kf, n_mp * 4);
  // copy-in: what the call leaves alone keeps the caller's contents
  st.out(A.mp_normal, n_mp * 12, true); st.out(A.mp_min_dist, n_mp * 4, true); st.out(A.mp_max_dist, n_mp * 4, true);
  st.out(A.mp_desc, n_mp * 32, true);
  FB_TRY(st.commit(nullptr));
  A.reuse_index = 0;   // the staged arrays are new device arrays every call
  IndexDropGuard drop(g->state);
  FB_TRY(fb_covis_refresh_points_dev(g, &M, &A, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_reserve_process_new_keyframe(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t n_features) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && n_q >= 0 && n_q <= g->K && n_features >= 0);
  PnkOff po;
  return g->reserve(plan_map_call(g->K, n_mp, n_obs, n_q, plan_new_keyframe(n_features, &po)));
}

int fb_covis_process_new_keyframe_dev(fb_covis *g, const fb_covis_map *M, const fb_new_keyframe_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_new_keyframe(g, M, a));
  FB_TRY(check_desc_aligned(&a->refresh));
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  const size_t NF = a->n_features;
  PnkOff po;
  IndexAsk ask;
  ask.tail = plan_new_keyframe(NF, &po);
  Index ix;
  uint8_t *b;
  FB_TRY(g->acquire(*M, ask, &ix, &b, s));
  int32_t *gain = (int32_t *)(b + po.gain), *gain_idx = (int32_t *)(b + po.gain_idx), *n_gain = (int32_t *)(b + po.n_gain);
  scratch_drop_index(g->state);                                         // the edge list grows: a later reuse_index rebuilds
  if (M->n_mp) FB_HIP(hipMemsetAsync(ix.nobs, 0x7f, (size_t)M->n_mp * 4, s));   // (the culling overlay's array is free here)
  k_pnk<<<1, CV_NT, 0, s>>>(*M, g->G, ix.start, ix.csr, ix.nobs, *a, gain, gain_idx, n_gain);
  FB_HIP(hipGetLastError());
  PtRun R;
  memset(&R, 0, sizeof(R));
  R.A = a->refresh; R.A.what = FB_REFRESH_NORMAL_DEPTH | FB_REFRESH_DESCRIPTOR;
  R.list = gain; R.d_n = n_gain; R.n_list = (int)NF; R.cap = g->K; R.extra_slot = a->slot; R.extra_idx = gain_idx;
  return launch_refresh(g, M, ix, R, s);
}

int fb_covis_process_new_keyframe(fb_covis *g, const fb_covis_map *HM, const fb_new_keyframe_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_TRY(check_new_keyframe(g, HM, ha));
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_new_keyframe_args A = *ha;
  fb_point_refresh_args &F = A.refresh;
  const size_t K = g->K, S = M.kp_stride, n_mp = M.n_mp, n_edges = (size_t)M.n_obs + (size_t)A.n_features;
  fb::Stager st;
  st.in(M.kf_n, K * 4); st.in(M.kf_mp, K * S * 4); st.in(M.kf_octave, K * S); st.in(M.kf_order, K * 8); st.in(M.mp_bad, n_mp);
  st.in(F.kf_Tcw, K * 48); st.in(F.kf_bad, K); st.in(F.kf_desc, K * S * 32); st.in(F.scale_factors, (size_t)F.n_levels * 4);
  st.in(F.mp_xw, n_mp * 12); st.in(F.mp_ref_kf, n_mp * 4);
  // the edge arrays are the map's: staged once, with the block the call owns
  st.out(A.obs_mp, n_edges * 4, true); st.out(A.obs_kf, n_edges * 4, true); st.out(A.obs_idx, n_edges * 4, true);
  st.out(A.d_n_added, 4, false); st.out(A.d_recent, (size_t)A.recent_cap * 4, true); st.out(A.d_n_recent, 4, true);
  st.out(F.mp_normal, n_mp * 12, true); st.out(F.mp_min_dist, n_mp * 4, true); st.out(F.mp_max_dist, n_mp * 4, true);
  st.out(F.mp_desc, n_mp * 32, true);
  FB_TRY(st.commit(nullptr));
  M.obs_mp = A.obs_mp; M.obs_kf = A.obs_kf; M.obs_idx = A.obs_idx;
  IndexDropGuard drop(g->state);
  FB_TRY(fb_covis_process_new_keyframe_dev(g, &M, &A, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_reserve_map_point_culling(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t recent_cap) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && n_q >= 0 && n_q <= g->K && recent_cap >= 0);
  MpcOff mo;
  return g->reserve(plan_map_call(g->K, n_mp, n_obs, n_q, plan_point_culling(n_mp, recent_cap, &mo)));
}

int fb_covis_map_point_culling_dev(fb_covis *g, const fb_covis_map *M, const fb_map_point_culling_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_culling(M, a));
  FB_ARG(a->kf_mp == M->kf_mp && (M->n_mp == 0 || a->mp_bad == M->mp_bad) && (M->n_obs == 0 || a->obs_kf == M->obs_kf));
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  const size_t n_mp = M->n_mp, cap = a->recent_cap;
  if (cap == 0) {
    FB_HIP(hipMemsetAsync(a->d_n_culled, 0, 4, s));
    FB_HIP(hipMemsetAsync(a->d_n_erased, 0, 4, s));
    FB_HIP(hipMemsetAsync(a->d_n_recent, 0, 4, s));
    return FB_OK;
  }
  MpcOff mo;
  IndexAsk ask;
  ask.tail = plan_point_culling(n_mp, cap, &mo);
  Index ix;
  uint8_t *tail;
  FB_TRY(g->acquire(*M, ask, &ix, &tail, s));
  MpcS S;
  mpc_map(tail, mo, &S);
  scratch_drop_index(g->state);                                         // edges become tombstones: a later reuse_index rebuilds
  const unsigned nb = (unsigned)((cap + PT_NT - 1) / PT_NT);
  if (n_mp) FB_HIP(hipMemsetAsync(S.first, 0x7f, n_mp * 4, s));
  k_mpc_decide<<<nb, PT_NT, 0, s>>>(*M, ix.start, *a, S, g->G.err);
  k_mpc_count<<<nb, PT_NT, 0, s>>>(ix.start, (int)cap, S);
  k_mpc_place<<<nb, PT_NT, 0, s>>>(ix.start, *a, S);
  k_mpc_erase<<<(unsigned)cap, 64, (size_t)pow2_at_least(g->K) * 8, s>>>(*M, g->G, ix.start, ix.csr, *a, S, g->K);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_map_point_culling(fb_covis *g, const fb_covis_map *HM, const fb_map_point_culling_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_TRY(check_culling(HM, ha));
  FB_ARG(ha->kf_mp == HM->kf_mp && (HM->n_mp == 0 || ha->mp_bad == HM->mp_bad) && (HM->n_obs == 0 || ha->obs_kf == HM->obs_kf));
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_map_point_culling_args A = *ha;
  const size_t K = g->K, S = M.kp_stride, n_mp = M.n_mp, n_obs = M.n_obs, cap = A.recent_cap;
  fb::Stager st;
  st.in(M.kf_n, K * 4); st.in(M.kf_octave, K * S); st.in(M.kf_order, K * 8); st.in(M.obs_mp, n_obs * 4); st.in(M.obs_idx, n_obs * 4);
  st.in(A.mp_first_kf_id, n_mp * 4); st.in(A.mp_found, n_mp * 4); st.in(A.mp_visible, n_mp * 4);
  // the three arrays the call edits are the map's: staged once
  st.out(A.kf_mp, K * S * 4, true); st.out(A.mp_bad, n_mp, true); st.out(A.obs_kf, n_obs * 4, true);
  st.out(A.d_recent, cap * 4, true); st.out(A.d_n_recent, 4, true);
  st.out(A.d_n_culled, 4, false); st.out(A.d_culled, cap * 4, true);
  st.out(A.d_n_erased, 4, false); st.out(A.d_erased, (size_t)A.erased_cap * 16, true);
  FB_TRY(st.commit(nullptr));
  M.kf_mp = A.kf_mp; M.mp_bad = A.mp_bad; M.obs_kf = A.obs_kf;
  IndexDropGuard drop(g->state);
  FB_TRY(fb_covis_map_point_culling_dev(g, &M, &A, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
