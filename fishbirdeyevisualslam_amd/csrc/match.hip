// match.hip -- ORBmatcher hot-path entry points as CDNA4 kernels (gfx950).
//
// Replaces (reference file:line):
//   DescriptorDistance                         src/ORBmatcher.cc:1951-1967
//   Frame::AssignFeaturesToGrid / PosInGrid*   src/Frame.cc:381-411, 548-570
//   Frame::GetFeaturesInArea[Birdview]         src/Frame.cc:493-546, 572-626
//   SearchByProjection(Frame&, const Frame&)   src/ORBmatcher.cc:1329-1471   (M3)
//   SearchByProjection(Frame&, vector<MP*>&)   src/ORBmatcher.cc:46-138      (M2)
//   BirdMapPointMatch                          src/ORBmatcher.cc:1763-1902   (M9)
//   BirdviewMatch (isProject=0)                src/ORBmatcher.cc:1602-1760   (M8)
//   ComputeThreeMaxima                         src/ORBmatcher.cc:1905-1946
//
// Layout: one workgroup per problem (frame pair).  The target frame's descriptor table
// (n x 32 B), keypoint x/y/octave and the grid CSR are staged once into LDS with coalesced
// 16-byte loads; every query lane then walks its grid window out of LDS and scores
// candidates with v_bcnt_u32_b32.  HBM traffic per problem is therefore the algorithmic
// minimum (each input byte read once, each output written once).
//
// Serial semantics: M2/M3/M4 skip a candidate that an EARLIER query already took (M2/M3: with a map
// point that has observations).  That dependency is resolved by the fixed-point iteration of
// fb_claims.h (fb::Claims: the rounds, the owner / assign arrays and their barriers; fb::commit_matches:
// assign array -> match array, count and rotation filter).  A kernel here only writes its own query loop
// between begin_round() and end_round().
#include "fb_common.h"

#include <type_traits>
#include "fb_claims.h"
#include "fb_distinctive.h"
#include "fb_edge_gather.h"
#include "fb_frame_geom.h"
#include "fb_primitives.h"
#include "fb_rot_hist.h"
#include "match_plan.h"

namespace {

constexpr int TH_HIGH = 100;      // ORBmatcher.cc:38
constexpr int TH_LOW = 50;        // :39
constexpr int NONE = 0x7fffffff;
constexpr int MATCH_THREADS = 1024;

struct TargetLds {  // target frame staged in LDS
  const uint4 *desc;     // [n][2]
  const float2 *xy;      // [n]
  const uint8_t *oct;    // [n] (nullptr when the kernel's callbacks do not ask for it: Carve::withOct)
  const uint16_t *cs;    // [ncell+1]
  const uint32_t *items; // [n] key point index | octave << 16 in cell order: the level test of a walk needs no second load
  uint32_t descLds;      // LDS byte address of the descriptor table, or DESC_NOT_IN_LDS (then `desc` points into HBM / L2)
};
constexpr uint32_t DESC_NOT_IN_LDS = 0xFFFFFFFFu;

// Distance of a query to key point i of the staged frame.  `desc` is a generic pointer (LDS or global, decided at launch), so
// reading through it is a FLAT load; the wave-uniform branch gives each side a typed load (ds_read_b128 /
// global_load_dwordx4).  Worth 2 % of k_proj_frame.  (Probe builds of that kernel's first round: callbacks compiled out 19 k
// of 135 k cycles, constant instead of this distance 131 k, no top-K insertion 21 k -- the insertion block of full_search is
// where the time goes)
__device__ __forceinline__ int target_hamming(const TargetLds &T, const uint32_t a[8], int i) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 b0, b1;
  if (T.descLds != DESC_NOT_IN_LDS) {
    typedef __attribute__((address_space(3))) const u32x4 lds_u4;
    lds_u4 *p = reinterpret_cast<lds_u4 *>((uintptr_t)(T.descLds + (uint32_t)i * 32u));
    b0 = p[0]; b1 = p[1];
  } else {
    typedef __attribute__((address_space(1))) const u32x4 glb_u4;
    glb_u4 *p = reinterpret_cast<glb_u4 *>((uintptr_t)(T.desc + (size_t)i * 2));
    b0 = p[0]; b1 = p[1];
  }
  return __popc(a[0] ^ b0.x) + __popc(a[1] ^ b0.y) + __popc(a[2] ^ b0.z) + __popc(a[3] ^ b0.w) +
         __popc(a[4] ^ b1.x) + __popc(a[5] ^ b1.y) + __popc(a[6] ^ b1.z) + __popc(a[7] ^ b1.w);
}

// Frame::GetFeaturesInArea (Frame.cc:493-546, inclusive cell loops) and
// Frame::GetFeaturesInAreaBirdview (Frame.cc:572-626, exclusive loops, no min offset).
template <bool BIRD, typename F>
__device__ __forceinline__ void for_area(const fb_grid_geom &g, const TargetLds &T, float x, float y, float r,
                                         int minLevel, int maxLevel, F &&f) {
  int nMinCellX, nMaxCellX, nMinCellY, nMaxCellY;
  if (BIRD) {
    nMinCellX = max(0, (int)floorf((x - r) * g.inv_w));
    if (nMinCellX >= g.cols) return;
    nMaxCellX = min(g.cols - 1, (int)ceilf((x + r) * g.inv_w));
    if (nMaxCellX < 0) return;
    nMinCellY = max(0, (int)floorf((y - r) * g.inv_h));
    if (nMinCellY >= g.rows) return;
    nMaxCellY = min(g.rows - 1, (int)ceilf((y + r) * g.inv_h));
    if (nMaxCellY < 0) return;
    nMaxCellX -= 1;  // ix < nMaxCellX
    nMaxCellY -= 1;
  } else {
    nMinCellX = max(0, (int)floorf((x - g.min_x - r) * g.inv_w));
    if (nMinCellX >= g.cols) return;
    nMaxCellX = min(g.cols - 1, (int)ceilf((x - g.min_x + r) * g.inv_w));
    if (nMaxCellX < 0) return;
    nMinCellY = max(0, (int)floorf((y - g.min_y - r) * g.inv_h));
    if (nMinCellY >= g.rows) return;
    nMaxCellY = min(g.rows - 1, (int)ceilf((y - g.min_y + r) * g.inv_h));
    if (nMaxCellY < 0) return;
  }
  const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
  // SIMT shape: the lanes of a wave walk different windows, so calling f (descriptor distance + bookkeeping) straight from the
  // item loop runs it once per loop position at which ANY lane has a key point, with one or two lanes active.  The key points a
  // lane finds are therefore queued -- eight 16-bit indices in four registers, oldest on top -- and f runs over the queues
  // after the walk: as many passes as the fullest queue of the wave, every lane that still has an entry taking part.  A full
  // queue is emptied on the spot.  The order in which a lane sees its key points is unchanged.  (Measured with the batched
  // loads below: round 0 of k_proj_frame 163 k -> 140 k cycles per frame, profiles/probes/m3_stamps.py.)
  uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
  int qn = 0;
  auto flush = [&]() {
    for (int t = qn - 1; t >= 0; t--) {  // position t: 0 = newest (low half of q0)
      const uint32_t w = (t >> 1) == 0 ? q0 : ((t >> 1) == 1 ? q1 : ((t >> 1) == 2 ? q2 : q3));
#ifndef FB_WALK_NO_F   // (probe builds: the walk skeleton alone, results wrong)
      f((int)((t & 1) ? (w >> 16) : (w & 0xFFFFu)));
#else
      asm volatile("" :: "v"(w));
#endif
    }
    qn = 0;
  };
  for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
    const int cbase = ix * g.rows;
    // cells (ix, nMinCellY..nMaxCellY) are contiguous in the CSR (cell id = ix*rows+iy)
    const int j0 = T.cs[cbase + nMinCellY], j1 = T.cs[cbase + nMaxCellY + 1];
    uint32_t itNext = j0 < j1 ? T.items[j0] : 0u;
    for (int j = j0; j < j1; j++) {
      // an item rejected by its level costs no LDS wait (the octave rides in the item word, the next item is in flight): the
      // windows of a dense region scan hundreds of items (up to 290 per walk on the bench's drive, 3.5 of them pass both tests)
      const uint32_t it = itNext;
      itNext = T.items[min(j + 1, j1 - 1)];
      const int idx = (int)(it & 0xFFFFu);
      if (bCheckLevels) {
        const int o = (int)(it >> 16);
        if (o < minLevel) continue;
        if (maxLevel >= 0 && o > maxLevel) continue;
      }
      const float2 p = T.xy[idx];
      const float distx = p.x - x, disty = p.y - y;
      if (fabsf(distx) < r && fabsf(disty) < r) {
        if (qn == 8) flush();
        q3 = (q3 << 16) | (q2 >> 16); q2 = (q2 << 16) | (q1 >> 16); q1 = (q1 << 16) | (q0 >> 16); q0 = (q0 << 16) | (uint32_t)idx;
        qn++;
      }
    }
  }
  flush();
}

using fb::rot_bin;

__device__ __forceinline__ void xform(const float *T, const float *X, float *o) {  // rows 0..2 of a 3x4
#pragma unroll
  for (int r = 0; r < 3; r++) o[r] = ((T[r * 4 + 0] * X[0] + T[r * 4 + 1] * X[1]) + T[r * 4 + 2] * X[2]) + T[r * 4 + 3];
}

__device__ __forceinline__ TargetLds stage_target(uint8_t *smem, const Carve &cv, int n, int ncell,
                                                  const fb_keypoint *kps, const uint8_t *desc, const int32_t *cs,
                                                  const int32_t *items, bool withDesc = true) {
  uint32_t *ldesc = reinterpret_cast<uint32_t *>(smem + cv.desc);
  float2 *lxy = reinterpret_cast<float2 *>(smem + cv.xy);
  uint8_t *loct = smem + cv.oct;
  uint16_t *lcs = reinterpret_cast<uint16_t *>(smem + cv.cs);
  uint32_t *litems = reinterpret_cast<uint32_t *>(smem + cv.items);
  const int tid = threadIdx.x, nt = blockDim.x;
  // descriptor table: n*32 B as 16-byte vectors (rows are 32-B aligned in the C-ABI arrays)
  const uint4 *src = reinterpret_cast<const uint4 *>(desc);
  uint4 *dst = reinterpret_cast<uint4 *>(ldesc);
  if (withDesc)
    for (int i = tid; i < n * 2; i += nt) dst[i] = src[i];
  for (int i = tid; i < n; i += nt) {
    const fb_keypoint k = kps[i];
    lxy[i] = make_float2(k.x, k.y);
    if (cv.hasOct) loct[i] = (uint8_t)k.octave;
  }
  for (int i = tid; i <= ncell; i += nt) lcs[i] = (uint16_t)cs[i];
  const int nitems = cs[ncell];
  for (int i = tid; i < nitems; i += nt) {
    const int idx = items[i];
    litems[i] = (uint32_t)idx | ((uint32_t)(kps[idx].octave & 0xff) << 16);
  }
  TargetLds T{withDesc ? reinterpret_cast<const uint4 *>(ldesc) : src, lxy, cv.hasOct ? loct : nullptr, lcs, litems,
              withDesc ? (uint32_t)(uintptr_t)ldesc : DESC_NOT_IN_LDS};
  return T;
}

// the staged target of the argument structs that call it cur_* (frame b of the batch)
template <typename Args>
__device__ __forceinline__ Carve cur_carve(const Args &A, bool descInLds, bool withOct = true) {
  return Carve(A.cur_stride, A.grid.cols * A.grid.rows, descInLds, withOct);
}
template <typename Args>
__device__ __forceinline__ TargetLds stage_cur(uint8_t *smem, const Carve &cv, const Args &A, int b, bool descInLds) {
  const int ncell = A.grid.cols * A.grid.rows;
  const size_t co = (size_t)b * A.cur_stride;
  return stage_target(smem, cv, A.n_cur[b], ncell, A.cur_kps + co, A.cur_desc + co * 32,
                      A.cur_cell_start + (size_t)b * (ncell + 1), A.cur_cell_items + co, descInLds);
}

// ---------------------------------------------------------------------------------------
// M3  SearchByProjection(CurrentFrame, LastFrame, th, bMono=true)
// ---------------------------------------------------------------------------------------
// Every round after the first re-decides each query from a per-query cache of its CACHE_K best admissible candidates
// (sorted by distance, ties in grid-walk order = the reference's "first minimum wins"), so the grid walk and the
// Hamming distances are done once; a query whose cached candidates are all taken and whose cache is incomplete
// falls back to the full walk.  cacheK = 0 (LDS too small) keeps the full walk every round.
// (Measured and dropped, round 3: round 0 -- projection, grid walk and distances of every query -- is 78 % of this kernel for
// one frame (profiles/probes/m3_stamps.py), so it was moved to its own grid of 256-query workgroups with the serial rule
// resolved on candidate lists afterwards, as M2 does.  Same results, no gain: 94 instead of 97 us per frame at batch 1 (a
// query's walk is a chain of dependent loads that is as long on its own workgroup, and the second kernel stages the grid
// again), and 0.226 instead of 0.137 ms per step at batch 256.)
#ifdef FB_MATCH_STAMPS
__device__ unsigned long long g_m3_stamps[8];  // probe build only (block 0): staging | order | round 0 | later rounds | commit | rounds | launches
#define M3_T0() unsigned long long mt_ = 0; if (blockIdx.x == 0 && threadIdx.x == 0) mt_ = __builtin_amdgcn_s_memtime();
#define M3_TICK(slot_) if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); atomicAdd(&g_m3_stamps[slot_], t_ - mt_); mt_ = t_; }
#define M3_COUNT(slot_) if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_m3_stamps[slot_], 1ull);
#else
#define M3_T0()
#define M3_TICK(slot_)
#define M3_COUNT(slot_)
#endif

// The body for frame b on a staged target T, whose cell lists came from the caller's arrays (k_proj_frame) or straight from
// the LDS of the grid build (k_frame_tail_front).  `own` = the first LDS byte behind the staged frame (Carve::end): none of the
// arrays there (M3Lds) is written before the first barrier here, so a caller may have staged from scratch arrays that lie there.  tail(matchL) runs once, by every thread, behind the stores of the
// final match array (matchL[i], i < ncur, in LDS).
template <typename Tail>
__device__ __forceinline__ void proj_frame_body(const fb_proj_frame_args &A, uint8_t *smem, size_t own, const TargetLds &T, int b,
                                                int cacheK, Tail &&tail) {
  // (its callbacks never ask for a target key point's octave by index: no by-index octave array in LDS, Carve::withOct = false)
  typedef unsigned short u16;
  const int tid = threadIdx.x, nt = blockDim.x;
  const size_t co = (size_t)b * A.cur_stride, lo = (size_t)b * A.last_stride;
  const int ncur = A.n_cur[b], nlast = A.n_last[b];
  M3_T0()
  M3Lds L;
  m3_layout(L, own, A.cur_stride, A.last_stride, cacheK);
  uint32_t *cache = lds_at<uint32_t>(smem, L.cache);
  u16 *perm = lds_at<u16>(smem, L.perm);
  uint8_t *meta = lds_at<uint8_t>(smem, L.meta);
  struct Shared { fb::ClaimFlags cf; int oct[FB_MAX_LEVELS + 1]; fb::RotHist rot; float T[12]; };
  __shared__ Shared s_;
  static_assert(up16(sizeof(Shared)) == STATIC_M3, "match_plan.h");
  auto &s_cf = s_.cf; auto &s_oct = s_.oct; auto &s_rot = s_.rot; auto &s_T = s_.T;
  if (tid < 12) s_T[tid] = A.cur_Tcw[(size_t)b * 12 + tid];
  if (tid <= FB_MAX_LEVELS) s_oct[tid] = 0;
  fb::Claims<u16> C(s_cf, lds_at<int>(smem, L.owners), A.cur_stride, lds_at<u16>(smem, L.assigns), A.last_stride,
                    A.cur_blocked ? A.cur_blocked + co : nullptr, ncur, nlast);
  float thEff = A.th;   // the second attempt (retry_below > 0 and fewer matches than that) searches with retry_th
  __syncthreads();
  M3_TICK(0)
  // The search radius depends only on the octave: hand the lanes of a wave queries of the same octave so that their
  // grid walks have the same length (the query INDEX keeps deciding priorities, only the processing order changes).
  auto oct_bin = [&](int q) -> int {
    const int o = A.last_valid[lo + q] ? A.last_octave[lo + q] : FB_MAX_LEVELS;
    return o < 0 ? 0 : (o > FB_MAX_LEVELS ? FB_MAX_LEVELS : o);
  };
  for (int q = tid; q < nlast; q += nt) atomicAdd(&s_oct[oct_bin(q)], 1);
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i <= FB_MAX_LEVELS; i++) { const int c = s_oct[i]; s_oct[i] = run; run += c; }
  }
  __syncthreads();
  for (int q = tid; q < nlast; q += nt) perm[atomicAdd(&s_oct[oct_bin(q)], 1)] = (u16)q;
  __syncthreads();
  M3_TICK(1)

  // full grid walk of query q against last round's claims; fill = also (re)build the query's cache.  The callback only APPENDS the eligible candidates (distance
  // <= TH_HIGH, walk order) to eight registers; the stable top-K selection runs after the walk, once, in straight-line code.
  // More than eight eligible candidates: the cache is left empty and incomplete, i.e. later rounds walk again.
  auto full_search = [&](int q, const bool fill) -> int {
    int best = NONE;
    uint32_t e0 = 0xFFFFFFFFu, e1 = e0, e2 = e0, e3 = e0, e4 = e0, e5 = e0, e6 = e0, e7 = e0;  // newest in e0
    int nElig = 0;
    if (A.last_valid[lo + q]) {
      float X[3] = {A.last_xw[(lo + q) * 3], A.last_xw[(lo + q) * 3 + 1], A.last_xw[(lo + q) * 3 + 2]};
      float pc[3];
      xform(s_T, X, pc);
      const float xc = pc[0], yc = pc[1];
      const float invzc = (float)(1.0 / pc[2]);
      if (!(invzc < 0)) {
        const float u = A.cam.fx * xc * invzc + A.cam.cx;
        const float v = A.cam.fy * yc * invzc + A.cam.cy;
        if (!(u < A.cam.min_x || u > A.cam.max_x) && !(v < A.cam.min_y || v > A.cam.max_y)) {
          const int oct = A.last_octave[lo + q];
          const float radius = thEff * A.scale_factors[oct];
          uint32_t d[8];
          fb::load_desc(A.last_desc + (lo + q) * 32, d);
          int bestDist = 256;
          for_area<false>(A.grid, T, u, v, radius, oct - 1, oct + 1, [&](int i2) {
            const int own = C.owner(i2);
            if (own == C.BLOCKED) return;  // occupied on entry: never a candidate
            const int dist = target_hamming(T, d, i2);
            if (fill && dist <= TH_HIGH) {
              nElig++;
              e7 = e6; e6 = e5; e5 = e4; e4 = e3; e3 = e2; e2 = e1; e1 = e0;
              e0 = ((uint32_t)dist << 16) | (uint32_t)i2;
            }
            if (own < q) return;        // taken by an earlier query
            if (dist < bestDist) { bestDist = dist; best = i2; }
          });
          if (bestDist > TH_HIGH) best = NONE;
        }
      }
    }
    if (fill) {
      // stable top-K by distance over the recorded candidates, oldest first (equal keys keep walk order; once an entry has
      // been displaced everything behind it moves down one place: comparing the displaced entry again would let it jump over
      // an equal-distance neighbour and break the walk order among ties)
      uint32_t top[CACHE_K];
#pragma unroll
      for (int k = 0; k < CACHE_K; k++) top[k] = 0xFFFFFFFFu;
      const bool over = nElig > 8;
      const uint32_t ent[8] = {e7, e6, e5, e4, e3, e2, e1, e0};  // position 7 = newest; the oldest recorded one is at 8 - nElig
#pragma unroll
      for (int i = 0; i < 8; i++) {
        if (i >= 8 - nElig && !over) {
          uint32_t e = ent[i];
          bool shift = false;
#pragma unroll
          for (int k = 0; k < CACHE_K; k++) {
            if (shift || (e >> 16) < (top[k] >> 16)) { const uint32_t t = top[k]; top[k] = e; e = t; shift = true; }
          }
        }
      }
      const int n = over ? 0 : (nElig < CACHE_K ? nElig : CACHE_K);
      uint32_t *cq = cache + (uint32_t)q * CACHE_K;
#pragma unroll
      for (int k = 0; k < CACHE_K; k++) cq[k] = top[k];
      meta[q] = (uint8_t)(n | ((nElig <= CACHE_K) ? 0x80 : 0));
    }
    return best;
  };

  // Tracking.cc:1339-1349 in one launch: nmatches = SearchByProjection(th); if (nmatches < 20) { fill(mvpMapPoints, NULL);
  // nmatches = SearchByProjection(2 * th); } -- the second search starts from scratch on the staged frame
  for (int attempt = 0; attempt < 2; attempt++) {
  C.start();
  for (int round = 0; C.more(round); round++) {
    C.begin_round();
    for (int pq = tid; pq < nlast; pq += nt) {
      const int q = perm[pq];
      int best = NONE;
      bool walk = round == 0 || cacheK == 0;
      const bool fillNow = walk && cacheK > 0;
      if (!walk) {
        const int m = meta[q], n = m & 0x7f;
        for (int k = 0; k < n; k++) {
          const int i2 = (int)(cache[(size_t)q * cacheK + k] & 0xFFFFu);
          if (!C.taken(i2, q)) { best = i2; break; }
        }
        walk = best == NONE && !(m & 0x80);
      }
      if (walk) best = full_search(q, fillNow);   // ONE call site: one copy of the walk and its callbacks in the kernel
      C.submit(q, best, best != NONE && A.last_obs_pos[lo + q]);
    }
    const bool done = C.end_round();
    if (round == 0) { M3_TICK(2) } else { M3_TICK(3) }
    M3_COUNT(5)
    if (done) break;
  }

  // commit: last writer wins; rotation histogram culling (ORBmatcher.cc:1446-1468)
  const int *matchL = fb::commit_matches<true>(C, fb::QueryIndex(), &s_rot, A.matcher.check_orientation != 0,
                                               [&](int q, int c) { return A.last_angle[lo + q] - A.cur_kps[co + c].angle; });
  if (attempt == 0 && A.retry_below > 0 && s_cf.n < A.retry_below) {  // (workgroup-uniform)
    thEff = A.retry_th;
    // matchL and the bins alias C.ownerB / C.assignB: which of the two buffers holds what is irrelevant for a search from
    // scratch (C.start() refills both A buffers, begin_round() the B owners)
    __syncthreads();
    continue;
  }
  for (int i = tid; i < ncur; i += nt) A.match_cur_to_last[co + i] = matchL[i];
  if (tid == 0) { A.nmatches[b] = s_cf.n; if (A.retried) A.retried[b] = attempt; }
  tail(matchL);
  break;
  }
  M3_TICK(4)
  M3_COUNT(6)
}

__global__ __launch_bounds__(MATCH_THREADS) void k_proj_frame(fb_proj_frame_args A, int cacheK, int descInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x;
  const Carve cv = cur_carve(A, descInLds != 0, false);
  const TargetLds T = stage_cur(smem, cv, A, b, descInLds != 0);
  proj_frame_body(A, smem, cv.end, T, b, cacheK, [](const int *) {});
}

// ---------------------------------------------------------------------------------------
// M4  SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)  (ORBmatcher.cc:1473-1600)
// Same greedy structure as M3; the search level comes from MapPoint::PredictScale and every
// accepted slot blocks all later key-frame points (mvpMapPoints[i2] != NULL, :1545).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(MATCH_THREADS) void k_proj_kf(fb_proj_kf_args A, int descInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const size_t co = (size_t)b * A.cur_stride, ko = (size_t)b * A.kf_stride;
  const int ncur = A.n_cur[b], nkf = A.n_kf[b];
  const Carve cv = cur_carve(A, descInLds != 0);
  const TargetLds T = stage_cur(smem, cv, A, b, descInLds != 0);
  struct Shared { fb::ClaimFlags cf; fb::RotHist rot; float T[12], Ow[3]; };
  __shared__ Shared s_;
  static_assert(up16(sizeof(Shared)) == STATIC_M4, "match_plan.h");
  auto &s_cf = s_.cf; auto &s_rot = s_.rot; auto &s_T = s_.T; auto &s_Ow = s_.Ow;
  if (tid < 12) s_T[tid] = A.cur_Tcw[(size_t)b * 12 + tid];
  if (tid == 64) fb::camera_centre(A.cur_Tcw + (size_t)b * 12, s_Ow);
  ClaimsLds L;  // the chosen slot of each point in 16 bits
  claims_layout(L, cv.end, A.cur_stride, A.kf_stride, 2, CLAIMS_U16_SLACK);
  fb::Claims<uint16_t> C(s_cf, lds_at<int>(smem, L.owners), A.cur_stride, lds_at<uint16_t>(smem, L.assigns), A.kf_stride,
                         A.cur_blocked ? A.cur_blocked + co : nullptr, ncur, nkf);
  C.start();

  // the geometric gates are cheap and are re-evaluated every round instead of being stored per point
  auto gate = [&](int q, float &u, float &v) -> int {
    if (!A.kf_valid[ko + q]) return -1;
    const float X[3] = {A.kf_xw[(ko + q) * 3], A.kf_xw[(ko + q) * 3 + 1], A.kf_xw[(ko + q) * 3 + 2]};
    float pc[3];
    xform(s_T, X, pc);
    const float invzc = (float)(1.0 / pc[2]);
    u = A.cam.fx * pc[0] * invzc + A.cam.cx;
    v = A.cam.fy * pc[1] * invzc + A.cam.cy;
    if ((u < A.cam.min_x || u > A.cam.max_x) || (v < A.cam.min_y || v > A.cam.max_y)) return -1;
    const float dist3D = fb::norm3(X[0] - s_Ow[0], X[1] - s_Ow[1], X[2] - s_Ow[2]);
    const float maxD = A.kf_max_dist[ko + q];
    if (dist3D < 0.8f * A.kf_min_dist[ko + q] || dist3D > 1.2f * maxD) return -1;
    return fb::predict_scale(maxD, dist3D, A.log_scale_factor, A.n_levels);
  };

  for (int round = 0; C.more(round); round++) {
    C.begin_round();
    for (int q = tid; q < nkf; q += nt) {
      int best = NONE;
      float u, v;
      const int lvl = gate(q, u, v);
      if (lvl >= 0) {
        const float radius = A.th * A.scale_factors[lvl];
        uint32_t d[8];
        fb::load_desc(A.kf_desc + (ko + q) * 32, d);
        int bestDist = 256;
        for_area<false>(A.grid, T, u, v, radius, lvl - 1, lvl + 1, [&](int i2) {
          if (C.taken(i2, q)) return;
          const int dist = target_hamming(T, d, i2);
          if (dist < bestDist) { bestDist = dist; best = i2; }
        });
        if (bestDist > A.orb_dist) best = NONE;
      }
      C.submit(q, best);
    }
    if (C.end_round()) break;
  }
  // a claimed slot blocks every later point: one claimer per slot
  const int *matchL = fb::commit_matches<false>(C, fb::QueryIndex(), &s_rot, A.matcher.check_orientation != 0,
                                                [&](int q, int c) { return A.kf_angle[ko + q] - A.cur_kps[co + c].angle; });
  for (int i = tid; i < ncur; i += nt) A.match_cur_to_kf[co + i] = matchL[i];
  if (tid == 0) A.nmatches[b] = s_cf.n;
}

// ---------------------------------------------------------------------------------------
// M2  SearchByProjection(Frame&, const vector<MapPoint*>&, th)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float m2_radius(const fb_proj_points_args &A, size_t e, bool bFactor, int lvl) {
  float r = A.mp_view_cos[e] > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos
  if (bFactor) r *= A.th;
  return r * A.scale_factors[lvl];
}

// The M2 decision (ORBmatcher.cc:85-127): best and second-best admissible candidate in walk order, then TH_HIGH and, when
// both sit on the same level, the ratio test.
struct M2Pick {
  int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
  __device__ __forceinline__ void take(int idx, int dist, int lev) {
    if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = lev; bestIdx = idx; }
    else if (dist < bestDist2) { bestLevel2 = lev; bestDist2 = dist; }
  }
  __device__ __forceinline__ int result(float nnratio) const {
    return (bestDist <= TH_HIGH && !(bestLevel == bestLevel2 && bestDist > nnratio * bestDist2)) ? bestIdx : NONE;
  }
};

#ifdef FB_MATCH_STAMPS
__device__ int g_m2_rounds[4];  // probe build only: rounds / queries in view / launches of k_proj_points (block 0)
#endif
// the full grid walk of query q (point e = mo + q) against last round's claims
__device__ __forceinline__ void m2_walk(const fb_proj_points_args &A, const TargetLds &T, const fb::Claims<int> &C, size_t e, int q,
                                        M2Pick &pick) {
  const int lvl = A.mp_level[e];
  uint32_t d[8];
  fb::load_desc(A.mp_desc + e * 32, d);
  for_area<false>(A.grid, T, A.mp_proj[e * 2], A.mp_proj[e * 2 + 1], m2_radius(A, e, A.th != 1.0f, lvl), lvl - 1, lvl, [&](int idx) {
    if (!C.taken(idx, q)) pick.take(idx, target_hamming(T, d, idx), (int)T.oct[idx]);
  });
}

// M2 behind the staging of frame b: the rounds of the fixed point, the commit and the store of the results.  `own` = the
// first LDS byte behind the staged frame (ClaimsLds).  pick(C, q) = how a query picks given last round's claims: its target
// or NONE.  count: the probe counters (k_proj_points only).
template <typename Pick>
__device__ __forceinline__ void m2_rounds(const fb_proj_points_args &A, uint8_t *smem, size_t own, int b, bool count, Pick &&pick) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const size_t co = (size_t)b * A.cur_stride, mo = (size_t)b * A.mp_stride;
  const int ncur = A.n_cur[b], nmp = A.n_mp[b];
  __shared__ fb::ClaimFlags s_cf;
  static_assert(up16(sizeof(s_cf)) == STATIC_M2, "match_plan.h");
  ClaimsLds L;
  claims_layout(L, own, A.cur_stride, A.mp_stride, 4, 0);
  fb::Claims<int> C(s_cf, lds_at<int>(smem, L.owners), A.cur_stride, lds_at<int>(smem, L.assigns), A.mp_stride,
                    A.cur_blocked ? A.cur_blocked + co : nullptr, ncur, nmp);
  C.start();
  for (int round = 0; C.more(round); round++) {
    C.begin_round();
    for (int q = tid; q < nmp; q += nt) {
      const int best = pick(C, q);
      C.submit(q, best, best != NONE && A.mp_obs_pos[mo + q]);
    }
    const bool done = C.end_round();
#ifdef FB_MATCH_STAMPS
    if (count && b == 0 && tid == 0) atomicAdd(&g_m2_rounds[0], 1);
#endif
    if (done) break;
  }
#ifdef FB_MATCH_STAMPS
  if (count && b == 0 && tid == 0) { atomicAdd(&g_m2_rounds[2], 1); int c = 0; for (int q = 0; q < nmp; q++) c += A.mp_track[mo + q]; atomicAdd(&g_m2_rounds[1], c); }
#endif
  const int *matchL = fb::commit_matches<true>(C, fb::QueryIndex());  // last writer wins
  for (int i = tid; i < ncur; i += nt) A.match_cur_to_mp[co + i] = matchL[i];
  if (tid == 0) A.nmatches[b] = s_cf.n;
}

__global__ __launch_bounds__(MATCH_THREADS) void k_proj_points(fb_proj_points_args A, int descInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x;
  const size_t mo = (size_t)b * A.mp_stride;
  const Carve cv = cur_carve(A, descInLds != 0);
  const TargetLds T = stage_cur(smem, cv, A, b, descInLds != 0);
  m2_rounds(A, smem, cv.end, b, true, [&](const fb::Claims<int> &C, int q) -> int {  // every round walks the grid
    if (!A.mp_track[mo + q]) return NONE;
    M2Pick pick;
    m2_walk(A, T, C, mo + q, q, pick);
    return pick.result(A.matcher.nnratio);
  });
}

// ---------------------------------------------------------------------------------------
// M2 in two phases (taken when the caller provides a workspace): the expensive, owner-independent part of a query -- the
// grid walk and the Hamming distances of its candidates -- is done ONCE, by many workgroups per problem; the serial
// "already taken" rule is then resolved by one workgroup per problem on the cached candidate lists.  In the one-kernel
// version every round repeated every walk inside a single workgroup: 0.68 ms per frame for a 4000-point local map at
// batch 1 (rocprof, round 3), most of a tracked frame.
//   candidate record: dist << 20 | octave << 16 | key point index, in grid-walk order (the order decides ties);
//   M2_K records per query + a count; a query with more candidates keeps count = M2_OVER and is walked again each round.
// ---------------------------------------------------------------------------------------
constexpr int M2_K = 8, M2_OVER = 255, M2_CAND_THREADS = 256;

__global__ __launch_bounds__(M2_CAND_THREADS) void k_m2_candidates(fb_proj_points_args A, uint32_t *cand, uint8_t *ncand) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const size_t mo = (size_t)b * A.mp_stride;
  const int nmp = A.n_mp[b];
  if ((int)(blockIdx.x * M2_CAND_THREADS) >= nmp) return;
  const TargetLds T = stage_cur(smem, cur_carve(A, false), A, b, false);  // the grid only: descriptors from HBM / L2
  __syncthreads();
  const int q = blockIdx.x * M2_CAND_THREADS + tid;
  if (q >= nmp) return;
  int n = 0;
  if (A.mp_track[mo + q]) {
    const int lvl = A.mp_level[mo + q];
    uint32_t d[8];
    fb::load_desc(A.mp_desc + (mo + q) * 32, d);
    uint32_t *out = cand + (mo + q) * M2_K;
    for_area<false>(A.grid, T, A.mp_proj[(mo + q) * 2], A.mp_proj[(mo + q) * 2 + 1], m2_radius(A, mo + q, A.th != 1.0f, lvl), lvl - 1, lvl,
                    [&](int idx) {
      if (n < M2_K) {
        const int dist = target_hamming(T, d, idx);
        out[n] = ((uint32_t)dist << 20) | ((uint32_t)T.oct[idx] << 16) | (uint32_t)idx;
      }
      n++;
    });
    if (n > M2_K) n = M2_OVER;
  }
  ncand[mo + q] = (uint8_t)n;
}

__global__ __launch_bounds__(MATCH_THREADS) void k_m2_resolve(fb_proj_points_args A, const uint32_t *cand, const uint8_t *ncand) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x;
  const size_t mo = (size_t)b * A.mp_stride;
  const Carve cv = cur_carve(A, false);
  const TargetLds T = stage_cur(smem, cv, A, b, false);
  m2_rounds(A, smem, cv.end, b, false, [&](const fb::Claims<int> &C, int q) -> int {  // a round reads the query's cached list
    const int nc = ncand[mo + q];
    if (nc == 0) return NONE;
    M2Pick pick;
    if (nc != M2_OVER) {
      const uint4 *cq = reinterpret_cast<const uint4 *>(cand + (mo + q) * M2_K);
      const uint4 c0 = cq[0];
      uint32_t c[M2_K] = {c0.x, c0.y, c0.z, c0.w, 0, 0, 0, 0};
      if (nc > 4) { const uint4 c1 = cq[1]; c[4] = c1.x; c[5] = c1.y; c[6] = c1.z; c[7] = c1.w; }
#pragma unroll
      for (int k = 0; k < M2_K; k++) {
        if (k >= nc) break;
        const int idx = (int)(c[k] & 0xFFFFu);
        if (C.taken(idx, q)) continue;
        pick.take(idx, (int)(c[k] >> 20), (int)((c[k] >> 16) & 0xF));
      }
    } else {  // more candidates than the cache holds: the full walk, descriptors from HBM / L2
      m2_walk(A, T, C, mo + q, q, pick);
    }
    return pick.result(A.matcher.nnratio);
  });
}

// ---------------------------------------------------------------------------------------
// M9  BirdMapPointMatch
// ---------------------------------------------------------------------------------------
// The body for frame b on a staged target T.  writer = BirdLds::writer, not written before the first barrier here.  cam = the
// frame's mvKeysBirdCamXYZ, [ncur][3], in global memory or LDS.  commit(writer) runs once, by every thread, behind the last
// barrier: writer[i], i < ncur, is the reference point that took key point i, or -1.
template <typename Commit>
__device__ __forceinline__ void bird_mappoints_body(const fb_bird_mp_args &A, const TargetLds &T, int *writer, int b, const float *cam,
                                                    Commit &&commit) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const size_t ro = (size_t)b * A.ref_stride;
  const int ncur = A.n_cur[b], nref = A.n_ref[b];
  struct Shared { float Tcw[12], Tbw[12]; int n; };
  __shared__ Shared s_;
  static_assert(up16(sizeof(Shared)) == STATIC_BIRD_MP, "match_plan.h");
  auto &s_Tcw = s_.Tcw; auto &s_Tbw = s_.Tbw; auto &s_n = s_.n;
  if (tid < 12) s_Tcw[tid] = A.cur_Tcw[(size_t)b * 12 + tid];
  for (int i = tid; i < ncur; i += nt) writer[i] = -1;
  if (tid == 0) s_n = 0;
  __syncthreads();
  if (tid < 12) {  // Tbw = Frame::Tbc * CurF.mTcw, ORBmatcher.cc:1784
    const int r = tid / 4, c = tid % 4;
    float s = (A.Tbc[r * 4 + 0] * s_Tcw[0 * 4 + c] + A.Tbc[r * 4 + 1] * s_Tcw[1 * 4 + c]) + A.Tbc[r * 4 + 2] * s_Tcw[2 * 4 + c];
    if (c == 3) s = s + A.Tbc[r * 4 + 3];
    s_Tbw[tid] = s;
  }
  __syncthreads();
  for (int i1 = tid; i1 < nref; i1 += nt) {
    if (!A.ref_valid[ro + i1]) continue;
    const float X[3] = {A.ref_xw[(ro + i1) * 3], A.ref_xw[(ro + i1) * 3 + 1], A.ref_xw[(ro + i1) * 3 + 2]};
    float lp[3];
    xform(s_Tbw, X, lp);
    if (fabsf(lp[2]) > 0.2) continue;
    // Converter::BaseXY2BirdPixel, Converter.cc:304-310
    const float ptx = (float)(A.bird_cols / 2 - lp[1] * A.meter2pixel);
    const float pty = (float)(A.bird_rows / 2 - (lp[0] - A.rear_axle_to_center) * A.meter2pixel);
    if (ptx < 0 || ptx >= A.bird_cols || pty < 0 || pty >= A.bird_rows) continue;
    uint32_t d[8];
    fb::load_desc(A.ref_desc + (ro + i1) * 32, d);
    int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx = -1;
    for_area<true>(A.grid, T, ptx, pty, (float)A.window_size, -1, -1, [&](int i2) {
      if (i2 >= ncur) return;
      const int dist = target_hamming(T, d, i2);
      if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx = i2; }
      else if (dist < bestDist2) bestDist2 = dist;
    });
    if (bestDist > TH_LOW) continue;
    if (!(bestDist < (float)bestDist2 * A.matcher.nnratio)) continue;
    if (!(bestIdx > 0)) continue;  // sic: vnMatches12[i1] > 0, ORBmatcher.cc:1871
    float pc[3];
    xform(s_Tcw, X, pc);
    const float *qv = cam + (size_t)bestIdx * 3;
    const float e0 = pc[0] - qv[0], e1 = pc[1] - qv[1], e2 = pc[2] - qv[2];
    const double disC = sqrt((double)e0 * e0 + (double)e1 * e1 + (double)e2 * e2);
    if (disC < A.filter_size) {
      atomicMax(&writer[bestIdx], i1);  // later i1 overwrites earlier
      atomicAdd(&s_n, 1);
    }
  }
  __syncthreads();
  commit(writer);
  if (tid == 0) A.ninliers[b] = s_n;
}

__global__ __launch_bounds__(MATCH_THREADS) void k_bird_mappoints(fb_bird_mp_args A, int descInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const size_t co = (size_t)b * A.cur_stride;
  const int ncur = A.n_cur[b];
  const Carve cv = cur_carve(A, descInLds != 0);
  const TargetLds T = stage_cur(smem, cv, A, b, descInLds != 0);
  BirdLds L;
  bird_layout(L, cv.end, A.cur_stride, false);
  bird_mappoints_body(A, T, lds_at<int>(smem, L.writer), b, A.cur_cam_xyz + co * 3, [&](const int *writer) {  // the caller pre-filled the match array
    for (int i = tid; i < ncur; i += nt)
      if (writer[i] >= 0) A.match_cur_to_ref[co + i] = writer[i];
  });
}

// ---------------------------------------------------------------------------------------
// M8  BirdviewMatch, isProject = 0
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(MATCH_THREADS) void k_birdview(fb_birdview_args A, int descInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const size_t co = (size_t)b * A.cur_stride, ro = (size_t)b * A.ref_stride;
  const int ncur = A.n_cur[b], nref = A.n_ref[b];
  const Carve cv = cur_carve(A, descInLds != 0);
  const TargetLds T = stage_cur(smem, cv, A, b, descInLds != 0);
  BirdviewLds L;
  birdview_layout(L, cv.end, A.ref_stride);
  int *m12 = lds_at<int>(smem, L.m12);
  int *bins = lds_at<int>(smem, L.bins);  // histogram bin of i1 or -1
  struct Shared { int n, nd; fb::RotHist rot; };
  __shared__ Shared s_;
  static_assert(up16(sizeof(Shared)) == STATIC_BIRDVIEW, "match_plan.h");
  auto &s_n = s_.n; auto &s_nd = s_.nd; auto &s_rot = s_.rot;
  s_rot.clear();
  if (tid == 0) { s_n = 0; s_nd = 0; }
  __syncthreads();
  const bool ori = A.matcher.check_orientation != 0;
  for (int i1 = tid; i1 < nref; i1 += nt) {
    int m = -1, md = INT_MAX, bin = -1;
    const fb_keypoint kp1 = A.ref_kps[ro + i1];
    if (!(kp1.octave > 0)) {
      uint32_t d[8];
      fb::load_desc(A.ref_desc + (ro + i1) * 32, d);
      int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx = -1;
      for_area<true>(A.grid, T, kp1.x, kp1.y, (float)A.window_size, kp1.octave, kp1.octave, [&](int i2) {
        if (i2 >= ncur) return;
        const int dist = target_hamming(T, d, i2);
        if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx = i2; }
        else if (dist < bestDist2) bestDist2 = dist;
      });
      if (bestDist <= TH_LOW) {
        if (bestDist < (float)bestDist2 * A.matcher.nnratio) { m = bestIdx; md = bestDist; atomicAdd(&s_n, 1); }
        if (ori) {  // pushed even when the ratio test failed, ORBmatcher.cc:1712-1722
          bin = rot_bin(kp1.angle - A.cur_kps[co + bestIdx].angle);
          s_rot.add(bin);
        }
      }
    }
    m12[i1] = m;
    bins[i1] = bin;
    A.match_dist[ro + i1] = md;
  }
  __syncthreads();
  if (ori) {
    s_rot.pick();
    for (int i1 = tid; i1 < nref; i1 += nt) {
      const int bin = bins[i1];
      if (bin < 0 || s_rot.keeps(bin)) continue;
      if (m12[i1] >= 0) { m12[i1] = -1; atomicSub(&s_n, 1); }
    }
    __syncthreads();
  }
  for (int i1 = tid; i1 < nref; i1 += nt) {
    const int m = m12[i1];
    A.match_ref_to_cur[ro + i1] = m;
    if (m > 0) atomicAdd(&s_nd, 1);  // sic: > 0, ORBmatcher.cc:1755
  }
  __syncthreads();
  if (tid == 0) { A.nmatches[b] = s_n; A.n_dmatches[b] = s_nd; }
}

// ---------------------------------------------------------------------------------------
// DescriptorDistance over n row pairs; one lane per pair, 2 x 16-byte loads per row.
// ---------------------------------------------------------------------------------------
__global__ void k_descriptor_distance(const uint4 *__restrict__ a, const uint4 *__restrict__ b, int n,
                                      int32_t *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 a0 = a[2 * i], a1 = a[2 * i + 1], b0 = b[2 * i], b1 = b[2 * i + 1];
  out[i] = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// ---------------------------------------------------------------------------------------
// AssignFeaturesToGrid: one workgroup per frame. count -> scan -> scatter -> per-cell sort
// (cells hold <1 keypoint on average; the sort restores ascending keypoint index, which is
// the push_back order of Frame.cc:389-396).
// ---------------------------------------------------------------------------------------
// The body for one frame, by the NT threads of a workgroup: cnt [ncell+1] and fillp [ncell] live in LDS; ci [kp_stride] is
// where the items are scattered and sorted (LDS, or the frame's global array).  On return (behind a barrier) cnt holds the
// cell starts and ci the items; nothing has been stored for the caller yet.
template <int NT>
__device__ __forceinline__ void grid_build_body(const fb_keypoint *__restrict__ k, int nk, const fb_grid_geom &g, int *cnt,
                                                int *fillp, int *ci) {
  const int tid = threadIdx.x, nt = NT;
  const int ncell = g.cols * g.rows;
  __shared__ int s_part[NT / 64];
  static_assert(sizeof(s_part) == (NT == 256 ? SCAN_PART_BYTES_256 : SCAN_PART_BYTES_1024), "match_plan.h");
  for (int i = tid; i <= ncell; i += nt) cnt[i] = 0;
  __syncthreads();
  auto cell_of = [&](const fb_keypoint &kp) -> int {
    const int posX = (int)roundf((kp.x - g.min_x) * g.inv_w);  // PosInGrid, Frame.cc:548-558
    const int posY = (int)roundf((kp.y - g.min_y) * g.inv_h);
    if (posX < 0 || posX >= g.cols || posY < 0 || posY >= g.rows) return -1;
    return posX * g.rows + posY;
  };
  for (int i = tid; i < nk; i += nt) {
    const int c = cell_of(k[i]);
    if (c >= 0) atomicAdd(&cnt[c], 1);
  }
  __syncthreads();
  // exclusive scan over ncell counters: per-thread chunk sums, then scan of the NT partials
  const int chunk = (ncell + nt - 1) / nt;
  const int c0 = min(tid * chunk, ncell), c1 = min(c0 + chunk, ncell);
  int s = 0;
  for (int c = c0; c < c1; c++) s += cnt[c];
  // exclusive scan of the NT chunk sums: shuffles inside a wave, the wave totals through LDS (one lane walking the
  // partials in LDS was half of k_grid_build at batch 1)
  int tot;
  int run = fb::block_excl_scan<NT>(s, s_part, &tot);
  if (tid == 0) cnt[ncell] = tot;
  __syncthreads();
  for (int c = c0; c < c1; c++) { const int v = cnt[c]; cnt[c] = run; fillp[c] = run; run += v; }
  __syncthreads();
  for (int i = tid; i < nk; i += nt) {
    const int c = cell_of(k[i]);
    if (c >= 0) ci[atomicAdd(&fillp[c], 1)] = i;
  }
  __syncthreads();
  __threadfence_block();
  for (int c = tid; c < ncell; c += nt) {  // insertion sort inside each cell
    const int a0 = cnt[c], a1 = cnt[c + 1];
    for (int i = a0 + 1; i < a1; i++) {
      const int v = ci[i];
      int j = i - 1;
      while (j >= a0 && ci[j] > v) { ci[j + 1] = ci[j]; j--; }
      ci[j + 1] = v;
    }
  }
  __syncthreads();
}

// the frame's CSR from LDS (or, for the items, from where they already are) to the caller's arrays
__device__ __forceinline__ void grid_store(const int *cnt, const int *li, int ncell, int32_t *cs, int32_t *cig) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i <= ncell; i += nt) cs[i] = cnt[i];
  if (li != cig) {
    const int nitems = cnt[ncell];
    for (int i = tid; i < nitems; i += nt) cig[i] = li[i];
  }
}

__global__ __launch_bounds__(256) void k_grid_build(const fb_keypoint *__restrict__ kps, const int32_t *__restrict__ n,
                                                    int kp_stride, fb_grid_geom g, int32_t *__restrict__ cell_start,
                                                    int32_t *__restrict__ cell_items, int itemsInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x;
  const int ncell = g.cols * g.rows;
  GridLds L;
  grid_layout(L, 0, ncell, kp_stride, itemsInLds != 0);
  int *cnt = lds_at<int>(smem, L.cnt);
  // the items are scattered, sorted per cell and written out from LDS (itemsInLds): the per-cell insertion sort on the
  // global array was a chain of dependent global accesses per cell, 12 cells per lane -- most of this kernel at batch 1
  int32_t *cig = cell_items + (size_t)b * kp_stride;
  int *ci = itemsInLds ? lds_at<int>(smem, L.items) : cig;
  grid_build_body<256>(kps + (size_t)b * kp_stride, min(max(n[b], 0), kp_stride), g, cnt, lds_at<int>(smem, L.fillp), ci);
  grid_store(cnt, ci, ncell, cell_start + (size_t)b * (ncell + 1), cig);
}

// Frame.cc:365-373: BirdPixel2BaseXY (Converter.cc:284-292) then BaseXY2CamXYZ (:312-318)
struct BirdCamK {
  int cols, rows;
  double pixel2meter, rear;
  float Tcb[12];
};
__device__ __forceinline__ void bird_key_to_cam(const fb_keypoint &kp, const BirdCamK &K, float o[3]) {
  float p[3];
  p[0] = (float)((K.rows / 2 - kp.y) * K.pixel2meter + K.rear);
  p[1] = (float)((K.cols / 2 - kp.x) * K.pixel2meter);
  p[2] = 0.f;
  xform(K.Tcb, p, o);
}
__global__ void k_bird_keys_to_cam(const fb_keypoint *__restrict__ kps, const int32_t *__restrict__ n, int kp_stride,
                                   BirdCamK K, float *__restrict__ cam) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n[b]) return;
  float o[3];
  bird_key_to_cam(kps[(size_t)b * kp_stride + i], K, o);
  float *dst = cam + ((size_t)b * kp_stride + i) * 3;
  dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

// ---------------------------------------------------------------------------------------
// The per-frame tail of the tracking step in one launch per camera, one workgroup per frame pair:
//   front: AssignFeaturesToGrid -> M3 -> front edges of PoseOptimizationWithBird, n_front, SetPose(prediction)
//   bird : AssignFeaturesToGrid -> mvKeysBirdCamXYZ -> M9 on a fresh mvpMapPointsBird -> bird edges, n_bird, fresh mvBirdOutlier
// The cell lists are built in LDS and staged from there (they are still stored: callers read them); the grid's scratch arrays
// lie where the matcher's own arrays begin (GridLds at Carve::end) and are dead before those are first written.
// ---------------------------------------------------------------------------------------
struct GridScratch { int *cnt, *fillp, *items; };
// builds frame b's grid at LDS offset `at`, stores it to cell_start / cell_items (written here, whatever the struct's const says)
template <typename Args>
__device__ __forceinline__ GridScratch tail_grid(uint8_t *smem, size_t at, const Args &A, int b, bool itemsInLds) {
  const int ncell = A.grid.cols * A.grid.rows;
  const size_t co = (size_t)b * A.cur_stride;
  GridLds L;
  grid_layout(L, at, ncell, A.cur_stride, itemsInLds);
  GridScratch G;
  G.cnt = lds_at<int>(smem, L.cnt);
  G.fillp = lds_at<int>(smem, L.fillp);
  int32_t *cig = const_cast<int32_t *>(A.cur_cell_items) + co;
  G.items = itemsInLds ? lds_at<int>(smem, L.items) : cig;
  grid_build_body<MATCH_THREADS>(A.cur_kps + co, min(max(A.n_cur[b], 0), A.cur_stride), A.grid, G.cnt, G.fillp, G.items);
  grid_store(G.cnt, G.items, ncell, const_cast<int32_t *>(A.cur_cell_start) + (size_t)b * (ncell + 1), cig);
  return G;
}

__global__ __launch_bounds__(MATCH_THREADS) void k_frame_tail_front(fb_frame_tail_front_args F, int cacheK, int descInLds,
                                                                    int itemsInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const fb_proj_frame_args &A = F.m3;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int ncell = A.grid.cols * A.grid.rows;
  const size_t co = (size_t)b * A.cur_stride;
  const int ncur = A.n_cur[b];
  const Carve cv(A.cur_stride, ncell, descInLds != 0, false);
  const GridScratch G = tail_grid(smem, cv.end, A, b, itemsInLds != 0);
  if (!itemsInLds) __syncthreads();  // the items come back from the global array
  const TargetLds T = stage_target(smem, cv, ncur, ncell, A.cur_kps + co, A.cur_desc + co * 32, G.cnt, G.items, descInLds != 0);
  if (tid == 0) F.n_front[b] = ncur;
  if (tid < 12) F.Tcw[(size_t)b * 12 + tid] = A.cur_Tcw[(size_t)b * 12 + tid];  // SetPose(prediction), Tracking.cc:1314-1320
  proj_frame_body(A, smem, cv.end, T, b, cacheK, [&](const int *matchL) {
    const float *mp = A.last_xw + (size_t)b * A.last_stride * 3;
    for (int i = tid; i < A.cur_stride; i += nt)
      fb::gather_front_edge(co + i, i < ncur ? matchL[i] : -1, A.cur_kps, mp, F.edge, F.front_xw, F.front_obs, F.front_inv_sigma2,
                            F.front_valid);
  });
}

__global__ __launch_bounds__(MATCH_THREADS) void k_frame_tail_bird(fb_frame_tail_bird_args F, BirdCamK K, int descInLds,
                                                                   int itemsInLds, int camInLds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const fb_bird_mp_args &A = F.m9;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int ncell = A.grid.cols * A.grid.rows;
  const size_t co = (size_t)b * A.cur_stride;
  const int ncur = A.n_cur[b];
  const Carve cv(A.cur_stride, ncell, descInLds != 0);
  const GridScratch G = tail_grid(smem, cv.end, A, b, itemsInLds != 0);
  if (!itemsInLds) __syncthreads();
  const TargetLds T = stage_target(smem, cv, ncur, ncell, A.cur_kps + co, A.cur_desc + co * 32, G.cnt, G.items, descInLds != 0);
  __syncthreads();  // the grid's scratch is dead: the LDS copy of the camera positions lies over it
  // mvKeysBirdCamXYZ: stored for the caller; M9 and the edges read the LDS copy (behind the body's writer array) when it fits
  BirdLds L;
  bird_layout(L, cv.end, A.cur_stride, camInLds != 0);
  float *gcam = const_cast<float *>(A.cur_cam_xyz) + co * 3;
  float *lcam = lds_at<float>(smem, L.cam);
  for (int i = tid; i < ncur; i += nt) {
    float o[3];
    bird_key_to_cam(A.cur_kps[co + i], K, o);
    gcam[i * 3] = o[0]; gcam[i * 3 + 1] = o[1]; gcam[i * 3 + 2] = o[2];
    if (camInLds) { lcam[i * 3] = o[0]; lcam[i * 3 + 1] = o[1]; lcam[i * 3 + 2] = o[2]; }
  }
  if (tid == 0) F.n_bird[b] = ncur;
  const float *cam = camInLds ? lcam : gcam;
  bird_mappoints_body(A, T, lds_at<int>(smem, L.writer), b, cam, [&](const int *writer) {
    const float *mp = A.ref_xw + (size_t)b * A.ref_stride * 3;
    for (int i = tid; i < A.cur_stride; i += nt) {
      const int m = i < ncur ? writer[i] : -1;   // a fresh mvpMapPointsBird: every slot of the stride is written
      A.match_cur_to_ref[co + i] = m;
      F.bird_outlier[co + i] = 1;                // mvBirdOutlier = vector<bool>(Nbird, true) of a fresh Frame (Frame.cc:356)
      fb::gather_bird_edge(co + i, m, A.cur_kps, cam + (size_t)i * 3, mp, F.edge, F.bird_xw, F.bird_xc, F.bird_inv_sigma2, F.bird_valid);
    }
  });
}

// (The LDS plan of every matcher -- which frames keep their descriptor table in LDS, which leave it in HBM / L2 -- is
// match_plan.h; DESIGN.md section 4 lists the variants and the shapes at which they change.)
bool m3_no_cache() {  // measurements: every round of M3 walks the grid again
  static const bool noCache = getenv("FB_M3_NO_CACHE") != nullptr;
  return noCache;
}

template <typename K>
int set_max_lds(K kernel, size_t bytes) {
  FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return FB_OK;
}

}  // namespace

extern "C" {

int fb_descriptor_distance_dev(const uint8_t *d_a, const uint8_t *d_b, int n, int32_t *d_out, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(n >= 0 && (n == 0 || (d_a && d_b && d_out)));
  if (n == 0) return FB_OK;
  fb::ProfScope prof_(fb::P_HAMMING, fb::as_stream(stream));
  k_descriptor_distance<<<(n + 255) / 256, 256, 0, fb::as_stream(stream)>>>(
      reinterpret_cast<const uint4 *>(d_a), reinterpret_cast<const uint4 *>(d_b), n, d_out);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_descriptor_distance(const uint8_t *a, const uint8_t *b, int n, int32_t *out) {
  FB_TRY(fb::check_device());
  FB_ARG(n >= 0);
  const size_t bytes = (size_t)n * 32;
  if (n) FB_ARG(a && b && out);
  fb::Stager st;
  st.in(a, bytes); st.in(b, bytes);
  st.out(out, (size_t)n * 4, false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_descriptor_distance_dev(a, b, n, out, nullptr));
  return st.fetch(nullptr);
}

int fb_grid_build_batch_dev(const fb_keypoint *d_keypoints, const int32_t *d_n, int batch, int kp_stride,
                            const fb_grid_geom *geom, int32_t *d_cell_start, int32_t *d_cell_items, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(geom && batch >= 0 && kp_stride > 0 && geom->cols > 0 && geom->rows > 0);
  if (batch == 0) return FB_OK;
  const int ncell = geom->cols * geom->rows;
  const GridPlan gp = plan_grid(0, ncell, kp_stride);
  FB_TRY(check_lds(gp.bytes, STATIC_GRID, "fb_grid_build_batch_dev"));
  FB_TRY(set_max_lds(k_grid_build, gp.bytes));
  fb::ProfScope prof_(fb::P_GRID, fb::as_stream(stream));
  k_grid_build<<<batch, 256, gp.bytes, fb::as_stream(stream)>>>(d_keypoints, d_n, kp_stride, *geom, d_cell_start, d_cell_items, gp.itemsInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_bird_keys_to_cam_dev(const fb_keypoint *d_kps, const int32_t *d_n, int batch, int kp_stride, int bird_cols,
                            int bird_rows, double pixel2meter, double rear_axle_to_center, const float *Tcb12,
                            float *d_cam_xyz, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(Tcb12 && batch >= 0 && kp_stride > 0);
  if (batch == 0) return FB_OK;
  BirdCamK K;
  K.cols = bird_cols; K.rows = bird_rows; K.pixel2meter = pixel2meter; K.rear = rear_axle_to_center;
  memcpy(K.Tcb, Tcb12, sizeof(K.Tcb));
  dim3 grid((kp_stride + 255) / 256, batch);
  fb::ProfScope prof_(fb::P_BIRDCAM, fb::as_stream(stream));
  k_bird_keys_to_cam<<<grid, 256, 0, fb::as_stream(stream)>>>(d_kps, d_n, kp_stride, K, d_cam_xyz);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_match_projection_frame_dev(const fb_proj_frame_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && A->cur_stride > 0 && A->last_stride >= 0 && A->cur_stride < 65536);
  if (A->batch == 0) return FB_OK;
  const int ncell = A->grid.cols * A->grid.rows;
  M3Plan p;
  FB_TRY(plan_m3(A->cur_stride, A->last_stride, ncell, m3_no_cache(), "fb_match_projection_frame", &p));
  FB_TRY(set_max_lds(k_proj_frame, p.bytes));
  fb::ProfScope prof_(fb::P_PROJ_FRAME, fb::as_stream(stream));
  k_proj_frame<<<A->batch, MATCH_THREADS, p.bytes, fb::as_stream(stream)>>>(*A, p.cacheK, p.descInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_match_projection_keyframe_dev(const fb_proj_kf_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && A->cur_stride > 0 && A->kf_stride >= 0 && A->cur_stride < 65536);
  FB_ARG(A->n_levels > 0 && A->n_levels <= FB_MAX_LEVELS);
  if (A->batch == 0) return FB_OK;
  const int ncell = A->grid.cols * A->grid.rows;
  DescPlan lp;
  ClaimsLds L;
  FB_TRY(plan_staged(A->cur_stride, ncell, [&](size_t at) { return claims_layout(L, at, A->cur_stride, A->kf_stride, 2, CLAIMS_U16_SLACK); },
                     STATIC_M4, "fb_match_projection_keyframe", &lp));
  const size_t lds = lp.bytes;
  FB_TRY(set_max_lds(k_proj_kf, lds));
  fb::ProfScope prof_(fb::P_PROJ_KF, fb::as_stream(stream));
  k_proj_kf<<<A->batch, MATCH_THREADS, lds, fb::as_stream(stream)>>>(*A, lp.descInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

#ifdef FB_MATCH_STAMPS
int fb_match_debug_m3(unsigned long long *dst8) {  // probe build only
  unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  FB_HIP(hipMemcpyFromSymbol(dst8, HIP_SYMBOL(g_m3_stamps), sizeof(z)));
  FB_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_m3_stamps), z, sizeof(z)));
  return FB_OK;
}
int fb_match_debug_m2(int *dst4) {  // probe build only
  int z[4] = {0, 0, 0, 0};
  FB_HIP(hipMemcpyFromSymbol(dst4, HIP_SYMBOL(g_m2_rounds), sizeof(z)));
  FB_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_m2_rounds), z, sizeof(z)));
  return FB_OK;
}
#endif

int fb_match_projection_points_dev(const fb_proj_points_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && A->cur_stride > 0 && A->mp_stride >= 0 && A->cur_stride < 65536);
  if (A->batch == 0) return FB_OK;
  const int ncell = A->grid.cols * A->grid.rows;
  const size_t wsNeed = fb_match_projection_points_workspace(A->batch, A->mp_stride);
  const bool haveWorkspace = A->workspace && A->workspace_bytes >= wsNeed && A->mp_stride > 0 && A->batch <= 65535 && ((uintptr_t)A->workspace % 16) == 0;
  M2Plan p;
  FB_TRY(plan_m2(A->cur_stride, A->mp_stride, ncell, haveWorkspace, "fb_match_projection_points", &p));
  if (p.twoPhase) {
    // two phases: candidate lists by many workgroups, then the serial rule on the lists (see k_m2_candidates)
    uint32_t *cand = reinterpret_cast<uint32_t *>(A->workspace);
    uint8_t *ncand = reinterpret_cast<uint8_t *>(cand + (size_t)A->batch * A->mp_stride * M2_K);
    FB_TRY(set_max_lds(k_m2_candidates, p.candBytes));
    FB_TRY(set_max_lds(k_m2_resolve, p.bytes));
    fb::ProfScope prof_(fb::P_PROJ_POINTS, fb::as_stream(stream));
    k_m2_candidates<<<dim3((A->mp_stride + M2_CAND_THREADS - 1) / M2_CAND_THREADS, A->batch), M2_CAND_THREADS, p.candBytes, fb::as_stream(stream)>>>(*A, cand, ncand);
    k_m2_resolve<<<A->batch, MATCH_THREADS, p.bytes, fb::as_stream(stream)>>>(*A, cand, ncand);
    FB_HIP(hipGetLastError());
    return FB_OK;
  }
  FB_TRY(set_max_lds(k_proj_points, p.bytes));
  fb::ProfScope prof_(fb::P_PROJ_POINTS, fb::as_stream(stream));
  k_proj_points<<<A->batch, MATCH_THREADS, p.bytes, fb::as_stream(stream)>>>(*A, p.descInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

size_t fb_match_projection_points_workspace(int batch, int mp_stride) {
  if (batch <= 0 || mp_stride <= 0) return 0;
  return (size_t)batch * mp_stride * (M2_K * 4 + 1) + 16;
}

int fb_match_bird_mappoints_dev(const fb_bird_mp_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && A->cur_stride > 0 && A->ref_stride >= 0 && A->cur_stride < 65536);
  if (A->batch == 0) return FB_OK;
  const int ncell = A->grid.cols * A->grid.rows;
  DescPlan lp;
  BirdLds L;
  FB_TRY(plan_staged(A->cur_stride, ncell, [&](size_t at) { return bird_layout(L, at, A->cur_stride, false); }, STATIC_BIRD_MP,
                     "fb_match_bird_mappoints", &lp));
  const size_t lds = lp.bytes;
  FB_TRY(set_max_lds(k_bird_mappoints, lds));
  fb::ProfScope prof_(fb::P_BIRD_MP, fb::as_stream(stream));
  k_bird_mappoints<<<A->batch, MATCH_THREADS, lds, fb::as_stream(stream)>>>(*A, lp.descInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_frame_tail_front_dev(const fb_frame_tail_front_args *F, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(F);
  const fb_proj_frame_args *A = &F->m3;
  FB_ARG(A->batch >= 0 && A->cur_stride > 0 && A->last_stride >= 0 && A->cur_stride < 65536);
  FB_ARG(A->grid.cols > 0 && A->grid.rows > 0 && F->edge.nlevels >= 1 && F->edge.nlevels <= FB_MAX_LEVELS);
  FB_ARG(A->cur_cell_start && A->cur_cell_items && F->n_front && F->Tcw && F->front_xw && F->front_obs && F->front_inv_sigma2 && F->front_valid);
  if (A->batch == 0) return FB_OK;
  const int ncell = A->grid.cols * A->grid.rows;
  // the matcher's plan is that of fb_match_projection_frame_dev; the grid's scratch shares the matcher's own arrays, with the
  // items in LDS when that fits (the bench's 64x48 cells at 2064 key points: descriptors, cache and items all in LDS)
  TailFrontPlan p;
  FB_TRY(plan_tail_front(A->cur_stride, A->last_stride, ncell, m3_no_cache(), "fb_frame_tail_front", &p));
  FB_TRY(set_max_lds(k_frame_tail_front, p.bytes));
  fb::ProfScope prof_(fb::P_TAIL_FRONT, fb::as_stream(stream));
  k_frame_tail_front<<<A->batch, MATCH_THREADS, p.bytes, fb::as_stream(stream)>>>(*F, p.cacheK, p.descInLds, p.itemsInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_frame_tail_bird_dev(const fb_frame_tail_bird_args *F, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(F);
  const fb_bird_mp_args *A = &F->m9;
  FB_ARG(A->batch >= 0 && A->cur_stride > 0 && A->ref_stride >= 0 && A->cur_stride < 65536);
  FB_ARG(A->grid.cols > 0 && A->grid.rows > 0 && F->edge.nlevels >= 1 && F->edge.nlevels <= FB_MAX_LEVELS);
  FB_ARG(A->cur_cell_start && A->cur_cell_items && A->cur_cam_xyz && A->match_cur_to_ref && F->n_bird && F->bird_outlier && F->bird_xw &&
         F->bird_xc && F->bird_inv_sigma2 && F->bird_valid);
  if (A->batch == 0) return FB_OK;
  const int ncell = A->grid.cols * A->grid.rows;
  TailBirdPlan p;
  FB_TRY(plan_tail_bird(A->cur_stride, ncell, "fb_frame_tail_bird", &p));
  FB_TRY(set_max_lds(k_frame_tail_bird, p.bytes));
  BirdCamK K;
  K.cols = A->bird_cols; K.rows = A->bird_rows; K.pixel2meter = F->pixel2meter; K.rear = A->rear_axle_to_center;
  memcpy(K.Tcb, F->Tcb, sizeof(K.Tcb));
  fb::ProfScope prof_(fb::P_TAIL_BIRD, fb::as_stream(stream));
  k_frame_tail_bird<<<A->batch, MATCH_THREADS, p.bytes, fb::as_stream(stream)>>>(*F, K, p.descInLds, p.itemsInLds, p.camInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_match_birdview_dev(const fb_birdview_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && A->cur_stride > 0 && A->ref_stride >= 0 && A->cur_stride < 65536);
  if (A->batch == 0) return FB_OK;
  const int ncell = A->grid.cols * A->grid.rows;
  DescPlan lp;
  BirdviewLds L;
  FB_TRY(plan_staged(A->cur_stride, ncell, [&](size_t at) { return birdview_layout(L, at, A->ref_stride); }, STATIC_BIRDVIEW,
                     "fb_match_birdview", &lp));
  const size_t lds = lp.bytes;
  FB_TRY(set_max_lds(k_birdview, lds));
  fb::ProfScope prof_(fb::P_BIRDVIEW, fb::as_stream(stream));
  k_birdview<<<A->batch, MATCH_THREADS, lds, fb::as_stream(stream)>>>(*A, lp.descInLds);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

// ---- host-pointer drop-ins: ONE staged upload, the same kernels, one staged download (fb::Stager) --------------

int fb_match_projection_frame(const fb_proj_frame_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0);
  fb_proj_frame_args D = *H;
  const size_t B = H->batch, cs = H->cur_stride, ls = H->last_stride, ncell = (size_t)H->grid.cols * H->grid.rows;
  fb::Stager st;
  st.in(D.n_cur, B * 4); st.in(D.cur_kps, B * cs * sizeof(fb_keypoint)); st.in(D.cur_desc, B * cs * 32);
  st.in(D.cur_cell_start, B * (ncell + 1) * 4); st.in(D.cur_cell_items, B * cs * 4); st.in(D.cur_blocked, B * cs);
  st.in(D.cur_Tcw, B * 48); st.in(D.n_last, B * 4); st.in(D.last_valid, B * ls); st.in(D.last_obs_pos, B * ls);
  st.in(D.last_xw, B * ls * 12); st.in(D.last_desc, B * ls * 32); st.in(D.last_octave, B * ls * 4);
  st.in(D.last_angle, B * ls * 4);
  st.out(D.match_cur_to_last, B * cs * 4, true);  // copy-in: entries past n keep the caller's contents
  st.out(D.nmatches, B * 4, false);
  st.out(D.retried, B * 4, false);
  FB_ARG(H->match_cur_to_last && H->nmatches);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_match_projection_frame_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_match_projection_keyframe(const fb_proj_kf_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0);
  fb_proj_kf_args D = *H;
  const size_t B = H->batch, cs = H->cur_stride, ks = H->kf_stride, ncell = (size_t)H->grid.cols * H->grid.rows;
  fb::Stager st;
  st.in(D.n_cur, B * 4); st.in(D.cur_kps, B * cs * sizeof(fb_keypoint)); st.in(D.cur_desc, B * cs * 32);
  st.in(D.cur_cell_start, B * (ncell + 1) * 4); st.in(D.cur_cell_items, B * cs * 4); st.in(D.cur_blocked, B * cs);
  st.in(D.cur_Tcw, B * 48); st.in(D.n_kf, B * 4); st.in(D.kf_valid, B * ks); st.in(D.kf_xw, B * ks * 12);
  st.in(D.kf_desc, B * ks * 32); st.in(D.kf_max_dist, B * ks * 4); st.in(D.kf_min_dist, B * ks * 4);
  st.in(D.kf_angle, B * ks * 4);
  st.out(D.match_cur_to_kf, B * cs * 4, true);
  st.out(D.nmatches, B * 4, false);
  FB_ARG(H->match_cur_to_kf && H->nmatches);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_match_projection_keyframe_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_match_projection_points(const fb_proj_points_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0);
  fb_proj_points_args D = *H;
  const size_t B = H->batch, cs = H->cur_stride, ms = H->mp_stride, ncell = (size_t)H->grid.cols * H->grid.rows;
  fb::DevBuf ws;  // the two-phase matcher's workspace (declared first: it goes back to the pool after the Stager has waited)
  fb::Stager st;
  st.in(D.n_cur, B * 4); st.in(D.cur_kps, B * cs * sizeof(fb_keypoint)); st.in(D.cur_desc, B * cs * 32);
  st.in(D.cur_cell_start, B * (ncell + 1) * 4); st.in(D.cur_cell_items, B * cs * 4); st.in(D.cur_blocked, B * cs);
  st.in(D.n_mp, B * 4); st.in(D.mp_track, B * ms); st.in(D.mp_obs_pos, B * ms); st.in(D.mp_proj, B * ms * 8);
  st.in(D.mp_level, B * ms * 4); st.in(D.mp_view_cos, B * ms * 4); st.in(D.mp_desc, B * ms * 32);
  st.out(D.match_cur_to_mp, B * cs * 4, true);
  st.out(D.nmatches, B * 4, false);
  FB_ARG(H->match_cur_to_mp && H->nmatches);
  static const bool onePhase = getenv("FB_M2_ONE_KERNEL") != nullptr;  // measurements / tests of the one-kernel version
  D.workspace = nullptr; D.workspace_bytes = 0;
  if (!onePhase && B * ms > 0) {
    D.workspace_bytes = fb_match_projection_points_workspace((int)B, (int)ms);
    FB_TRY(ws.alloc(D.workspace_bytes));
    D.workspace = ws.p;
  }
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_match_projection_points_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_match_bird_mappoints(const fb_bird_mp_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0);
  fb_bird_mp_args D = *H;
  const size_t B = H->batch, cs = H->cur_stride, rs = H->ref_stride, ncell = (size_t)H->grid.cols * H->grid.rows;
  fb::Stager st;
  st.in(D.n_cur, B * 4); st.in(D.cur_kps, B * cs * sizeof(fb_keypoint)); st.in(D.cur_desc, B * cs * 32);
  st.in(D.cur_cam_xyz, B * cs * 12); st.in(D.cur_cell_start, B * (ncell + 1) * 4); st.in(D.cur_cell_items, B * cs * 4);
  st.in(D.cur_Tcw, B * 48); st.in(D.n_ref, B * 4); st.in(D.ref_valid, B * rs); st.in(D.ref_xw, B * rs * 12);
  st.in(D.ref_desc, B * rs * 32);
  st.out(D.match_cur_to_ref, B * cs * 4, true);  // in/out
  st.out(D.ninliers, B * 4, false);
  FB_ARG(H->match_cur_to_ref && H->ninliers);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_match_bird_mappoints_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_match_birdview(const fb_birdview_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0);
  fb_birdview_args D = *H;
  const size_t B = H->batch, cs = H->cur_stride, rs = H->ref_stride, ncell = (size_t)H->grid.cols * H->grid.rows;
  fb::Stager st;
  st.in(D.n_cur, B * 4); st.in(D.cur_kps, B * cs * sizeof(fb_keypoint)); st.in(D.cur_desc, B * cs * 32);
  st.in(D.cur_cell_start, B * (ncell + 1) * 4); st.in(D.cur_cell_items, B * cs * 4); st.in(D.n_ref, B * 4);
  st.in(D.ref_kps, B * rs * sizeof(fb_keypoint)); st.in(D.ref_desc, B * rs * 32);
  st.out(D.match_ref_to_cur, B * rs * 4, true);
  st.out(D.match_dist, B * rs * 4, true);
  st.out(D.nmatches, B * 4, false);
  st.out(D.n_dmatches, B * 4, false);
  FB_ARG(H->match_ref_to_cur && H->match_dist && H->nmatches && H->n_dmatches);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_match_birdview_dev(&D, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"

#include "match_kf.inc"
