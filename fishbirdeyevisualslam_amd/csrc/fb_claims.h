/*
 * fb_claims.h -- the matchers' serial rule "a target that an EARLIER query took is skipped", resolved in parallel, and
 * the commit of its result.  Device only; the ONE statement of the scheme for k_proj_frame (M3), k_proj_kf (M4),
 * k_proj_points / k_m2_resolve (M2), k_proj_sim3 and k_match_bow_t (M5/M6).
 *
 * Fixed point: every round ALL queries pick their best target given the previous round's claims.  owner[c] is the
 * smallest index among the queries that claimed target c, and query q honours only claims of q' < q.  By induction on q
 * the rounds converge to exactly the serial result (query 0 is final after round 0, query q after at most round q, hence
 * the bound of more()); in practice 2-3 rounds.  The rounds stop when no query changed its mind.
 *
 *   fb::Claims<AT> C(s_flags, owners, tStride, assigns, qStride, blocked0, nTargets, nQueries);   // ClaimsLds, match_plan.h
 *   C.start();
 *   for (int round = 0; C.more(round); round++) {
 *     C.begin_round();
 *     for (the kernel's own query loop)        // every query exactly once, by any lane, in any order
 *       C.submit(q, best target that is not C.taken(idx, q) or NONE, does q block later queries);
 *     if (C.end_round()) break;
 *   }
 *   const int *match = fb::commit_matches<LAST_WINS>(C, value of a query[, &s_rot, check, angle difference]);
 *
 * k_init_match (match_kf.inc) is not a user: there a claim is a list of (query, distance) pairs per target.
 */
#ifndef FB_CLAIMS_H_
#define FB_CLAIMS_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fb_rot_hist.h"

namespace fb {

struct ClaimFlags { int changed, n; };  // one per workgroup, in __shared__ memory: "a query changed" | matches committed

struct QueryIndex { __device__ __forceinline__ int operator()(int q) const { return q; } };  // commit_matches: the match of a target is its query

// AT = element type of the per-query assignment, uint16_t (targets < 65535) or int.  The object is a handful of
// workgroup-uniform pointers and counts; the arrays are the caller's LDS: owner [2][tStride] ints, assign [2][qStride] ATs.
template <typename AT>
struct Claims {
  static constexpr int NONE = 0x7fffffff;  // no target; in an assign array (AT)NONE, i.e. 0xFFFF in 16 bits
  static constexpr int BLOCKED = -1;       // owner of a target that was occupied on entry: blocks every query
  ClaimFlags &f;
  int *ownerA, *ownerB;      // [nT] last round's claims (read) | this round's (atomicMin)
  AT *assignA, *assignB;     // [nQ] last round's choice | this round's
  const uint8_t *blocked0;   // [nT] or nullptr
  const int nT, nQ;

  __device__ __forceinline__ Claims(ClaimFlags &flags, int *owners, int tStride, AT *assigns, int qStride,
                                    const uint8_t *blocked, int nTargets, int nQueries)
      : f(flags), ownerA(owners), ownerB(owners + tStride), assignA(assigns), assignB(assigns + qStride),
        blocked0(blocked), nT(nTargets), nQ(nQueries) {}

  __device__ __forceinline__ void reset(int *owner) const {
    for (int i = threadIdx.x; i < nT; i += blockDim.x) owner[i] = (blocked0 && blocked0[i]) ? BLOCKED : NONE;
  }
  // a search from scratch (whatever the four arrays hold)
  __device__ __forceinline__ void start() {
    reset(ownerA);
    for (int q = threadIdx.x; q < nQ; q += blockDim.x) assignA[q] = (AT)NONE;
    __syncthreads();
  }
  __device__ __forceinline__ bool more(int round) const { return round <= nQ + 1; }
  __device__ __forceinline__ void begin_round() {
    reset(ownerB);
    if (threadIdx.x == 0) f.changed = 0;
    __syncthreads();
  }
  // last round's owner of target idx: BLOCKED, a query index, or NONE
  __device__ __forceinline__ int owner(int idx) const { return ownerA[idx]; }
  __device__ __forceinline__ bool taken(int idx, int q) const { return ownerA[idx] < q; }
  // claims: q blocks later queries on `best` (only looked at when best != NONE)
  __device__ __forceinline__ void submit(int q, int best, bool claims = true) {
    const AT a = (AT)best;
    assignB[q] = a;
    if (a != assignA[q]) f.changed = 1;
    if (best != NONE && claims) atomicMin(&ownerB[best], q);
  }
  // true = fixed point reached.  The first barrier ends the round's writes; the second keeps a fast wave from clearing
  // `changed` (begin_round) before every wave has read it.
  __device__ __forceinline__ bool end_round() {
    __syncthreads();
    const int changed = f.changed;
    int *t = ownerA; ownerA = ownerB; ownerB = t;
    AT *u = assignA; assignA = assignB; assignB = u;
    __syncthreads();
    return !changed;
  }
};

// Commit: assign array -> per-target match array (-1 = none) + count in C.f.n.  Returns the match array, which reuses
// this round's owner array (and the bins reuse this round's assign array): after the rounds both are free, and a
// following C.start() may overwrite either.  Ends with a barrier: array and count may be read at once.
//   LAST_WINS  several queries may hold one target (their claims did not block): the largest query keeps it, as the
//              serial loop's last write does.  false: claims always block, one query per target, a plain store.
//   val(q)     what is written for query q
//   rot, ori, angle(v, c)   optional rotation-consistency filter (ORBmatcher.cc:1446-1468): every match votes with the bin of
//              its angle difference (v = val(q), c = its target), matches outside the three most voted bins are dropped
//              and discounted.  k_birdview, k_init_match and k_match_triangulation vote and drop on their own: they vote for
//              matches they do not keep, or index the bins differently (see fb_rot_hist.h).
struct NoAngle { __device__ __forceinline__ float operator()(int, int) const { return 0.0f; } };
template <bool LAST_WINS, typename AT, typename Val, typename Angle = NoAngle>
__device__ __forceinline__ const int *commit_matches(Claims<AT> &C, Val val, RotHist *rot = nullptr, bool ori = false,
                                                     Angle angle = Angle()) {
  const int tid = threadIdx.x, nt = blockDim.x;
  int *matchL = C.ownerB;
  AT *binQ = C.assignB;  // histogram bin of each accepted query
  for (int i = tid; i < C.nT; i += nt) matchL[i] = -1;
  if (rot) rot->clear();
  if (tid == 0) C.f.n = 0;
  __syncthreads();
  for (int q = tid; q < C.nQ; q += nt) {
    const int c = C.assignA[q];
    if (c == (AT)C.NONE) continue;
    const int v = val(q);
    if (LAST_WINS) atomicMax(&matchL[c], v); else matchL[c] = v;
    atomicAdd(&C.f.n, 1);
    if (ori) {
      const int bin = rot_bin(angle(v, c));
      rot->add(bin);
      binQ[q] = (AT)bin;
    }
  }
  __syncthreads();
  if (ori) {
    rot->pick();
    for (int q = tid; q < C.nQ; q += nt) {
      const int c = C.assignA[q];
      if (c == (AT)C.NONE) continue;
      if (!rot->keeps(binQ[q])) {
        matchL[c] = -1;
        atomicSub(&C.f.n, 1);
      }
    }
    __syncthreads();
  }
  return matchL;
}

}  // namespace fb
#endif
