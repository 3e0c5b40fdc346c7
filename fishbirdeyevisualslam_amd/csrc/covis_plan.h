// covis_plan.h -- where everything of a covisibility handle (fb_covis, covis.hip and its covis_*.inc) lies in device
// memory, and what its scratch holds from one call to the next.
//   graph    the persistent block: W, rank, inv, err and the spanning tree
//   scratch  one allocation that a map-taking call lays out as [window head?][front index][bird index?][tail]:
//              window head  the lists of a fb_covis_local_window_dev (fb_covis_local_window_header reads them later)
//              index        the point -> edge index (CSR) of a fb_covis_map
//              tail         what one call keeps for itself, behind the index it reads
// Each part is described once, by a function that fills a POD of offsets and returns the part's bytes: there is no second
// size formula.  Every region starts on a 256-byte boundary.  plan_call() puts the parts of one call together; a
// fb_covis_reserve* and its call read the same plan.
//
// ScratchState records what the scratch holds (a window head, an index) and scratch_*() are its only writers: whether a
// call may read the index or the window header again is decided here and nowhere else.
//
// No HIP header and no handle: plain host code (tests/cpp/covis_plan_test.cpp compiles it with g++).  Unnamed namespace:
// one translation unit at a time.
#ifndef FB_COVIS_PLAN_H_
#define FB_COVIS_PLAN_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/fishbird.h"

namespace {

// the launch shapes and list lengths the sizes depend on
constexpr int CV_NT = 1024;
constexpr int CV_SCAN_ITEMS = 4;                       // consecutive ints per thread of a scan tile
constexpr int CV_SCAN_TILE = CV_NT * CV_SCAN_ITEMS;
constexpr int PT_NT = 256;                             // entries of the recent list per workgroup (MapPointCulling)
constexpr int LM_EXPAND = FB_LOCAL_MAP_MAX_EXPAND;     // the expansion loop stops once the list is longer than this
constexpr int LM_NEIGH = FB_KFDB_COVIS;                // GetBestCovisibilityKeyFrames(10)
constexpr int LM_HDR = 64;                             // ints of header per sequence
constexpr size_t CL_ENTRY_BYTES = 184;                 // sizeof(ClEntry), covis_correct.inc

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t scan_tiles(size_t n_pt) { return (n_pt + 1 + CV_SCAN_TILE - 1) / CV_SCAN_TILE; }   // tiles of a scan over n_pt + 1 ints
inline int lm_list(int K) { return std::max(K, LM_EXPAND + 4); }   // voters <= K; with an expansion <= 80 + 3

struct Regions {        // consecutive regions of one part
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += up256(bytes); return o; }
};

// ---- the parts ------------------------------------------------------------------------------------------------------------
struct GraphOff { size_t W, rank, inv, err, parent, linked, first; };
inline size_t plan_graph(size_t K, GraphOff *o) {
  Regions r;
  o->W = r.take(K * K * 2); o->rank = r.take(K * 4); o->inv = r.take(K * 4); o->err = r.take(4);
  o->parent = r.take(K * 4); o->linked = r.take(K); o->first = r.take(K);
  return r.off;
}

struct IndexOff { size_t start, fill, nobs, csr, dead, bsum, counter; };
inline size_t plan_index(size_t n_mp, size_t n_obs, size_t n_q, size_t K, IndexOff *o) {
  Regions r;
  o->start = r.take((n_mp + 1) * 4); o->fill = r.take(n_mp * 4);   // adjacent: index_build clears both with one memset
  o->nobs = r.take(n_mp * 4);
  o->csr = r.take(n_obs * 4); o->dead = r.take(n_obs * 4); o->bsum = r.take(scan_tiles(n_mp) * 4);
  o->counter = r.take(n_q * K * 2);
  r.take(256);          // spare: the index has always been sized with it, and a caller's reserve counts on the totals
  return r.off;
}

struct WinSideOff { size_t ptkey, plist, eoff, bsum; };
struct WinOff { size_t hdr, lpos, widx, wslot, rowcnt, wfixed, fixkey; WinSideOff side[2]; };
// the per-key-frame arrays, in front of everything per point: fb_covis_local_window_header finds them without the map's sizes
inline void win_kf_regions(Regions &r, size_t K, WinOff *o) {
  o->hdr = r.take(256);
  o->lpos = r.take(K * 4); o->widx = r.take(K * 4); o->wslot = r.take(K * 4); o->rowcnt = r.take(K * 4);
  o->wfixed = r.take(K); o->fixkey = r.take(K * 8);
}
inline size_t plan_window(size_t K, size_t n_mp, size_t n_mpb, WinOff *o) {
  Regions r;
  win_kf_regions(r, K, o);
  const size_t n[2] = {n_mp, n_mpb};
  for (int sd = 0; sd < 2; sd++) {
    o->side[sd].ptkey = r.take(n[sd] * 4); o->side[sd].plist = r.take(n[sd] * 4);
    o->side[sd].eoff = r.take((n[sd] + 1) * 4); o->side[sd].bsum = r.take(scan_tiles(n[sd]) * 4);
  }
  return r.off;
}

// hdr, voters, rows, wslot: one 256-byte-granular stride per sequence (lm_ints(), covis_tree.inc); the rest is shared
struct LmOff { size_t hdr, voters, rows, wslot, rowcnt, ptkey, plist; int list; };
inline size_t plan_local_map(size_t batch, size_t K, size_t n_mp, LmOff *o) {
  Regions r;
  o->list = lm_list((int)K);
  const size_t L = (size_t)o->list;
  o->hdr = r.take(batch * up256(LM_HDR * 4)); o->voters = r.take(batch * up256(LM_EXPAND * 4));
  o->rows = r.take(batch * up256((size_t)LM_EXPAND * LM_NEIGH * 4)); o->wslot = r.take(batch * up256(L * 4));
  o->rowcnt = r.take(L * 4); o->ptkey = r.take(n_mp * 4); o->plist = r.take(n_mp * 4);
  return r.off;
}

struct ClOff { size_t hdr, pos, tab, ow_old, owner, bhead, bnext; };
inline size_t plan_correct_loop(size_t K, size_t n_mp, size_t n_mpb, size_t bird_stride, ClOff *o) {
  Regions r;
  o->hdr = r.take(256); o->pos = r.take(K * 4); o->tab = r.take(K * CL_ENTRY_BYTES); o->ow_old = r.take(K * 12);
  o->owner = r.take(n_mp * 4); o->bhead = r.take(n_mpb * 4); o->bnext = r.take(K * bird_stride * 4);
  return r.off;
}

struct MpcOff { size_t first, val, dec, rowbase, bcnt; };
inline size_t plan_point_culling(size_t n_mp, size_t recent_cap, MpcOff *o) {
  Regions r;
  o->first = r.take(n_mp * 4); o->val = r.take(recent_cap * 4); o->dec = r.take(recent_cap * 4); o->rowbase = r.take(recent_cap * 4);
  o->bcnt = r.take(((recent_cap + PT_NT - 1) / PT_NT) * 12 + 12);
  return r.off;
}

struct PnkOff { size_t gain, gain_idx, n_gain; };
inline size_t plan_new_keyframe(size_t n_features, PnkOff *o) {
  Regions r;
  o->gain = r.take(n_features * 4); o->gain_idx = r.take(n_features * 4); o->n_gain = r.take(4);
  return r.off;
}

// fb_covis_replace_points_dev / fb_covis_loop_fuse_dev: the log of the edges that changed owner or were added in this call.
// head[mp] / next[e]: the edges a point gained, as a linked list; home[e]: obs_mp as it came in (the index's owner of e).
struct FzOff { size_t head, next, home; };
inline size_t plan_point_fuse(size_t n_mp, size_t n_obs, size_t n_new, FzOff *o) {
  Regions r;
  o->head = r.take(n_mp * 4); o->next = r.take((n_obs + n_new) * 4); o->home = r.take(n_obs * 4);
  return r.off;
}

// fb_covis_search_and_fuse_dev, behind the log: one key frame's copy (key points, descriptors, N, Scw, grid) and the loop
// points as the search's lists; used again for every key frame of the set
struct SafOff { size_t mark, kps, kdesc, n_kf, n_list, pose, cell_start, cell_items, valid, xw, normal, mind, maxd, desc, best, rep; };
inline size_t plan_search_and_fuse(size_t n_mp, size_t S, size_t n_loop, size_t cells, SafOff *o) {
  Regions r;
  o->mark = r.take(n_mp * 4); o->kps = r.take(S * 24); o->kdesc = r.take(S * 32); o->n_kf = r.take(4); o->n_list = r.take(4);
  o->pose = r.take(48); o->cell_start = r.take((cells + 1) * 4); o->cell_items = r.take(S * 4); o->valid = r.take(n_loop);
  o->xw = r.take(n_loop * 12); o->normal = r.take(n_loop * 12); o->mind = r.take(n_loop * 4); o->maxd = r.take(n_loop * 4);
  o->desc = r.take(n_loop * 32); o->best = r.take(n_loop * 4); o->rep = r.take(n_loop * 4);
  return r.off;
}

// fb_covis_search_in_neighbors_dev, behind the log: the flags and lists of the call (hdr: the window's header ints, then
// ok, the clamped target and candidate counts and cur as the query of the closing UpdateConnections), the snapshot of cur's
// row, one key frame's copy and one point list of `list` entries (the snapshot or the candidates), used again for every
// Fuse, and the first-occurrence arrays of the window's point collection over `n_targets` list entries
struct SinOff {
  size_t hdr, snap, wslot, rowcnt, ptkey, plist, kps, kdesc, n_kf, n_list, pose, ow, cell_start, cell_items, valid, xw, normal, mind, maxd,
      desc, best;
};
inline size_t plan_search_in_neighbors(size_t n_mp, size_t S, size_t n_targets, size_t list, size_t cells, SinOff *o) {
  Regions r;
  o->hdr = r.take(256); o->snap = r.take(S * 4); o->wslot = r.take((n_targets + 1) * 4); o->rowcnt = r.take((n_targets + 1) * 4);
  o->ptkey = r.take(n_mp * 4); o->plist = r.take(n_mp * 4);
  o->kps = r.take(S * 24); o->kdesc = r.take(S * 32); o->n_kf = r.take(4); o->n_list = r.take(4); o->pose = r.take(48); o->ow = r.take(12);
  o->cell_start = r.take((cells + 1) * 4); o->cell_items = r.take(S * 4); o->valid = r.take(list);
  o->xw = r.take(list * 12); o->normal = r.take(list * 12); o->mind = r.take(list * 4); o->maxd = r.take(list * 4);
  o->desc = r.take(list * 32); o->best = r.take(list * 4);
  return r.off;
}

// the bird lists of every key frame (mvpBirdConnectedKeyFrames and their weights), in the format of W: a block of its own,
// allocated by the first bird call, so that plan_graph stays what a handle without the bird side pays
struct BirdGraphOff { size_t WB; };
inline size_t plan_bird_graph(size_t K, BirdGraphOff *o) {
  Regions r;
  o->WB = r.take(K * K * 2);
  return r.off;
}

// fb_covis_local_bird_map_dev: the list after the push_front holds at most K + 1 members
struct LbOff { size_t hdr, wlist, wnear, cnt, pos, eoff, plist, bsum; };
inline size_t plan_local_bird_map(size_t K, size_t n_mpb, LbOff *o) {
  Regions r;
  o->hdr = r.take(256); o->wlist = r.take((K + 1) * 4); o->wnear = r.take(K + 1); o->cnt = r.take((K + 1) * 4);
  o->pos = r.take(n_mpb * 4); o->eoff = r.take((n_mpb + 1) * 4); o->plist = r.take(n_mpb * 4); o->bsum = r.take(scan_tiles(n_mpb) * 4);
  return r.off;
}

// The consistency groups of LoopClosing::DetectLoop (covis_loop.inc): a block of its own, allocated by the first call, like
// the bird lists.  Two buffers of up to cap groups (previous and current; which is which is the handle's flag): a bitset
// over the slots and a counter per group, and the number of groups of each buffer.  Behind them the scratch of one
// fb_covis_detect_loop_dev: per previous group the first consistent candidate, per candidate its bitset, its number of
// pushes (then their exclusive scan) and three flags.
inline size_t loop_words(size_t K) { return (K + 31) / 32; }
struct LoopGroupsOff { size_t bits[2], cons[2], ng, first, cbits, cnt, any, enough, valid; };
inline size_t plan_loop_groups(size_t K, size_t cap, LoopGroupsOff *o) {
  Regions r;
  const size_t nw = loop_words(K);
  for (int b = 0; b < 2; b++) { o->bits[b] = r.take(cap * nw * 4); o->cons[b] = r.take(cap * 4); }
  o->ng = r.take(2 * 4);
  o->first = r.take(cap * 4); o->cbits = r.take(K * nw * 4); o->cnt = r.take(K * 4);
  o->any = r.take(K); o->enough = r.take(K); o->valid = r.take(K);
  return r.off;
}

// fb_covis_loop_map_points_dev: the list walked (the ordered vector and the matched key frame: at most K + 1 entries) and
// the first-occurrence arrays of the window's point collection
struct LoopPointsOff { size_t hdr, wslot, rowcnt, ptkey, plist; };
inline size_t plan_loop_points(size_t K, size_t n_mp, LoopPointsOff *o) {
  Regions r;
  o->hdr = r.take(256); o->wslot = r.take((K + 1) * 4); o->rowcnt = r.take((K + 1) * 4);
  o->ptkey = r.take(n_mp * 4); o->plist = r.take(n_mp * 4);
  return r.off;
}

// fb_covis_loop_connections_dev, behind an index with set_cap counter rows: LoopConnections as one bit row per set member
// and the rows' sizes
struct LoopConnOff { size_t bits, rowcnt; };
inline size_t plan_loop_connections(size_t set_cap, size_t K, LoopConnOff *o) {
  Regions r;
  o->bits = r.take(set_cap * loop_words(K) * 4); o->rowcnt = r.take(set_cap * 4);
  return r.off;
}

// ---- one call -------------------------------------------------------------------------------------------------------------
struct CallPlan { size_t head, front, bird, tail, total; };   // where each part begins (an absent part is empty)
inline CallPlan plan_call(size_t head_bytes, size_t front_bytes, size_t bird_bytes, size_t tail_bytes) {
  CallPlan c;
  c.head = 0; c.front = head_bytes; c.bird = c.front + front_bytes; c.tail = c.bird + bird_bytes; c.total = c.tail + tail_bytes;
  return c;
}
// a call on one map: [index][tail]
inline CallPlan plan_map_call(size_t K, size_t n_mp, size_t n_obs, size_t n_q, size_t tail_bytes) {
  IndexOff io;
  return plan_call(0, plan_index(n_mp, n_obs, n_q, K, &io), 0, tail_bytes);
}
// the window: [head][front index][bird index]
inline CallPlan plan_window_call(size_t K, size_t n_mp, size_t n_obs, size_t n_mpb, size_t n_bobs) {
  WinOff wo;
  IndexOff io;
  const size_t head = plan_window(K, n_mp, n_mpb, &wo), front = plan_index(n_mp, n_obs, 0, K, &io);
  return plan_call(head, front, plan_index(n_mpb, n_bobs, 0, K, &io), 0);
}
// the local map behind an index that a window (front side) or an update_connections of n_q queries built
inline CallPlan plan_local_map_call(size_t K, size_t n_mp, size_t n_obs, size_t n_q, size_t batch, bool with_window) {
  WinOff wo;
  IndexOff io;
  LmOff lo;
  return plan_call(with_window ? plan_window(K, n_mp, 0, &wo) : 0, plan_index(n_mp, n_obs, n_q, K, &io), 0, plan_local_map(batch, K, n_mp, &lo));
}

// The bird calls (update_bird_connections, local_bird_map) behind whatever the scratch holds up to `behind` (the end of the
// front index that a later reuse_index reads, or 0): [..behind][bird index][local bird map].  Neither call keeps anything
// from one call to the next, so the two share the plan: the first uses the index only, the second the tail only.
inline CallPlan plan_bird_call(size_t behind, size_t K, size_t n_mpb, size_t n_bobs) {
  IndexOff io;
  LbOff lo;
  return plan_call(behind, 0, plan_index(n_mpb, n_bobs, 0, K, &io), plan_local_bird_map(K, n_mpb, &lo));
}

// ---- what the scratch holds -----------------------------------------------------------------------------------------------
inline bool same_map(const fb_covis_map &a, const fb_covis_map &b) {
  return a.max_keyframes == b.max_keyframes && a.kp_stride == b.kp_stride && a.n_mp == b.n_mp && a.n_obs == b.n_obs && a.kf_n == b.kf_n &&
         a.kf_mp == b.kf_mp && a.kf_octave == b.kf_octave && a.mp_bad == b.mp_bad && a.obs_mp == b.obs_mp && a.obs_kf == b.obs_kf &&
         a.obs_idx == b.obs_idx && a.kf_order == b.kf_order;
}

struct ScratchState {
  size_t capacity;      // bytes allocated
  bool win_valid;       // [0, win_bytes) holds the lists of a window call made with cap_kf = win_cap_kf
  size_t win_bytes;
  int win_cap_kf;
  bool index_valid;     // [index_head, index_end) holds the index of index_map; a tail goes behind index_end
  size_t index_head, index_end;
  fb_covis_map index_map;
};

struct IndexStep {      // what a call does about its index
  bool refused;         // reuse was asked for on another map than the index is of: FB_ERR_ARG
  bool reuse;
  size_t index_at, tail_at, total;   // total: what the scratch must hold (a reuse fits by definition)
};

// Reuse or rebuild.  A reuse needs a valid index of the same map whose end leaves room for the tail; otherwise the index is
// rebuilt once at `head`, with the tail behind it.
inline IndexStep scratch_decide(const ScratchState &S, bool want_reuse, const fb_covis_map &M, size_t head, size_t index_bytes, size_t tail_bytes) {
  IndexStep st;
  st.refused = false;
  st.reuse = want_reuse && S.index_valid;
  if (st.reuse && !same_map(S.index_map, M)) { st.refused = true; st.reuse = false; }   // the caller's statement, as far as it can be checked
  if (st.reuse && S.index_end + tail_bytes > S.capacity) st.reuse = false;              // growing the scratch would lose the index
  st.index_at = st.reuse ? S.index_head : head;
  st.tail_at = st.reuse ? S.index_end : head + index_bytes;
  st.total = st.reuse ? S.capacity : st.tail_at + tail_bytes;
  return st;
}

inline void scratch_clear(ScratchState &S) { S = ScratchState{}; }
// the scratch was allocated anew: nothing of the old one is left
inline void scratch_grown(ScratchState &S, size_t bytes) { scratch_clear(S); S.capacity = bytes; }
// An index is about to be written at `at`.  A kept one replaces the recorded index, which stays invalid until
// scratch_build_done; the other kind (the window's bird side, behind the front index) is the call's own.
inline void scratch_build_begins(ScratchState &S, size_t at, bool kept) {
  if (at < S.win_bytes) S.win_valid = false;   // it lies where the window's lists were
  if (kept) S.index_valid = false;
}
// its build was enqueued without error
inline void scratch_build_done(ScratchState &S, size_t at, size_t end, const fb_covis_map &M, bool kept) {
  if (!kept) return;
  S.index_valid = true; S.index_head = at; S.index_end = end; S.index_map = M;
}
// The index is of arrays that are gone (a host-pointer call's staged copies) or were edited (process_new_keyframe,
// map_point_culling): a later reuse_index rebuilds.
inline void scratch_drop_index(ScratchState &S) { S.index_valid = false; }
// where a call that keeps nothing puts its own arrays: behind the recorded index, so that a later reuse_index still finds it
inline size_t scratch_behind_index(const ScratchState &S) { return S.index_valid ? S.index_end : 0; }
inline void scratch_window_begins(ScratchState &S) { S.win_valid = false; }
// every launch of the window call was enqueued without error
inline void scratch_window_done(ScratchState &S, size_t head_bytes, int cap_kf) { S.win_valid = true; S.win_bytes = head_bytes; S.win_cap_kf = cap_kf; }

struct IndexDropGuard { // a host-pointer call: whichever way it returns, no index of its staged arrays is left behind
  ScratchState &S;
  explicit IndexDropGuard(ScratchState &s) : S(s) {}
  ~IndexDropGuard() { scratch_drop_index(S); }
  IndexDropGuard(const IndexDropGuard &) = delete;
  IndexDropGuard &operator=(const IndexDropGuard &) = delete;
};

}  // namespace

#endif
