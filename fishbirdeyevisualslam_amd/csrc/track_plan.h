// track_plan.h -- where every buffer of a frame handle (fb_frame, track.hip) lies: named regions of three arenas, each
// arena one allocation.
//   members  what KeyFrame(Frame&) copies: fb_frame_copy_dev is one copy of this arena
//   bow      mBowVec / mFeatVec, allocated by the first ComputeBoW (or a copy from a frame that has them)
//   scratch  what the stages hand each other inside one call.  Each region belongs to one stream side: between a fork and
//            its join (SideStream, fb_frame_extract_dev) the caller's stream touches FRONT regions only and the handle's
//            stream BIRD regions only.  Two regions are lent out under a second name; nothing else overlaps.
// Every region starts on a 256-byte boundary (descriptor rows are read as uint4).
// One optional block lies outside the arenas: plan_redescribe_status() at the end of this file.
//
// No HIP header and no handle: plan_frame() is plain host code (tests/cpp/track_plan_test.cpp compiles it with g++).  It
// fills a local plan and assigns the caller's only on success.  Unnamed namespace: one translation unit at a time.
#ifndef FB_TRACK_PLAN_H_
#define FB_TRACK_PLAN_H_

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/fishbird.h"

namespace fb {
void set_error(const char *fmt, ...);
}

namespace {

enum FrameArena { FA_MEMBERS, FA_BOW, FA_SCRATCH, FA_COUNT };
enum FrameSide { FS_NONE, FS_FRONT, FS_BIRD };  // FRONT = the caller's stream, BIRD = the handle's own
constexpr int FILL_NONE = -1;                   // the region starts uninitialised

enum FrameRegionId {
  // members, in the order of the copy
  FR_n, FR_kps, FR_kps_un, FR_desc, FR_cs, FR_ci, FR_mp, FR_outlier,
  FR_nb, FR_bkps, FR_bdesc, FR_bcam, FR_bcs, FR_bci, FR_mpb, FR_boutlier,
  FR_Tcw, FR_counts, FR_seen_mark,
  // bow
  FR_bow_nw, FR_bow_ids, FR_bow_vals, FR_fv_nn, FR_fv_ids, FR_fv_start, FR_fv_items,
  // scratch of the caller's stream
  FR_m3_valid, FR_m3_obs, FR_m3_xw, FR_m3_desc, FR_m3_oct, FR_m3_ang, FR_m_front,
  FR_l_seen, FR_l_blocked, FR_l_inview, FR_l_obs, FR_l_proj, FR_l_level, FR_l_cos, FR_l_desc, FR_l_n, FR_m_local, FR_m2_ws,
  FR_e_fxw, FR_e_fobs, FR_e_finf, FR_e_fvalid, FR_e_bxw, FR_e_bxc, FR_e_binf, FR_e_bvalid,
  // scratch of the handle's stream
  FR_m9_valid, FR_m9_xw, FR_m9_desc, FR_m9_n, FR_m_bird, FR_ones, FR_m8_m12, FR_m8_dist, FR_m8_n, FR_m8_nd,
  FR_nb_pre, FR_bkps_pre, FR_bdesc_pre,
  // a second name for a region that is free while the borrower runs
  FR_guidance_keep, FR_bow_has_mp,
  FR_COUNT
};

struct FrameRegion {
  const char *name;
  int arena, side;
  int fill;      // byte fb_frame_create fills the region with, or FILL_NONE
  int alias_of;  // the region this one IS, or -1
  size_t off, bytes;
};

struct FramePlan {
  FrameRegion r[FR_COUNT];
  size_t arena_bytes[FA_COUNT];  // a multiple of 256 each
};

inline int plan_frame(const fb_frame_params &p, int cap_, FramePlan *out) {
  if (p.batch < 1 || p.batch > 65535 || cap_ < 1 || p.map_cap < 1 || p.local_mp_cap < 1 || p.local_mpb_cap < 1) {
    fb::set_error("plan_frame: batch %d, capacity %d, map_cap %d, local_mp_cap %d, local_mpb_cap %d", p.batch, cap_, p.map_cap,
                  p.local_mp_cap, p.local_mpb_cap);
    return FB_ERR_ARG;
  }
  FramePlan P;
  memset(&P, 0, sizeof(P));
  const size_t B = p.batch, cap = cap_, mc = p.map_cap, lm = p.local_mp_cap, lb = p.local_mpb_cap, KP = sizeof(fb_keypoint);
  auto put = [&P](int id, const char *name, int arena, int side, size_t bytes, int fill = FILL_NONE) {
    P.r[id] = FrameRegion{name, arena, side, fill, -1, P.arena_bytes[arena], bytes};
    P.arena_bytes[arena] += (bytes + 255) & ~(size_t)255;
  };
  auto lend = [&P](int id, const char *name, int side, int host) {
    P.r[id] = P.r[host];
    P.r[id].name = name; P.r[id].side = side; P.r[id].fill = FILL_NONE; P.r[id].alias_of = host;
  };
  const int M = FA_MEMBERS, W = FA_BOW, S = FA_SCRATCH;
  // mvpMapPoints = NULL, mvbOutlier = false (Frame.cc:327-328); mvpMapPointsBird = NULL, mvBirdOutlier = true (:355-356)
  put(FR_n, "n", M, FS_NONE, B * 4, 0);
  put(FR_kps, "kps", M, FS_NONE, B * cap * KP);
  put(FR_kps_un, "kps_un", M, FS_NONE, B * cap * KP);
  put(FR_desc, "desc", M, FS_NONE, B * cap * 32);
  put(FR_cs, "cs", M, FS_NONE, B * (64 * 48 + 1) * 4);
  put(FR_ci, "ci", M, FS_NONE, B * cap * 4);
  put(FR_mp, "mp", M, FS_NONE, B * cap * 4, 0xff);
  put(FR_outlier, "outlier", M, FS_NONE, B * cap, 0);
  put(FR_nb, "nb", M, FS_NONE, B * 4, 0);
  put(FR_bkps, "bkps", M, FS_NONE, B * cap * KP);
  put(FR_bdesc, "bdesc", M, FS_NONE, B * cap * 32);
  put(FR_bcam, "bcam", M, FS_NONE, B * cap * 12);
  put(FR_bcs, "bcs", M, FS_NONE, B * (32 * 32 + 1) * 4);
  put(FR_bci, "bci", M, FS_NONE, B * cap * 4);
  put(FR_mpb, "mpb", M, FS_NONE, B * cap * 4, 0xff);
  put(FR_boutlier, "boutlier", M, FS_NONE, B * cap, 1);
  put(FR_Tcw, "Tcw", M, FS_NONE, B * 48, 0);
  put(FR_counts, "counts", M, FS_NONE, B * FB_CNT_COUNT * 4, 0);
  put(FR_seen_mark, "seen_mark", M, FS_NONE, B * mc, 0);  // mnLastFrameSeen == mnId per map point (k_discard writes, k_local_points reads)

  put(FR_bow_nw, "bow_nw", W, FS_NONE, B * 4);
  put(FR_bow_ids, "bow_ids", W, FS_NONE, B * cap * 4);
  put(FR_bow_vals, "bow_vals", W, FS_NONE, B * cap * 8);
  put(FR_fv_nn, "fv_nn", W, FS_NONE, B * 4);
  put(FR_fv_ids, "fv_ids", W, FS_NONE, B * cap * 4);
  put(FR_fv_start, "fv_start", W, FS_NONE, B * (cap + 1) * 4);
  put(FR_fv_items, "fv_items", W, FS_NONE, B * cap * 4);

  put(FR_m3_valid, "m3_valid", S, FS_FRONT, B * cap);
  put(FR_m3_obs, "m3_obs", S, FS_FRONT, B * cap);
  put(FR_m3_xw, "m3_xw", S, FS_FRONT, B * cap * 12);
  put(FR_m3_desc, "m3_desc", S, FS_FRONT, B * cap * 32);
  put(FR_m3_oct, "m3_oct", S, FS_FRONT, B * cap * 4);
  put(FR_m3_ang, "m3_ang", S, FS_FRONT, B * cap * 4);
  put(FR_m_front, "m_front", S, FS_FRONT, B * cap * 4);
  put(FR_l_seen, "l_seen", S, FS_FRONT, B * mc);
  put(FR_l_blocked, "l_blocked", S, FS_FRONT, B * cap);
  put(FR_l_inview, "l_inview", S, FS_FRONT, B * lm);
  put(FR_l_obs, "l_obs", S, FS_FRONT, B * lm);
  put(FR_l_proj, "l_proj", S, FS_FRONT, B * lm * 8);
  put(FR_l_level, "l_level", S, FS_FRONT, B * lm * 4);
  put(FR_l_cos, "l_cos", S, FS_FRONT, B * lm * 4);
  put(FR_l_desc, "l_desc", S, FS_FRONT, B * lm * 32);
  put(FR_l_n, "l_n", S, FS_FRONT, B * 4);
  put(FR_m_local, "m_local", S, FS_FRONT, B * cap * 4);
  put(FR_m2_ws, "m2_ws", S, FS_FRONT, fb_match_projection_points_workspace((int)B, (int)lm));
  // k_edges writes the front AND the bird edges on the caller's stream, after the join; the optimiser reads them there
  put(FR_e_fxw, "e_fxw", S, FS_FRONT, B * cap * 12);
  put(FR_e_fobs, "e_fobs", S, FS_FRONT, B * cap * 8);
  put(FR_e_finf, "e_finf", S, FS_FRONT, B * cap * 4);
  put(FR_e_fvalid, "e_fvalid", S, FS_FRONT, B * cap);
  put(FR_e_bxw, "e_bxw", S, FS_FRONT, B * cap * 12);
  put(FR_e_bxc, "e_bxc", S, FS_FRONT, B * cap * 12);
  put(FR_e_binf, "e_binf", S, FS_FRONT, B * cap * 4);
  put(FR_e_bvalid, "e_bvalid", S, FS_FRONT, B * cap);

  put(FR_m9_valid, "m9_valid", S, FS_BIRD, B * lb);
  put(FR_m9_xw, "m9_xw", S, FS_BIRD, B * lb * 12);
  put(FR_m9_desc, "m9_desc", S, FS_BIRD, B * lb * 32);
  put(FR_m9_n, "m9_n", S, FS_BIRD, B * 4);
  put(FR_m_bird, "m_bird", S, FS_BIRD, B * cap * 4);
  put(FR_ones, "ones", S, FS_BIRD, B * lb, 1);  // ref_valid of "the whole table is the list"; never written again
  put(FR_m8_m12, "m8_m12", S, FS_BIRD, B * cap * 4);
  put(FR_m8_dist, "m8_dist", S, FS_BIRD, B * cap * 4);
  put(FR_m8_n, "m8_n", S, FS_BIRD, B * 4);
  put(FR_m8_nd, "m8_nd", S, FS_BIRD, B * 4);
  put(FR_nb_pre, "nb_pre", S, FS_BIRD, B * 4);
  put(FR_bkps_pre, "bkps_pre", S, FS_BIRD, B * cap * KP);
  put(FR_bdesc_pre, "bdesc_pre", S, FS_BIRD, B * cap * 32);

  // The guidance kernel's verdicts during extraction, on the handle's stream: l_blocked is written by k_local_points alone
  // (TrackLocalMap), which no stream runs while the frame is being extracted.
  lend(FR_guidance_keep, "guidance_keep", FS_BIRD, FR_l_blocked);
  // SearchByBoW's "the key-frame slot holds a good point": SearchByProjection (m3_valid's owner) is not part of that stage.
  lend(FR_bow_has_mp, "bow_has_mp", FS_FRONT, FR_m3_valid);
  *out = P;
  return FB_OK;
}

// The status bytes of fb_frame_set_bird_redescribe (one per bird slot, written by k_describe_at on the handle's stream): not
// a region of the scratch arena but a block of its own, allocated when the switch is first turned on -- like the BoW arena, a
// handle that never asks for it holds none of it, and the region list above stays the list of what every handle holds.
inline size_t plan_redescribe_status(const fb_frame_params &p, int cap) { return (size_t)p.batch * (size_t)cap; }

}  // namespace

#endif
