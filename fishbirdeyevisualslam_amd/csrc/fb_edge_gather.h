/*
 * fb_edge_gather.h -- the edge construction loops of PoseOptimizationWithBird (Optimizer.cc:525-571 front, :575-602 bird),
 * one key point slot at a time: slot o of the frame becomes edge o.  ONE statement for k_gather_front / k_gather_bird
 * (pose.hip) and for the fused per-frame tail kernels (match.hip), which build the edges from the matches they have just
 * committed.  A slot without a match only clears its valid byte: its other edge fields keep what they held.
 */
#ifndef FB_EDGE_GATHER_H_
#define FB_EDGE_GATHER_H_

#include <hip/hip_runtime.h>

#include <cstring>

#include "fb_common.h"

namespace fb {

typedef fb_pose_gather_levels GatherK;  // include/fishbird.h: float inv_sigma2[FB_MAX_LEVELS]; int32_t nlevels

inline GatherK make_gather_k(const float *inv_level_sigma2, int nlevels) {
  GatherK G;
  memset(&G, 0, sizeof(G));
  G.nlevels = nlevels;
  for (int i = 0; i < nlevels; i++) G.inv_sigma2[i] = inv_level_sigma2[i];
  return G;
}

// o = slot in the batch-wide arrays, m = its match (index into the frame's map points mp_xw, or < 0)
__device__ __forceinline__ void gather_front_edge(size_t o, int m, const fb_keypoint *kps, const float *mp_xw, const GatherK &G,
                                                  float *xw, float *obs, float *inf, uint8_t *valid) {
  if (m < 0) { valid[o] = 0; return; }
  const fb_keypoint kp = kps[o];
  const float *X = mp_xw + (size_t)m * 3;
  xw[o * 3] = X[0]; xw[o * 3 + 1] = X[1]; xw[o * 3 + 2] = X[2];
  obs[o * 2] = kp.x; obs[o * 2 + 1] = kp.y;
  inf[o] = G.inv_sigma2[kp.octave];
  valid[o] = 1;
}

// cam = the slot's own camera-frame position (mvKeysBirdCamXYZ[i]), wherever the caller keeps it
__device__ __forceinline__ void gather_bird_edge(size_t o, int m, const fb_keypoint *kps, const float *cam, const float *mpb_xw,
                                                 const GatherK &G, float *xw, float *xc, float *inf, uint8_t *valid) {
  if (m < 0) { valid[o] = 0; return; }
  const float *X = mpb_xw + (size_t)m * 3;
  xw[o * 3] = X[0]; xw[o * 3 + 1] = X[1]; xw[o * 3 + 2] = X[2];
  xc[o * 3] = cam[0]; xc[o * 3 + 1] = cam[1]; xc[o * 3 + 2] = cam[2];
  inf[o] = G.inv_sigma2[kps[o].octave];
  valid[o] = 1;
}

}  // namespace fb
#endif
