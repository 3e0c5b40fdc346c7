/*
 * fb_rot_hist.h -- the matchers' rotation-consistency filter (ORBmatcher.cc: rotHist, ComputeThreeMaxima): every accepted
 * match votes for the bin of its angle difference, and matches outside the three most voted bins are dropped.
 * This header owns the histogram, the bin arithmetic and the choice of the three bins.  The loops that vote and drop:
 * k_proj_frame, k_proj_kf and k_match_bow_t vote once per committed match and drop by query, the same loop in all three,
 * which is fb::commit_matches (fb_claims.h).  k_birdview (votes for matches that failed the ratio test), k_init_match
 * (votes for every acceptance, keeps only the last one per target) and k_match_triangulation (bins indexed by the KF1
 * feature, no claim rounds) carry quirks of the reference and keep their own.
 */
#ifndef FB_ROT_HIST_H_
#define FB_ROT_HIST_H_

#include <hip/hip_runtime.h>

namespace fb {

constexpr int HISTO_LENGTH = 30;  // ORBmatcher.cc:40

__device__ __forceinline__ int rot_bin(float rot) {  // ORBmatcher.cc:1434-1439, :237-243
  const float factor = 1.0f / HISTO_LENGTH;
  if (rot < 0.0f) rot += 360.0f;
  int bin = (int)roundf(rot * factor);
  if (bin == HISTO_LENGTH) bin = 0;
  return bin;
}

// ComputeThreeMaxima, ORBmatcher.cc:1905-1946
static __device__ void three_maxima(const int *sz, int &ind1, int &ind2, int &ind3) {
  int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;  // (the outputs may live next to sz: decide in registers, store once)
  for (int i = 0; i < HISTO_LENGTH; i++) {
    const int s = sz[i];
    if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
    else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
    else if (s > max3) { max3 = s; i3 = i; }
  }
  if (max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
  else if (max3 < 0.1f * (float)max1) { i3 = -1; }
  ind1 = i1; ind2 = i2; ind3 = i3;
}

// One per workgroup, in __shared__ memory.  clear() and the add() calls are separated by the caller's barrier, and so
// are the add() calls and pick(); pick() ends with the barrier after which keeps() may be asked.
struct RotHist {
  int hist[HISTO_LENGTH], ind[3];
  __device__ __forceinline__ void clear() { if (threadIdx.x < HISTO_LENGTH) hist[threadIdx.x] = 0; }
  __device__ __forceinline__ void add(int bin) { atomicAdd(&hist[bin], 1); }
  __device__ __forceinline__ void pick() {
    if (threadIdx.x == 0) three_maxima(hist, ind[0], ind[1], ind[2]);
    __syncthreads();
  }
  __device__ __forceinline__ bool keeps(int bin) const { return bin == ind[0] || bin == ind[1] || bin == ind[2]; }
};

}  // namespace fb
#endif
