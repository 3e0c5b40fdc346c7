/*
 * fb_distinctive.h -- the choice MapPoint::ComputeDistinctiveDescriptors makes (src/MapPoint.cc:272-301), for one wave:
 * the observation whose median Hamming distance to all N observations is least, the first one among equals.  One copy
 * for k_distinctive (match_kf.inc, descriptors as a CSR) and k_pt_refresh (covis_points.inc, descriptors of key frames).
 */
#ifndef FB_DISTINCTIVE_H_
#define FB_DISTINCTIVE_H_

#include "fb_common.h"

namespace fb {

// at(j) -> const uint4 * of descriptor j (two uint4, LDS or global), j in [0, N), N >= 1.  Lane i owns rows i, i + 64, ...
// The median of a row, vDists[(int)(0.5 * (N - 1))] of the sorted row, is the smallest v with #{j : dist(i, j) <= v} >= k + 1:
// found by bisection on the distance value (0..256), counting over the row each step -- no sort.  `median < BestMedian` is
// strict, so the smallest index among the least medians wins.  Every lane returns the winner.
template <typename At>
__device__ __forceinline__ int distinctive_pick(int lane, int N, At at) {
  const int k = (int)(0.5 * (N - 1));
  int bestMedian = INT_MAX, bestIdx = INT_MAX;
  for (int i = lane; i < N; i += 64) {
    uint32_t d[8];
    const uint4 *mine = at(i);
    const uint4 a = mine[0], c = mine[1];
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = c.x; d[5] = c.y; d[6] = c.z; d[7] = c.w;
    int lo = 0, hi = 256;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      int cnt = 0;
      for (int j = 0; j < N; j++) cnt += (hamming256(d, at(j)) <= mid) ? 1 : 0;
      if (cnt >= k + 1) hi = mid; else lo = mid + 1;
    }
    if (lo < bestMedian) { bestMedian = lo; bestIdx = i; }  // ascending i per lane: first minimum kept
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int om = __shfl_xor(bestMedian, o, 64), oi = __shfl_xor(bestIdx, o, 64);
    if (om < bestMedian || (om == bestMedian && oi < bestIdx)) { bestMedian = om; bestIdx = oi; }
  }
  return bestIdx;
}

}  // namespace fb
#endif
