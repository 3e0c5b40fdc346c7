// fb_sim3_pairs.h -- the HIP side that sim3_solver.hip and opt_sim3.hip share: the walk over matches12 (it keeps what
// s3::keep_pair of sim3_plan.h keeps), the only rowmul, the one large-LDS opt-in.  k_sim3_prepare calls the walk; k_optimize_sim3
// has the same walk written out, since through the function that kernel ran 1 % longer.
// Unnamed namespace like the kernels: the header belongs to one translation unit at a time.
#ifndef FB_SIM3_PAIRS_H_
#define FB_SIM3_PAIRS_H_

#include <atomic>
#include "fb_common.h"
#include "fb_primitives.h"
#include "sim3_plan.h"

namespace {
namespace s3 {

// Rcw*X + tcw of a cv::Mat 3x3 * 3x1 product in float, row r of the row-major 3x4 T.  The pragma makes the
// text mean the same in a file that build.py compiles with contraction allowed.
__device__ __forceinline__ float rowmul(const float *T, int r, float X, float Y, float Z) {
#pragma clang fp contract(off)
  return ((T[r * 4] * X + T[r * 4 + 1] * Y) + T[r * 4 + 2] * Z) + T[r * 4 + 3];
}

// The constructor loop of Sim3Solver (Sim3Solver.cc:56-101) and the edge loop of OptimizeSim3 (Optimizer.cc:1613-1692) for
// candidate c, by one NT-thread workgroup: i1 = 0 .. min(n_kf, stride) - 1 in chunks of NT, the kept pairs compacted in
// ascending i1 by a block scan (s_wv: [NT / 64] ints of LDS).  kf1_index == NULL is i1 itself, as OptimizeSim3 takes it
// (:1624); kf2_index == NULL is the slot.  emit(row, i1, k1, k2, o1, o2, P1c, P2c) runs on the thread of each kept pair.
// -> the number of kept pairs (every thread gets it)
template <int NT, typename Emit>
__device__ __forceinline__ int walk_pairs(const fb_kf_target &kf1, const fb_kf_target &kf2, const fb_mp_list &mp1, const fb_mp_list &mp2,
                                          const float *T1w, const float *T2w, int c, const int32_t *matches12, const int32_t *kf1_index,
                                          const int32_t *kf2_index, int *s_wv, Emit &&emit) {
  const int tid = threadIdx.x, s1 = kf1.kf_stride, s2 = kf2.kf_stride;
  int n1 = kf1.n_kf[0];
  n1 = n1 < 0 ? 0 : (n1 > s1 ? s1 : n1);
  const int32_t *m12 = matches12 + (size_t)c * s1;
  const float *xw2 = mp2.mp_xw + (size_t)c * s2 * 3;
  const float *T2 = T2w + (size_t)c * 12;
  struct Src {
    int i1;
    const uint8_t *v1, *v2;
    const int32_t *ix1, *ix2;
    const fb_keypoint *kps1, *kps2;
    __device__ bool valid1() const { return v1[i1] != 0; }
    __device__ bool valid2(int j) const { return v2[j] != 0; }
    __device__ int k1() const { return ix1 ? ix1[i1] : i1; }
    __device__ int k2(int j) const { return ix2 ? ix2[j] : j; }
    __device__ int o1(int k) const { return kps1[k].octave; }
    __device__ int o2(int k) const { return kps2[k].octave; }
  };
  Src src{0, mp1.mp_valid, mp2.mp_valid + (size_t)c * s2, kf1_index, kf2_index ? kf2_index + (size_t)c * s2 : nullptr,
          kf1.kf_kps, kf2.kf_kps + (size_t)c * s2};
  int base = 0;
  for (int c0 = 0; c0 < n1; c0 += NT) {
    const int i1 = c0 + tid;
    int j = -1, k1 = -1, k2 = -1, o1 = 0, o2 = 0;
    bool keep = false;
    if (i1 < n1) {
      j = m12[i1];
      src.i1 = i1;
      keep = keep_pair(j, s1, s2, src, &k1, &k2, &o1, &o2);
    }
    int tot;
    const int row = base + fb::block_excl_scan<NT>(keep ? 1 : 0, s_wv, &tot);
    if (keep) {  // row < s1: at most one row per i1 < n1 <= s1
      const float *X1 = mp1.mp_xw + (size_t)i1 * 3, *X2 = xw2 + (size_t)j * 3;
      float P1c[3], P2c[3];
      for (int q = 0; q < 3; q++) {
        P1c[q] = rowmul(T1w, q, X1[0], X1[1], X1[2]);
        P2c[q] = rowmul(T2, q, X2[0], X2[1], X2[2]);
      }
      emit(row, i1, k1, k2, o1, o2, P1c, P2c);
    }
    base += tot;
  }
  return base;
}

// A kernel whose dynamic LDS may exceed the 64 KiB default is told to the runtime once per device and process, with the byte
// count its plan allows.  (One static per kernel: the template argument.)
template <auto Kernel>
inline int allow_large_lds(size_t bytes) {
  static std::atomic<bool> done[64];
  int dev = 0;
  FB_HIP(hipGetDevice(&dev));
  if (dev >= 0 && dev < 64 && done[dev].load()) return FB_OK;
  FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (dev >= 0 && dev < 64) done[dev].store(true);
  return FB_OK;
}

}  // namespace s3
}  // namespace
#endif
