/*
 * fb_sort_scan.h -- workgroup-wide LDS routines shared by bow.hip and kfdb.hip: bitonic sort of 64-bit keys
 * (optionally dragging a 32-bit payload along) and an exclusive scan of one int per thread.
 */
#ifndef FB_SORT_SCAN_H_
#define FB_SORT_SCAN_H_

#include <hip/hip_runtime.h>

namespace fb {

// ascending sort of key[0..n2) (n2 a power of two >= 2, unused entries = ~0ull); ends with a barrier
__device__ __forceinline__ void bitonic_sort(unsigned long long *key, int n2, int tid, int nt) {
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += nt) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = key[i], b = key[ixj];
          const bool up = (i & k) == 0;
          if ((a > b) == up) { key[i] = b; key[ixj] = a; }
        }
      }
      __syncthreads();
    }
}

// the same with val[i] following key[i] (keys are distinct where the payload matters)
__device__ __forceinline__ void bitonic_sort_kv(unsigned long long *key, int *val, int n2, int tid, int nt) {
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += nt) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = key[i], b = key[ixj];
          const bool up = (i & k) == 0;
          if ((a > b) == up) {
            key[i] = b; key[ixj] = a;
            const int va = val[i]; val[i] = val[ixj]; val[ixj] = va;
          }
        }
      }
      __syncthreads();
    }
}

// exclusive scan of one int per thread over an NT-thread block (s_wv: [NT / 64] ints of LDS); *total = block sum
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int *s_wv, int *total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
  __syncthreads();
  if (lane == 63) s_wv[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; w++) { const int x = s_wv[w]; if (w < wv) base += x; tot += x; }
  *total = tot;
  return base + inc - v;
}

}  // namespace fb
#endif
