/*
 * fb_primitives.h -- the wave-wide and workgroup-wide device routines of every kernel file: butterfly reductions and the
 * inclusive scan over the 64 lanes, the exclusive scan / sum of one int per thread over a workgroup, and the bitonic
 * sort in LDS.  Results that are held bit-exact against the oracle (candidate order, compaction order, CSR order, fp64
 * sums) depend on the exact text here: one copy, so that a fix reaches every caller.
 */
#ifndef FB_PRIMITIVES_H_
#define FB_PRIMITIVES_H_

#include <hip/hip_runtime.h>

namespace fb {

// sum over the 64 lanes, every lane gets it.  The exchange order (32 .. 1) is part of the result for float / double.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// maximum over the 64 lanes, every lane gets it (float: a NaN never replaces a number; double: fmax)
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(v, o, 64); if (t > v) v = t; }
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// inclusive scan over the 64 lanes
__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
  return v;
}

// exclusive scan of one int per thread over an NT-thread block (s_wv: [NT / 64] ints of LDS); *total = block sum
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int *s_wv, int *total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int inc = wave_incl_scan(v);
  __syncthreads();
  if (lane == 63) s_wv[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; w++) { const int x = s_wv[w]; if (w < wv) base += x; tot += x; }
  *total = tot;
  return base + inc - v;
}

// sum of one int per thread over an NT-thread block (s_wv: [NT / 64] ints of LDS); every thread gets it
template <int NT>
__device__ __forceinline__ int block_sum(int v, int *s_wv) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_wv[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < NT / 64; w++) t += s_wv[w];
  return t;
}

// ascending sort of key[0..n2) (n2 a power of two >= 2, unused entries = the key type's maximum); ends with a barrier
template <typename K>
__device__ __forceinline__ void bitonic_sort(K *key, int n2, int tid, int nt) {
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += nt) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const K a = key[i], b = key[ixj];
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

}  // namespace fb
#endif
