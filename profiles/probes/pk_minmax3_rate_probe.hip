// Issue rate of v_pk_minimum3_f16 / v_pk_maximum3_f16 against v_min3_i32 on gfx950: a long run of instructions on 8
// independent accumulator chains, timed per wave with s_memtime, for one workgroup of 1, 4, 8 and 16 waves (one
// workgroup lives on one CU: 4 waves = one per SIMD, 16 waves = four per SIMD).  Prints ticks per instruction and wave,
// and the SIMD's instructions per tick; the RATIO between the rows of one wave count is the result (the tick is the
// counter's own unit).
//   hipcc --offload-arch=gfx950 -O3 pk_minmax3_rate_probe.hip -o pk_minmax3_rate_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#define REP8(x) x x x x x x x x
constexpr int ITERS = 512, PER_ITER = 64;  // 8 chains x 8 per iteration
template <int KIND>
__global__ __launch_bounds__(1024) void k(unsigned *sink, unsigned long long *ticks) {
  // operands: halves in [1280, 1792] as in the score network (valid for the integer form too)
  unsigned a0 = 0x66006600u + threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
  const unsigned b = 0x66106610u, c = 0x65f065f0u + threadIdx.x;
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
  for (int i = 0; i < ITERS; i++) {
#define STEP(op) asm volatile(op " %0, %0, %8, %9\n" op " %1, %1, %8, %9\n" op " %2, %2, %8, %9\n" op " %3, %3, %8, %9\n" \
                              op " %4, %4, %8, %9\n" op " %5, %5, %8, %9\n" op " %6, %6, %8, %9\n" op " %7, %7, %8, %9" \
                              : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c));
    if (KIND == 0) { REP8(STEP("v_min3_i32")) }
    if (KIND == 1) { REP8(STEP("v_pk_minimum3_f16")) }
    if (KIND == 2) { REP8(STEP("v_pk_maximum3_f16")) }
#undef STEP
  }
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_sched_barrier(0);
  sink[threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
  if ((threadIdx.x & 63) == 0) ticks[threadIdx.x >> 6] = t1 - t0;
}
template <int KIND>
void run(const char *name, unsigned *sink, unsigned long long *ticks) {
  const int waves[4] = {1, 4, 8, 16};
  for (int w = 0; w < 4; w++) {
    unsigned long long h[16];
    for (int rep = 0; rep < 2; rep++) {  // the first launch warms the instruction cache
      k<KIND><<<1, 64 * waves[w]>>>(sink, ticks);
      if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return; }
    }
    if (hipMemcpy(h, ticks, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return;
    double sum = 0, mx = 0;
    for (int i = 0; i < waves[w]; i++) { sum += (double)h[i]; if ((double)h[i] > mx) mx = (double)h[i]; }
    const double n = (double)ITERS * PER_ITER, perSimd = waves[w] < 4 ? 1.0 : waves[w] / 4.0;
    printf("%-20s waves %2d  ticks/instr/wave %.4f  instr/tick/SIMD %.3f\n", name, waves[w], sum / waves[w] / n, perSimd * n / mx);
  }
}
int main() {
  unsigned *sink; unsigned long long *ticks;
  if (hipMalloc(&sink, 1024 * 4) != hipSuccess || hipMalloc(&ticks, 16 * 8) != hipSuccess) { printf("no device\n"); return 1; }
  run<0>("v_min3_i32", sink, ticks);
  run<1>("v_pk_minimum3_f16", sink, ticks);
  run<2>("v_pk_maximum3_f16", sink, ticks);
  return 0;
}
