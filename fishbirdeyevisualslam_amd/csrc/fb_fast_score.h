// FAST-9-16 corner score (cv::cornerScore<16>): the min / max network over the 16 arcs of 9, written ONCE over an "ops"
// struct, so that the 32-bit integer form (one pixel per lane) and the packed binary16 form (two pixels per lane, orb.hip)
// are the same text.  Compiles for host and device: tests/cpp/fast_score_packed_ref.cpp instantiates it on the CPU.
//
// An ops struct provides
//   T                    the value type (one difference, or two packed ones)
//   sub(v, c)            centre - tap                             (exact: every quantity is an integer in [-255, 255])
//   min3(a, b, c), max3(a, b, c)
//   lowest(), highest()  identities of max3 / min3 (-256 / +256)
//   finish(A, Bm)        max(max(A, -Bm) - 1, 0) in the form the caller stores
#pragma once

#if defined(__HIPCC__)
#define FB_SCORE_HD __host__ __device__ __forceinline__
#else
#define FB_SCORE_HD inline
#endif

namespace fbscore {

// Offset of ring pixel i (0..15, the order of cv::FAST's pattern) from the CENTRE in an image of pitch tp.
FB_SCORE_HD constexpr int ring_offset(int i, int tp) {
  constexpr int dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
  constexpr int dy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
  return dy[i] * tp + dx[i];
}

// d[i] = centre - ring pixel i.  Sliding min / max over the 16 arcs of 9 in three-operand form:
// arc of 3 -> arc of 9 = three arcs of 3 -> reduction, 40 three-operand instructions per polarity.
template <class Ops>
FB_SCORE_HD typename Ops::T score_network(const typename Ops::T (&d)[16]) {
  typedef typename Ops::T T;
  T mn3[16], mx3[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    mn3[i] = Ops::min3(d[i], d[(i + 1) & 15], d[(i + 2) & 15]);
    mx3[i] = Ops::max3(d[i], d[(i + 1) & 15], d[(i + 2) & 15]);
  }
  T A = Ops::lowest(), Bm = Ops::highest();
#pragma unroll
  for (int i = 0; i < 16; i += 2) {
    const T a0 = Ops::min3(mn3[i], mn3[(i + 3) & 15], mn3[(i + 6) & 15]);
    const T a1 = Ops::min3(mn3[i + 1], mn3[(i + 4) & 15], mn3[(i + 7) & 15]);
    const T b0 = Ops::max3(mx3[i], mx3[(i + 3) & 15], mx3[(i + 6) & 15]);
    const T b1 = Ops::max3(mx3[i + 1], mx3[(i + 4) & 15], mx3[(i + 7) & 15]);
    A = Ops::max3(A, a0, a1);
    Bm = Ops::min3(Bm, b0, b1);
  }
  return Ops::finish(A, Bm);
}

// one pixel, 32-bit integers (v_min3_i32 / v_max3_i32 on the device)
struct IntOps {
  typedef int T;
  static FB_SCORE_HD int sub(int v, int c) { return v - c; }
  static FB_SCORE_HD int min3(int a, int b, int c) { const int m = a < b ? a : b; return m < c ? m : c; }
  static FB_SCORE_HD int max3(int a, int b, int c) { const int m = a > b ? a : b; return m > c ? m : c; }
  static FB_SCORE_HD int lowest() { return -256; }
  static FB_SCORE_HD int highest() { return 256; }
  static FB_SCORE_HD int finish(int A, int Bm) { return max3(A, -Bm, 1) - 1; }  // = max(max(A, -Bm) - 1, 0)
};

// Packed form: two pixels per 32-bit word, min / max on IEEE binary16 pairs (MinMax supplies min3 / max3 on such
// words: the three-operand packed instructions on the device, a bit-level binary16 model in the CPU test).
// Encoding: for an integer k in [0, 1023] the half 1024 + k has the bit pattern 0x6400 + k (ulp 1 in that binade).  The
// two bytes of a tap pair are packed as plain 16-bit integers, the centre pair carries the bias 0x6600, and ONE packed
// 16-bit integer subtraction gives 0x6600 + d, the half 1536 + d for d = centre - tap in [-255, 255] (1281..1791 stays
// inside the binade).  min and max commute with the common bias, so the network runs on the biased values as they
// are; only finish() has to negate: 1536 - Bm is the pattern 0xcc00 - (0x6600 + Bm), again an integer subtraction.
// max3(A, -Bm, 1) - 1 = max(max(A, -Bm) - 1, 0) then is one max3 against 0x6601 and a subtraction of 0x6601, which
// leaves the clamped score as a plain byte in bits 0-7 and 16-23.  Every half the min / max see lies in
// [1280, 1792]: no NaN, no infinity, no denormal and no zero of either sign can occur, so neither the NaN rule of the
// minimum / maximum instructions nor the denormal mode matters.
FB_SCORE_HD unsigned pk_sub_u16(unsigned a, unsigned b) {  // per 16-bit half, wrapping
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned short u16x2_ __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, (u16x2_)(__builtin_bit_cast(u16x2_, a) - __builtin_bit_cast(u16x2_, b)));
#else
  return ((a - b) & 0xffffu) | (((a >> 16) - (b >> 16)) << 16);
#endif
}
FB_SCORE_HD unsigned pk_pair(unsigned x0, unsigned x1) { return x0 | (x1 << 16); }       // two tap bytes
FB_SCORE_HD unsigned pk_centre(unsigned x0, unsigned x1) { return pk_pair(x0, x1) + 0x66006600u; }  // + the bias
template <class MinMax>
struct PackedOps {
  typedef unsigned T;
  static FB_SCORE_HD unsigned sub(unsigned centre, unsigned taps) { return pk_sub_u16(centre, taps); }
  static FB_SCORE_HD unsigned min3(unsigned a, unsigned b, unsigned c) { return MinMax::min3(a, b, c); }
  static FB_SCORE_HD unsigned max3(unsigned a, unsigned b, unsigned c) { return MinMax::max3(a, b, c); }
  static FB_SCORE_HD unsigned lowest() { return 0x65006500u; }   // 1536 - 256
  static FB_SCORE_HD unsigned highest() { return 0x67006700u; }  // 1536 + 256
  static FB_SCORE_HD unsigned finish(unsigned A, unsigned Bm) {  // -> the clamped scores in bytes 0 and 2, bytes 1 and 3 zero
    return pk_sub_u16(MinMax::max3(A, pk_sub_u16(0xcc00cc00u, Bm), 0x66016601u), 0x66016601u);
  }
};

}  // namespace fbscore
