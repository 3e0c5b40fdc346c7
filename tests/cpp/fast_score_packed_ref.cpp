// CPU check of the FAST score network of csrc/fb_fast_score.h -- TEST INFRASTRUCTURE (tests/test_fast_score_packed.py).
//
// The header's network is instantiated twice on the host: with the plain int ops, and with the packed ops over a
// bit-level model of the packed binary16 min3 / max3 (every half is DECODED to its real value with the helpers below,
// compared as a real number and the selected operand's pattern is returned, as IEEE minimum / maximum do), so that the
// encoding trick itself is what gets checked.  No _Float16: the helpers are explicit.  Both are compared with the
// oracle's own fast_score (oracle/orb_oracle.cpp, an anonymous-namespace function: this file includes that source
// to reach it; the library built here is loaded on its own and never mixed with liboracle.so).
#include <cmath>
#include <cstdint>

#include "../../oracle/orb_oracle.cpp"
#include "../../fishbirdeyevisualslam_amd/csrc/fb_fast_score.h"

namespace {

long long g_bad_class = 0;  // halves seen by min3 / max3 that were NaN, infinite, denormal or zero (must stay 0)

// IEEE 754 binary16 -> double (every binary16 value is exact in a double)
double h2d(unsigned h) {
  const int s = (h >> 15) & 1, e = (h >> 10) & 31, m = h & 1023;
  double v;
  if (e == 0) v = std::ldexp((double)m, -24);  // zero / denormal
  else if (e == 31) v = m ? NAN : INFINITY;
  else v = std::ldexp((double)(1024 + m), e - 25);
  return s ? -v : v;
}

// double -> binary16, round to nearest even (used by the encoding checks)
unsigned d2h(double v) {
  if (std::isnan(v)) return 0x7e00;
  const unsigned s = std::signbit(v) ? 0x8000u : 0u;
  double a = std::fabs(v);
  if (a >= 65520.0) return s | 0x7c00;
  if (a < std::ldexp(1.0, -14)) return s | (unsigned)std::nearbyint(std::ldexp(a, 24));  // denormal (or the first normal)
  int e;
  const double f = std::frexp(a, &e);                                  // a = f * 2^e, f in [0.5, 1)
  const unsigned q = (unsigned)std::nearbyint(std::ldexp(f, 11));      // 1024..2048
  return s | (unsigned)(((e + 14) << 10) + (q - 1024));                // q == 2048 carries into the exponent
}

void classify(unsigned h) {
  const int e = (h >> 10) & 31;
  if (e == 0 || e == 31) g_bad_class++;
}

unsigned sel_half(unsigned a, unsigned b, bool wantMin) {
  classify(a);
  classify(b);
  const double x = h2d(a), y = h2d(b);
  if (std::isnan(x) || std::isnan(y)) return 0x7e00;  // minimum / maximum propagate a NaN
  if (x == y) return wantMin ? ((a & 0x8000) ? a : b) : ((a & 0x8000) ? b : a);  // -0 < +0
  return (x < y) == wantMin ? a : b;
}

struct ModelMinMax {
  static unsigned op3(unsigned a, unsigned b, unsigned c, bool wantMin) {
    const unsigned lo = sel_half(sel_half(a & 0xffff, b & 0xffff, wantMin), c & 0xffff, wantMin);
    const unsigned hi = sel_half(sel_half(a >> 16, b >> 16, wantMin), c >> 16, wantMin);
    return lo | (hi << 16);
  }
  static unsigned min3(unsigned a, unsigned b, unsigned c) { return op3(a, b, c, true); }
  static unsigned max3(unsigned a, unsigned b, unsigned c) { return op3(a, b, c, false); }
};
typedef fbscore::PackedOps<ModelMinMax> ModelOps;

int score_int(const uint8_t *p) {  // 7x7 patch, centre at (3, 3)
  const uint8_t *c = p + 3 * 7 + 3;
  int d[16];
  for (int i = 0; i < 16; i++) d[i] = fbscore::IntOps::sub(c[0], c[fbscore::ring_offset(i, 7)]);
  return fbscore::score_network<fbscore::IntOps>(d);
}

unsigned score_packed(const uint8_t *p0, const uint8_t *p1) {
  const uint8_t *c0 = p0 + 3 * 7 + 3, *c1 = p1 + 3 * 7 + 3;
  const unsigned v = fbscore::pk_centre(c0[0], c1[0]);
  unsigned d[16];
  for (int i = 0; i < 16; i++) d[i] = ModelOps::sub(v, fbscore::pk_pair(c0[fbscore::ring_offset(i, 7)], c1[fbscore::ring_offset(i, 7)]));
  return fbscore::score_network<ModelOps>(d);
}

int score_oracle(const uint8_t *p) {
  Image im;
  im.w = im.h = 7;
  im.d.assign(p, p + 49);
  return std::max(fast_score(im, 3, 3), 0);  // the extractor stores the score clamped at 0
}

}  // namespace

extern "C" {

// n patches of 49 bytes.  Patch i is scored in the LOW half paired with patch n-1-i in the HIGH half, so every patch
// passes through both halves.  out[3 * i + 0..2] = oracle, int network, packed network (low-half result of pair i);
// returns the number of patches whose high-half result differs from their low-half result, or -1 if a result word had
// a non-zero byte 1 or 3.
long long fsp_score_batch(const uint8_t *patches, long long n, int *out) {
  long long halves_differ = 0;
  for (long long i = 0; i < n; i++) {
    const unsigned r = score_packed(patches + 49 * i, patches + 49 * (n - 1 - i));
    if (r & 0xff00ff00u) return -1;
    out[3 * i + 0] = score_oracle(patches + 49 * i);
    out[3 * i + 1] = score_int(patches + 49 * i);
    out[3 * i + 2] = (int)(r & 0xff);
    const unsigned r2 = score_packed(patches + 49 * (n - 1 - i), patches + 49 * i);
    if ((r2 >> 16) != (r & 0xff)) halves_differ++;
  }
  return halves_differ;
}

long long fsp_bad_class_count() { return g_bad_class; }

// The encoding itself, exhaustively: returns the number of failures of
//  (a) sub(pk_centre(v, v'), pk_pair(c, c')) decodes to 1536 + (v - c) | 1536 + (v' - c') for all byte pairs,
//      and equals the binary16 ENCODING of that number (d2h);
//  (b) lowest() / highest() decode to 1536 -/+ 256;
//  (c) finish(A, Bm) == max(max(A, -Bm) - 1, 0) in both halves for all A, Bm in [-256, 256] (biased patterns).
long long fsp_check_encoding() {
  long long bad = 0;
  for (int v = 0; v < 256; v++)
    for (int c = 0; c < 256; c++) {
      const int v2 = 255 - v, c2 = (c * 7 + 3) & 255;
      const unsigned r = ModelOps::sub(fbscore::pk_centre(v, v2), fbscore::pk_pair(c, c2));
      if (h2d(r & 0xffff) != 1536.0 + (v - c) || h2d(r >> 16) != 1536.0 + (v2 - c2)) bad++;
      if ((r & 0xffff) != d2h(1536.0 + (v - c)) || (r >> 16) != d2h(1536.0 + (v2 - c2))) bad++;
    }
  if (h2d(ModelOps::lowest() & 0xffff) != 1280.0 || h2d(ModelOps::lowest() >> 16) != 1280.0) bad++;
  if (h2d(ModelOps::highest() & 0xffff) != 1792.0 || h2d(ModelOps::highest() >> 16) != 1792.0) bad++;
  for (int A = -256; A <= 256; A++)
    for (int Bm = -256; Bm <= 256; Bm++) {
      const int A2 = -A, B2 = (Bm * 5 + 17) % 257;
      const unsigned a = d2h(1536.0 + A) | (d2h(1536.0 + A2) << 16), b = d2h(1536.0 + Bm) | (d2h(1536.0 + B2) << 16);
      const unsigned r = ModelOps::finish(a, b);
      const int e0 = std::max(std::max(A, -Bm) - 1, 0), e1 = std::max(std::max(A2, -B2) - 1, 0);
      if ((int)(r & 0xffff) != e0 || (int)(r >> 16) != e1) bad++;
    }
  return bad;
}

}  // extern "C"
