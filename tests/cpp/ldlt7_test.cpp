// ldlt7_test.cpp -- fb::ldlt<7> (csrc/fb_se3.h, the LinearSolverDense restatement of the Sim3 optimiser) on the host: the
// failure rule (a negative pivot -> false, x untouched), a solve against a known answer, the zero pivot of a fixed-scale
// system (row / column 6 of H is 0: the pivot is lambda alone), and that a NaN system does NOT report failure (every
// comparison with NaN is false), which is the branch a non-finite candidate takes on the device.
#include <cmath>
#include <cstdio>

#include "fb_se3.h"

#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
  double H[49], b[7], x[7], want[7];
  // SPD: H = M^T M + I with a fixed M
  double M[49];
  unsigned st = 7u;
  for (int i = 0; i < 49; i++) { st = st * 1664525u + 1013904223u; M[i] = ((st >> 8) / 16777216.0) - 0.5; }
  for (int i = 0; i < 7; i++)
    for (int j = 0; j < 7; j++) {
      double s = i == j ? 1.0 : 0.0;
      for (int k = 0; k < 7; k++) s += M[k * 7 + i] * M[k * 7 + j];
      H[i * 7 + j] = s;
    }
  for (int i = 0; i < 7; i++) want[i] = i - 3.0;
  const double lambda = 0.25;
  for (int i = 0; i < 7; i++) {
    double s = lambda * want[i];
    for (int j = 0; j < 7; j++) s += H[i * 7 + j] * want[j];
    b[i] = s;
  }
  EXPECT(fb::ldlt<7>(H, lambda, b, x));
  for (int i = 0; i < 7; i++) EXPECT(std::fabs(x[i] - want[i]) < 1e-12);
  // fixed scale: row and column 6 are exactly 0, the pivot is lambda; x[6] = b[6] / lambda
  double Hf[49], bf[7];
  for (int i = 0; i < 49; i++) Hf[i] = (i / 7 == 6 || i % 7 == 6) ? 0.0 : H[i];
  for (int i = 0; i < 7; i++) bf[i] = i == 6 ? 0.5 : b[i];
  EXPECT(fb::ldlt<7>(Hf, lambda, bf, x) && x[6] == 0.5 / lambda);
  // indefinite: a negative pivot in the middle -> false, x not written
  double Hn[49];
  for (int i = 0; i < 49; i++) Hn[i] = H[i];
  Hn[3 * 7 + 3] = -50.0;
  for (int i = 0; i < 7; i++) x[i] = 77.0;
  EXPECT(!fb::ldlt<7>(Hn, lambda, b, x));
  for (int i = 0; i < 7; i++) EXPECT(x[i] == 77.0);
  // lambda can repair it, as setLambda does
  EXPECT(fb::ldlt<7>(Hn, 100.0, b, x));
  // NaN: no comparison is true, so no failure is reported and x is NaN
  Hn[0] = std::nan("");
  EXPECT(fb::ldlt<7>(Hn, 100.0, b, x) && std::isnan(x[0]));
  // the same rule in dimension 6 (the pose optimiser's wrapper)
  double H6[36], b6[6], x6[6];
  for (int i = 0; i < 6; i++) { b6[i] = 1; for (int j = 0; j < 6; j++) H6[i * 6 + j] = i == j ? (i == 2 ? -1.0 : 1.0) : 0.0; }
  EXPECT(!fb::ldlt6(H6, 0.5, b6, x6) && fb::ldlt6(H6, 2.0, b6, x6) && x6[2] == 1.0);
  printf("ldlt7_test ok\n");
  return 0;
}
