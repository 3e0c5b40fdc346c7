/*
 * fb_lm.h -- optimize(n) of g2o's OptimizationAlgorithmLevenberg for ONE free vertex, written once for every
 * single-workgroup optimiser (pose.hip: SE3, dimension 6; opt_sim3.hip: Sim3, dimension 7).
 *   OptimizationAlgorithmLevenberg::solve  Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-164
 *   computeLambdaInit / computeScale       :166-189 (tau = 1e-5)
 *   SparseOptimizer::optimize              the loop over solve() that stops at the first result other than OK
 *
 * The shared state St lives in LDS and has: DIM; T, Ttrial, Teval (the vertex estimate, the trial estimate, the estimate
 * the edges' errors were last computed at); H[DIM * DIM], b[DIM], x[DIM]; red[1 + DIM (DIM + 1) / 2 + DIM] = the robust
 * chi2, the upper triangle of H row by row, b; ok2.
 * solve.solve(H, lambda, b, x) is LinearSolverDense on (H + lambda I) x = b; solve.oplus(x, T) the vertex' oplusImpl (it
 * may change x, as VertexSim3Expmap's does with a fixed scale).
 * TRIAL_LINEARISES = true: eval(T, robust) leaves all of red at T and ends in a barrier, so the pass at an accepted trial is
 * the linearisation of the next iteration.  false: eval(T, robust, linearise) leaves only red[0] unless `linearise`, and
 * an iteration that follows an accepted step starts with a linearising pass of its own (g2o's computeActiveErrors +
 * buildSystem at the top of solve()); for an edge whose Jacobian costs many error evaluations.
 * `solver` is true in the one thread that solves and moves S.T.  Every thread of the workgroup calls this and keeps the
 * same lambda / rho / chi2 from the shared sums, so all of them reach every barrier.
 */
#ifndef FB_LM_H_
#define FB_LM_H_

#include <hip/hip_runtime.h>
#include <math.h>

// Optional phase-stamp hooks of a diagnostic build: a file that wants them defines FB_LM_T0() / FB_LM_TICK(slot) before
// this header (they expand where the schedule is instantiated); nothing otherwise.  Slots: 4 solve, 5 oplus, 6 barrier.
#ifndef FB_LM_T0
#define FB_LM_T0()
#define FB_LM_TICK(slot_)
#endif

namespace fb {

template <int DIM>
__device__ __forceinline__ void unpack_system(const double *red, double *H, double *b) {
  int k = 1;
  for (int i = 0; i < DIM; i++)
    for (int j = i; j < DIM; j++) { H[i * DIM + j] = red[k]; H[j * DIM + i] = red[k]; k++; }
  for (int i = 0; i < DIM; i++) b[i] = red[1 + DIM * (DIM + 1) / 2 + i];
}

template <bool TRIAL_LINEARISES, class Solve, class St, class Eval>
__device__ __forceinline__ void lm_optimize(St &S, const Solve &solve, bool solver, bool robust, Eval &eval, int niter) {
  constexpr int DIM = St::DIM;
  if constexpr (TRIAL_LINEARISES) eval(S.T, robust);
  else eval(S.T, robust, true);
  if (solver) { unpack_system<DIM>(S.red, S.H, S.b); S.Teval = S.T; }
  double currentChi = S.red[0];
  __syncthreads();
  double lambda = 0, ni = 2;
  int nBadLM = 0;
  [[maybe_unused]] bool stale = false;  // (only without TRIAL_LINEARISES) S.H / S.b belong to the estimate before the last accepted step
  for (int iter = 0; iter < niter; iter++) {
    if constexpr (!TRIAL_LINEARISES) {
      if (stale) {
        eval(S.T, robust, true);
        if (solver) { unpack_system<DIM>(S.red, S.H, S.b); S.Teval = S.T; }
        currentChi = S.red[0];
        __syncthreads();
        stale = false;
      }
    }
    const double iniChi = currentChi;
    if (iter == 0) {
      double m = 0;
      for (int j = 0; j < DIM; j++) m = fmax(fabs(S.H[j * DIM + j]), m);
      lambda = 1e-5 * m;
      ni = 2;
      nBadLM = 0;
    }
    double rho = 0;
    int qmax = 0;
    do {
      {
        FB_LM_T0()
        if (solver) {
          S.ok2 = solve.solve(S.H, lambda, S.b, S.x) ? 1 : 0;
          FB_LM_TICK(4)
          S.Ttrial = solve.oplus(S.x, S.T);
          S.Teval = S.Ttrial;
          FB_LM_TICK(5)
        }
        __syncthreads();
        FB_LM_TICK(6)
      }
      if constexpr (TRIAL_LINEARISES) eval(S.Ttrial, robust);
      else eval(S.Ttrial, robust, false);
      double tempChi = S.red[0];
      if (!S.ok2) tempChi = 1.7976931348623157e308;
      rho = currentChi - tempChi;
      double scale = 0;
      for (int j = 0; j < DIM; j++) scale += S.x[j] * (lambda * S.x[j] + S.b[j]);
      scale += 1e-3;
      rho /= scale;
      const bool accept = rho > 0 && isfinite(tempChi);
      __syncthreads();  // everyone has read red/x/b
      if (accept) {
        double alpha = 1. - pow((2 * rho - 1), 3);
        alpha = fmin(alpha, 2. / 3.);
        const double scaleFactor = fmax(1. / 3., alpha);
        lambda *= scaleFactor;
        ni = 2;
        currentChi = tempChi;
        if (solver) {
          S.T = S.Ttrial;
          if constexpr (TRIAL_LINEARISES) unpack_system<DIM>(S.red, S.H, S.b);
        }
        if constexpr (!TRIAL_LINEARISES) stale = true;
      } else {
        lambda *= ni;
        ni *= 2;
      }
      __syncthreads();
      qmax++;
    } while (rho < 0 && qmax < 10);
    if (qmax == 10 || rho == 0) break;  // Terminate
    if ((iniChi - currentChi) * 1e3 < iniChi) nBadLM++;
    else nBadLM = 0;
    if (nBadLM >= 3) break;
  }
}

}  // namespace fb
#endif
