// lmeds_math.h -- per-lane arithmetic of the least-median-of-squares estimators (csrc/lmeds.hip), written once for the device and
// for the host (tests/emu/emu_lmeds.cpp compiles it with g++).  The algorithm is OpenCV 3.4's LMeDSPointSetRegistrator::run, which
// cv2.findFundamentalMat(.., cv2.RANSAC, ..) falls back to below 15 correspondences (the reference's dsac_tools/utils_opencv.py:157)
// and which cv2.findEssentialMat runs with method LMEDS; the contract is spelled out in include/dfepe.h (dfepe_lmeds_fundamental).
// Sampler and minimal solvers are ransac_math.h's and ransac5_math.h's, unchanged.  New here: the errors themselves (the RANSAC
// kernels only compare them against a threshold and avoid the divisions), the median of N of them, sigma, and the selection rule.
#pragma once
#include "ransac5_math.h"

namespace lm {

constexpr double kOutlierRatio = 0.45;     // the outlier ratio OpenCV's LMedS assumes for its fixed iteration count
constexpr double kNoRoot = -1.0;           // median-table codes (medians themselves are >= 0 or +inf)
constexpr double kNoSample = -2.0;
constexpr uint32_t kInfBits = 0x7F800000u;
constexpr uint32_t kPadBits = 0x7FFFFFFFu; // fills a lane's unused slots: above every error pattern, never reached by a rank < N

// niters of the whole run: RANSACUpdateNumIters(confidence, 0.45, m, max_iters), m = 7 or 5.
RS_HD int num_iters(int model_points, double confidence, int max_iters) {
  return model_points == rs::kSample ? rs::update_num_iters(confidence, kOutlierRatio, max_iters)
                                     : r5::update_num_iters(confidence, kOutlierRatio, max_iters);
}

RS_HD uint32_t float_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
RS_HD float bits_float(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// An fp64 error rounded to fp32; anything that is not a finite non-negative number counts as +inf.
RS_HD float err_float(double e) {
  const float f = (float)e;
  return (f >= 0.0f && f < __builtin_inff()) ? f : __builtin_inff();
}
RS_HD uint32_t err_bits(double e) { return float_bits(err_float(e)) & 0x7FFFFFFFu; }  // -0 cannot occur; the mask keeps 31 value bits

// OpenCV's FMEstimatorCallback::computeError: max(d1^2, d2^2) in px^2, d2 the distance of x2 to the line F x1, d1 the distance of
// x1 to the line F^T x2.  A zero line norm or a non-finite quotient gives NaN, which err_float turns into +inf.
RS_HD double f_error(const double* F, double x1, double y1, double x2, double y2) {
  const double a = F[0] * x1 + F[1] * y1 + F[2], b = F[3] * x1 + F[4] * y1 + F[5], c = F[6] * x1 + F[7] * y1 + F[8];
  const double r = x2 * a + y2 * b + c;
  const double a2 = F[0] * x2 + F[3] * y2 + F[6], b2 = F[1] * x2 + F[4] * y2 + F[7];
  const double rr = r * r, s2 = a * a + b * b, s1 = a2 * a2 + b2 * b2;
  const double d2 = rr / s2, d1 = rr / s1;
  const bool ok = s1 > 0.0 && s2 > 0.0 && d1 == d1 && d2 == d2;
  return ok ? (d1 > d2 ? d1 : d2) : __builtin_nan("");
}

// OpenCV's EMEstimatorCallback::computeError: the Sampson error in normalised coordinates.
RS_HD double e_error(const double* E, double x1, double y1, double x2, double y2) {
  const double a = E[0] * x1 + E[1] * y1 + E[2], b = E[3] * x1 + E[4] * y1 + E[5], c = E[6] * x1 + E[7] * y1 + E[8];
  const double r = x2 * a + y2 * b + c;
  const double a2 = E[0] * x2 + E[3] * y2 + E[6], b2 = E[1] * x2 + E[4] * y2 + E[7];
  const double den = a * a + b * b + a2 * a2 + b2 * b2;
  return den > 0.0 ? r * r / den : __builtin_nan("");
}

// ---- the median of N fp32 error patterns held 64 lanes x R registers ------------------------------------------------------
// Non-negative floats order like their bit patterns (what OpenCV's sort relies on).  A wavefront holds the N patterns as R
// registers per lane, slot j of lane l being correspondence 64 j + l and kPadBits past N.  W is the wavefront: w.sum(f) and
// w.max(f) apply f to every lane's register array (const uint32_t (&)[R]) and return the sum / maximum over the 64 lanes -- a
// cross-lane reduction on the device, a loop over the lanes on the host.  Every loop over the registers has constant bounds, so
// on the device the array is never indexed at run time.

constexpr int kLadder[7] = {1, 2, 4, 8, 16, 32, 64};
RS_HD int regs_for(int N) {  // registers per lane of the smallest rung that holds N
  int r = 1;
  while (64 * r < N) r *= 2;
  return r;
}

// The pattern of rank k (0-based, ascending, duplicates counted) among the wavefront's values, found from the most significant of
// the 31 value bits down: a round counts the values that agree with the bits decided so far and have a 0 in the round's bit; when
// rank k is among them the bit is 0, otherwise it is 1 and k drops by that count.  31 rounds of R compares and one reduction.
template <int R, class W>
RS_HD uint32_t select_rank(W& w, int k) {
  uint32_t prefix = 0u, decided = 0u;
  for (int b = 30; b >= 0; --b) {
    const uint32_t look = decided | (1u << b);
    const int zeros = w.sum([&](const uint32_t(&v)[R]) {
      int c = 0;
#pragma unroll
      for (int j = 0; j < R; ++j) c += (((v[j] ^ prefix) & look) == 0u) ? 1 : 0;
      return c;
    });
    if (k >= zeros) {
      prefix |= 1u << b;
      k -= zeros;
    }
    decided = look;
  }
  return prefix;
}

// OpenCV's median of the sorted errors: sorted[N/2] for odd N, (sorted[N/2 - 1] + sorted[N/2]) * 0.5f (sum in fp32) for even N.
// The lower neighbour of the rank-N/2 value is the largest value below it when exactly N/2 values are below it, otherwise (a run
// of equal values reaches down over rank N/2 - 1) the value itself.
template <int R, class W>
RS_HD float median_of(W& w, int N) {
  const uint32_t hi = select_rank<R>(w, N / 2);
  if (N & 1) return bits_float(hi);
  const int below = w.sum([&](const uint32_t(&v)[R]) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) c += (v[j] < hi) ? 1 : 0;
    return c;
  });
  uint32_t lo = hi;
  if (below == N / 2)
    lo = (uint32_t)w.max([&](const uint32_t(&v)[R]) {
      uint32_t m = 0u;
#pragma unroll
      for (int j = 0; j < R; ++j) m = (v[j] < hi && v[j] > m) ? v[j] : m;
      return (int)m;
    });
  return (bits_float(lo) + bits_float(hi)) * 0.5f;
}

// sigma of the winner and the squared fp32 bound its inliers stay under.
RS_HD double sigma_of(double min_median, int N, int model_points) {
  const double s = 2.5 * 1.4826 * (1.0 + 5.0 / (double)(N - model_points)) * sqrt(min_median);
  return s > 0.001 ? s : 0.001;
}
RS_HD float inlier_bound(double sigma) { return (float)(sigma * sigma); }

// The sequential selection rule over one pair's median table med[k * ROOTS + r] (k < niters): through k = 0, 1, ... and the
// roots in order a model whose median is strictly below the best so far (DBL_MAX at the start: +inf never wins) becomes the
// best; an iteration without a sample ends the loop.  Writes the winning (k, r) or (-1, -1), *iters = the k the loop stopped at,
// and returns the best median (DBL_MAX without a model).  This is the definition; the select launch evaluates it a wavefront at
// a time.
template <int ROOTS>
RS_HD double select_best(const double* med, int niters, int* best_k, int* best_r, int* iters) {
  double best = DBL_MAX;
  int k = 0;
  *best_k = -1;
  *best_r = -1;
  for (; k < niters; ++k) {
    if (med[ROOTS * k] == kNoSample) break;
    for (int r = 0; r < ROOTS; ++r) {
      const double m = med[ROOTS * k + r];
      if (m >= 0.0 && m < best) {
        best = m;
        *best_k = k;
        *best_r = r;
      }
    }
  }
  *iters = k;
  return best;
}

}  // namespace lm
