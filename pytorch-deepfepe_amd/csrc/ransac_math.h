// ransac_math.h -- per-lane arithmetic of the RANSAC fundamental-matrix estimator (csrc/ransac.hip), written once for the device
// and for the host (tests/emu/emu_ransac.cpp compiles it with g++).  The algorithm is OpenCV 3.4's findFundamentalMat(FM_RANSAC),
// which the reference calls in dsac_tools/utils_opencv.py:157; the contract is spelled out in include/dfepe.h
// (dfepe_ransac_fundamental).  Everything here is a pure function of its arguments: no LDS, no wavefront operations.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ inline
#else
#define RS_HD inline
#endif

namespace rs {

constexpr int kSample = 7;          // points per minimal sample (7-point solver)
constexpr int kMaxAttempts = 1000;  // draws of a sample before an iteration gives up (OpenCV's maxAttempts)
constexpr int kMaxRoots = 3;
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
// Count-table codes (dfepe_ransac_fundamental's hyp_counts): a root that does not exist, an iteration that drew no sample.
constexpr int kNoRoot = -1;
constexpr int kNoSample = -2;

RS_HD uint64_t splitmix64(uint64_t x) {
  x += kGolden;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// The index stream of iteration k: draw c (c = 0, 1, ...) is splitmix64(key + c * kGolden) with key = splitmix64(seed ^
// splitmix64(k)), mapped to [0, N) by Lemire's multiply-shift of its upper 32 bits.  Keyed by (seed, k) only, never by the pair.
struct Stream {
  uint64_t key;
  uint64_t ctr;
};
RS_HD Stream stream_of(uint64_t seed, int k) { return Stream{splitmix64(seed ^ splitmix64((uint64_t)k)), 0ull}; }
RS_HD int draw_index(Stream& s, int N) {
  const uint64_t x = splitmix64(s.key + s.ctr * kGolden);
  s.ctr += 1;
  return (int)(((x >> 32) * (uint64_t)N) >> 32);
}

// OpenCV's haveCollinearPoints for a complete sample (non-partial checkSubset): the LAST point against every line through two
// earlier ones.  Differences in float (as OpenCV forms them from Point2f), the test in double; the products of two float
// differences are exact in double, so the result does not depend on whether the compiler fuses the subtraction.
RS_HD bool collinear_last(const float* x, const float* y) {
  const int i = kSample - 1;
#pragma unroll
  for (int j = 0; j < i; ++j) {
    const double dx1 = (double)(x[j] - x[i]), dy1 = (double)(y[j] - y[i]);
#pragma unroll
    for (int k = 0; k < j; ++k) {
      const double dx2 = (double)(x[k] - x[i]), dy2 = (double)(y[k] - y[i]);
      if (fabs(dx2 * dy1 - dy2 * dx1) <= (double)FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
    }
  }
  return false;
}

// One iteration's sample: 7 distinct indices, redrawn (continuing the same stream) while the sample is collinear in either image.
// P: callable, P(i) -> object with .x .y .z .w = (x1, y1, x2, y2) of correspondence i in pixels.  false after kMaxAttempts.
template <class P>
RS_HD bool draw_sample(uint64_t seed, int k, int N, const P& pts, int* idx) {
  Stream s = stream_of(seed, k);
  for (int att = 0; att < kMaxAttempts; ++att) {
    float x1[kSample], y1[kSample], x2[kSample], y2[kSample];
#pragma unroll
    for (int i = 0; i < kSample; ++i) {
      int v;
      bool dup;
      do {
        v = draw_index(s, N);
        dup = false;
#pragma unroll
        for (int j = 0; j < i; ++j) dup = dup || (idx[j] == v);
      } while (dup);
      idx[i] = v;
      const auto m = pts(v);
      x1[i] = m.x; y1[i] = m.y; x2[i] = m.z; y2[i] = m.w;
    }
    if (!collinear_last(x1, y1) && !collinear_last(x2, y2)) return true;
  }
  return false;
}

RS_HD double det3(const double* a, const double* b, const double* c) {  // det of the matrix with columns a, b, c
  return a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1]) + c[0] * (a[1] * b[2] - a[2] * b[1]);
}

// Real roots of c3 l^3 + c2 l^2 + c1 l + c0 (Numerical Recipes' trigonometric / Cardano form), each polished by two Newton
// steps, ascending.  Returns their number.
RS_HD int solve_cubic(double c3, double c2, double c1, double c0, double* r) {
  int n = 0;
  if (c3 == 0.0) {
    if (c2 == 0.0) {
      if (c1 == 0.0) return 0;
      r[0] = -c0 / c1;
      return 1;
    }
    const double d = c1 * c1 - 4.0 * c2 * c0;
    if (d < 0.0) return 0;
    const double q = -0.5 * (c1 + (c1 >= 0.0 ? sqrt(d) : -sqrt(d)));
    r[0] = q / c2;
    r[1] = (q != 0.0) ? c0 / q : r[0];
    n = 2;
  } else {
    const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
    const double Q = (a * a - 3.0 * b) / 9.0;
    const double R = (2.0 * a * a * a - 9.0 * a * b + 27.0 * c) / 54.0;
    const double Q3 = Q * Q * Q;
    const double d = Q3 - R * R;
    if (d >= 0.0) {
      const double ratio = (Q3 > 0.0) ? fmin(fmax(R / sqrt(Q3), -1.0), 1.0) : 0.0;
      const double theta = acos(ratio), sq = -2.0 * sqrt(fmax(Q, 0.0));
      const double two_pi = 6.283185307179586476925;
      r[0] = sq * cos(theta / 3.0) - a / 3.0;
      r[1] = sq * cos((theta + two_pi) / 3.0) - a / 3.0;
      r[2] = sq * cos((theta - two_pi) / 3.0) - a / 3.0;
      n = 3;
    } else {
      double e = cbrt(sqrt(-d) + fabs(R));
      if (R > 0.0) e = -e;
      r[0] = (e + Q / e) - a / 3.0;
      n = 1;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (i >= n) break;
    double x = r[i];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const double f = ((c3 * x + c2) * x + c1) * x + c0, df = (3.0 * c3 * x + 2.0 * c2) * x + c1;
      if (df != 0.0) x -= f / df;
    }
    r[i] = x;
  }
  // ascending (a three-element network; n <= 3)
  if (n >= 2 && r[1] < r[0]) { const double t = r[0]; r[0] = r[1]; r[1] = t; }
  if (n == 3) {
    if (r[2] < r[1]) { const double t = r[1]; r[1] = r[2]; r[2] = t; }
    if (r[1] < r[0]) { const double t = r[0]; r[0] = r[1]; r[1] = t; }
  }
  return n;
}

// The 2-D null space of the 7x9 system in normalised coordinates: Householder QR of A^T (9x7); the last two columns of Q span
// the null space of A.  Rows of A: [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] (so that x2^T F x1 = 0).
RS_HD void null_space7(const double* x1, const double* y1, const double* x2, const double* y2, double* f1, double* f2) {
  double M[9][kSample];  // column j = row j of A
#pragma unroll
  for (int j = 0; j < kSample; ++j) {
    M[0][j] = x2[j] * x1[j]; M[1][j] = x2[j] * y1[j]; M[2][j] = x2[j];
    M[3][j] = y2[j] * x1[j]; M[4][j] = y2[j] * y1[j]; M[5][j] = y2[j];
    M[6][j] = x1[j];         M[7][j] = y1[j];         M[8][j] = 1.0;
  }
  double beta[kSample];
#pragma unroll
  for (int j = 0; j < kSample; ++j) {
    double nn = 0.0;
#pragma unroll
    for (int r = j; r < 9; ++r) nn += M[r][j] * M[r][j];
    const double nrm = sqrt(nn);
    const double alpha = (M[j][j] < 0.0) ? nrm : -nrm;
    M[j][j] -= alpha;  // M[j..8][j] is now the Householder vector v_j
    const double vv = nn - 2.0 * alpha * (M[j][j] + alpha) + alpha * alpha;  // |x - alpha e|^2
    beta[j] = (vv > 0.0) ? 2.0 / vv : 0.0;
#pragma unroll
    for (int c = j + 1; c < kSample; ++c) {
      double s = 0.0;
#pragma unroll
      for (int r = j; r < 9; ++r) s += M[r][j] * M[r][c];
      s *= beta[j];
#pragma unroll
      for (int r = j; r < 9; ++r) M[r][c] -= s * M[r][j];
    }
  }
#pragma unroll
  for (int r = 0; r < 9; ++r) { f1[r] = (r == 7) ? 1.0 : 0.0; f2[r] = (r == 8) ? 1.0 : 0.0; }
#pragma unroll
  for (int j = kSample - 1; j >= 0; --j) {  // Q e = H_0 H_1 ... H_6 e
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int r = j; r < 9; ++r) { s1 += M[r][j] * f1[r]; s2 += M[r][j] * f2[r]; }
    s1 *= beta[j];
    s2 *= beta[j];
#pragma unroll
    for (int r = j; r < 9; ++r) { f1[r] -= s1 * M[r][j]; f2[r] -= s2 * M[r][j]; }
  }
}

// The 7-point solver on one sample given in pixels.  The sample is normalised first (centroid to the origin, RMS distance
// sqrt(2), per image); each root l of det(l F1 + (1 - l) F2) = 0 (ascending) gives F = T2^T (l F1 + (1 - l) F2) T1 in pixels,
// scaled so that F22 = 1 where |F22| > DBL_EPSILON.  F: 3 x 9 doubles, row-major 3x3 each.  Returns the number of roots (0..3).
RS_HD int seven_point(const float* px1, const float* py1, const float* px2, const float* py2, double* F) {
  double T[2][3];  // per image: s, cx, cy (x_n = s (x - cx))
  double x1[kSample], y1[kSample], x2[kSample], y2[kSample];
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const float* px = v ? px2 : px1;
    const float* py = v ? py2 : py1;
    double cx = 0.0, cy = 0.0;
#pragma unroll
    for (int i = 0; i < kSample; ++i) { cx += (double)px[i]; cy += (double)py[i]; }
    cx /= kSample;
    cy /= kSample;
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < kSample; ++i) {
      const double dx = (double)px[i] - cx, dy = (double)py[i] - cy;
      ss += dx * dx + dy * dy;
    }
    const double s = (ss > 0.0) ? sqrt(2.0 * kSample / ss) : 1.0;
    T[v][0] = s; T[v][1] = cx; T[v][2] = cy;
#pragma unroll
    for (int i = 0; i < kSample; ++i) {
      const double xn = s * ((double)px[i] - cx), yn = s * ((double)py[i] - cy);
      if (v) { x2[i] = xn; y2[i] = yn; } else { x1[i] = xn; y1[i] = yn; }
    }
  }
  double f1[9], f2[9];
  null_space7(x1, y1, x2, y2, f1, f2);
  double D[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) D[k] = f1[k] - f2[k];
  // det(F2 + l D) = c3 l^3 + c2 l^2 + c1 l + c0 by columns (a = F2's, b = D's)
  double a0[3], a1[3], a2[3], b0[3], b1[3], b2[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    a0[r] = f2[3 * r]; a1[r] = f2[3 * r + 1]; a2[r] = f2[3 * r + 2];
    b0[r] = D[3 * r];  b1[r] = D[3 * r + 1];  b2[r] = D[3 * r + 2];
  }
  const double c0 = det3(a0, a1, a2), c3 = det3(b0, b1, b2);
  const double c1 = det3(b0, a1, a2) + det3(a0, b1, a2) + det3(a0, a1, b2);
  const double c2 = det3(a0, b1, b2) + det3(b0, a1, b2) + det3(b0, b1, a2);
  double lam[3];
  const int n = solve_cubic(c3, c2, c1, c0, lam);
#pragma unroll
  for (int i = 0; i < kMaxRoots; ++i) {
    if (i >= n) break;
    double Fn[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Fn[k] = f2[k] + lam[i] * D[k];
    // F = T2^T Fn T1 with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
    const double s1 = T[0][0], u1 = -T[0][0] * T[0][1], w1 = -T[0][0] * T[0][2];
    const double s2 = T[1][0], u2 = -T[1][0] * T[1][1], w2 = -T[1][0] * T[1][2];
    double G[9];  // Fn T1
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      G[3 * r + 0] = Fn[3 * r + 0] * s1;
      G[3 * r + 1] = Fn[3 * r + 1] * s1;
      G[3 * r + 2] = Fn[3 * r + 0] * u1 + Fn[3 * r + 1] * w1 + Fn[3 * r + 2];
    }
    double* Fo = F + 9 * i;
#pragma unroll
    for (int c = 0; c < 3; ++c) {  // T2^T G
      Fo[c] = s2 * G[c];
      Fo[3 + c] = s2 * G[3 + c];
      Fo[6 + c] = u2 * G[c] + w2 * G[3 + c] + G[6 + c];
    }
    if (fabs(Fo[8]) > DBL_EPSILON) {
      const double sc = 1.0 / Fo[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) Fo[k] *= sc;
      Fo[8] = 1.0;
    }
  }
  return n;
}

// Iteration k of a pair, whole: its sample drawn, gathered and solved.  The count (median) launch and the select launch both go
// through here, which is what makes the winner come out again bit for bit.  Returns the number of roots, or kNoSample.
template <class P>
RS_HD int solve_iteration(uint64_t seed, int k, int N, const P& pts, double* F) {
  int idx[kSample];
  if (!draw_sample(seed, k, N, pts, idx)) return kNoSample;
  float x1[kSample], y1[kSample], x2[kSample], y2[kSample];
#pragma unroll
  for (int i = 0; i < kSample; ++i) {
    const auto m = pts(idx[i]);
    x1[i] = m.x; y1[i] = m.y; x2[i] = m.z; y2[i] = m.w;
  }
  return seven_point(x1, y1, x2, y2, F);
}

// OpenCV's FMEstimatorCallback::computeError decision without the divisions: err = max(d1^2, d2^2) <= t2, with d2 the distance of
// x2 to the line F x1 and d1 the distance of x1 to the line F^T x2 (both share the residual r = x2^T F x1).
RS_HD bool is_inlier(const double* F, double x1, double y1, double x2, double y2, double t2) {
  const double a = F[0] * x1 + F[1] * y1 + F[2], b = F[3] * x1 + F[4] * y1 + F[5], c = F[6] * x1 + F[7] * y1 + F[8];
  const double r = x2 * a + y2 * b + c;
  const double a2 = F[0] * x2 + F[3] * y2 + F[6], b2 = F[1] * x2 + F[4] * y2 + F[7];
  const double rr = r * r;
  return rr <= t2 * (a * a + b * b) && rr <= t2 * (a2 * a2 + b2 * b2);
}

// OpenCV's RANSACUpdateNumIters(p, ep, M, niters) for the three model sizes built (7-point F, five-point E, 4-point H);
// (1 - ep)^M by multiplications, each M in its own fixed order, so that every build forms the same value.
template <int M>
RS_HD int update_num_iters(double p, double ep, int niters) {
  static_assert(M == 7 || M == 5 || M == 4, "model sizes of the estimators built");
  p = fmin(fmax(p, 0.0), 1.0);
  ep = fmin(fmax(ep, 0.0), 1.0);
  const double num = fmax(1.0 - p, DBL_MIN);
  const double q = 1.0 - ep, q2 = q * q, q4 = q2 * q2;
  double den;
  if constexpr (M == 7) den = 1.0 - q4 * q2 * q;
  else if constexpr (M == 5) den = 1.0 - q4 * q;
  else den = 1.0 - q2 * q2;
  if (den < DBL_MIN) return 0;
  const double ln = log(num), ld = log(den);
  return (ld >= 0.0 || -ln >= niters * (-ld)) ? niters : (int)rint(ln / ld);
}

// The sequential selection rule of all three RANSAC estimators over one pair's count table counts[k * ROOTS + r] (k < max_iters;
// ROOTS slots an iteration, SAMPLE points a model: <3, 7> F, <10, 5> E, <1, 4> H).  Writes the winning (k, r) or (-1, -1) and
// returns the best count (0 when no model); *iters = iterations consumed (the k the loop stopped at).  This is the definition:
// the select launches evaluate the same rule a wavefront at a time (select_wave, csrc/robust_dev.h).
template <int ROOTS, int SAMPLE>
RS_HD int select_best(const int* counts, int N, double confidence, int max_iters, int* best_k, int* best_r, int* iters) {
  int best = 0, niters = max_iters, k = 0;
  *best_k = -1;
  *best_r = -1;
  for (; k < niters; ++k) {
    if (counts[ROOTS * k] == kNoSample) break;  // as OpenCV: the loop ends (and no model exists when k == 0)
    for (int r = 0; r < ROOTS; ++r) {
      const int c = counts[ROOTS * k + r];
      if (c > (best > SAMPLE - 1 ? best : SAMPLE - 1)) {
        best = c;
        *best_k = k;
        *best_r = r;
        niters = update_num_iters<SAMPLE>(confidence, (double)(N - c) / N, niters);
      }
    }
  }
  *iters = k;
  return best;
}

// The 7-point estimator's instantiations under the names its callers and the host emulation use.
RS_HD int update_num_iters(double p, double ep, int niters) { return update_num_iters<kSample>(p, ep, niters); }
RS_HD int select_best(const int* counts, int N, double confidence, int max_iters, int* best_k, int* best_r, int* iters) {
  return select_best<kMaxRoots, kSample>(counts, N, confidence, max_iters, best_k, best_r, iters);
}

}  // namespace rs
