// correct_matches_math.h -- per-lane arithmetic of the optimal correction of a correspondence onto an epipolar geometry
// (csrc/correct_matches.hip), written once for the device and for the host (tests/emu/emu_correct_matches.cpp compiles it with
// g++).  The algorithm is Hartley & Sturm's, as in OpenCV's correctMatches, which the reference calls on its grid of virtual
// points in dsac_tools/utils_misc.py:176,206; the contract is spelled out in include/dfepe.h (dfepe_correct_matches).
// Everything here is fp64 and a pure function of its arguments: no LDS, no wavefront operations, and no array that is indexed
// at run time (every loop over an array is fully unrolled), so the device code keeps all of it in registers.
//
// The route, for F and the pair (p, q) with q'^T F p' = 0 wanted:
//   1 epipoles e1 (F e1 = 0), e2 (e2^T F = 0) as the largest cross product of two rows / two columns of F;
//   2 translate p and q to the origins, scale the epipoles to ex^2 + ey^2 = 1 and rotate them onto (1, 0, f): the geometry
//     becomes G = [[f1 f2 d, -f2 c, -f2 d], [-f1 b, a, b], [-f1 d, c, d]];
//   3 the epipolar lines of the first image are the pencil through (1, 0, f1); written homogeneously, the line through
//     (0, tau, ups) -- t = tau / ups is Hartley & Zisserman's parameter, ups = 0 their t = infinity -- has the squared distance
//       s(tau, ups) = tau^2 / (ups^2 + f1^2 tau^2) + C^2 / (A^2 + f2^2 C^2),   A = a tau + b ups, C = c tau + d ups
//     to the two origins, and its stationary points are the real roots of the binary sextic (H&Z eq. 12.7, homogenised)
//       g = tau ups (A^2 + f2^2 C^2)^2 - (a d - b c) (ups^2 + f1^2 tau^2)^2 A C;
//   4 every real root is found in one of two charts, t = tau / ups in [-1, 1] and u = ups / tau in [-1, 1] (the same
//     coefficients in reverse order), so that no root bound is needed, a vanishing leading coefficient is an ordinary root
//     near u = 0, and u = 0 itself is the candidate t = infinity;
//   5 the candidate of smallest s gives the closest points (tau^2 f1, tau ups, tau^2 f1^2 + ups^2) and
//     (f2 C^2, -A C, f2^2 C^2 + A^2), which are rotated and translated back.
//
// Roots in [-1, 1] of a polynomial of degree N: between two consecutive roots of its derivative it is monotonic, so the roots
// of the fifth derivative (linear) bracket those of the fourth, and so on up to the sextic.  Every level has a fixed number of
// slots (N for degree N) and every bracket that holds a sign change gets the same kBisect halvings and kNewton Newton steps:
// the iteration counts do not depend on the data, and lanes of a wavefront differ only in which brackets they skip.
#pragma once
#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define CM_HD __host__ __device__ inline
#else
#define CM_HD inline
#endif

namespace cm {

constexpr int kDeg = 6;
constexpr int kMaxCand = 2 * kDeg + 1;  // six slots per chart and t = infinity
constexpr int kBisect = 36;             // halvings of a bracket of width <= 2: 3e-11 absolute
constexpr int kNewton = 3;              // then quadratic convergence to the last bits

struct Result {
  double x1, y1, x2, y2, cost;  // corrected p, corrected q, |p - p'|^2 + |q - q'|^2
};

CM_HD bool finite(double x) { return fabs(x) <= DBL_MAX; }

// p(x) for the coefficients c[0..N] (c[k] of x^k)
template <int N>
CM_HD double horner(const double* c, double x) {
  double r = c[N];
#pragma unroll
  for (int k = N - 1; k >= 0; --k) r = fma(r, x, c[k]);
  return r;
}

// The root of p (degree N) in [lo, hi], where p changes sign; below_lo: p(lo) < 0.
template <int N>
CM_HD double refine(const double* c, double lo, double hi, bool below_lo) {
#pragma unroll 1
  for (int it = 0; it < kBisect; ++it) {
    const double m = 0.5 * (lo + hi);
    const bool below = horner<N>(c, m) < 0.0;
    lo = (below == below_lo) ? m : lo;
    hi = (below == below_lo) ? hi : m;
  }
  double x = 0.5 * (lo + hi);
#pragma unroll 1
  for (int it = 0; it < kNewton; ++it) {
    double f = c[N], df = 0.0;
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
      df = fma(df, x, f);
      f = fma(f, x, c[k]);
    }
    const double xn = x - f / df;
    x = (xn >= lo && xn <= hi) ? xn : x;  // a step out of the bracket (or a NaN) is not taken
  }
  return x;
}

// One level: the roots in [-1, 1] of p (degree N) from the N - 1 slots of its derivative (ascending in [-1, 1]; a slot that
// is no root only splits a monotonic stretch in two).  out[i] is the root in bracket i when bit i of the result is set, and the
// bracket's upper end otherwise, so that out is ascending again.  The sign of zero counts as positive on both sides of a
// breakpoint: a sign change is seen by exactly one bracket.
template <int N>
CM_HD unsigned level(const double* c, const double* slots, double* out) {
  double lo = -1.0;
  bool below_lo = horner<N>(c, lo) < 0.0;
  unsigned found = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double hi = (i < N - 1) ? slots[i < N - 1 ? i : 0] : 1.0;
    const bool below_hi = horner<N>(c, hi) < 0.0;
    double x = hi;
    if (below_lo != below_hi) {
      x = refine<N>(c, lo, hi, below_lo);
      found |= 1u << i;
    }
    out[i] = x;
    lo = hi;
    below_lo = below_hi;
  }
  return found;
}

// Real roots in [-1, 1] of the sextic c[0..6]: roots[i] is one when bit i of the result is set.
CM_HD unsigned roots_unit(const double* c, double* roots) {
  double d1[6], d2[5], d3[4], d4[3], d5[2];
#pragma unroll
  for (int k = 0; k < 6; ++k) d1[k] = (k + 1) * c[k + 1];
#pragma unroll
  for (int k = 0; k < 5; ++k) d2[k] = (k + 1) * d1[k + 1];
#pragma unroll
  for (int k = 0; k < 4; ++k) d3[k] = (k + 1) * d2[k + 1];
#pragma unroll
  for (int k = 0; k < 3; ++k) d4[k] = (k + 1) * d3[k + 1];
#pragma unroll
  for (int k = 0; k < 2; ++k) d5[k] = (k + 1) * d4[k + 1];
  double s1[1], s2[2], s3[3], s4[4], s5[5];
  const double x = -d5[0] / d5[1];
  s1[0] = (x > -1.0 && x < 1.0) ? x : 1.0;
  level<2>(d4, s1, s2);
  level<3>(d3, s2, s3);
  level<4>(d2, s3, s4);
  level<5>(d1, s4, s5);
  return level<6>(c, s5, roots);
}

// The geometry of one correspondence after translation, scaling and rotation.
struct Frame {
  double a, b, c, d, f1, f2;    // G11, G12, G21, G22 and the third coordinates of the two epipoles
  double ex1, ey1, ex2, ey2;    // the unit directions of the translated epipoles (the rotations)
  bool ok;                      // false: the point sits on an epipole
};

// the cross product of largest norm among u x v, u x w, v x w
CM_HD void null_vector(const double* u, const double* v, const double* w, double* e) {
  const double a0 = u[1] * v[2] - u[2] * v[1], a1 = u[2] * v[0] - u[0] * v[2], a2 = u[0] * v[1] - u[1] * v[0];
  const double b0 = u[1] * w[2] - u[2] * w[1], b1 = u[2] * w[0] - u[0] * w[2], b2 = u[0] * w[1] - u[1] * w[0];
  const double c0 = v[1] * w[2] - v[2] * w[1], c1 = v[2] * w[0] - v[0] * w[2], c2 = v[0] * w[1] - v[1] * w[0];
  const double na = a0 * a0 + a1 * a1 + a2 * a2, nb = b0 * b0 + b1 * b1 + b2 * b2, nc = c0 * c0 + c1 * c1 + c2 * c2;
  const bool ta = na >= nb && na >= nc, tb = !ta && nb >= nc;
  e[0] = ta ? a0 : (tb ? b0 : c0);
  e[1] = ta ? a1 : (tb ? b1 : c1);
  e[2] = ta ? a2 : (tb ? b2 : c2);
}

CM_HD Frame frame_of(const double* Fin, double px, double py, double qx, double qy) {
  double F[9], m = 0.0;
#pragma unroll
  for (int j = 0; j < 9; ++j) m = fmax(m, fabs(Fin[j]));
#pragma unroll
  for (int j = 0; j < 9; ++j) F[j] = Fin[j] / m;  // the sextic is homogeneous of degree 4 in F
  double e1[3], e2[3];
  null_vector(F, F + 3, F + 6, e1);  // orthogonal to the rows
  const double c0[3] = {F[0], F[3], F[6]}, c1[3] = {F[1], F[4], F[7]}, c2[3] = {F[2], F[5], F[8]};
  null_vector(c0, c1, c2, e2);       // orthogonal to the columns
  // translated epipoles, T^-1 e
  double ex1 = e1[0] - px * e1[2], ey1 = e1[1] - py * e1[2];
  double ex2 = e2[0] - qx * e2[2], ey2 = e2[1] - qy * e2[2];
  const double n1 = ex1 * ex1 + ey1 * ey1, n2 = ex2 * ex2 + ey2 * ey2;
  Frame fr;
  fr.ok = n1 > 0.0 && n2 > 0.0;
  const double r1 = 1.0 / sqrt(n1), r2 = 1.0 / sqrt(n2);
  ex1 *= r1; ey1 *= r1; ex2 *= r2; ey2 *= r2;
  fr.f1 = e1[2] * r1;
  fr.f2 = e2[2] * r2;
  // F' = T2^T F T1: the third column gains p, then the third row gains q
  const double f02 = fma(px, F[0], fma(py, F[1], F[2]));
  const double f12 = fma(px, F[3], fma(py, F[4], F[5]));
  const double g20 = fma(qx, F[0], fma(qy, F[3], F[6]));
  const double g21 = fma(qx, F[1], fma(qy, F[4], F[7]));
  const double g22 = fma(qx, f02, fma(qy, f12, fma(px, F[6], fma(py, F[7], F[8]))));
  // G = R2 F' R1^T, R = [[ex, ey, 0], [-ey, ex, 0], [0, 0, 1]]: only its lower right 2x2 is needed
  const double h01 = ex1 * F[1] - ey1 * F[0], h11 = ex1 * F[4] - ey1 * F[3];
  fr.a = ex2 * h11 - ey2 * h01;
  fr.b = ex2 * f12 - ey2 * f02;
  fr.c = ex1 * g21 - ey1 * g20;
  fr.d = g22;
  fr.ex1 = ex1; fr.ey1 = ey1; fr.ex2 = ex2; fr.ey2 = ey2;
  return fr;
}

// Coefficients of the sextic in t (g[k] of t^k, i.e. of tau^k ups^(6-k)), divided by the largest magnitude among them.
CM_HD void sextic_of(const Frame& fr, double* g) {
  const double a = fr.a, b = fr.b, c = fr.c, d = fr.d, f1s = fr.f1 * fr.f1, f2s = fr.f2 * fr.f2;
  const double p0 = b * b + f2s * d * d, p1 = 2.0 * (a * b + f2s * c * d), p2 = a * a + f2s * c * c;  // A^2 + f2^2 C^2
  const double det = a * d - b * c, s0 = b * d, s1 = a * d + b * c, s2 = a * c;                       // A C
  const double f1q = f1s * f1s;
  g[0] = -det * s0;
  g[1] = p0 * p0 - det * s1;
  g[2] = 2.0 * p0 * p1 - det * (s2 + 2.0 * f1s * s0);
  g[3] = 2.0 * p0 * p2 + p1 * p1 - det * (2.0 * f1s * s1);
  g[4] = 2.0 * p1 * p2 - det * (2.0 * f1s * s2 + f1q * s0);
  g[5] = p2 * p2 - det * (f1q * s1);
  g[6] = -det * (f1q * s2);
  double m = 0.0;
#pragma unroll
  for (int k = 0; k <= kDeg; ++k) m = fmax(m, fabs(g[k]));
  const double r = 1.0 / m;
#pragma unroll
  for (int k = 0; k <= kDeg; ++k) g[k] *= r;
}

CM_HD double cost_of(const Frame& fr, double tau, double ups) {
  const double A = fr.a * tau + fr.b * ups, C = fr.c * tau + fr.d * ups;
  return tau * tau / (ups * ups + fr.f1 * fr.f1 * tau * tau) + C * C / (A * A + fr.f2 * fr.f2 * C * C);
}

// The correction of (p, q) under F (row-major).  KEEP: also list the candidates that were evaluated, as t = tau / ups
// (infinity for ups = 0), in cand[0 .. *ncand) (kMaxCand entries) -- the host emulation's view; the kernel passes false.
template <bool KEEP>
CM_HD Result correct(const double* F, double px, double py, double qx, double qy, double* cand, int* ncand) {
  const Frame fr = frame_of(F, px, py, qx, qy);
  double g[kDeg + 1];
  sextic_of(fr, g);
  double best = cost_of(fr, 1.0, 0.0), btau = 1.0, bups = 0.0;  // t = infinity
  best = (best == best) ? best : HUGE_VAL;
  int n = 0;
  if (KEEP) cand[n++] = HUGE_VAL;
#pragma unroll 1
  for (int chart = 0; chart < 2; ++chart) {
    double c[kDeg + 1], r[kDeg];
#pragma unroll
    for (int k = 0; k <= kDeg; ++k) c[k] = chart ? g[kDeg - k] : g[k];
    const unsigned found = roots_unit(c, r);
#pragma unroll
    for (int i = 0; i < kDeg; ++i) {
      const bool is_root = (found >> i) & 1u;
      const double tau = chart ? 1.0 : r[i], ups = chart ? r[i] : 1.0;
      const double s = cost_of(fr, tau, ups);
      if (KEEP && is_root) cand[n++] = tau / ups;
      const bool take = is_root && s < best;
      best = take ? s : best;
      btau = take ? tau : btau;
      bups = take ? ups : bups;
    }
  }
  if (KEEP) *ncand = n;
  // the closest points of the two lines to the origins, rotated (R^T) and translated back
  const double A = fr.a * btau + fr.b * bups, C = fr.c * btau + fr.d * bups;
  const double X1 = btau * btau * fr.f1, Y1 = btau * bups, W1 = btau * btau * fr.f1 * fr.f1 + bups * bups;
  const double X2 = fr.f2 * C * C, Y2 = -A * C, W2 = fr.f2 * fr.f2 * C * C + A * A;
  Result out;
  out.x1 = px + (fr.ex1 * X1 - fr.ey1 * Y1) / W1;
  out.y1 = py + (fr.ey1 * X1 + fr.ex1 * Y1) / W1;
  out.x2 = qx + (fr.ex2 * X2 - fr.ey2 * Y2) / W2;
  out.y2 = qy + (fr.ey2 * X2 + fr.ex2 * Y2) / W2;
  out.cost = best;
  if (!(fr.ok && finite(out.x1) && finite(out.y1) && finite(out.x2) && finite(out.y2) && finite(out.cost))) {
    const double qn = NAN;
    out.x1 = out.y1 = out.x2 = out.y2 = out.cost = qn;
  }
  return out;
}

}  // namespace cm
