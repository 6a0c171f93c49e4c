// ransac5_math.h -- per-lane arithmetic of the RANSAC essential-matrix estimator (csrc/ransac5.hip), written once for the device
// and for the host (tests/emu/emu_ransac5.cpp compiles it with g++).  The algorithm is OpenCV 3.4's findEssentialMat(RANSAC),
// which the reference calls in dsac_tools/utils_opencv.py:147-151; the contract is spelled out in include/dfepe.h
// (dfepe_ransac_essential).  The random stream is ransac_math.h's.
//
// The minimal solver is Nister's: the 4-D null space {X, Y, Z, W} of the 5x9 epipolar system, the ten cubic constraints
// (2 E E^T E - tr(E E^T) E = 0, det E = 0) on E = x X + y Y + z Z + W as a 10x20 matrix over the monomials of degree <= 3,
// Gauss-Jordan elimination of the ten monomials of highest order in (x, y), the 3x3 polynomial matrix B(z) with B (x, y, 1)^T = 0,
// the real roots of det B(z) (degree 10), (x, y) from B's null vector, and Gauss-Newton steps on (x, y, z) against the ten
// constraints themselves.
//
// Nothing here that is indexed at run time lives in a local array: the 10x20 matrix (1600 bytes) and every other table go through
// a workspace `w` of kWork doubles that the caller provides -- w[i] must give a double& -- which is a plain array on the host and
// a lane-strided view of LDS on the device, so that the device code has no scratch memory.  Local arrays are only ever indexed by
// fully unrolled loops.
#pragma once
#include "ransac_math.h"

namespace r5 {

constexpr int kSample = 5;
constexpr int kMaxRoots = 10;
constexpr int kNoRoot = -1;

// workspace layout (doubles)
constexpr int kOffN = 0;     // [4][9]   null-space basis X, Y, Z, W (rows of 9: a 3x3 row-major each)
constexpr int kOffQ = 36;    // [6][10]  E E^T - tr/2 I (upper triangle, quadratic polynomials); later B(z): [3][13]
constexpr int kOffA = 96;    // [10][20] constraint matrix; before it the QR of the null space; after it the polynomial tables
constexpr int kOffE = kOffA; // [10][9]  the solutions, written last
constexpr int kWork = 296;
constexpr int kOffD = kOffA + 32;    // [11][11] derivative m of det B(z), coefficient of z^j at [m][j] (written after the matrix is used)
constexpr int kOffR0 = kOffA + 153;  // [10] roots of the odd derivatives
constexpr int kOffR1 = kOffA + 163;  // [10] roots of the even derivatives; at the end those of det B(z) itself

// A monomial x^i y^j z^k of degree <= 3 has the code 16 i + 4 j + k: codes add when monomials multiply.
RS_HD int lin_code(int a) { return a == 0 ? 16 : (a == 1 ? 4 : (a == 2 ? 1 : 0)); }  // x, y, z, 1
// column of the constraint matrix: the ten eliminated monomials x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy, then
// x z^2, x z, x, y z^2, y z, y, z^3, z^2, z, 1
RS_HD int col_of(int code) {
  static constexpr signed char t[49] = {19, 18, 17, 16, 15, 14, 13, -1, 7,  6,  -1, -1, 1,  -1, -1, -1, 12, 11, 10, -1, 9,  8,  -1, -1, 3,
                                        -1, -1, -1, -1, -1, -1, -1, 5,  4,  -1, -1, 2,  -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0};
  return t[code];
}
// slot of a monomial of degree <= 2 in a quadratic polynomial, and the code of a slot
RS_HD int quad_of(int code) {
  static constexpr signed char t[33] = {9, 8, 7, -1, 6, 5, -1, -1, 4, -1, -1, -1, -1, -1, -1, -1, 3,
                                        2, -1, -1, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0};
  return t[code];
}
RS_HD int quad_code(int s) {
  static constexpr signed char t[10] = {32, 20, 17, 16, 8, 5, 4, 2, 1, 0};
  return t[s];
}

// One iteration's sample: 5 distinct indices of ransac_math.h's stream (no geometric rejection).
RS_HD void draw_sample(uint64_t seed, int k, int N, int* idx) {
  rs::Stream s = rs::stream_of(seed, k);
#pragma unroll
  for (int i = 0; i < kSample; ++i) {
    int v;
    bool dup;
    do {
      v = rs::draw_index(s, N);
      dup = false;
#pragma unroll
      for (int j = 0; j < i; ++j) dup = dup || (idx[j] == v);
    } while (dup);
    idx[i] = v;
  }
}

// Pixels to normalised coordinates, q = ((x - K02) / K00, (y - K12) / K11), and the threshold in the same units.
struct Cam {
  double fx, fy, cx, cy;
};
RS_HD Cam cam_of(const float* K) { return Cam{(double)K[0], (double)K[4], (double)K[2], (double)K[5]}; }
RS_HD double norm_x(const Cam& c, float x) { return ((double)x - c.cx) / c.fx; }
RS_HD double norm_y(const Cam& c, float y) { return ((double)y - c.cy) / c.fy; }
RS_HD double threshold2(const Cam& c, double threshold) {
  const double t = threshold / ((c.fx + c.fy) / 2.0);
  return t * t;
}

// The 4-D null space of the 5x9 system, rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1]: Householder QR of A^T (9x5), the
// last four columns of Q, into w[kOffN ..].  Uses w[kOffA .. kOffA + 50) as its table.
template <class W>
RS_HD void null_space5(W& w, const double* x1, const double* y1, const double* x2, const double* y2) {
  const int M = kOffA, BETA = kOffA + 45;  // M[r][j] = w[M + 5 r + j]: column j = row j of A
#pragma unroll
  for (int j = 0; j < kSample; ++j) {
    w[M + 0 + j] = x2[j] * x1[j];  w[M + 5 + j] = x2[j] * y1[j];  w[M + 10 + j] = x2[j];
    w[M + 15 + j] = y2[j] * x1[j]; w[M + 20 + j] = y2[j] * y1[j]; w[M + 25 + j] = y2[j];
    w[M + 30 + j] = x1[j];         w[M + 35 + j] = y1[j];         w[M + 40 + j] = 1.0;
  }
  for (int j = 0; j < kSample; ++j) {
    double nn = 0.0;
    for (int r = j; r < 9; ++r) nn += w[M + 5 * r + j] * w[M + 5 * r + j];
    const double nrm = sqrt(nn);
    const double d = w[M + 5 * j + j];
    const double alpha = (d < 0.0) ? nrm : -nrm;
    w[M + 5 * j + j] = d - alpha;  // M[j..8][j] is now the Householder vector v_j
    const double vv = nn - 2.0 * alpha * d + alpha * alpha;  // |x - alpha e|^2
    const double beta = (vv > 0.0) ? 2.0 / vv : 0.0;
    w[BETA + j] = beta;
    for (int c = j + 1; c < kSample; ++c) {
      double s = 0.0;
      for (int r = j; r < 9; ++r) s += w[M + 5 * r + j] * w[M + 5 * r + c];
      s *= beta;
      for (int r = j; r < 9; ++r) w[M + 5 * r + c] -= s * w[M + 5 * r + j];
    }
  }
  for (int v = 0; v < 4; ++v) {  // Q e_(5 + v) = H_0 H_1 ... H_4 e_(5 + v)
    const int F = kOffN + 9 * v;
    for (int r = 0; r < 9; ++r) w[F + r] = (r == kSample + v) ? 1.0 : 0.0;
    for (int j = kSample - 1; j >= 0; --j) {
      double s = 0.0;
      for (int r = j; r < 9; ++r) s += w[M + 5 * r + j] * w[F + r];
      s *= w[BETA + j];
      for (int r = j; r < 9; ++r) w[F + r] -= s * w[M + 5 * r + j];
    }
  }
}

// The ten cubic constraints on E = x X + y Y + z Z + W into the 10x20 matrix w[kOffA + 20 row + column].
template <class W>
RS_HD void constraints(W& w) {
  for (int i = 0; i < 60; ++i) w[kOffQ + i] = 0.0;
  for (int i = 0; i < 200; ++i) w[kOffA + i] = 0.0;
  // (E E^T)_ik = sum_j E_ij E_kj for i <= k; pairs in the order 00 01 02 11 12 22
  int pr = 0;
  for (int i = 0; i < 3; ++i)
    for (int k = i; k < 3; ++k, ++pr)
      for (int j = 0; j < 3; ++j)
        for (int a = 0; a < 4; ++a) {
          const double ea = w[kOffN + 9 * a + 3 * i + j];
          for (int b = 0; b < 4; ++b) w[kOffQ + 10 * pr + quad_of(lin_code(a) + lin_code(b))] += ea * w[kOffN + 9 * b + 3 * k + j];
        }
  for (int s = 0; s < 10; ++s) {  // L = E E^T - tr(E E^T) / 2 I
    const double t = 0.5 * (w[kOffQ + s] + w[kOffQ + 30 + s] + w[kOffQ + 50 + s]);
    w[kOffQ + s] -= t;
    w[kOffQ + 30 + s] -= t;
    w[kOffQ + 50 + s] -= t;
  }
  // rows 0..8: (L E)_ij = sum_k L_ik E_kj (half of 2 E E^T E - tr(E E^T) E)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int row = kOffA + 20 * (3 * i + j);
      for (int k = 0; k < 3; ++k) {
        const int lo = i < k ? i : k, hi = i < k ? k : i;
        const int L = kOffQ + 10 * (lo == 0 ? hi : (lo == 1 ? 2 + hi : 5));
        for (int s = 0; s < 10; ++s) {
          const double l = w[L + s];
          const int qc = quad_code(s);
          for (int a = 0; a < 4; ++a) w[row + col_of(qc + lin_code(a))] += l * w[kOffN + 9 * a + 3 * k + j];
        }
      }
    }
  // row 9: det E by its first row; the minors go through the (now free) first slots of the L table
  for (int c = 0; c < 3; ++c) {
    const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;  // cofactor of E_0c = E_1c1 E_2c2 - E_1c2 E_2c1
    for (int s = 0; s < 10; ++s) w[kOffQ + s] = 0.0;
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b)
        w[kOffQ + quad_of(lin_code(a) + lin_code(b))] += w[kOffN + 9 * a + 3 + c1] * w[kOffN + 9 * b + 6 + c2] -
                                                         w[kOffN + 9 * a + 3 + c2] * w[kOffN + 9 * b + 6 + c1];
    for (int s = 0; s < 10; ++s) {
      const double m = w[kOffQ + s];
      const int qc = quad_code(s);
      for (int a = 0; a < 4; ++a) w[kOffA + 180 + col_of(qc + lin_code(a))] += m * w[kOffN + 9 * a + c];
    }
  }
}

// Gauss-Jordan elimination of columns 0..9 with row pivoting; rows 0..3 are only carried as far as they serve as pivot rows
// (rows 4..9 are what B(z) is read from).  false when a pivot is zero.
template <class W>
RS_HD bool eliminate(W& w) {
  const int A = kOffA;
  for (int c = 0; c < 10; ++c) {
    int p = c;
    double best = fabs(w[A + 20 * c + c]);
    for (int r = c + 1; r < 10; ++r) {
      const double v = fabs(w[A + 20 * r + c]);
      if (v > best) { best = v; p = r; }
    }
    if (!(best > 0.0)) return false;
    if (p != c)
      for (int j = c; j < 20; ++j) {
        const double t = w[A + 20 * c + j];
        w[A + 20 * c + j] = w[A + 20 * p + j];
        w[A + 20 * p + j] = t;
      }
    const double inv = 1.0 / w[A + 20 * c + c];
    for (int j = c; j < 20; ++j) w[A + 20 * c + j] *= inv;
    for (int r = 0; r < 10; ++r) {
      if (r == c || (r < 4 && r < c)) continue;
      const double f = w[A + 20 * r + c];
      if (f == 0.0) continue;
      for (int j = c + 1; j < 20; ++j) w[A + 20 * r + j] -= f * w[A + 20 * c + j];
      w[A + 20 * r + c] = 0.0;
    }
  }
  return true;
}

// dst[i + j] += sign a[i] b[j] (polynomials by ascending power, in the workspace)
template <class W>
RS_HD void poly_mac(W& w, int dst, int a, int na, int b, int nb, double sign) {
  for (int i = 0; i < na; ++i) {
    const double ai = sign * w[a + i];
    for (int j = 0; j < nb; ++j) w[dst + i + j] += ai * w[b + j];
  }
}

// derivative m of det B(z) at z (Horner over the stored coefficients)
template <class W>
RS_HD double deriv_at(W& w, int m, double z) {
  const int D = kOffD + 11 * m;
  double acc = w[D + 10 - m];
  for (int j = 9 - m; j >= 0; --j) acc = acc * z + w[D + j];
  return acc;
}

// B(z) from the eliminated rows 4..9 (pairs e/f, g/h, i/j: <k> = <e> - z <f>, ...), det B(z) and its real roots, ascending,
// into w[kOffR1 ..].  Returns their number.  The roots are isolated between the real roots of the derivative, level by level from
// the ninth derivative down (on each such interval the polynomial is monotonic), inside the Cauchy bound, and refined by Newton
// steps that fall back to bisection.
template <class W>
RS_HD int roots_of_det(W& w) {
  for (int m = 0; m < 3; ++m) {
    const int e = kOffA + 20 * (4 + 2 * m), f = e + 20, B = kOffQ + 13 * m;
    for (int v = 0; v < 2; ++v) {  // the x part (columns 10..12) and the y part (13..15): degree 3
      const int c = 10 + 3 * v, o = B + 4 * v;
      w[o + 3] = -w[f + c];
      w[o + 2] = w[e + c] - w[f + c + 1];
      w[o + 1] = w[e + c + 1] - w[f + c + 2];
      w[o + 0] = w[e + c + 2];
    }
    w[B + 12] = -w[f + 16];  // the constant part (columns 16..19): degree 4
    w[B + 11] = w[e + 16] - w[f + 17];
    w[B + 10] = w[e + 17] - w[f + 18];
    w[B + 9] = w[e + 18] - w[f + 19];
    w[B + 8] = w[e + 19];
  }
  // det B by its first row; P = coefficients, T = an 8-coefficient temporary
  const int P = kOffA, T = kOffA + 11;
  const int k = kOffQ, l = kOffQ + 13, m = kOffQ + 26;
  for (int i = 0; i < 19; ++i) w[P + i] = 0.0;
  poly_mac(w, T, l + 4, 4, m + 8, 5, 1.0);   // ly m1 - l1 my
  poly_mac(w, T, l + 8, 5, m + 4, 4, -1.0);
  poly_mac(w, P, k, 4, T, 8, 1.0);
  for (int i = 0; i < 8; ++i) w[T + i] = 0.0;
  poly_mac(w, T, l, 4, m + 8, 5, 1.0);       // lx m1 - l1 mx
  poly_mac(w, T, l + 8, 5, m, 4, -1.0);
  poly_mac(w, P, k + 4, 4, T, 8, -1.0);
  for (int i = 0; i < 8; ++i) w[T + i] = 0.0;
  poly_mac(w, T, l, 4, m + 4, 4, 1.0);       // lx my - ly mx
  poly_mac(w, T, l + 4, 4, m, 4, -1.0);
  poly_mac(w, P, k + 8, 5, T, 7, 1.0);

  const double lead = fabs(w[P + 10]);
  double big = 0.0;
  for (int i = 0; i < 10; ++i) big = fmax(big, fabs(w[P + i]));
  if (!(lead > 0.0) || !(big <= 1e25 * lead)) return 0;
  const double R = 1.0 + big / lead;  // Cauchy: every root (of every derivative too: Gauss-Lucas) has |z| < R
  for (int j = 0; j <= 10; ++j) w[kOffD + j] = w[P + j];
  for (int d = 1; d <= 10; ++d)
    for (int j = 0; j <= 10 - d; ++j) w[kOffD + 11 * d + j] = w[kOffD + 11 * (d - 1) + j + 1] * (double)(j + 1);

  int nprev = 0;
  for (int d = 9; d >= 0; --d) {
    const int prev = (d & 1) ? kOffR1 : kOffR0, cur = (d & 1) ? kOffR0 : kOffR1;
    int n = 0;
    double a = -R, fa = deriv_at(w, d, a);
    for (int t = 0; t <= nprev; ++t) {
      const double b = (t == nprev) ? R : w[prev + t];
      const double fb = deriv_at(w, d, b);
      if ((fa < 0.0 && fb > 0.0) || (fa > 0.0 && fb < 0.0)) {
        double lo = fa < 0.0 ? a : b, hi = fa < 0.0 ? b : a;  // f(lo) < 0 < f(hi)
        double x = 0.5 * (a + b);
        for (int it = 0; it < 200; ++it) {
          const double f = deriv_at(w, d, x);
          if (f == 0.0) break;
          if (f < 0.0) lo = x; else hi = x;
          const double df = deriv_at(w, d + 1, x);
          double xn = x - f / df;
          const double mn = fmin(lo, hi), mx = fmax(lo, hi);
          if (!(xn > mn && xn < mx)) xn = 0.5 * (lo + hi);
          const double step = fabs(xn - x);
          x = xn;
          if (step <= 4.0 * DBL_EPSILON * fabs(x)) break;
        }
        w[cur + n] = x;
        ++n;
      }
      a = b;
      fa = fb;
    }
    nprev = n;
  }
  return nprev;
}

// The ten constraints at E: c[0..8] = 2 E E^T E - tr(E E^T) E, c[9] = det E.
RS_HD void residual(const double* E, double* c) {
  double T[9];  // E E^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) T[3 * i + k] = E[3 * i] * E[3 * k] + E[3 * i + 1] * E[3 * k + 1] + E[3 * i + 2] * E[3 * k + 2];
  const double tr = T[0] + T[4] + T[8];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      c[3 * i + j] = 2.0 * (T[3 * i] * E[j] + T[3 * i + 1] * E[3 + j] + T[3 * i + 2] * E[6 + j]) - tr * E[3 * i + j];
  c[9] = E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]);
}

// The derivative of residual() at E in the direction D.
RS_HD void residual_dir(const double* E, const double* D, double* c) {
  double T[9], S[9];  // E E^T, D E^T + E D^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      T[3 * i + k] = E[3 * i] * E[3 * k] + E[3 * i + 1] * E[3 * k + 1] + E[3 * i + 2] * E[3 * k + 2];
      S[3 * i + k] = D[3 * i] * E[3 * k] + D[3 * i + 1] * E[3 * k + 1] + D[3 * i + 2] * E[3 * k + 2] + E[3 * i] * D[3 * k] +
                     E[3 * i + 1] * D[3 * k + 1] + E[3 * i + 2] * D[3 * k + 2];
    }
  const double tr = T[0] + T[4] + T[8], dtr = S[0] + S[4] + S[8];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      c[3 * i + j] = 2.0 * (S[3 * i] * E[j] + S[3 * i + 1] * E[3 + j] + S[3 * i + 2] * E[6 + j] + T[3 * i] * D[j] +
                            T[3 * i + 1] * D[3 + j] + T[3 * i + 2] * D[6 + j]) -
                     dtr * E[3 * i + j] - tr * D[3 * i + j];
  c[9] = D[0] * (E[4] * E[8] - E[5] * E[7]) - D[1] * (E[3] * E[8] - E[5] * E[6]) + D[2] * (E[3] * E[7] - E[4] * E[6]) +
         D[3] * (E[2] * E[7] - E[1] * E[8]) + D[4] * (E[0] * E[8] - E[2] * E[6]) + D[5] * (E[1] * E[6] - E[0] * E[7]) +
         D[6] * (E[1] * E[5] - E[2] * E[4]) + D[7] * (E[2] * E[3] - E[0] * E[5]) + D[8] * (E[0] * E[4] - E[1] * E[3]);
}

constexpr int kPolish = 4;            // Gauss-Newton steps per root
constexpr double kMaxResidual = 1e-9; // a polished root is a solution when every constraint of the unit-norm E is below this

// The five-point solver on one sample in normalised coordinates.  Writes the solutions, in ascending z, to w[kOffE + 9 r + j]:
// each of unit Frobenius norm with its entry of largest magnitude (the first such) positive.  Returns their number (0..10).
template <class W>
RS_HD int five_point(W& w, const double* x1, const double* y1, const double* x2, const double* y2) {
  null_space5(w, x1, y1, x2, y2);
  constraints(w);
  if (!eliminate(w)) return 0;
  const int nz = roots_of_det(w);
  int n = 0;
  for (int r = 0; r < nz; ++r) {
    const double z = w[kOffR1 + r];
    // (x, y, 1) spans the null space of B(z): the largest of the three cross products of its rows
    double Bz[9];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const int B = kOffQ + 13 * m;
      Bz[3 * m] = ((w[B + 3] * z + w[B + 2]) * z + w[B + 1]) * z + w[B];
      Bz[3 * m + 1] = ((w[B + 7] * z + w[B + 6]) * z + w[B + 5]) * z + w[B + 4];
      Bz[3 * m + 2] = (((w[B + 12] * z + w[B + 11]) * z + w[B + 10]) * z + w[B + 9]) * z + w[B + 8];
    }
    double v[3] = {0.0, 0.0, 0.0}, vbest = -1.0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const double* p = Bz + 3 * m;
      const double* q = Bz + 3 * ((m + 1) % 3);
      const double c0 = p[1] * q[2] - p[2] * q[1], c1 = p[2] * q[0] - p[0] * q[2], c2 = p[0] * q[1] - p[1] * q[0];
      const double nn = c0 * c0 + c1 * c1 + c2 * c2;
      if (nn > vbest) { vbest = nn; v[0] = c0; v[1] = c1; v[2] = c2; }
    }
    if (!(fabs(v[2]) > 0.0)) continue;
    double s[3] = {v[0] / v[2], v[1] / v[2], z};
    double E[9];
    for (int it = 0; it <= kPolish; ++it) {
#pragma unroll
      for (int j = 0; j < 9; ++j) E[j] = s[0] * w[kOffN + j] + s[1] * w[kOffN + 9 + j] + s[2] * w[kOffN + 18 + j] + w[kOffN + 27 + j];
      if (it == kPolish) break;
      double c[10], J[30], D[9];
      residual(E, c);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int j = 0; j < 9; ++j) D[j] = w[kOffN + 9 * a + j];
        residual_dir(E, D, J + 10 * a);
      }
      double H[9], g[3];  // J^T J, J^T c
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        g[a] = 0.0;
#pragma unroll
        for (int i = 0; i < 10; ++i) g[a] += J[10 * a + i] * c[i];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          double h = 0.0;
#pragma unroll
          for (int i = 0; i < 10; ++i) h += J[10 * a + i] * J[10 * b + i];
          H[3 * a + b] = h;
        }
      }
      const double det = rs::det3(H, H + 3, H + 6);  // symmetric: rows are columns
      if (!(fabs(det) > 0.0)) break;
      s[0] -= rs::det3(g, H + 3, H + 6) / det;
      s[1] -= rs::det3(H, g, H + 6) / det;
      s[2] -= rs::det3(H, H + 3, g) / det;
    }
    double nn = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) nn += E[j] * E[j];
    if (!(nn > 0.0) || !(nn < DBL_MAX)) continue;
    double sc = 1.0 / sqrt(nn), big = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j)
      if (fabs(E[j]) > big) { big = fabs(E[j]); sc = E[j] < 0.0 ? -fabs(sc) : fabs(sc); }
#pragma unroll
    for (int j = 0; j < 9; ++j) E[j] *= sc;
    double c[10], worst = 0.0;
    residual(E, c);
#pragma unroll
    for (int i = 0; i < 10; ++i) worst = fmax(worst, fabs(c[i]));
    if (!(worst <= kMaxResidual)) continue;  // not a solution (the polish did not converge)
#pragma unroll
    for (int j = 0; j < 9; ++j) w[kOffE + 9 * n + j] = E[j];
    ++n;
  }
  return n;
}

// OpenCV's EMEstimatorCallback::computeError decision (the Sampson error) without the division:
// (q2^T E q1)^2 <= t2 ((E q1)_0^2 + (E q1)_1^2 + (E^T q2)_0^2 + (E^T q2)_1^2).
RS_HD bool is_inlier(const double* E, double x1, double y1, double x2, double y2, double t2) {
  const double a = E[0] * x1 + E[1] * y1 + E[2], b = E[3] * x1 + E[4] * y1 + E[5], c = E[6] * x1 + E[7] * y1 + E[8];
  const double r = x2 * a + y2 * b + c;
  const double a2 = E[0] * x2 + E[3] * y2 + E[6], b2 = E[1] * x2 + E[4] * y2 + E[7];
  return r * r <= t2 * (a * a + b * b + a2 * a2 + b2 * b2);
}

// A view of a workspace whose element i is at p[i * S]: S lanes side by side in LDS, each with every S-th double (S = 1: a
// plain array).
template <int S>
struct LaneWork {
  double* p;
  RS_HD double& operator[](int i) const { return p[i * S]; }
};

// Iteration k of a pair, whole: its sample drawn, gathered into normalised coordinates and solved; the solutions are left in
// w[kOffE ..].  Every launch that needs iteration k's models (ransac5.hip, lmeds.hip: count / median and select) goes through
// here, which is what makes the winner come out again bit for bit.  P as in rs::draw_sample.  Returns the number of solutions.
template <class W, class P>
RS_HD int solve_iteration(W& w, const P& pts, const Cam& cam, uint64_t seed, int k, int N) {
  int idx[kSample];
  draw_sample(seed, k, N, idx);
  double x1[kSample], y1[kSample], x2[kSample], y2[kSample];
#pragma unroll
  for (int i = 0; i < kSample; ++i) {
    const auto m = pts(idx[i]);
    x1[i] = norm_x(cam, m.x); y1[i] = norm_y(cam, m.y); x2[i] = norm_x(cam, m.z); y2[i] = norm_y(cam, m.w);
  }
  return five_point(w, x1, y1, x2, y2);
}

// The iteration bound and the sequential selection rule are ransac_math.h's, with 5 points and 10 slots; this table never holds
// rs::kNoSample (five distinct indices always exist), so that rule's stop is never taken here.
RS_HD int update_num_iters(double p, double ep, int niters) { return rs::update_num_iters<kSample>(p, ep, niters); }
RS_HD int select_best(const int* counts, int N, double confidence, int max_iters, int* best_k, int* best_r, int* iters) {
  return rs::select_best<kMaxRoots, kSample>(counts, N, confidence, max_iters, best_k, best_r, iters);
}

}  // namespace r5
