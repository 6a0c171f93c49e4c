// eight_point_adjoint_math.h -- per-problem arithmetic of the adjoint of the textbook normalised eight-point solvers
// (csrc/eight_point_adjoint.hip), written once for the device and for the host (tests/emu/emu_eight_point_adjoint.cpp compiles it
// with g++).  What it differentiates, in fp64 from the fp32 inputs:
//   _F_from_XY                     deepFEPE/dsac_tools/utils_F.py:223-275
//   _E_from_XY, _E_from_XY_batch   deepFEPE/dsac_tools/utils_F.py:104-155, 157-221
// i.e. dfepe_w8pt_fwd with DFEPE_W8PT_SQRT2 | NO_ROWNORM (+ FORCE_110, NO_HARTLEY).  The contract is in include/dfepe.h.  No HIP
// types in here; floating-point contraction is off for the translation unit that includes this header, as in epi_adjoint_math.h.
// tests/eight_point_adjoint_ref.py restates the same arithmetic in numpy.
//
// A problem is one pair under one weight set.  Forward, recomputed:
//   per image (unless NO_HARTLEY)   c = mean p, s = sqrt(2) / mean |p - c|, p~ = s (p - c) / (1 + 1e-10)   (_de_homo's guard),
//                                   T = [[s,0,-s cx],[0,s,-s cy],[0,0,1]]; the means are unweighted
//   rows   a_i = [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] of the normalised points, A_i = w_i a_i (w = 1 without weights)
//   M9 = A^T A = sum_k lam_k q_k q_k^T, f = q_9 of the smallest lam, |f| = 1;  F0 = reshape(f, 3, 3) = U diag(s1, s2, s3) V^T
//   M = U diag(s1, s2, 0) V^T, or U diag(1, 1, 0) V^T with FORCE_110;  out = T2^T M T1
// The sign of f is chosen so that <out, F_out> >= 0 for the F_out the caller passes.
// Adjoint.  T1 and T2 are CONSTANTS: the reference builds them with torch.tensor([[S1, 0, ...]]) (utils_F.py:25,35; :52,65 in the
// batch form), which detaches them, so its own autograd never differentiates the centroid or the scale.
//   G = T2 g_F T1^T, G^ = U^T G V, g_F0 = U P V^T with
//     rank-2 step (SURVEY.md A.3, M = F0 - s3 u3 v3^T), d_k = s_k^2 - s3^2, k = 1, 2:
//       P = G^, except P_33 = 0,  P_k3 = G^_k3 + s3 (s3 G^_k3 + s_k G^_3k) / d_k,  P_3k = G^_3k + s3 (s_k G^_k3 + s3 G^_3k) / d_k
//     FORCE_110 (the output does not depend on how the 1-2 plane is split, so no term divides by s1 - s2):
//       P = 0, except P_12 = -P_21 = (G^_12 - G^_21) / (s1 + s2),
//       P_k3 = (s_k G^_k3 + s3 G^_3k) / d_k,  P_3k = (s3 G^_k3 + s_k G^_3k) / d_k
//   g_f = vec(g_F0);  u = sum_{k != 9} q_k (q_k^T g_f) / (lam_9 - lam_k)
//   per row: r = A_i . f (the constant 0 when N = 8, see point_adjoint), t = A_i . u, g_A = r u + t f, g_w = a_i . g_A,
//   g_a = w_i g_A, then to the normalised points by the product rule on a_i, and g_X = s1 / (1 + 1e-10) g_p~1, g_Y likewise with s2
//   (NO_HARTLEY: g_p = g_p~).
// Guard rule, one for every denominator above (lam_9 - lam_k, s_k^2 - s3^2, s1 + s2) and for the s1, s2 that svd3 normalises the
// left singular vectors by (a rank-1 F0 gives u2 = 0, not a NaN): guard_den(), which keeps the sign and floors the
// magnitude at 1e-30, as guard_den16 of w8pt16_bwd_body.h does: a repeated eigen- or singular value gives a large but finite
// gradient, never a NaN of its own making.
//
// Sums over the correspondences are taken as the wavefront takes them: lane l adds n = l, l + 64, ... in order, the 64 partial sums
// go through the balanced tree of ds::tree_sum64 (wave_sum on the device).
#pragma once
#include <math.h>

#pragma STDC FP_CONTRACT OFF

#if defined(__HIPCC__)
#define E8_HD __host__ __device__ inline
#else
#define E8_HD inline
#endif

namespace e8 {

constexpr int kLanes = 64;
constexpr int kProblemsPerBlock = 4;  // one wavefront each
constexpr int kSweeps9 = 16, kSweeps3 = 12;  // caps of the two Jacobi iterations; both stop as soon as a sweep rotates nothing
constexpr double kDeHomo = 1.0 + 1e-10;

// Doubles of per-problem scratch that dense_step() works in: the 9x9 matrix, its eigenvectors, the eigenvalues' slot is the
// diagonal.  On the device this lives in LDS and one lane runs the step.
constexpr int kDenseDoubles = 81 + 81;

E8_HD double guard_den(double d) {
  const double lim = 1e-30;
  return (fabs(d) < lim) ? ((d < 0.0) ? -lim : lim) : d;
}

struct Norm {  // one image's Hartley transform; NO_HARTLEY: c = 0, s = 1 and no 1e-10 guard
  double cx, cy, s;
};

E8_HD void normalized(const Norm& t, bool hartley, double x, double y, double* o) {
  if (!hartley) {
    o[0] = x; o[1] = y;
    return;
  }
  o[0] = (t.s * (x - t.cx)) / kDeHomo;
  o[1] = (t.s * (y - t.cy)) / kDeHomo;
}

E8_HD void row(const double* p1, const double* p2, double* a) {
  a[0] = p2[0] * p1[0]; a[1] = p2[0] * p1[1]; a[2] = p2[0];
  a[3] = p2[1] * p1[0]; a[4] = p2[1] * p1[1]; a[5] = p2[1];
  a[6] = p1[0]; a[7] = p1[1]; a[8] = 1.0;
}

// m[45] += upper triangle of (w a)(w a)^T, row by row: (0,0), (0,1), ..., (0,8), (1,1), ...
E8_HD void accumulate(const double* a, double w, double* m) {
  double A[9];
  for (int k = 0; k < 9; ++k) A[k] = w * a[k];
  int idx = 0;
  for (int i = 0; i < 9; ++i)
    for (int j = i; j < 9; ++j) m[idx++] += A[i] * A[j];
}

// The rotation that annihilates the off-diagonal g of [[a, g], [g, b]]: (c, s) with t = s / c the smaller root.
E8_HD void schur(double a, double b, double g, double* c, double* s) {
  const double theta = (b - a) / (2.0 * g);
  const double t = ((theta >= 0.0) ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  *c = 1.0 / sqrt(t * t + 1.0);
  *s = t * *c;
}

// Cyclic Jacobi on the symmetric 9x9 A (row-major, full; destroyed: its diagonal ends as the eigenvalues); V[c * 9 + k] = component c
// of eigenvector k.  A rotation is skipped where |a_pq| <= 2^-60 sqrt|a_pp a_qq| (a NaN skips too, so the loop ends on any input).
E8_HD void jacobi9(double* A, double* V) {
  for (int i = 0; i < 81; ++i) V[i] = 0.0;
  for (int i = 0; i < 9; ++i) V[10 * i] = 1.0;
  for (int sweep = 0; sweep < kSweeps9; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 8; ++p) {
      for (int q = p + 1; q < 9; ++q) {
        const double app = A[10 * p], aqq = A[10 * q], apq = A[9 * p + q];
        if (!(fabs(apq) > 8.673617379884035e-19 * sqrt(fabs(app * aqq)))) continue;
        rotated = true;
        double c, s;
        schur(app, aqq, apq, &c, &s);
        for (int k = 0; k < 9; ++k) {  // columns p, q
          const double akp = A[9 * k + p], akq = A[9 * k + q];
          A[9 * k + p] = c * akp - s * akq;
          A[9 * k + q] = s * akp + c * akq;
        }
        for (int k = 0; k < 9; ++k) {  // rows p, q
          const double apk = A[9 * p + k], aqk = A[9 * q + k];
          A[9 * p + k] = c * apk - s * aqk;
          A[9 * q + k] = s * apk + c * aqk;
        }
        A[9 * p + q] = 0.0;
        A[9 * q + p] = 0.0;
        for (int k = 0; k < 9; ++k) {
          const double vkp = V[9 * k + p], vkq = V[9 * k + q];
          V[9 * k + p] = c * vkp - s * vkq;
          V[9 * k + q] = s * vkp + c * vkq;
        }
      }
    }
    if (!rotated) break;
  }
}

// One-sided Jacobi SVD of the 3x3 F (row-major): F = U diag(s) V^T, s descending and >= 0, U and V row-major with the vectors in
// their columns.  u3 = +-(u1 x u2), oriented along F v3, so a vanishing s3 costs u3 nothing.
E8_HD void svd3(const double* F, double* U, double* s, double* V) {
  double W[9];
  for (int i = 0; i < 9; ++i) { W[i] = F[i]; V[i] = 0.0; }
  V[0] = V[4] = V[8] = 1.0;
  for (int sweep = 0; sweep < kSweeps3; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p) {
      for (int q = p + 1; q < 3; ++q) {
        const double al = (W[p] * W[p] + W[3 + p] * W[3 + p]) + W[6 + p] * W[6 + p];
        const double be = (W[q] * W[q] + W[3 + q] * W[3 + q]) + W[6 + q] * W[6 + q];
        const double ga = (W[p] * W[q] + W[3 + p] * W[3 + q]) + W[6 + p] * W[6 + q];
        if (!(fabs(ga) > 8.673617379884035e-19 * sqrt(al * be))) continue;
        rotated = true;
        double c, sn;
        schur(al, be, ga, &c, &sn);
        for (int k = 0; k < 3; ++k) {
          const double wp = W[3 * k + p], wq = W[3 * k + q];
          W[3 * k + p] = c * wp - sn * wq;
          W[3 * k + q] = sn * wp + c * wq;
          const double vp = V[3 * k + p], vq = V[3 * k + q];
          V[3 * k + p] = c * vp - sn * vq;
          V[3 * k + q] = sn * vp + c * vq;
        }
      }
    }
    if (!rotated) break;
  }
  double n[3];
  for (int j = 0; j < 3; ++j) n[j] = sqrt((W[j] * W[j] + W[3 + j] * W[3 + j]) + W[6 + j] * W[6 + j]);
  int o[3] = {0, 1, 2};  // descending
  if (n[o[0]] < n[o[1]]) { const int t = o[0]; o[0] = o[1]; o[1] = t; }
  if (n[o[1]] < n[o[2]]) { const int t = o[1]; o[1] = o[2]; o[2] = t; }
  if (n[o[0]] < n[o[1]]) { const int t = o[0]; o[0] = o[1]; o[1] = t; }
  double Vs[9];
  for (int j = 0; j < 3; ++j) {
    s[j] = n[o[j]];
    for (int k = 0; k < 3; ++k) Vs[3 * k + j] = V[3 * k + o[j]];
  }
  for (int i = 0; i < 9; ++i) V[i] = Vs[i];
  for (int j = 0; j < 2; ++j)
    for (int k = 0; k < 3; ++k) U[3 * k + j] = W[3 * k + o[j]] / guard_den(s[j]);  // a rank-1 F0 (s2 = 0): u2 = 0, no NaN
  double u3[3] = {U[3] * U[7] - U[6] * U[4], U[6] * U[1] - U[0] * U[7], U[0] * U[4] - U[3] * U[1]};
  const double d = (u3[0] * W[o[2]] + u3[1] * W[3 + o[2]]) + u3[2] * W[6 + o[2]];
  const double sg = (d < 0.0) ? -1.0 : 1.0;
  for (int k = 0; k < 3; ++k) U[3 * k + 2] = sg * u3[k];
}

// C = A B, A^T B or A B^T for row-major 3x3.
E8_HD void mul3(const double* A, bool tA, const double* B, bool tB, double* C) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc += (tA ? A[3 * k + r] : A[3 * r + k]) * (tB ? B[3 * c + k] : B[3 * k + c]);
      C[3 * r + c] = acc;
    }
}

E8_HD void hartley_matrix(const Norm& t, bool hartley, double* T) {
  for (int i = 0; i < 9; ++i) T[i] = 0.0;
  T[0] = T[4] = T[8] = 1.0;
  if (hartley) {
    T[0] = T[4] = t.s;
    T[2] = -(t.s * t.cx);
    T[5] = -(t.s * t.cy);
  }
}

// The dense step of one problem.  m45: the upper triangle of M9 (accumulate()'s order).  work: kDenseDoubles doubles.
// F_out, g_F: the caller's fp32 values widened.  Writes f[9] (oriented) and u[9].
E8_HD void dense_step(const double* m45, const Norm& t1, const Norm& t2, bool hartley, bool force110, const double* F_out,
                      const double* g_F, double* work, double* f, double* u) {
  double* A = work;
  double* Q = work + 81;
  int idx = 0;
  for (int i = 0; i < 9; ++i)
    for (int j = i; j < 9; ++j) {
      A[9 * i + j] = m45[idx];
      A[9 * j + i] = m45[idx];
      ++idx;
    }
  jacobi9(A, Q);
  int k9 = 0;
  for (int k = 1; k < 9; ++k)
    if (A[10 * k] < A[10 * k9]) k9 = k;
  const double lam9 = A[10 * k9];
  double F0[9];
  for (int c = 0; c < 9; ++c) F0[c] = Q[9 * c + k9];
  double U[9], s[3], V[9];
  svd3(F0, U, s, V);
  double T1[9], T2[9];
  hartley_matrix(t1, hartley, T1);
  hartley_matrix(t2, hartley, T2);
  // out = T2^T M T1 and its orientation against F_out
  const double d1 = force110 ? 1.0 : s[0], d2 = force110 ? 1.0 : s[1];
  double M[9], tmp[9], out[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[3 * r + c] = d1 * (U[3 * r] * V[3 * c]) + d2 * (U[3 * r + 1] * V[3 * c + 1]);
  mul3(T2, true, M, false, tmp);
  mul3(tmp, false, T1, false, out);
  double dot = 0.0;
  for (int c = 0; c < 9; ++c) dot += out[c] * F_out[c];
  const double sg = (dot < 0.0) ? -1.0 : 1.0;
  for (int c = 0; c < 9; ++c) {
    f[c] = sg * F0[c];
    U[c] = sg * U[c];  // -F0 = (-U) diag(s) V^T
  }
  // G^ = U^T (T2 g_F T1^T) V
  double G[9], Gh[9], P[9];
  mul3(T2, false, g_F, false, tmp);
  mul3(tmp, false, T1, true, G);
  mul3(U, true, G, false, tmp);
  mul3(tmp, false, V, false, Gh);
  for (int c = 0; c < 9; ++c) P[c] = force110 ? 0.0 : Gh[c];
  P[8] = 0.0;
  if (force110) {
    P[1] = (Gh[1] - Gh[3]) / guard_den(s[0] + s[1]);
    P[3] = -P[1];
  }
  for (int k = 0; k < 2; ++k) {
    const double dk = guard_den(s[k] * s[k] - s[2] * s[2]);
    const double gk3 = Gh[3 * k + 2], g3k = Gh[6 + k];
    if (force110) {
      P[3 * k + 2] = (s[k] * gk3 + s[2] * g3k) / dk;
      P[6 + k] = (s[2] * gk3 + s[k] * g3k) / dk;
    } else {
      P[3 * k + 2] = gk3 + (s[2] * (s[2] * gk3 + s[k] * g3k)) / dk;
      P[6 + k] = g3k + (s[2] * (s[k] * gk3 + s[2] * g3k)) / dk;
    }
  }
  double gf[9];
  mul3(U, false, P, false, tmp);
  mul3(tmp, false, V, true, gf);
  for (int c = 0; c < 9; ++c) u[c] = 0.0;
  for (int k = 0; k < 9; ++k) {
    if (k == k9) continue;
    double proj = 0.0;
    for (int c = 0; c < 9; ++c) proj += Q[9 * c + k] * gf[c];
    const double coef = proj / guard_den(lam9 - A[10 * k]);
    for (int c = 0; c < 9; ++c) u[c] += coef * Q[9 * c + k];
  }
}

// One correspondence: p1, p2 the normalised points, w the weight.  gp[4] = (g_x1, g_y1, g_x2, g_y2) w.r.t. the ORIGINAL points
// (scale1, scale2 = s / (1 + 1e-10), or 1 with NO_HARTLEY), *gw the weight's gradient.  exact_null (N = 8): eight rows in nine
// unknowns have an exact null vector, A f = 0 whatever the points and weights are, so r is the constant 0 and not the rounding noise
// that A_i . f evaluates to; g_w is then identically 0, as it is in exact arithmetic.
E8_HD void point_adjoint(const double* p1, const double* p2, double w, const double* f, const double* u, double scale1,
                         double scale2, bool exact_null, double* gp, double* gw) {
  double a[9];
  row(p1, p2, a);
  double af = 0.0, au = 0.0;
  for (int k = 0; k < 9; ++k) {
    af += a[k] * f[k];
    au += a[k] * u[k];
  }
  const double r = exact_null ? 0.0 : w * af, t = w * au;
  double gA[9], ga[9], acc = 0.0;
  for (int k = 0; k < 9; ++k) {
    gA[k] = r * u[k] + t * f[k];
    acc += a[k] * gA[k];
    ga[k] = w * gA[k];
  }
  *gw = exact_null ? 0.0 : acc;  // acc = 2 w (a . f)(a . u), and a . f = 0
  gp[0] = scale1 * ((ga[0] * p2[0] + ga[3] * p2[1]) + ga[6]);
  gp[1] = scale1 * ((ga[1] * p2[0] + ga[4] * p2[1]) + ga[7]);
  gp[2] = scale2 * ((ga[0] * p1[0] + ga[1] * p1[1]) + ga[2]);
  gp[3] = scale2 * ((ga[3] * p1[0] + ga[4] * p1[1]) + ga[5]);
}

}  // namespace e8
