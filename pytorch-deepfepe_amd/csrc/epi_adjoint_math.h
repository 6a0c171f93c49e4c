// epi_adjoint_math.h -- per-point arithmetic of the adjoints of the epipolar distances (csrc/epi_adjoint.hip), written once for the
// device and for the host (tests/emu/emu_epi_adjoint.cpp compiles it with g++).  What it differentiates, in fp64:
//   _sampson_dist, _sym_epi_dist, _epi_distance   deepFEPE/dsac_tools/utils_F.py:291-361
//   compute_epi_residual (w.r.t. the points)      deepFEPE/dsac_tools/utils_F.py:400-413
// The contract is in include/dfepe.h.  No HIP types in here; floating-point contraction is off for the translation unit that
// includes this header, as in corr_eval_math.h and triangulate_math.h, so a product and the sum it feeds are two roundings on the
// device as on the host.  tests/epi_adjoint_ref.py restates the same derivatives in numpy.
//
// Notation: x = (x0, x1, x2), y likewise (without the homogeneous flag the third coordinate is the constant 1 and gets no
// gradient); a = F x, b = F^T y, s = y^T F x, A = a0^2 + a1^2, Q = b0^2 + b1^2.  Every metric is e(s, A, Q), so
//   de = cs ds + cA dA + cQ dQ
//   ds/dF_rc = y_r x_c          ds/dx = b                          ds/dy = a
//   dA/dF_rc = 2 a_r x_c [r<2]  dA/dx_c = 2 (a0 F_0c + a1 F_1c)    dA/dy = 0
//   dQ/dF_rc = 2 b_c y_r [c<2]  dQ/dy_r = 2 (b0 F_r0 + b1 F_r1)    dQ/dx = 0
// and a kind only has to say what (cs, cA, cQ) are.  sign(0) = 0, as torch differentiates abs(); with a clamp the gradient passes
// where e <= clamp_at, as torch.clamp(max=) passes it at the bound.
#pragma once
#include <math.h>

#pragma STDC FP_CONTRACT OFF

#if defined(__HIPCC__)
#define EA_HD __host__ __device__ inline
#else
#define EA_HD inline
#endif

namespace ea {

constexpr int kChunk = 1024;  // consecutive points of one pair that one workgroup owns (dfepe_epi_adjoint_chunk)

struct Terms {
  double a[3], b[3], s, A, Q;
};

EA_HD double sign0(double v) { return (v > 0.0) ? 1.0 : ((v < 0.0) ? -1.0 : 0.0); }

// F row-major, fp32 values widened exactly.
EA_HD Terms terms(const double* F, const double* x, const double* y) {
  Terms t;
  for (int r = 0; r < 3; ++r) t.a[r] = (F[3 * r] * x[0] + F[3 * r + 1] * x[1]) + F[3 * r + 2] * x[2];  // F x
  for (int c = 0; c < 3; ++c) t.b[c] = (F[c] * y[0] + F[3 + c] * y[1]) + F[6 + c] * y[2];              // F^T y
  t.s = (y[0] * t.a[0] + y[1] * t.a[1]) + y[2] * t.a[2];
  t.A = t.a[0] * t.a[0] + t.a[1] * t.a[1];
  t.Q = t.b[0] * t.b[0] + t.b[1] * t.b[1];
  return t;
}

// The scalar a reduced loss adds up: kinds 0 and 1, and the first plane of kind 2.  clamp_at < 0: no clamp; a NaN stays a NaN.
EA_HD double value(int kind, const Terms& t, double clamp_at, double eps) {
  if (kind == 0) {
    double e = (t.s * t.s) * (1.0 / (t.A + eps) + 1.0 / (t.Q + eps));
    if (clamp_at >= 0.0 && e > clamp_at) e = clamp_at;
    return e;
  }
  if (kind == 1) return (t.s * t.s) / (t.A + t.Q);
  const double as = fabs(t.s);
  return 0.5 * (as / sqrt(t.A) + as / sqrt(t.Q));
}

// (cs, cA, cQ) of sum_p g[p] e_p: one plane for kinds 0 and 1 (g1 = g2 = 0), the three planes (mean, d1, d2) for kind 2.
EA_HD void coeffs(int kind, const Terms& t, double clamp_at, double eps, double g0, double g1, double g2, double* cs, double* cA,
                  double* cQ) {
  const double s = t.s;
  if (kind == 0) {
    const double iA = 1.0 / (t.A + eps), iQ = 1.0 / (t.Q + eps);
    const double R = iA + iQ;
    const bool pass = !(clamp_at >= 0.0) || ((s * s) * R <= clamp_at);
    const double g = pass ? g0 : 0.0;
    *cs = g * ((2.0 * s) * R);
    *cA = -(g * ((s * s) * (iA * iA)));
    *cQ = -(g * ((s * s) * (iQ * iQ)));
  } else if (kind == 1) {
    const double iD = 1.0 / (t.A + t.Q);
    *cs = g0 * ((2.0 * s) * iD);
    *cA = -(g0 * ((s * s) * (iD * iD)));
    *cQ = *cA;
  } else {
    const double h1 = g1 + 0.5 * g0, h2 = g2 + 0.5 * g0;  // what reaches d1 and d2
    const double rA = sqrt(t.A), rQ = sqrt(t.Q), as = fabs(s), sg = sign0(s);
    *cs = sg * (h1 / rA + h2 / rQ);
    *cA = -(h1 * (as / ((2.0 * t.A) * rA)));
    *cQ = -(h2 * (as / ((2.0 * t.Q) * rQ)));
  }
}

// One point's contribution: gF[9] (row-major, to be summed over the pair's points), gx[3], gy[3] (the third entries are computed
// always and dropped by the caller for 2-D points).
EA_HD void point_adjoint(const double* F, const double* x, const double* y, const Terms& t, double cs, double cA, double cQ,
                         double* gF, double* gx, double* gy) {
  const double cA2 = 2.0 * cA, cQ2 = 2.0 * cQ;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      double v = cs * (y[r] * x[c]);
      if (r < 2) v = v + cA2 * (t.a[r] * x[c]);
      if (c < 2) v = v + cQ2 * (t.b[c] * y[r]);
      gF[3 * r + c] = v;
    }
  }
  for (int c = 0; c < 3; ++c) gx[c] = cs * t.b[c] + cA2 * (t.a[0] * F[c] + t.a[1] * F[3 + c]);
  for (int r = 0; r < 3; ++r) gy[r] = cs * t.a[r] + cQ2 * (t.b[0] * F[3 * r] + t.b[1] * F[3 * r + 1]);
}

// compute_epi_residual w.r.t. its points (the adjoint w.r.t. F is dfepe_epi_residual_bwd).  In the notation of
// tests/epipolar_ref.py: l1 = F^T x2, l2 = F x1, dd = x2^T F x1, n = |l[:2]|, i = 1 / (n + 1e-6), S = i1 + i2, d = |dd| S,
//   dd/dx1 = sign(dd) S l1 - k2 F[:2,:]^T l2[:2]     k2 = |dd| i2^2 / n2   (0 where n2 = 0)
//   dd/dx2 = sign(dd) S l2 - k1 F[:,:2] l1[:2]       k1 = |dd| i1^2 / n1   (0 where n1 = 0)
// times g where d <= clamp_at, 0 elsewhere.
EA_HD void residual_point_adjoint(const double* F, const double* x1, const double* x2, double clamp_at, double g, double* g1,
                                  double* g2) {
  const Terms t = terms(F, x1, x2);  // a = l2, b = l1, s = dd
  const double n1 = sqrt(t.Q), n2 = sqrt(t.A);
  const double i1 = 1.0 / (n1 + 1e-6), i2 = 1.0 / (n2 + 1e-6);
  const double S = i1 + i2, ad = fabs(t.s);
  const double gg = (ad * S <= clamp_at) ? g : 0.0;
  const double sgS = gg * (sign0(t.s) * S);
  const double k1 = (n1 > 0.0) ? gg * ((ad * (i1 * i1)) / n1) : 0.0;
  const double k2 = (n2 > 0.0) ? gg * ((ad * (i2 * i2)) / n2) : 0.0;
  for (int c = 0; c < 3; ++c) g1[c] = sgS * t.b[c] - k2 * (t.a[0] * F[c] + t.a[1] * F[3 + c]);
  for (int r = 0; r < 3; ++r) g2[r] = sgS * t.a[r] - k1 * (t.b[0] * F[3 * r] + t.b[1] * F[3 * r + 1]);
}

}  // namespace ea
