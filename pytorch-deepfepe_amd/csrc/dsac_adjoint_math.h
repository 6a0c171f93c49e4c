// dsac_adjoint_math.h -- per-lane arithmetic of the adjoint of the DSAC hypothesis loop (csrc/dsac_adjoint.hip), written once for
// the device and for the host (tests/emu/emu_dsac_adjoint.cpp compiles it with g++).  Built on ea::terms / ea::coeffs /
// ea::point_adjoint (epi_adjoint_math.h: the Sampson distance is its kind 1) and on dsac_math.h (ds::inv3, ds::normalized_point,
// ds::e_to_f, ds::refit_weight).  The contract is in include/dfepe.h (dfepe_dsac_bwd).  No HIP types in here; floating-point
// contraction is off for the translation unit that includes this header (epi_adjoint_math.h says so), so a product and the sum it
// feeds are two roundings on the device as on the host.  tests/dsac_adjoint_ref.py restates the same stages in numpy.
//
// What is differentiated is dfepe_dsac's stages on the fp32 values it wrote, every fp32 rounding between stages taken as the
// identity:  score_h = sum_n s_hn,  s = 1 / (1 + exp(beta (d - thresh))),  d = sampson(K^-T E_sample K^-1; x_n, y_n),
//            w = sqrt(s),  E_refit = fit(K^-1 points, w),  loss_h = mean_n sampson(M_h; x_n, y_n),
//            quality_n = sum_{h sampled n} score_h / (counts_n + 1e-10),  exp_loss = sum_h softmax(alpha score)_h loss_h.
#pragma once
#include <math.h>

#include "dsac_math.h"

namespace da {

constexpr int kPointLanes = 64;  // correspondences of one pair that one workgroup of the points launch owns (a lane each)
constexpr int kPointWaves = 4;   // its wavefronts: wavefront v adds the hypotheses [v Hq, (v + 1) Hq), Hq = ceil(H / 4)

// Head: what reaches loss_h and score_h.  p = softmax(alpha score)_h, Lbar = sum_h p_h loss_h, both in fp64.
DS_HD double head_loss(double g_loss, double g_exp, double p) { return g_loss + g_exp * p; }
DS_HD double head_score_exp(double g_exp, double alpha, double p, double loss, double Lbar) { return (g_exp * alpha) * (p * (loss - Lbar)); }
// d quality_n / d score_h for a sampled n: the vote's own quotient.
DS_HD double head_vote(double g_quality, double count) { return g_quality / (count + 1e-10); }

// What reaches d_hn: through the score (ds/dd = -beta s (1 - s)) and through the refit's weight w = sqrt(s)
// (dw/dd = -(beta / 2) w (1 - s): the limit, finite everywhere and 0 at s = 0, where 1 / (2 sqrt(s)) is not).  No division.
DS_HD double score_coeff(double beta, double s, double w, double t_score, double t_w) {
  return -(beta * (1.0 - s)) * (s * t_score + 0.5 * (w * t_w));
}

// g0 d sampson(M; x, y) / d(M, x, y) for the pixel correspondence (x, y): gM[9] row-major, gx[2], gy[2].
DS_HD void sampson_adjoint(const double* M, double x0, double x1, double y0, double y1, double g0, double* gM, double* gx, double* gy) {
  const double x[3] = {x0, x1, 1.0}, y[3] = {y0, y1, 1.0};
  const ea::Terms t = ea::terms(M, x, y);
  double cs, cA, cQ, gx3[3], gy3[3];
  ea::coeffs(1, t, -1.0, 0.0, g0, 0.0, 0.0, &cs, &cA, &cQ);
  ea::point_adjoint(M, x, y, t, cs, cA, cQ, gM, gx3, gy3);
  gx[0] = gx3[0]; gx[1] = gx3[1];
  gy[0] = gy3[0]; gy[1] = gy3[1];
}

// F = K^-T E K^-1  =>  the gradient w.r.t. E is K^-1 G K^-T.
DS_HD void f_to_e_adjoint(const double* Ki, const double* G, double* out) {
  double T[9];  // G K^-T
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T[3 * r + c] = (G[3 * r] * Ki[3 * c] + G[3 * r + 1] * Ki[3 * c + 1]) + G[3 * r + 2] * Ki[3 * c + 2];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) out[3 * r + c] = (Ki[3 * r] * T[c] + Ki[3 * r + 1] * T[3 + c]) + Ki[3 * r + 2] * T[6 + c];
}

// The gradient gp[2] w.r.t. the K^-1 point _de_homo(K^-1 (x, y, 1)) = (u, v) / (w + 1e-10) taken back to the pixel (x, y).
DS_HD void pixel_from_normalized(const double* Ki, double x, double y, const double* gp, double* gpix) {
  const double u = (Ki[0] * x + Ki[1] * y) + Ki[2], v = (Ki[3] * x + Ki[4] * y) + Ki[5], w = (Ki[6] * x + Ki[7] * y) + Ki[8];
  const double ig = 1.0 / (w + 1e-10);
  const double gu = gp[0] * ig, gv = gp[1] * ig;
  const double gw = -((gp[0] * (u * ig) + gp[1] * (v * ig)) * ig);
  gpix[0] = (gu * Ki[0] + gv * Ki[3]) + gw * Ki[6];
  gpix[1] = (gu * Ki[1] + gv * Ki[4]) + gw * Ki[7];
}

}  // namespace da
