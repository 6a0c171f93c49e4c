// corr_eval_math.h -- per-lane arithmetic of the correspondence evaluation (csrc/corr_eval.hip), written once for the device and
// for the host (tests/emu/emu_corr_eval.cpp compiles it with g++).  What it restates, in fp64:
//   epi_distance_np            deepFEPE/dsac_tools/utils_F.py:363-385   dist3 = |y^T F x| (1/|(F x)_12| + 1/|(F^T y)_12|)
//   Result_processor.get_mask  deepFEPE/utils/eval_tools.py:145-147     score < mask_thd
//   inlier_ratio_from_est      eval_tools.py:164-174                    sum(dist < thd) / kept
//   inlier_ratio               eval_tools.py:70-104                     the per-pair table, its mean over the pairs, num_corrs
// The contract is in include/dfepe.h.
//
// The order of operations is the reference's: the two reciprocals are taken first, added, and the sum multiplies the numerator
// (dist3 = nominator * (recp1 + recp2)), so a point with F x = 0 gives 0 * inf = NaN where numpy gives it, and a numerator
// that is not 0 gives +inf.  Every association is spelled out and floating-point contraction is off for the translation unit
// that includes this header, as in odometry_math.h: a product and the sum it feeds are two roundings on the device as on the
// host, and tests/corr_eval_ref.py restates the same operations in numpy term for term.  numpy's own matrix products go through
// a BLAS whose summation order and fused operations are not specified; the difference is inside the bound corr_eval_ref.py
// derives, and the decided-set rule of the tests is stated against that bound.
#pragma once
#include <math.h>

#pragma STDC FP_CONTRACT OFF

#if defined(__HIPCC__)
#define CE_HD __host__ __device__ inline
#else
#define CE_HD inline
#endif

namespace ce {

constexpr int kMaxThds = 16;  // inlier thresholds per call, and mask thresholds per call

// (x1, y1, x2, y2) fp32 widened to fp64 (exact); F row-major.  The homogeneous coordinate is 1, so its products are exact.
CE_HD double epi_dist3(const double* F, double x1, double y1, double x2, double y2) {
  // Y @ F: the row vector y^T F
  const double a0 = (x2 * F[0] + y2 * F[3]) + F[6];
  const double a1 = (x2 * F[1] + y2 * F[4]) + F[7];
  const double a2 = (x2 * F[2] + y2 * F[5]) + F[8];
  const double nominator = fabs((a0 * x1 + a1 * y1) + a2);
  // F @ X^T, rows 0 and 1
  const double p0 = (F[0] * x1 + F[1] * y1) + F[2];
  const double p1 = (F[3] * x1 + F[4] * y1) + F[5];
  // F^T @ Y^T, rows 0 and 1
  const double q0 = (F[0] * x2 + F[3] * y2) + F[6];
  const double q1 = (F[1] * x2 + F[4] * y2) + F[7];
  const double recp_y_to_fx = 1.0 / sqrt(p0 * p0 + p1 * p1);
  const double recp_x_to_fy = 1.0 / sqrt(q0 * q0 + q1 * q1);
  return nominator * (recp_y_to_fx + recp_x_to_fy);
}

// get_mask: strict, and a NaN score is not kept.
CE_HD bool kept(double score, double mask_thd) { return score < mask_thd; }

// est_arr < thd: strict, and a NaN distance is no inlier (it stays in the denominator).
CE_HD bool inlier(double dist, double inlier_thd) { return dist < inlier_thd; }

// np.sum(est_arr < thd) / est_arr.shape[0]: 0 / 0 is NaN, as numpy's float64 division gives.
CE_HD double ratio_of(int cnt, int num) { return (double)cnt / (double)num; }

// table.mean(axis=0): numpy adds the B rows in index order (a pairwise sum only splits above 8 terms per lane of the reduction,
// and a reduction over the first axis of a C-ordered [B, Ti] array is done row by row), then divides by B.  NaN propagates.
CE_HD double mean_of(const double* col, int stride, int B) {
  double s = 0.0;
  for (int b = 0; b < B; ++b) s = s + col[(long)b * stride];
  return s / (double)B;
}

}  // namespace ce
