// detector_eval_math.h -- per-lane arithmetic of the front-end detector evaluation (csrc/detector_eval.hip), written once for the
// device and for the host (tests/emu/emu_detector_eval.cpp compiles it with g++).  What it restates: compute_repeatability
// (evaluations/detector_evaluation.py:150-279), the matching score (deepFEPE/evaluate_frontend.py:176-183) and the nn mean AP
// (evaluate_frontend.py:185-275, scikit-learn's average_precision_score); the contract is in include/dfepe.h.  All of it is fp64.
//
// The inverse warp.  The reference warps image-2 points by numpy.linalg.inv(H).  A projective map is defined up to scale, and
// inv(H) = adj(H) / det(H), so the warp by the adjugate gives the same point (the factor leaves with the division by w) without
// a division by the determinant; a singular H has an adjugate too, and what its warp gives goes through the inside tests like
// every other value.  A point whose homogeneous w is 0 gives what the division gives (an infinity or a NaN); every inside test is
// written as comparisons that such a value fails.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DE_HD __host__ __device__ inline
#else
#define DE_HD inline
#endif

namespace de {

constexpr int kMaxN = 4096;  // points per image and pair, entries per pair of the average precision

// adj(H): the transposed cofactors, each a difference of two products.
DE_HD void adjugate(const double* H, double* A) {
  A[0] = H[4] * H[8] - H[5] * H[7];
  A[1] = H[2] * H[7] - H[1] * H[8];
  A[2] = H[1] * H[5] - H[2] * H[4];
  A[3] = H[5] * H[6] - H[3] * H[8];
  A[4] = H[0] * H[8] - H[2] * H[6];
  A[5] = H[2] * H[3] - H[0] * H[5];
  A[6] = H[3] * H[7] - H[4] * H[6];
  A[7] = H[1] * H[6] - H[0] * H[7];
  A[8] = H[0] * H[4] - H[1] * H[3];
}

// warp_keypoints (detector_evaluation.py:136-148): (x, y, 1) H^T, then the division by the third coordinate.
DE_HD void warp(const double* H, double x, double y, double* wx, double* wy) {
  const double X = H[0] * x + H[1] * y + H[2];
  const double Y = H[3] * x + H[4] * y + H[5];
  const double W = H[6] * x + H[7] * y + H[8];
  *wx = X / W;
  *wy = Y / W;
}

// filter_keypoints / keep_true_keypoints: 0 <= x < width, 0 <= y < height.  A NaN fails.
DE_HD bool inside_half_open(double x, double y, int height, int width) {
  return x >= 0.0 && x < (double)width && y >= 0.0 && y < (double)height;
}

// warpLabels of the superpoint package as include/dfepe.h states it: 0 <= x <= width - 1, 0 <= y <= height - 1, not truncated.
DE_HD bool inside_closed(double x, double y, int height, int width) {
  return x >= 0.0 && x <= (double)(width - 1) && y >= 0.0 && y <= (double)(height - 1);
}

// The order of a stable ascending numpy argsort as an unsigned key: -inf < .. < -0 = +0 < .. < +inf < NaN (every NaN alike).
// Never 0: the kernels keep 0 for a point that the filter dropped.
DE_HD uint64_t prob_key(double p) {
  if (p != p) return ~0ull;
  if (p == 0.0) p = 0.0;  // -0 and +0 compare equal
  union { double d; uint64_t u; } v;
  v.d = p;
  return (v.u >> 63) ? ~v.u : (v.u | (1ull << 63));
}

// Whether point j stands after point i in that argsort: the k points that stand last are kept, so among equal probabilities
// the higher index.
DE_HD bool stands_after(uint64_t key_j, int j, uint64_t key_i, int i) { return key_j > key_i || (key_j == key_i && j > i); }

// select_k_best: `sorted[-min(k, n):]`; numpy reads [-0:] as the whole array, so k = 0 (and n = 0) keeps every point.
DE_HD bool selected(int rank_from_last, int keep_k, int n) {
  const int start = keep_k < n ? keep_k : n;
  return start == 0 || rank_from_last < start;
}

// Squared distance; the minimum is taken over these and the root once (sqrt is monotone and correctly rounded, so the root of
// the smallest square is the smallest root).
DE_HD double dist2(double ax, double ay, double bx, double by) {
  const double dx = ax - bx, dy = ay - by;
  return dx * dx + dy * dy;
}

// repeatability and localization error of one threshold from the two counts, the kept sizes and the two sums (lines 264-279):
// 0 and -1 when nothing is counted; the reference divides each sum by the count before adding them.
DE_HD double repeatability_of(int count1, int count2, int kept1, int kept2) {
  const int c = count1 + count2;
  return c > 0 ? (double)c / (double)(kept1 + kept2) : 0.0;
}
DE_HD double loc_err_of(int count1, int count2, double sum1, double sum2) {
  const int c = count1 + count2;
  return c > 0 ? sum1 / (double)c + sum2 / (double)c : -1.0;
}

// evaluate_frontend.py:181: (inliers.sum() * 2) / (n_keypoints1 + n_unwarped); a zero denominator gives what the division gives.
DE_HD double matching_score(int n_inliers, int n_kp1, int n_unwarped) {
  return (double)(2ll * (long long)n_inliers) / (double)((long long)n_kp1 + (long long)n_unwarped);
}

// One positive's share of the average precision: TP(s_i) / CNT(s_i) (include/dfepe.h); cnt >= 1 unless the score is a NaN.
DE_HD double ap_term(int tp, int cnt) { return (double)tp / (double)cnt; }

}  // namespace de
