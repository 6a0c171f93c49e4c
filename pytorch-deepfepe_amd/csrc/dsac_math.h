// dsac_math.h -- per-lane arithmetic of the DSAC hypothesis loop (csrc/dsac.hip), written once for the device and for the host
// (tests/emu/emu_dsac.cpp compiles it with g++).  What it restates, in fp64:
//   the K^-1 points of _E_from_XY                 deepFEPE/dsac_tools/utils_F.py:111-112, utils_misc.py:69-78
//   F = K^-T E K^-1 (_E_to_F)                     deepFEPE/dsac_tools/utils_F.py:464-469
//   the soft inlier weight                        deepFEPE/dsac_tools/dsac.py:67-74
//   HLoss, the mean Sampson distance              deepFEPE/dsac_tools/H_loss.py:28-29
//   the per-correspondence vote                   deepFEPE/dsac_tools/dsac.py:163-165, 194
// The Sampson distance itself is ea::terms / ea::value(kind 1) of epi_adjoint_math.h.  The contract is in include/dfepe.h.  No HIP
// types in here; floating-point contraction is off for the translation unit that includes this header (epi_adjoint_math.h says so),
// so a product and the sum it feeds are two roundings on the device as on the host.  tests/dsac_ref.py restates the stages in numpy.
#pragma once
#include <math.h>

#include "epi_adjoint_math.h"

#if defined(__HIPCC__)
#define DS_HD __host__ __device__ inline
#else
#define DS_HD inline
#endif

namespace ds {

constexpr int kHypsPerBlock = 4;  // hypotheses of one pair that one workgroup scores: one wavefront each (dfepe_dsac_hyps_per_block)
constexpr int kVoteChunk = 256;   // consecutive correspondences of one pair that one workgroup votes on (dfepe_dsac_vote_chunk)
constexpr int kVoteTile = 16;     // hypotheses whose index lists that workgroup holds in LDS at a time (dfepe_dsac_vote_tile)
constexpr int kMinSample = 8, kMaxSample = 16;
constexpr int kLanes = 64;

// K^-1 by the adjugate; K row-major, fp32 values widened exactly.  A singular K gives inf / NaN, which stay in their own pair.
DS_HD void inv3(const double* K, double* Ki) {
  const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[5] * K[6] - K[3] * K[8], c02 = K[3] * K[7] - K[4] * K[6];
  const double det = (K[0] * c00 + K[1] * c01) + K[2] * c02;
  const double id = 1.0 / det;
  Ki[0] = c00 * id; Ki[1] = (K[2] * K[7] - K[1] * K[8]) * id; Ki[2] = (K[1] * K[5] - K[2] * K[4]) * id;
  Ki[3] = c01 * id; Ki[4] = (K[0] * K[8] - K[2] * K[6]) * id; Ki[5] = (K[2] * K[3] - K[0] * K[5]) * id;
  Ki[6] = c02 * id; Ki[7] = (K[1] * K[6] - K[0] * K[7]) * id; Ki[8] = (K[0] * K[4] - K[1] * K[3]) * id;
}

// _de_homo(K^-1 (x, y, 1)) with its 1e-10 guard, rounded once to the fp32 the fit kernels read.
DS_HD void normalized_point(const double* Ki, double x, double y, float* out) {
  const double u = (Ki[0] * x + Ki[1] * y) + Ki[2], v = (Ki[3] * x + Ki[4] * y) + Ki[5], w = (Ki[6] * x + Ki[7] * y) + Ki[8];
  const double g = w + 1e-10;
  out[0] = (float)(u / g);
  out[1] = (float)(v / g);
}

// F = K^-T E K^-1, kept in fp64.
DS_HD void e_to_f(const double* Ki, const double* E, double* F) {
  double T[9];  // E K^-1
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T[3 * r + c] = (E[3 * r] * Ki[c] + E[3 * r + 1] * Ki[3 + c]) + E[3 * r + 2] * Ki[6 + c];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) F[3 * r + c] = (Ki[r] * T[c] + Ki[3 + r] * T[3 + c]) + Ki[6 + r] * T[6 + c];
}

// _sampson_dist of the pixel correspondence (x, y) under the 3x3 M.
DS_HD double sampson(const double* M, double x0, double x1, double y0, double y1) {
  const double x[3] = {x0, x1, 1.0}, y[3] = {y0, y1, 1.0};
  return ea::value(1, ea::terms(M, x, y), -1.0, 0.0);
}

// 1 - sigmoid(beta (d - thresh)) as the one quotient it is: no cancellation near 1, exp overflow gives 0, a NaN stays a NaN.
DS_HD double soft_inlier(double d, double thresh, double beta) { return 1.0 / (1.0 + exp(beta * (d - thresh))); }

// The refit's row weight: sqrt of the soft weight AS WRITTEN (fp32), so that the output `soft` defines the refit.
DS_HD float refit_weight(float soft) { return (float)sqrt((double)soft); }

// The sum of the 64 per-lane partial sums as the wavefront adds them (wave_sum, dfepe_common.h): a balanced binary tree over the
// lanes in order.  Addition commutes exactly, so the tree's shape is all that matters.  Overwrites v.
DS_HD double tree_sum64(double* v) {
  for (int step = 1; step < kLanes; step *= 2)
    for (int i = 0; i < kLanes; i += 2 * step) v[i] = v[i] + v[i + step];
  return v[0];
}

// N_scores / (N_counts + 1e-10) in the reference's float32 (dsac.py:194).
DS_HD float quality(float n_scores, float n_counts) { return n_scores / (n_counts + 1e-10f); }

}  // namespace ds
