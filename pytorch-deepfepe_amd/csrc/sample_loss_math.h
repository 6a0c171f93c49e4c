// sample_loss_math.h -- per-lane arithmetic of the sample-loss branch (csrc/sample_loss.hip), written once for the device and for the
// host (tests/emu/emu_sample_loss.cpp compiles it with g++).  The contract is in include/dfepe.h (dfepe_sample_multisets and what
// follows it), the algorithm in DESIGN.md 3.22, the restatement in tests/sample_loss_ref.py.  What it restates:
//   np.random.choice(n, topK, p=p), 100 times per pair     deepFEPE/models/DeepFNetSampleLoss.py:401-409  (the law, not the stream)
//   torch.topk of get_unique                               DeepFNetSampleLoss.py:345-362
//   prod(1000 w) / (sum over the sets + 1e-10)             DeepFNetSampleLoss.py:418-419
//   compute_epi_residual summed over the virtual points    deepFEPE/train_good_utils.py:402-410, dsac_tools/utils_F.py:400-413
// The draw and the top-K rule are integer arithmetic on 32- and 64-bit words (a float is only looked at through its bits), so the
// kernel, the host build and the restatement agree bit for bit.  The floating-point parts are fp64 with contraction off (the pragma
// of epi_adjoint_math.h covers this header too), so a product and the sum it feeds are two roundings on the device as on the host.
//
//   draw     quantised weights q and their exclusive prefix sums P[0..n] exactly as sampler_math.h makes them.  Draw j of set h of
//            pair b: t = mulhi64(r64_j, P[n]) in [0, P[n]); the index is the largest i < n with P[i] <= t, by binary search.
//            P[i+1] > t, so q[i] > 0: what is not drawable is never drawn.  Every draw is independent of the others (WITH
//            replacement), a set uses the r64 of draws 0 .. K-1 of its stream: 2 K words, no rejection loop.  The bias of a draw is
//            at most P[n] / 2^64 (sampler_math.h, "bounded"): < 2^-24 at N = 1000.  Without a drawable weight (P[n] = 0) the index
//            is mulhi64(r64_j, n): uniform with replacement.
//   top-K    order_key maps a float to a 32-bit word whose unsigned order is the order of the values, with -0 = +0 and every NaN
//            on top; ties go to the lowest index.  A position is (key << 32) | ~index: the K largest in descending order are the
//            K largest positions, each the largest one below its predecessor.
#pragma once
#include <stdint.h>

#include "epi_adjoint_math.h"
#include "sampler_math.h"

namespace sl {

constexpr int kMinDraws = 8, kMaxDraws = 32;  // K: draws per set
constexpr int kMaxVirt = 2048;                // M: virtual points of a pair that the loss kernels keep in LDS (24 bytes each)
constexpr int kScatterChunk = 2048;           // cells of a pair's idx that dfepe_sample_scatter_bwd stages at a time (any H K)

// Draw j of a set.  P null: uniform over 0 .. n-1.
SM_HD int draw_one(sm::Stream& s, int j, const uint64_t* P, int n) {
  const uint64_t r = sm::next64(s, j);
  if (!P) return (int)sm::mulhi64(r, (uint64_t)n);
  const uint64_t t = sm::mulhi64(r, P[n]);
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (P[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- top-K ---------------------------------------------------------------------------------------------------------------------------
SM_HD uint32_t order_key(uint32_t bits) {
  if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xff800001u;  // NaN: right above +inf, as torch.topk orders it (never all ones:
                                                               // ~0 is the "below everything so far" a search starts from)
  if (bits == 0x80000000u) bits = 0u;                          // -0 = +0
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
SM_HD uint64_t position(uint32_t bits, int i) { return ((uint64_t)order_key(bits) << 32) | (uint64_t)(0xffffffffu - (uint32_t)i); }
SM_HD int position_index(uint64_t pos) { return (int)(0xffffffffu - (uint32_t)(pos & 0xffffffffu)); }

// The largest position below `below` among i = first, first + step, ... < n (0: none; a position is never 0, i < 2^31).
SM_HD uint64_t best_below(const uint32_t* bits, int n, int first, int step, uint64_t below) {
  uint64_t best = 0;
  for (int i = first; i < n; i += step) {
    const uint64_t p = position(bits[i], i);
    if (p < below && p > best) best = p;
  }
  return best;
}

// ---- accu ----------------------------------------------------------------------------------------------------------------------------
// prod_k (1000 w[idx_k]) of one set in fp64: each factor is exact (a float times 1000 has 34 significant bits), K - 1 roundings.
SM_HD int safe_index(int i, int N) { return i < 0 ? 0 : (i >= N ? N - 1 : i); }
SM_HD double set_product(const float* w, const int* idx, int K, int N) {
  double p = 1.0;
  for (int k = 0; k < K; ++k) p = p * (1000.0 * (double)w[safe_index(idx[k], N)]);
  return p;
}

// ---- the loss ------------------------------------------------------------------------------------------------------------------------
// T v, each coordinate formed in fp64 and rounded once to float, as dfepe_floss_fwd forms the reference's float32 pts_eval.
SM_HD void eval_point(const float* T, const float* v, float* x) {
  const double a = v[0], b = v[1], c = v[2];
  for (int r = 0; r < 3; ++r) x[r] = (float)(((double)T[3 * r] * a + (double)T[3 * r + 1] * b) + (double)T[3 * r + 2] * c);
}

// compute_epi_residual of one point: l1 = F^T x2 (= b), l2 = F x1 (= a), dd = x2^T F x1 (= s), d = |dd| (1/(|l1[:2]| + 1e-6) +
// 1/(|l2[:2]| + 1e-6)), min(d, clamp_at).
SM_HD double residual(const double* F, const float* x1, const float* x2, double clamp_at) {
  const double x[3] = {x1[0], x1[1], x1[2]}, y[3] = {x2[0], x2[1], x2[2]};
  const ea::Terms t = ea::terms(F, x, y);
  const double d = fabs(t.s) * (1.0 / (sqrt(t.Q) + 1e-6) + 1.0 / (sqrt(t.A) + 1e-6));
  return d > clamp_at ? clamp_at : d;  // a NaN stays a NaN
}

// Its adjoint w.r.t. F, ADDED to gF[9]: in the notation of epi_adjoint_math.h d = e(s, A, Q) with
//   cs = sign(s) S, cA = -|s| i2^2 / (2 n2), cQ = -|s| i1^2 / (2 n1)   (n1 = sqrt Q, n2 = sqrt A, i = 1 / (n + 1e-6), S = i1 + i2)
// where d <= clamp_at, nothing elsewhere (torch.clamp(max=) passes the gradient at the bound); a term whose norm is 0 is 0.
SM_HD void residual_adjoint_F(const double* F, const float* x1, const float* x2, double clamp_at, double* gF) {
  const double x[3] = {x1[0], x1[1], x1[2]}, y[3] = {x2[0], x2[1], x2[2]};
  const ea::Terms t = ea::terms(F, x, y);
  const double n1 = sqrt(t.Q), n2 = sqrt(t.A);
  const double i1 = 1.0 / (n1 + 1e-6), i2 = 1.0 / (n2 + 1e-6);
  const double S = i1 + i2, ad = fabs(t.s);
  if (!(ad * S <= clamp_at)) return;
  const double cs = ea::sign0(t.s) * S;
  const double cA = (n2 > 0.0) ? -((ad * (i2 * i2)) / (2.0 * n2)) : 0.0;
  const double cQ = (n1 > 0.0) ? -((ad * (i1 * i1)) / (2.0 * n1)) : 0.0;
  double g[9], gx[3], gy[3];
  ea::point_adjoint(F, x, y, t, cs, cA, cQ, g, gx, gy);
  for (int c = 0; c < 9; ++c) gF[c] = gF[c] + g[c];
}

// ---- the scatter ---------------------------------------------------------------------------------------------------------------------
// What cell (h, k) of a pair sends to the correspondence it names: directly g_w_sel, and through accu
//   d accu_h / d w_n = (count of n in set h) accu_h / w_n - accu_h sum_h' (count of n in set h') accu_h' / w_n
// so with G = sum_h g_accu_h accu_h every cell adds accu_h (g_accu_h - G) / w_n: cell_accu is the numerator.
SM_HD double cell_accu(double accu_h, double g_accu_h, double G) { return accu_h * (g_accu_h - G); }
SM_HD float scatter_finish(double direct, double through_accu, float w) {
  return (float)(direct + ((w != 0.0f) ? through_accu / (double)w : 0.0));
}

}  // namespace sl
