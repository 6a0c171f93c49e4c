// sp_process_math.h -- per-lane arithmetic of the SuperPoint output processing (csrc/sp_process.hip), written once for the
// device and for the host (tests/emu/emu_sp_process.cpp compiles it with g++).  What it restates is the reference's
// process_SP_output (deepFEPE/train_good_utils.py:727-755): flattenDetection, heatmap_to_nms (nms_fast), pred_soft_argmax and
// sample_desc_from_points.  Those are methods of the superpoint package, which is not part of the reference's tree: the
// formulas below are the published algorithm as include/dfepe.h states it, unpinned.  Arithmetic is fp64 over fp32 data and is
// rounded once where a value leaves.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SP_HD __host__ __device__ inline
#else
#define SP_HD inline
#endif

namespace sp {

constexpr int kCell = 8;             // pixels per cell side; 64 detection channels and the dustbin
constexpr int kChannels = 65;
constexpr double kEps = 1e-6;        // every epsilon of pred_soft_argmax
constexpr long kMaxPixels = 1L << 24;  // H * W of one image; beyond: DFEPE_ERR_UNSUPPORTED
constexpr int kLdsPixels = 12288;    // dfepe_sp_nms keeps heat and state of an image of up to this many pixels in LDS (60 KiB)
constexpr int kMaxPatch = 63;        // patch_size of the soft-argmax

// ---- greedy NMS as a fixpoint ------------------------------------------------------------------------------------------
enum State : unsigned char { kNone = 0, kUndecided = 1, kKept = 2, kSuppressed = 3 };

// set_nan2zero (models/model_utils.py:5-15).
SP_HD float nan2zero(float v) { return (v != v) ? 0.0f : v; }

// A candidate: h >= conf_thresh.  NaN fails the comparison.
SP_HD bool candidate(float h, float conf_thresh) { return h >= conf_thresh; }

// nms_fast visits candidates by confidence descending; among equals the lower row-major index goes first (a stated rule: the
// reference's argsort is not stable).  True when candidate a is visited before candidate b.
SP_HD bool outranks(float ha, long ia, float hb, long ib) { return ha > hb || (ha == hb && ia < ib); }

// One round for one undecided candidate, given what its window holds among the candidates that outrank it.
SP_HD State decide(bool outranking_kept, bool outranking_undecided) {
  return outranking_kept ? kSuppressed : (outranking_undecided ? kUndecided : kKept);
}

// The same over a whole window: heat and state are the image's [H,W] planes (wherever they live).  Reads states that other lanes
// may be deciding in the same round; a decided state is final and is the greedy loop's decision, so the result does not depend
// on which of the two values is seen.
template <class Heat, class Stat>
SP_HD State decide_pixel(const Heat& heat, const Stat& state, int H, int W, int d, int y, int x) {
  const long i = (long)y * W + x;
  const float hi = heat[i];
  const int y0 = y - d < 0 ? 0 : y - d, y1 = y + d > H - 1 ? H - 1 : y + d;
  const int x0 = x - d < 0 ? 0 : x - d, x1 = x + d > W - 1 ? W - 1 : x + d;
  bool pending = false;
  for (int yy = y0; yy <= y1; ++yy) {
    for (int xx = x0; xx <= x1; ++xx) {
      const long j = (long)yy * W + xx;
      const unsigned char s = state[j];
      if (s == kNone || s == kSuppressed || j == i) continue;
      if (!outranks(heat[j], j, hi, i)) continue;
      if (s == kKept) return kSuppressed;
      pending = true;
    }
  }
  return decide(false, pending);
}

// The border rule, applied after the loop: a kept point leaves when x < r, x >= W - r, y < r or y >= H - r.
SP_HD bool inside_border(int y, int x, int H, int W, int r) { return x >= r && x < W - r && y >= r && y < H - r; }

SP_HD long nms_capacity(int H, int W, int d) {
  if (H <= 0 || W <= 0 || d < 0) return 0;
  const long s = (long)d + 1;
  return ((H + s - 1) / s) * ((W + s - 1) / s);
}

// ---- flattenDetection ------------------------------------------------------------------------------------------------
// softmax over the 65 channels of one cell: v[c * stride] are the logits, NaN read as 0.  In three passes (maximum, sum,
// probability) so that a lane keeps no array.
SP_HD double cell_max(const float* v, long stride) {
  double m = (double)nan2zero(v[0]);
  for (int c = 1; c < kChannels; ++c) {
    const double t = (double)nan2zero(v[c * stride]);
    m = t > m ? t : m;
  }
  return m;
}
SP_HD double cell_sum(const float* v, long stride, double m) {
  double s = 0.0;
  for (int c = 0; c < kChannels; ++c) s += exp((double)nan2zero(v[c * stride]) - m);
  return s;
}
SP_HD double cell_prob(float vc, double m, double s) { return exp((double)nan2zero(vc) - m) / s; }
// sum over the 64 detection channels of g_c p_c, g the heatmap's gradient at the cell's pixels (row stride W): the softmax
// adjoint is p_c (g_c - dot), with g = 0 for the dustbin.
SP_HD double cell_dot(const float* v, long stride, double m, double s, const float* g, long W) {
  double dot = 0.0;
  for (int c = 0; c < kChannels - 1; ++c) dot += (double)g[(c / kCell) * W + (c % kCell)] * cell_prob(v[c * stride], m, s);
  return dot;
}

// ---- pred_soft_argmax ------------------------------------------------------------------------------------------------
struct Patch {      // what one kept point's patch yields; everything the adjoint needs again
  double denom;     // sum(h) + eps
  double qmax;      // max of the clamped q
  int ties;         // entries equal to qmax
  double inv_d;     // 1 / (sum(e) + eps)
  double ox, oy;    // sum(x e) / (sum(e) + eps), sum(y e) / (sum(e) + eps): the offsets before p//2 leaves
  int valid;        // 0: sum(h) <= 0 (or NaN): offset (0,0), no gradient
};

SP_HD double clamp_q(double q) { return q < 0.0 ? kEps : q; }

// h: the image's heat plane, (cx, cy) the point, p the odd patch size; the patch lies inside the image (the caller checked).
// e = exp(log q - max log q) is evaluated as written.
SP_HD Patch soft_argmax(const float* h, int W, int cx, int cy, int p) {
  Patch r;
  const int c = p / 2;
  const float* base = h + (long)(cy - c) * W + (cx - c);
  double s = 0.0;
  for (int j = 0; j < p; ++j)
    for (int i = 0; i < p; ++i) s += (double)base[(long)j * W + i];
  r.denom = s + kEps;
  r.valid = (s > 0.0) ? 1 : 0;
  r.qmax = 0.0; r.ties = 0; r.inv_d = 0.0; r.ox = c; r.oy = c;
  if (!r.valid) return r;
  double m = -INFINITY;
  for (int j = 0; j < p; ++j)
    for (int i = 0; i < p; ++i) {
      const double q = clamp_q((double)base[(long)j * W + i] / r.denom);
      if (q > m) { m = q; r.ties = 1; } else if (q == m) { ++r.ties; }
    }
  r.qmax = m;
  const double lmax = log(m);
  double se = 0.0, sx = 0.0, sy = 0.0;
  for (int j = 0; j < p; ++j)
    for (int i = 0; i < p; ++i) {
      const double q = clamp_q((double)base[(long)j * W + i] / r.denom);
      const double e = exp(log(q) - lmax);
      se += e; sx += i * e; sy += j * e;
    }
  r.inv_d = 1.0 / (se + kEps);
  r.ox = sx * r.inv_d;
  r.oy = sy * r.inv_d;
  return r;
}

// The adjoint of one patch entry with respect to its q, for upstream (gx, gy): through e = q / qmax, the maximum's share
// spread evenly over its ties (what torch's amax does), nothing through a clamped entry.
SP_HD double grad_q(const Patch& r, double hval, int i, int j, double gx, double gy) {
  const double q0 = hval / r.denom;
  if (q0 < 0.0) return 0.0;
  double g = (gx * (i - r.ox) + gy * (j - r.oy)) * r.inv_d / r.qmax;
  if (q0 == r.qmax) g -= (gx * r.ox + gy * r.oy) * kEps * r.inv_d / (r.qmax * r.ties);
  return g;
}

// sum_j grad_q_j q_j over the patch: the share every entry receives through the normaliser sum(h) + eps.
SP_HD double grad_norm_share(const Patch& r, const float* h, int W, int cx, int cy, int p, double gx, double gy) {
  const int c = p / 2;
  const float* base = h + (long)(cy - c) * W + (cx - c);
  double a = 0.0;
  for (int j = 0; j < p; ++j)
    for (int i = 0; i < p; ++i) {
      const double hv = (double)base[(long)j * W + i];
      a += grad_q(r, hv, i, j, gx, gy) * (hv / r.denom);
    }
  return a;
}

// d off / d h of the entry at patch position (i, j), given the share above.
SP_HD double grad_h(const Patch& r, double hval, int i, int j, double gx, double gy, double share) {
  return (grad_q(r, hval, i, j, gx, gy) - share) / r.denom;
}

// ---- sample_desc_from_points -------------------------------------------------------------------------------------------
struct Taps {
  int x0, y0;          // the upper-left tap; the others are +1
  double w00, w01, w10, w11;  // weights of (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1)
};

// (x, y) in pixels of the [8Hc, 8Wc] image -> grid_sample's taps in the [Hc, Wc] map.
SP_HD Taps bilinear_taps(double x, double y, int Hc, int Wc, int align_corners) {
  const double gx = x / (0.5 * kCell * Wc) - 1.0, gy = y / (0.5 * kCell * Hc) - 1.0;
  const double ix = align_corners ? (gx + 1.0) * 0.5 * (Wc - 1) : ((gx + 1.0) * Wc - 1.0) * 0.5;
  const double iy = align_corners ? (gy + 1.0) * 0.5 * (Hc - 1) : ((gy + 1.0) * Hc - 1.0) * 0.5;
  const double fx = floor(ix), fy = floor(iy);
  Taps t;
  // a position that is NaN or further than a cell outside has no tap inside: zero padding gives 0
  if (!(fx >= -1.0 && fx < (double)Wc && fy >= -1.0 && fy < (double)Hc)) {
    t.x0 = t.y0 = -2;
    t.w00 = t.w01 = t.w10 = t.w11 = 0.0;
    return t;
  }
  t.x0 = (int)fx;
  t.y0 = (int)fy;
  const double ax = ix - fx, ay = iy - fy;
  t.w00 = (1.0 - ax) * (1.0 - ay); t.w01 = ax * (1.0 - ay); t.w10 = (1.0 - ax) * ay; t.w11 = ax * ay;
  return t;
}

// One tap: zero outside the map, and a NaN descriptor value read as 0 (set_nan2zero on desc, train_good_utils.py:742).
SP_HD double tap(const float* plane, int Hc, int Wc, int y, int x) {
  return (x >= 0 && x < Wc && y >= 0 && y < Hc) ? (double)nan2zero(plane[(long)y * Wc + x]) : 0.0;
}

SP_HD double sample(const float* plane, int Hc, int Wc, const Taps& t) {
  return t.w00 * tap(plane, Hc, Wc, t.y0, t.x0) + t.w01 * tap(plane, Hc, Wc, t.y0, t.x0 + 1) +
         t.w10 * tap(plane, Hc, Wc, t.y0 + 1, t.x0) + t.w11 * tap(plane, Hc, Wc, t.y0 + 1, t.x0 + 1);
}

}  // namespace sp
