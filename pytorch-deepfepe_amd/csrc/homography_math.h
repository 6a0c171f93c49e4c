// homography_math.h -- per-lane arithmetic of the RANSAC homography estimator (csrc/homography.hip), written once for the device
// and for the host (tests/emu/emu_homography.cpp compiles it with g++).  The algorithm is OpenCV 3.4's findHomography(RANSAC):
// HomographyEstimatorCallback, RANSACPointSetRegistrator, the refit over the inliers and the LMSolver refinement, which the
// reference calls in evaluations/descriptor_evaluation.py:93 and deepFEPE/evaluate_frontend.py:234; the contract is spelled out
// in include/dfepe.h (dfepe_ransac_homography).  The stream, the Lemire map and the count-table codes are those of ransac_math.h.
//
// Two kinds of code live here.  Pure functions of their arguments (sampling, the 4-point solve, the error), and the
// refit / refinement drivers, which are templates over a context Ctx that supplies the sums over a pair's inliers:
//   ctx.reduce(kind, par, out)  fills out[0 .. 45] with the sums of `kind` over the inliers (out[45]: a maximum), same in every lane
//   ctx.leader()                whether this lane does the small dense algebra (the host: always; the device: lane 0)
//   ctx.sync()                  makes the leader's writes visible to the others (the host: nothing; the device: a barrier)
// All matrices of the drivers live in a Work record the caller places (the device: LDS, so that no array is indexed dynamically
// in registers); the host and the device therefore run the same statements and differ only in the order of the sums.
#pragma once
#include "ransac_math.h"

namespace hg {

constexpr int kSample = 4;  // points per minimal sample
constexpr int kLmIters = 10;
constexpr int kSweeps = 50;  // cyclic Jacobi: sweeps at most (9x9 and 8x8 converge in 6..9)
constexpr int kRed = 46;     // reduction record: 45 sums and one maximum

// rs::collinear_last for a sample of 4: the last point against every line through two earlier ones.
RS_HD bool collinear_last4(const float* x, const float* y) {
  const int i = kSample - 1;
#pragma unroll
  for (int j = 0; j < i; ++j) {
    const double dx1 = (double)(x[j] - x[i]), dy1 = (double)(y[j] - y[i]);
#pragma unroll
    for (int k = 0; k < j; ++k) {
      const double dx2 = (double)(x[k] - x[i]), dy2 = (double)(y[k] - y[i]);
      if (fabs(dx2 * dy1 - dy2 * dx1) <= (double)FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
    }
  }
  return false;
}

// det of [[xa ya 1], [xb yb 1], [xc yc 1]] in double from float coordinates, expanded along the last column.
RS_HD double det_tri(float xa, float ya, float xb, float yb, float xc, float yc) {
  const double a0 = xa, a1 = ya, b0 = xb, b1 = yb, c0 = xc, c1 = yc;
  return (b0 * c1 - b1 * c0) - (a0 * c1 - a1 * c0) + (a0 * b1 - a1 * b0);
}

// OpenCV's orientation test of HomographyEstimatorCallback::checkSubset: over the four triples, the number with
// det(src) * det(dst) < 0 must be 0 or 4 (a homography keeps or flips the orientation of every triple alike).
RS_HD bool orientation_ok(const float* x1, const float* y1, const float* x2, const float* y2) {
  int neg = 0;
#define HG_TRIPLE(a, b, c) \
  neg += (det_tri(x1[a], y1[a], x1[b], y1[b], x1[c], y1[c]) * det_tri(x2[a], y2[a], x2[b], y2[b], x2[c], y2[c]) < 0.0) ? 1 : 0
  HG_TRIPLE(0, 1, 2);
  HG_TRIPLE(0, 1, 3);
  HG_TRIPLE(0, 2, 3);
  HG_TRIPLE(1, 2, 3);
#undef HG_TRIPLE
  return neg == 0 || neg == 4;
}

// One iteration's sample: 4 distinct indices, redrawn (continuing the same stream) while checkSubset fails.
// P: callable, P(i) -> object with .x .y .z .w = (x1, y1, x2, y2).  false after rs::kMaxAttempts.
template <class P>
RS_HD bool draw_sample4(uint64_t seed, int k, int N, const P& pts, int* idx) {
  rs::Stream s = rs::stream_of(seed, k);
  for (int att = 0; att < rs::kMaxAttempts; ++att) {
    float x1[kSample], y1[kSample], x2[kSample], y2[kSample];
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
      const auto m = pts(v);
      x1[i] = m.x; y1[i] = m.y; x2[i] = m.z; y2[i] = m.w;
    }
    if (!collinear_last4(x1, y1) && !collinear_last4(x2, y2) && orientation_ok(x1, y1, x2, y2)) return true;
  }
  return false;
}

// H = T_dst^-1 H0 T_src for x_n = s (x - c) per axis, scaled to H[8] = 1.  c, s: (src x, src y, dst x, dst y).
// false when H[8] is zero or not finite (OpenCV would divide by it).
RS_HD bool denormalise(const double* h0, const double* c, const double* s, double* H) {
  double G[9];  // H0 T_src
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    G[3 * r + 0] = h0[3 * r + 0] * s[0];
    G[3 * r + 1] = h0[3 * r + 1] * s[1];
    G[3 * r + 2] = h0[3 * r + 2] - h0[3 * r + 0] * (c[0] * s[0]) - h0[3 * r + 1] * (c[1] * s[1]);
  }
  const double ix = 1.0 / s[2], iy = 1.0 / s[3];
  double Hh[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Hh[k] = ix * G[k] + c[2] * G[6 + k];
    Hh[3 + k] = iy * G[3 + k] + c[3] * G[6 + k];
    Hh[6 + k] = G[6 + k];
  }
  const double h8 = Hh[8];
  if (!(fabs(h8) > 0.0) || !(fabs(h8) <= DBL_MAX)) return false;
  const double sc = 1.0 / h8;
#pragma unroll
  for (int k = 0; k < 8; ++k) H[k] = Hh[k] * sc;
  H[8] = 1.0;
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) fin = fin && (fabs(H[k]) <= DBL_MAX);
  return fin;
}

// runKernel on a minimal sample given in pixels: normalisation by centroid and n / sum |x - c| per axis (no model when a sum
// is below FLT_EPSILON), then the null vector of the 8x9 system directly -- Householder QR of its transpose (9x8), the last
// column of Q, as rs::null_space7 does -- instead of the smallest eigenvector of L^T L; de-normalised and scaled to H[8] = 1.
RS_HD bool solve4(const float* px1, const float* py1, const float* px2, const float* py2, double* H) {
  double c[4] = {0.0, 0.0, 0.0, 0.0}, s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < kSample; ++i) { c[0] += (double)px1[i]; c[1] += (double)py1[i]; c[2] += (double)px2[i]; c[3] += (double)py2[i]; }
#pragma unroll
  for (int a = 0; a < 4; ++a) c[a] /= kSample;
#pragma unroll
  for (int i = 0; i < kSample; ++i) {
    s[0] += fabs((double)px1[i] - c[0]); s[1] += fabs((double)py1[i] - c[1]);
    s[2] += fabs((double)px2[i] - c[2]); s[3] += fabs((double)py2[i] - c[3]);
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if (s[a] < (double)FLT_EPSILON) return false;
    s[a] = (double)kSample / s[a];
  }
  double M[9][8];  // column j = row j of the system
#pragma unroll
  for (int i = 0; i < kSample; ++i) {
    const double X = ((double)px1[i] - c[0]) * s[0], Y = ((double)py1[i] - c[1]) * s[1];
    const double x = ((double)px2[i] - c[2]) * s[2], y = ((double)py2[i] - c[3]) * s[3];
    const int j = 2 * i;
    M[0][j] = X;   M[1][j] = Y;   M[2][j] = 1.0; M[3][j] = 0.0; M[4][j] = 0.0; M[5][j] = 0.0;
    M[6][j] = -x * X; M[7][j] = -x * Y; M[8][j] = -x;
    M[0][j + 1] = 0.0; M[1][j + 1] = 0.0; M[2][j + 1] = 0.0; M[3][j + 1] = X; M[4][j + 1] = Y; M[5][j + 1] = 1.0;
    M[6][j + 1] = -y * X; M[7][j + 1] = -y * Y; M[8][j + 1] = -y;
  }
  double beta[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    double nn = 0.0;
#pragma unroll
    for (int r = j; r < 9; ++r) nn += M[r][j] * M[r][j];
    const double nrm = sqrt(nn);
    const double alpha = (M[j][j] < 0.0) ? nrm : -nrm;
    M[j][j] -= alpha;
    const double vv = nn - 2.0 * alpha * (M[j][j] + alpha) + alpha * alpha;
    beta[j] = (vv > 0.0) ? 2.0 / vv : 0.0;
#pragma unroll
    for (int cc = j + 1; cc < 8; ++cc) {
      double t = 0.0;
#pragma unroll
      for (int r = j; r < 9; ++r) t += M[r][j] * M[r][cc];
      t *= beta[j];
#pragma unroll
      for (int r = j; r < 9; ++r) M[r][cc] -= t * M[r][j];
    }
  }
  double h0[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) h0[r] = (r == 8) ? 1.0 : 0.0;
#pragma unroll
  for (int j = 7; j >= 0; --j) {
    double t = 0.0;
#pragma unroll
    for (int r = j; r < 9; ++r) t += M[r][j] * h0[r];
    t *= beta[j];
#pragma unroll
    for (int r = j; r < 9; ++r) h0[r] -= t * M[r][j];
  }
  return denormalise(h0, c, s, H);
}

// OpenCV's HomographyEstimatorCallback::computeError decision without the divisions: with w = H6 x + H7 y + 1,
// (X - x' w)^2 + (Y - y' w)^2 <= t^2 w^2; w == 0 is never an inlier.
RS_HD bool is_inlier(const double* H, double x1, double y1, double x2, double y2, double t2) {
  const double w = H[6] * x1 + H[7] * y1 + H[8];
  const double dx = (H[0] * x1 + H[1] * y1 + H[2]) - x2 * w, dy = (H[3] * x1 + H[4] * y1 + H[5]) - y2 * w;
  return (w != 0.0) && (dx * dx + dy * dy <= t2 * (w * w));
}

// The gather-and-solve half of an iteration: solve4 on the four correspondences idx of a pair (P as in draw_sample4).  The pair
// of exactly four points comes here directly with idx = {0, 1, 2, 3}.
template <class P>
RS_HD bool solve_sample(const P& pts, const int* idx, double* H) {
  float x1[kSample], y1[kSample], x2[kSample], y2[kSample];
#pragma unroll
  for (int i = 0; i < kSample; ++i) {
    const auto m = pts(idx[i]);
    x1[i] = m.x; y1[i] = m.y; x2[i] = m.z; y2[i] = m.w;
  }
  return solve4(x1, y1, x2, y2, H);
}

// Iteration k of a pair, whole: its sample drawn, gathered and solved.  The count launch calls this and the select launch its
// two halves (so that the pair of four points can enter at the second), which is what makes the winner come out again bit for
// bit.  1: H holds the model; 0: the solve gave none (rs::kNoRoot in the count table); rs::kNoSample: no sample.
template <class P>
RS_HD int solve_iteration(uint64_t seed, int k, int n, const P& pts, double* H) {
  int idx[kSample];
  if (!draw_sample4(seed, k, n, pts, idx)) return rs::kNoSample;
  return solve_sample(pts, idx, H) ? 1 : 0;
}

// The iteration bound and the sequential selection rule over one pair's count table counts[k] (rs::kNoRoot = the solve gave no
// model, rs::kNoSample = no sample) are ransac_math.h's, with 4 points and one slot an iteration (so no best root to report).
RS_HD int update_num_iters4(double p, double ep, int niters) { return rs::update_num_iters<kSample>(p, ep, niters); }
RS_HD int select_best(const int* counts, int N, double confidence, int max_iters, int* best_k, int* iters) {
  int slot;
  return rs::select_best<1, kSample>(counts, N, confidence, max_iters, best_k, &slot, iters);
}

// ---- sums over the inliers: what one correspondence adds to the record acc[kRed] ------------------------------------------
enum Kind { kSum = 0, kAbs = 1, kLtL = 2, kLmFull = 3, kLmRes = 4 };

RS_HD int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // lower triangle, j <= i

// kSum: acc[0..3] += (x1, y1, x2, y2).  kAbs (par = c[4]): acc[0..3] += |x - c|.
// kLtL (par = c[4], s[4]): acc[tri(i, j)] += the two rows' products (45 entries of L^T L).
// kLmFull (par = h[8]): acc[tri(i, j)] (36) += J^T J, acc[36..43] += J^T r, acc[44] += |r|^2, acc[45] = max |r|_inf.
// kLmRes: acc[44], acc[45] only.
template <int KIND>
RS_HD void point_add(const double* par, double x1, double y1, double x2, double y2, double* acc) {
  if (KIND == kSum) {
    acc[0] += x1; acc[1] += y1; acc[2] += x2; acc[3] += y2;
  } else if (KIND == kAbs) {
    acc[0] += fabs(x1 - par[0]); acc[1] += fabs(y1 - par[1]); acc[2] += fabs(x2 - par[2]); acc[3] += fabs(y2 - par[3]);
  } else if (KIND == kLtL) {
    const double X = (x1 - par[0]) * par[4], Y = (y1 - par[1]) * par[5], x = (x2 - par[2]) * par[6], y = (y2 - par[3]) * par[7];
    const double Lx[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -x * X, -x * Y, -x};
    const double Ly[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -y * X, -y * Y, -y};
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) acc[i * (i + 1) / 2 + j] += Lx[i] * Lx[j] + Ly[i] * Ly[j];
  } else {
    const double w = par[6] * x1 + par[7] * y1 + 1.0;
    const double wi = (fabs(w) > DBL_EPSILON) ? 1.0 / w : 0.0;
    const double xi = (par[0] * x1 + par[1] * y1 + par[2]) * wi, yi = (par[3] * x1 + par[4] * y1 + par[5]) * wi;
    const double rx = xi - x2, ry = yi - y2;
    acc[44] += rx * rx + ry * ry;
    acc[45] = fmax(acc[45], fmax(fabs(rx), fabs(ry)));
    if (KIND == kLmFull) {
      const double Jx[8] = {x1 * wi, y1 * wi, wi, 0.0, 0.0, 0.0, -x1 * wi * xi, -y1 * wi * xi};
      const double Jy[8] = {0.0, 0.0, 0.0, x1 * wi, y1 * wi, wi, -x1 * wi * yi, -y1 * wi * yi};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) acc[i * (i + 1) / 2 + j] += Jx[i] * Jx[j] + Jy[i] * Jy[j];
        acc[36 + i] += Jx[i] * rx + Jy[i] * ry;
      }
    }
  }
}

// ---- small dense algebra on memory the caller places ----------------------------------------------------------------------
// Cyclic Jacobi eigen decomposition of the symmetric n x n matrix A (row-major, full storage, destroyed: its diagonal becomes
// the eigenvalues) with the eigenvectors in the columns of V.  Numerical Recipes' rotation and its skip rule: after three sweeps
// an off-diagonal element that no longer changes either diagonal neighbour when added a hundredfold is set to zero.
RS_HD void jacobi_eig(double* A, double* V, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[i * n + j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) off += fabs(A[p * n + q]);
    if (off == 0.0) break;
    for (int p = 0; p < n - 1; ++p) {
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q], app = A[p * n + p], aqq = A[q * n + q];
        const double g = 100.0 * fabs(apq);
        if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
          A[p * n + q] = 0.0;
          A[q * n + p] = 0.0;
          continue;
        }
        if (!(fabs(apq) > 0.0)) continue;
        const double hh = aqq - app;
        double t;
        if (fabs(hh) + g == fabs(hh)) {
          t = apq / hh;
        } else {
          const double theta = 0.5 * hh / apq;
          t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
          if (theta < 0.0) t = -t;
        }
        const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
        for (int k = 0; k < n; ++k) {  // A <- A G (columns p, q)
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {  // A <- G^T A (rows p, q)
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk;
          A[q * n + k] = s * apk + c * aqk;
        }
        A[p * n + q] = 0.0;
        A[q * n + p] = 0.0;
        for (int k = 0; k < n; ++k) {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
    }
  }
}

// What the drivers keep per pair (the device: in LDS).
struct Work {
  double red[kRed];  // the last reduction
  double A[81];      // matrix handed to the Jacobi (9x9 L^T L, or 8x8 J^T J + lambda D)
  double V[81];
  double JtJ[64];    // the current J^T J, full storage
  double v[8], D[8], d[8], h[8], hd[8];
  double par[8];
  double H[9];
  double scal[4];  // leader -> all: (ok flag, max |A^-1_ii|)
};

// runKernel over the pair's inliers (n of them, n >= 4): the n-point form -- centroids, n / sum |x - c|, the 9x9 L^T L summed in
// fp64, its eigenvector of the smallest eigenvalue by cyclic Jacobi.  true: W.H holds the result (visible to every lane).
template <class Ctx>
RS_HD bool refit(Ctx& ctx, Work& W, int n) {
  ctx.reduce(kSum, W.par, W.red);
  if (ctx.leader()) {
    for (int a = 0; a < 4; ++a) W.par[a] = W.red[a] / n;
  }
  ctx.sync();
  ctx.reduce(kAbs, W.par, W.red);
  if (ctx.leader()) {
    bool ok = true;
    for (int a = 0; a < 4; ++a) {
      ok = ok && !(W.red[a] < (double)FLT_EPSILON);
      W.par[4 + a] = (double)n / W.red[a];
    }
    W.scal[0] = ok ? 1.0 : 0.0;
  }
  ctx.sync();
  if (W.scal[0] == 0.0) return false;
  ctx.reduce(kLtL, W.par, W.red);
  if (ctx.leader()) {
    for (int i = 0; i < 9; ++i)
      for (int j = 0; j <= i; ++j) {
        W.A[i * 9 + j] = W.red[tri(i, j)];
        W.A[j * 9 + i] = W.red[tri(i, j)];
      }
    jacobi_eig(W.A, W.V, 9);
    int m = 0;
    for (int i = 1; i < 9; ++i)
      if (W.A[i * 9 + i] < W.A[m * 9 + m]) m = i;
    double h0[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h0[i] = W.V[i * 9 + m];
    double Hh[9];
    const bool ok = denormalise(h0, W.par, W.par + 4, Hh);
    if (ok) {
#pragma unroll
      for (int i = 0; i < 9; ++i) W.H[i] = Hh[i];
    }
    W.scal[0] = ok ? 1.0 : 0.0;
  }
  ctx.sync();
  return W.scal[0] != 0.0;
}

// d = (JtJ + lambda diag(D))^-1 v by the symmetric eigen decomposition Q diag(w) Q^T; an eigenvalue with
// |w_i| <= 2 DBL_EPSILON sum_j |w_j| counts as zero (its direction contributes nothing), as OpenCV's SVD back-substitution does.
// lambda < 0: D is ignored and scal[1] = max_i |(JtJ^-1)_ii| is written instead of d.  Leader only.
RS_HD void lm_solve(Work& W, double lambda) {
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) W.A[i * 8 + j] = W.JtJ[i * 8 + j] + ((i == j && lambda > 0.0) ? lambda * W.D[i] : 0.0);
  jacobi_eig(W.A, W.V, 8);
  double sum = 0.0;
  for (int i = 0; i < 8; ++i) sum += fabs(W.A[i * 8 + i]);
  const double thr = 2.0 * DBL_EPSILON * sum;
  if (lambda < 0.0) {
    double mx = 0.0;
    for (int i = 0; i < 8; ++i) {
      double t = 0.0;
      for (int j = 0; j < 8; ++j) {
        const double wj = W.A[j * 8 + j];
        if (fabs(wj) > thr) t += W.V[i * 8 + j] * W.V[i * 8 + j] / wj;
      }
      mx = fmax(mx, fabs(t));
    }
    W.scal[1] = mx;
    return;
  }
  double* y = W.par;  // free during the refinement
  for (int j = 0; j < 8; ++j) {
    double t = 0.0;
    for (int i = 0; i < 8; ++i) t += W.V[i * 8 + j] * W.v[i];
    const double wj = W.A[j * 8 + j];
    y[j] = (fabs(wj) > thr) ? t / wj : 0.0;
  }
  for (int i = 0; i < 8; ++i) {
    double t = 0.0;
    for (int j = 0; j < 8; ++j) t += W.V[i * 8 + j] * y[j];
    W.d[i] = t;
  }
}

RS_HD void lm_take(Work& W) {  // red (kLmFull) -> JtJ, v.  Leader only.
  for (int i = 0; i < 8; ++i) {
    for (int j = 0; j <= i; ++j) {
      W.JtJ[i * 8 + j] = W.red[tri(i, j)];
      W.JtJ[j * 8 + i] = W.red[tri(i, j)];
    }
    W.v[i] = W.red[36 + i];
  }
}

// The refinement of include/dfepe.h (dfepe_ransac_homography, step 7) on W.h[0..7]; Rs (may be null, kLmIters doubles): every
// iteration's gain ratio R, NaN for an iteration not run.  Returns the iterations run; S0, S1: |r|^2 before and after.
template <class Ctx>
RS_HD int lm_refine(Ctx& ctx, Work& W, double* Rs, double* S0, double* S1) {
  ctx.reduce(kLmFull, W.h, W.red);
  if (ctx.leader()) {
    lm_take(W);
    for (int i = 0; i < 8; ++i) W.D[i] = W.JtJ[i * 8 + i];
  }
  ctx.sync();
  double S = W.red[44], rmax = W.red[45], lambda = 1.0, lc = 0.75;  // the same values in every lane: the flow below is uniform
  *S0 = S;
  int it = 0;
  for (; it < kLmIters;) {
    if (ctx.leader()) {
      lm_solve(W, lambda);
      for (int i = 0; i < 8; ++i) W.hd[i] = W.h[i] - W.d[i];
    }
    ctx.sync();
    ctx.reduce(kLmRes, W.hd, W.red);
    const double Sd = W.red[44];
    double dS = 0.0, dv = 0.0, dmax = 0.0;
    for (int i = 0; i < 8; ++i) {
      double Ad = 0.0;
      for (int j = 0; j < 8; ++j) Ad += W.JtJ[i * 8 + j] * W.d[j];
      dS += W.d[i] * (2.0 * W.v[i] - Ad);
      dv += W.d[i] * W.v[i];
      dmax = fmax(dmax, fabs(W.d[i]));
    }
    const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1.0);
    if (Rs != nullptr && ctx.leader()) Rs[it] = R;
    if (R > 0.75) {
      lambda *= 0.5;
      if (lambda < lc) lambda = 0.0;
    } else if (R < 0.25) {
      double nu = (Sd - S) / (fabs(dv) > DBL_EPSILON ? dv : 1.0) + 2.0;
      nu = fmin(fmax(nu, 2.0), 10.0);
      if (lambda == 0.0) {
        ctx.sync();
        if (ctx.leader()) lm_solve(W, -1.0);
        ctx.sync();
        lambda = lc = 1.0 / fmax(DBL_EPSILON, W.scal[1]);
        nu *= 0.5;
      }
      lambda *= nu;
    }
    ctx.sync();  // every lane has read red, d, v, JtJ
    if (Sd < S) {
      if (ctx.leader())
        for (int i = 0; i < 8; ++i) W.h[i] = W.hd[i];
      ctx.sync();
      ctx.reduce(kLmFull, W.h, W.red);
      if (ctx.leader()) lm_take(W);
      ctx.sync();
      S = W.red[44];
      rmax = W.red[45];
    }
    ++it;
    if (dmax < (double)FLT_EPSILON || rmax < (double)FLT_EPSILON) break;
  }
  *S1 = S;
  return it;
}

// Transfer distance |H x1 - x2| of one correspondence (evaluate_frontend.getInliers); w == 0 divides as numpy does (inf / NaN).
RS_HD double transfer_dist(const double* H, double x1, double y1, double x2, double y2) {
  const double w = H[6] * x1 + H[7] * y1 + H[8];
  const double dx = (H[0] * x1 + H[1] * y1 + H[2]) / w - x2, dy = (H[3] * x1 + H[4] * y1 + H[5]) / w - y2;
  return sqrt(dx * dx + dy * dy);
}

// Mean distance of the four image corners (0,0), (0,h-1), (w-1,0), (w-1,h-1) warped by two homographies
// (descriptor_evaluation.compute_homography's mean_dist).
RS_HD double corner_mean_dist(const double* He, const double* Hg, int height, int width) {
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = (k >> 1) ? (double)(width - 1) : 0.0, y = (k & 1) ? (double)(height - 1) : 0.0;
    const double we = He[6] * x + He[7] * y + He[8], wg = Hg[6] * x + Hg[7] * y + Hg[8];
    const double dx = (Hg[0] * x + Hg[1] * y + Hg[2]) / wg - (He[0] * x + He[1] * y + He[2]) / we;
    const double dy = (Hg[3] * x + Hg[4] * y + Hg[5]) / wg - (He[3] * x + He[4] * y + He[5]) / we;
    sum += sqrt(dx * dx + dy * dy);
  }
  return sum / 4.0;
}

}  // namespace hg
