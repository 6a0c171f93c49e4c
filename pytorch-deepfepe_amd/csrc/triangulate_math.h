// triangulate_math.h -- per-lane arithmetic of the two-view structure kernels (csrc/triangulate.hip): the DLT triangulation of
// one correspondence (cv2.triangulatePoints), the point, its two depths, and the projection of a point into an image.  Written
// once for the device and for the host (tests/emu/emu_triangulate.cpp compiles it with g++); the contract is spelled out in
// include/dfepe.h.  Everything is fp64 from the fp32 inputs and a pure function of its arguments: no LDS, no wavefront operation,
// and no array that is indexed at run time (every loop over an array is fully unrolled), so the device code stays in registers.
//
// The null vector.  The cheirality kernels (cheirality_body.h) take the smallest eigenvector of the normal matrix A^T A from an
// fp32 stage and one fp64 Rayleigh-quotient iteration: enough for their sign decisions, not for values (one iteration leaves
// 1e-9 .. 1e-7, and on a short baseline the fp32 stage cannot tell the two smallest eigenvalues apart at all).  Here the vector
// is the last right singular vector of the 4x4 matrix A ITSELF, by the one-sided Jacobi method (Hestenes): plane rotations of
// column pairs (p, q) of A, accumulated in V, until all columns are orthogonal to working precision; the columns of A V are then
// the left singular vectors times the singular values, and the column of V that belongs to the shortest one is the null vector.
// A^T A is never formed, so the vector's error is that of a backward-stable SVD of A (a few 2^-53 s1 / gap), not that of an
// eigenvector of a rounded normal matrix; there is no start vector and no shift to get wrong; every quantity that decides a
// rotation is a ratio of same-degree products of entries of A, so scaling both cameras by a power of two changes no bit.
// Cost: at most six rotations per sweep, 3 to 6 sweeps on the tests' families (quadratic convergence; the last sweep only finds
// every pair orthogonal), 12 to 25 rotations per correspondence, ~150 fp64 instructions each.
#pragma once
#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define TRI_HD __host__ __device__ inline
#else
#define TRI_HD inline
#endif

namespace tri {

constexpr unsigned kCameraMotion = 1u;  // DFEPE_POSE_CAMERA_MOTION
constexpr int kMaxSweeps = 30;          // the tests' families need <= 6; a bound, so that no input can spin a lane
// a column pair is orthogonal when |a_p . a_q| <= 2^-51 |a_p| |a_q| (LAPACK's dgesvj: sqrt(m) eps); compared squared
constexpr double kOrth2 = 0x1p-102;

TRI_HD bool finite(double x) { return fabs(x) <= DBL_MAX; }
TRI_HD double qnan() { return __builtin_nan(""); }

// Unit 2-norm null vector X (w = X[3] >= 0) of A = [x1 P1_3 - P1_1; y1 P1_3 - P1_2; x2 P2_3 - P2_1; y2 P2_3 - P2_2].
// P1, P2: 3x4 row-major.  false (X untouched) when an entry of A is not finite or A = 0.
TRI_HD bool null_vector(const double* P1, const double* P2, double x1, double y1, double x2, double y2, double* X) {
  double a[4][4], v[4][4];  // a[c]: column c of A (then of A V), v[c]: column c of V
  double sum = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    a[c][0] = x1 * P1[8 + c] - P1[c];
    a[c][1] = y1 * P1[8 + c] - P1[4 + c];
    a[c][2] = x2 * P2[8 + c] - P2[c];
    a[c][3] = y2 * P2[8 + c] - P2[4 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sum += fabs(a[c][r]);
      v[c][r] = (r == c) ? 1.0 : 0.0;
    }
  }
  if (!finite(sum) || sum == 0.0) return false;
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          alpha += a[p][r] * a[p][r];
          beta += a[q][r] * a[q][r];
          gamma += a[p][r] * a[q][r];
        }
        if (gamma * gamma > kOrth2 * alpha * beta) {
          rotated = true;
          // tan of the smaller rotation angle; a huge zeta (gamma tiny) gives t = 0 and the identity
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double ap = a[p][r], aq = a[q][r], vp = v[p][r], vq = v[q][r];
            a[p][r] = cs * ap - sn * aq;
            a[q][r] = sn * ap + cs * aq;
            v[p][r] = cs * vp - sn * vq;
            v[q][r] = sn * vp + cs * vq;
          }
        }
      }
    }
    if (!rotated) break;
  }
  // the column of the smallest singular value (first minimum), by selects: no run-time index
  double best = a[0][0] * a[0][0] + a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3];
  double x[4] = {v[0][0], v[0][1], v[0][2], v[0][3]};
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    const double n = a[c][0] * a[c][0] + a[c][1] * a[c][1] + a[c][2] * a[c][2] + a[c][3] * a[c][3];
    const bool take = n < best;
    best = take ? n : best;
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = take ? v[c][r] : x[r];
  }
  const double inv = 1.0 / sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
  const double sg = (x[3] < 0.0) ? -inv : inv;
#pragma unroll
  for (int r = 0; r < 4; ++r) X[r] = x[r] * sg;
  return true;
}

// Rt [3,4] fp32 -> scene motion (R [9], t [3]) in fp64: Rt itself, or with kCameraMotion its inverse R = Rc^T, t = -Rc^T tc
// (utils_misc._inv_Rt).
TRI_HD void scene_motion(const float* Rt, unsigned flags, double* R, double* t) {
  if (flags & kCameraMotion) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)Rt[4 * c + r];
      t[r] = -((double)Rt[r] * (double)Rt[3] + (double)Rt[4 + r] * (double)Rt[7] + (double)Rt[8 + r] * (double)Rt[11]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)Rt[4 * r + c];
      t[r] = (double)Rt[4 * r + 3];
    }
  }
}

// P1 = K [I | 0], P2 = K [R | t]
TRI_HD void cameras(const float* K, const double* R, const double* t, double* P1, double* P2) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double k0 = (double)K[3 * r], k1 = (double)K[3 * r + 1], k2 = (double)K[3 * r + 2];
    P1[4 * r] = k0; P1[4 * r + 1] = k1; P1[4 * r + 2] = k2; P1[4 * r + 3] = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) P2[4 * r + c] = k0 * R[c] + k1 * R[3 + c] + k2 * R[6 + c];
    P2[4 * r + 3] = k0 * t[0] + k1 * t[1] + k2 * t[2];
  }
}

TRI_HD double clamp_keep_nan(double z, double lim) { return (z > lim) ? lim : ((z < -lim) ? -lim : z); }

struct Structure {
  double X[3], z1, z2;
};

// The point of one correspondence in the frame of camera 1 and its depths in both cameras: X = Xh[:3] / w, z1 = X[2],
// z2 = (R X + t)[2], all times `scale`; the depths then clamped to [-clamp, clamp] when clamp > 0 (NaN stays NaN).  w = 0 gives
// what the division gives.  A correspondence without a null vector (null_vector() false) gives NaN.
TRI_HD Structure structure(const double* P1, const double* P2, const double* R, const double* t, double x1, double y1, double x2,
                           double y2, double scale, double clamp) {
  Structure s;
  double Xh[4];
  if (!null_vector(P1, P2, x1, y1, x2, y2, Xh)) {
    s.X[0] = s.X[1] = s.X[2] = s.z1 = s.z2 = qnan();
    return s;
  }
  const double X0 = Xh[0] / Xh[3], X1 = Xh[1] / Xh[3], X2 = Xh[2] / Xh[3];
  const double z2 = R[6] * X0 + R[7] * X1 + R[8] * X2 + t[2];
  s.X[0] = X0 * scale; s.X[1] = X1 * scale; s.X[2] = X2 * scale;
  s.z1 = X2 * scale;
  s.z2 = z2 * scale;
  if (clamp > 0.0) { s.z1 = clamp_keep_nan(s.z1, clamp); s.z2 = clamp_keep_nan(s.z2, clamp); }
  return s;
}

// u = K (R X + t): the image point is (u[0] / u[2], u[1] / u[2]) and its depth u[2]
TRI_HD void project(const float* K, const double* R, const double* t, double X0, double X1, double X2, double* u) {
  double c[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) c[r] = R[3 * r] * X0 + R[3 * r + 1] * X1 + R[3 * r + 2] * X2 + t[r];
#pragma unroll
  for (int r = 0; r < 3; ++r) u[r] = (double)K[3 * r] * c[0] + (double)K[3 * r + 1] * c[1] + (double)K[3 * r + 2] * c[2];
}

// utils_misc.within on the fp32 values that are written: NaN is outside
TRI_HD bool within(float x, float y, float xlim, float ylim) { return (x >= 0.0f) && (y >= 0.0f) && (x <= xlim) && (y <= ylim); }

}  // namespace tri
