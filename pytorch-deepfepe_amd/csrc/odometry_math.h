// odometry_math.h -- the arithmetic of the odometry evaluation (csrc/odometry.hip), written once for the device and for the host
// (tests/emu/emu_odometry.cpp compiles it with g++).  It restates, in fp64, what the reference does on the host with numpy:
//   relative_pose_cam_to_body   Train_model_pipeline.py:1098-1108   inv(C) @ M @ C
//   get_abs_poses               deepFEPE/utils/eval_tools.py:268-284 last = pose @ last; abs.append(inv(last)[:3])
//   compensate_poses            eval_tools.py:252-265
//   compute_pose_error          eval_tools.py:309-331
//   pose_seq_ate                eval_tools.py:334-375                (one window of it: odo::snippet)
// A pose is a 3x4 affine map, row-major, with the implied last row (0, 0, 0, 1).
//
// Every expression below is written with its association spelled out, and floating-point contraction is switched off for the
// translation unit that includes this header: a product and the sum it feeds are two roundings on the device as on the host.
// The kernels therefore compute, for a given association order of the chain, exactly what the host build of this header
// computes, and tests/odometry_ref.py can restate the same operations in numpy term for term.  (The work is latency-sized; the
// lost fused multiply-adds cost nothing that can be measured.)
//
// No array here is indexed at run time except through the caller's pointers, and every loop over a pose is fully unrolled, so
// the device code keeps the poses in registers.
#pragma once
#include <math.h>

#pragma STDC FP_CONTRACT OFF

#if defined(__HIPCC__)
#define ODO_HD __host__ __device__ inline
#else
#define ODO_HD inline
#endif

namespace odo {

struct Aff {
  double m[12];
};

ODO_HD Aff identity() {
  Aff r;
#pragma unroll
  for (int k = 0; k < 12; ++k) r.m[k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
  return r;
}

ODO_HD Aff load(const double* p) {
  Aff r;
#pragma unroll
  for (int k = 0; k < 12; ++k) r.m[k] = p[k];
  return r;
}

ODO_HD void store(double* p, const Aff& a) {
#pragma unroll
  for (int k = 0; k < 12; ++k) p[k] = a.m[k];
}

// A . B of two affine maps: r_ij = (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j, and + a_i3 for the translation column.  With the identity
// on either side the result is the other operand bit for bit (finite entries).
ODO_HD Aff affine_mul(const Aff& A, const Aff& B) {
  Aff r;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = (A.m[4 * i] * B.m[j] + A.m[4 * i + 1] * B.m[4 + j]) + A.m[4 * i + 2] * B.m[8 + j];
      if (j == 3) v = v + A.m[4 * i + 3];
      r.m[4 * i + j] = v;
    }
  }
  return r;
}

// General inverse of a 3x3 (row-major a[9] -> inv[9]): adjugate over determinant, one division per entry.  Not the transpose:
// the reference calls numpy.linalg.inv, and its inputs are rotations only to float32.  A singular input gives inf / NaN.
ODO_HD void inv3(const double* a, double* inv) {
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[2] * a[7] - a[1] * a[8], c02 = a[1] * a[5] - a[2] * a[4];
  const double c10 = a[5] * a[6] - a[3] * a[8], c11 = a[0] * a[8] - a[2] * a[6], c12 = a[2] * a[3] - a[0] * a[5];
  const double c20 = a[3] * a[7] - a[4] * a[6], c21 = a[1] * a[6] - a[0] * a[7], c22 = a[0] * a[4] - a[1] * a[3];
  const double det = (a[0] * c00 + a[1] * c10) + a[2] * c20;
  inv[0] = c00 / det; inv[1] = c01 / det; inv[2] = c02 / det;
  inv[3] = c10 / det; inv[4] = c11 / det; inv[5] = c12 / det;
  inv[6] = c20 / det; inv[7] = c21 / det; inv[8] = c22 / det;
}

// inv([A | t]) = [A^-1 | -(A^-1 t)]
ODO_HD Aff affine_inv(const Aff& A) {
  double a[9], ai[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a[3 * i + j] = A.m[4 * i + j];
  }
  inv3(a, ai);
  Aff r;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) r.m[4 * i + j] = ai[3 * i + j];
    r.m[4 * i + 3] = -((ai[3 * i] * A.m[3] + ai[3 * i + 1] * A.m[7]) + ai[3 * i + 2] * A.m[11]);
  }
  return r;
}

// relative_pose_cam_to_body: inv(C) @ M @ C, evaluated left to right as numpy does.
ODO_HD Aff conjugate(const Aff& M, const Aff& C) { return affine_mul(affine_mul(affine_inv(C), M), C); }

// One column of compensate_poses: Rinv (q), the 3x3 inverse of the first pose applied to a column.
ODO_HD void comp_col(const double* Rinv, double q0, double q1, double q2, double* o0, double* o1, double* o2) {
  *o0 = (Rinv[0] * q0 + Rinv[1] * q1) + Rinv[2] * q2;
  *o1 = (Rinv[3] * q0 + Rinv[4] * q1) + Rinv[5] * q2;
  *o2 = (Rinv[6] * q0 + Rinv[7] * q1) + Rinv[8] * q2;
}

// One pose of compensate_poses: the first pose's translation t0 is subtracted from the translation, then all four columns are
// multiplied from the left by Rinv.  (The reference subtracts in place through a view of the first pose; numpy buffers the
// overlapping operand, so every pose, the first included, loses the original t0.)
ODO_HD Aff compensate_pose(const double* P, const double* Rinv, const double* t0) {
  Aff r;
#pragma unroll
  for (int j = 0; j < 3; ++j) comp_col(Rinv, P[j], P[4 + j], P[8 + j], &r.m[j], &r.m[4 + j], &r.m[8 + j]);
  comp_col(Rinv, P[3] - t0[0], P[7] - t0[1], P[11] - t0[2], &r.m[3], &r.m[7], &r.m[11]);
  return r;
}

ODO_HD void compensate_t(const double* P, const double* Rinv, const double* t0, double* t) {
  comp_col(Rinv, P[3] - t0[0], P[7] - t0[1], P[11] - t0[2], &t[0], &t[1], &t[2]);
}

struct Snippet {
  double ate, re, scale;
};

// One window of pose_seq_ate: est, gt point at the window's first pose (L poses of 12 doubles each).  pose_seq_ate calls
// compute_pose_error(est_snip, gt_snip), whose parameters are named (gt, pred): the function's "gt" is the ESTIMATE and its
// "pred" the GROUND TRUTH, so
//   scale = sum(est_t . gt_t) / sum(gt_t^2),  ATE = |est_t - scale gt_t| / L,
//   RE = (sum_i atan2(|(R01 - R10, R12 - R21, R02 - R20)|, tr R - 1)) / L  with  R = est_R inv(gt_R).
// Sums run over the poses in order and over x, y, z within a pose.  Ground-truth translations that are all zero give 0 / 0 or
// x / 0 exactly as numpy does; nothing is trapped.  With comp_out != nullptr the compensated estimate [L,12] is stored there.
ODO_HD Snippet snippet(const double* est, const double* gt, int L, bool compensate, double* comp_out) {
  double Re[9], Rg[9], te[3], tg[3];
  if (compensate) {
    double a[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) a[3 * i + j] = est[4 * i + j];
      te[i] = est[4 * i + 3];
    }
    inv3(a, Re);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) a[3 * i + j] = gt[4 * i + j];
      tg[i] = gt[4 * i + 3];
    }
    inv3(a, Rg);
  }
  double num = 0.0, den = 0.0, re = 0.0;
  for (int i = 0; i < L; ++i) {
    const Aff E = compensate ? compensate_pose(est + 12 * i, Re, te) : load(est + 12 * i);
    const Aff G = compensate ? compensate_pose(gt + 12 * i, Rg, tg) : load(gt + 12 * i);
    if (comp_out != nullptr) store(comp_out + 12 * i, E);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      num = num + E.m[4 * c + 3] * G.m[4 * c + 3];
      den = den + G.m[4 * c + 3] * G.m[4 * c + 3];
    }
    double g[9], gi[9], R[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) g[3 * r + c] = G.m[4 * r + c];
    }
    inv3(g, gi);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * r + c] = (E.m[4 * r] * gi[c] + E.m[4 * r + 1] * gi[3 + c]) + E.m[4 * r + 2] * gi[6 + c];
    }
    const double s0 = R[1] - R[3], s1 = R[5] - R[7], s2 = R[2] - R[6];
    const double s = sqrt((s0 * s0 + s1 * s1) + s2 * s2);
    const double c = ((R[0] + R[4]) + R[8]) - 1.0;
    re = re + atan2(s, c);
  }
  Snippet out;
  out.scale = num / den;
  double sq = 0.0;
  for (int i = 0; i < L; ++i) {
    double e[3], g[3];
    if (compensate) {
      compensate_t(est + 12 * i, Re, te, e);
      compensate_t(gt + 12 * i, Rg, tg, g);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        e[c] = est[12 * i + 4 * c + 3];
        g[c] = gt[12 * i + 4 * c + 3];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double d = e[c] - out.scale * g[c];
      sq = sq + d * d;
    }
  }
  out.ate = sqrt(sq) / (double)L;
  out.re = re / (double)L;
  return out;
}

// The aligned pose of a window: the window's first estimate as given (not compensated), its translation times scale.
ODO_HD Aff aligned_pose(const double* est, double scale) {
  Aff r = load(est);
  r.m[3] = r.m[3] * scale;
  r.m[7] = r.m[7] * scale;
  r.m[11] = r.m[11] * scale;
  return r;
}

}  // namespace odo
