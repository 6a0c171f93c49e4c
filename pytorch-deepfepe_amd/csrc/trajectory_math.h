// trajectory_math.h -- the per-item arithmetic of the KITTI odometry table (csrc/trajectory.hip), written once for the device and
// for the host (tests/emu/emu_trajectory.cpp compiles it with g++).  It restates, in fp64, the published KITTI devkit /
// kitti-odom-eval evaluation on top of the affine products and inverses of odometry_math.h:
//   one segment's error row     E = inv(inv(est_first) est_last) (inv(gt_first) gt_last), r = arccos(clamp((tr E_R - 1) / 2)), t = |E_t|
//   one RPE term                E = inv(inv(gt_i) gt_i+1) (inv(est_i) est_i+1), the same r and t
//   one ATE term                |gt_xyz - est_xyz|^2
//   one step of the path length |gt_xyz,i - gt_xyz,i-1|
//   Umeyama's closed form from the means, sigma_x^2 and the covariance C, with the 3x3 SVD it needs
// Floating-point contraction is off here as in odometry_math.h and for the same reason: the host build computes what the device
// computes, term for term (up to the last place of acos and sqrt in the two math libraries).
//
// The SVD is the symmetric Jacobi iteration on C^T C, applied one-sidedly (Hestenes): every rotation is the one that would zero an
// off-diagonal entry of C^T C, computed from the current columns' Gram entries and applied to the columns of C (and of V) instead
// of to C^T C, so small singular values keep their relative accuracy instead of being read off a squared matrix.  At convergence
// the columns of C V are orthogonal: their norms are the singular values (in no particular order), they themselves are U D.
// No array is indexed at run time; the pairs are template arguments.
#pragma once
#include "odometry_math.h"

namespace traj {

enum Mode { kNone = 0, kScale = 1, kScale7dof = 2, k7dof = 3, k6dof = 4 };  // _lib.TRAJ_MODES, in this order

struct RelErr {
  double cosarg, angle, trans;
};

// (tr R - 1) / 2 clamped to [-1, 1] (a NaN stays a NaN), its arccos, and the length of the translation
ODO_HD RelErr rel_err(const odo::Aff& E) {
  RelErr o;
  const double a = (((E.m[0] + E.m[5]) + E.m[10]) - 1.0) / 2.0;
  o.cosarg = a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a);
  o.angle = acos(o.cosarg);
  o.trans = sqrt((E.m[3] * E.m[3] + E.m[7] * E.m[7]) + E.m[11] * E.m[11]);
  return o;
}

ODO_HD odo::Aff motion(const odo::Aff& from, const odo::Aff& to) { return odo::affine_mul(odo::affine_inv(from), to); }

// the error of the estimated motion first -> last against the ground truth's, as the devkit's segment loop forms it
ODO_HD RelErr segment_err(const odo::Aff& Ef, const odo::Aff& El, const odo::Aff& Gf, const odo::Aff& Gl) {
  const odo::Aff dG = motion(Gf, Gl), dE = motion(Ef, El);
  return rel_err(odo::affine_mul(odo::affine_inv(dE), dG));
}

// row = [first, r / len, t / len, len, len / (0.1 (last - first + 1))]
ODO_HD RelErr segment_row(const odo::Aff& Ef, const odo::Aff& El, const odo::Aff& Gf, const odo::Aff& Gl, int first, int last, double len,
                          double* row) {
  const RelErr e = segment_err(Ef, El, Gf, Gl);
  row[0] = (double)first;
  row[1] = e.angle / len;
  row[2] = e.trans / len;
  row[3] = len;
  row[4] = len / (0.1 * (double)(last - first + 1));
  return e;
}

// the relative pose error of one frame pair: the operands the other way round
ODO_HD RelErr rpe_term(const odo::Aff& E0, const odo::Aff& E1, const odo::Aff& G0, const odo::Aff& G1) {
  const odo::Aff dG = motion(G0, G1), dE = motion(E0, E1);
  return rel_err(odo::affine_mul(odo::affine_inv(dG), dE));
}

ODO_HD double ate_term(const double* E, const double* G) {
  const double dx = G[3] - E[3], dy = G[7] - E[7], dz = G[11] - E[11];
  return (dx * dx + dy * dy) + dz * dz;
}

ODO_HD double step_len(const double* G0, const double* G1) {
  const double dx = G1[3] - G0[3], dy = G1[7] - G0[7], dz = G1[11] - G0[11];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

ODO_HD double det3(const double* a) {
  return (a[0] * (a[4] * a[8] - a[5] * a[7]) + a[1] * (a[5] * a[6] - a[3] * a[8])) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}

// One Jacobi rotation of columns P, Q of a (row-major 3x3) and of v.  Returns whether it rotated.
template <int P, int Q>
ODO_HD bool jacobi_pair(double* a, double* v) {
  const double alpha = (a[P] * a[P] + a[3 + P] * a[3 + P]) + a[6 + P] * a[6 + P];
  const double beta = (a[Q] * a[Q] + a[3 + Q] * a[3 + Q]) + a[6 + Q] * a[6 + Q];
  const double gamma = (a[P] * a[Q] + a[3 + P] * a[3 + Q]) + a[6 + P] * a[6 + Q];
  if (!(fabs(gamma) > 2.220446049250313e-16 * sqrt(alpha * beta))) return false;  // orthogonal to working precision (or NaN)
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double ap = a[3 * i + P], aq = a[3 * i + Q];
    a[3 * i + P] = c * ap - s * aq;
    a[3 * i + Q] = s * ap + c * aq;
    const double vp = v[3 * i + P], vq = v[3 * i + Q];
    v[3 * i + P] = c * vp - s * vq;
    v[3 * i + Q] = s * vp + c * vq;
  }
  return true;
}

struct Svd3 {
  double u[9], d[3], v[9];  // C = U diag(d) V^T, row-major; d is not sorted
  int k;                    // the column of the smallest singular value
};

// The column K of U as the cross product of the other two, signed to agree with the column of C V it stands for (a zero one: +).
template <int K>
ODO_HD void complete_column(double* u, const double* a) {
  constexpr int I = (K + 1) % 3, J = (K + 2) % 3;
  const double x = u[3 + I] * u[6 + J] - u[6 + I] * u[3 + J];
  const double y = u[6 + I] * u[J] - u[I] * u[6 + J];
  const double z = u[I] * u[3 + J] - u[3 + I] * u[J];
  const double sg = ((x * a[K] + y * a[3 + K]) + z * a[6 + K]) < 0.0 ? -1.0 : 1.0;
  u[K] = sg * x;
  u[3 + K] = sg * y;
  u[6 + K] = sg * z;
}

// The columns of U are those of C V over their norms, except the one of the smallest singular value: a planar trajectory gives a
// C of rank 2, whose third column of C V is zero (or rounding noise) and has no direction to normalise, while Umeyama's rotation
// is still determined.  That column is the cross product of the other two (which it is, up to its sign, for every C), so U is
// orthogonal whenever two singular values are not negligible.  With two negligible ones (a collinear trajectory) the columns are
// 0 / 0 or noise: r is undetermined there.
ODO_HD Svd3 svd3(const double* C) {
  Svd3 o;
  double a[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    a[k] = C[k];
    o.v[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 30; ++sweep) {  // a 3x3 converges in four or five sweeps; the cap only bounds a pathological input
    bool r = jacobi_pair<0, 1>(a, o.v);
    r = jacobi_pair<0, 2>(a, o.v) || r;
    r = jacobi_pair<1, 2>(a, o.v) || r;
    if (!r) break;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    o.d[j] = sqrt((a[j] * a[j] + a[3 + j] * a[3 + j]) + a[6 + j] * a[6 + j]);
#pragma unroll
    for (int i = 0; i < 3; ++i) o.u[3 * i + j] = a[3 * i + j] / o.d[j];
  }
  o.k = (o.d[2] <= o.d[0] && o.d[2] <= o.d[1]) ? 2 : ((o.d[1] <= o.d[0]) ? 1 : 0);
  if (o.k == 0) complete_column<0>(o.u, a);
  else if (o.k == 1) complete_column<1>(o.u, a);
  else complete_column<2>(o.u, a);
  return o;
}

struct Sim {
  double r[9], t[3], c;
};

ODO_HD Sim identity_sim() {
  Sim o;
#pragma unroll
  for (int k = 0; k < 9; ++k) o.r[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
  o.t[0] = o.t[1] = o.t[2] = 0.0;
  o.c = 1.0;
  return o;
}

// Umeyama from the means mx, my, sigma_x^2 = sx and C = (1/m) sum (y - my)(x - mx)^T: C = U D V^T, S = diag(1, 1, -1) when
// det(U) det(V^T) < 0 (the -1 on the smallest singular value), r = U S V^T, c = tr(D S) / sx (1 without scale), t = my - c r mx.
// sx = 0 gives the IEEE result of the formula; nothing is trapped.
ODO_HD Sim umeyama(const double* mx, const double* my, double sx, const double* C, bool with_scale) {
  const Svd3 f = svd3(C);
  const bool flip = det3(f.u) * det3(f.v) < 0.0;
  const int k = f.k;
  const double s0 = (flip && k == 0) ? -1.0 : 1.0, s1 = (flip && k == 1) ? -1.0 : 1.0, s2 = (flip && k == 2) ? -1.0 : 1.0;
  Sim o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int l = 0; l < 3; ++l)
      o.r[3 * i + l] = (s0 * (f.u[3 * i] * f.v[3 * l]) + s1 * (f.u[3 * i + 1] * f.v[3 * l + 1])) + s2 * (f.u[3 * i + 2] * f.v[3 * l + 2]);
  }
  o.c = with_scale ? ((s0 * f.d[0] + s1 * f.d[1]) + s2 * f.d[2]) / sx : 1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) o.t[i] = my[i] - o.c * ((o.r[3 * i] * mx[0] + o.r[3 * i + 1] * mx[1]) + o.r[3 * i + 2] * mx[2]);
  return o;
}

// the aligned pose: the translation times c, then (7dof, 6dof) the whole pose multiplied from the left by [r | t]
ODO_HD odo::Aff apply_sim(const odo::Aff& P, const Sim& s, bool rigid_part) {
  odo::Aff e = P;
  e.m[3] = e.m[3] * s.c;
  e.m[7] = e.m[7] * s.c;
  e.m[11] = e.m[11] * s.c;
  if (!rigid_part) return e;
  odo::Aff T;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) T.m[4 * i + j] = s.r[3 * i + j];
    T.m[4 * i + 3] = s.t[i];
  }
  return odo::affine_mul(T, e);
}

}  // namespace traj
