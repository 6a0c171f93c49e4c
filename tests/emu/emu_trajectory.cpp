// Host build of csrc/trajectory_math.h (the per-item arithmetic of dfepe_trajectory_align and dfepe_kitti_odometry_errors) for
// tests/test_kitti_odom_ref_cpu.py: one segment row, one RPE term, one ATE term, one step of the path length, the 3x3 SVD and
// Umeyama's closed form, each for an array of items.  Test infrastructure only: the product never loads it.
#include "trajectory_math.h"

extern "C" {

// k segments: poses [k,12] each, first / last [k], len [k] -> rows [k,5], cosarg / angle / trans [k] (before the division by len)
void emu_segment_rows(const double* ef, const double* el, const double* gf, const double* gl, const int* first, const int* last,
                      const double* len, int k, double* rows, double* cosarg, double* angle, double* trans) {
  for (int i = 0; i < k; ++i) {
    const traj::RelErr e = traj::segment_row(odo::load(ef + 12L * i), odo::load(el + 12L * i), odo::load(gf + 12L * i),
                                             odo::load(gl + 12L * i), first[i], last[i], len[i], rows + 5L * i);
    cosarg[i] = e.cosarg;
    angle[i] = e.angle;
    trans[i] = e.trans;
  }
}

// est, gt [m,12]: the m - 1 RPE terms and the m ATE terms; step [m] with step[0] = 0
void emu_frame_terms(const double* est, const double* gt, int m, double* cosarg, double* angle, double* trans, double* ate_sq,
                     double* step) {
  for (int i = 0; i < m; ++i) {
    ate_sq[i] = traj::ate_term(est + 12L * i, gt + 12L * i);
    step[i] = i > 0 ? traj::step_len(gt + 12L * (i - 1), gt + 12L * i) : 0.0;
    if (i + 1 < m) {
      const traj::RelErr e = traj::rpe_term(odo::load(est + 12L * i), odo::load(est + 12L * (i + 1)), odo::load(gt + 12L * i),
                                            odo::load(gt + 12L * (i + 1)));
      cosarg[i] = e.cosarg;
      angle[i] = e.angle;
      trans[i] = e.trans;
    }
  }
}

// C [9] -> u [9], d [3], v [9]
void emu_svd3(const double* C, double* u, double* d, double* v) {
  const traj::Svd3 f = traj::svd3(C);
  for (int k = 0; k < 9; ++k) {
    u[k] = f.u[k];
    v[k] = f.v[k];
  }
  for (int k = 0; k < 3; ++k) d[k] = f.d[k];
}

// -> rtc [13]: r, t, c
void emu_umeyama(const double* mx, const double* my, double sx, const double* C, int with_scale, double* rtc) {
  const traj::Sim s = traj::umeyama(mx, my, sx, C, with_scale != 0);
  for (int k = 0; k < 9; ++k) rtc[k] = s.r[k];
  for (int k = 0; k < 3; ++k) rtc[9 + k] = s.t[k];
  rtc[12] = s.c;
}

// poses [k,12] -> the aligned poses
void emu_apply_sim(const double* poses, int k, const double* rtc, int rigid_part, double* out) {
  traj::Sim s;
  for (int j = 0; j < 9; ++j) s.r[j] = rtc[j];
  for (int j = 0; j < 3; ++j) s.t[j] = rtc[9 + j];
  s.c = rtc[12];
  for (int i = 0; i < k; ++i) odo::store(out + 12L * i, traj::apply_sim(odo::load(poses + 12L * i), s, rigid_part != 0));
}
}
