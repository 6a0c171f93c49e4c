// Host build of csrc/triangulate_math.h (the per-lane arithmetic of dfepe_triangulate, dfepe_two_view_structure and
// dfepe_reproject) for tests/test_triangulate_ref_cpu.py: the loops below are the kernels of csrc/triangulate.hip with the lane
// index as loop variable, the outputs rounded to float as the kernels round them.  Test infrastructure only: the product never
// loads it.
#include "triangulate_math.h"

extern "C" {

int emu_max_sweeps() { return tri::kMaxSweeps; }

// n correspondences under one pair of cameras: P1, P2 [12], matches [n,4], Xh [n,4]
void emu_triangulate(const float* P1, const float* P2, const float* matches, int n, float* Xh) {
  double A[12], B[12];
  for (int k = 0; k < 12; ++k) { A[k] = (double)P1[k]; B[k] = (double)P2[k]; }
  for (int i = 0; i < n; ++i) {
    const float* m = matches + 4 * (long)i;
    double X[4];
    const bool ok = tri::null_vector(A, B, (double)m[0], (double)m[1], (double)m[2], (double)m[3], X);
    for (int k = 0; k < 4; ++k) Xh[4 * (long)i + k] = ok ? (float)X[k] : __builtin_nanf("");
  }
}

// one pair: Rt [12], K [9], matches [n,4], winner (< 0: no pose), scale (has_scale), clamp; X [n,3], z1, z2 [n]
void emu_two_view_structure(const float* Rt, unsigned flags, const float* K, const float* matches, int n, int winner, int has_scale,
                            float scale, float clamp, float* X, float* z1, float* z2) {
  for (int i = 0; i < n; ++i) {
    tri::Structure s;
    s.X[0] = s.X[1] = s.X[2] = s.z1 = s.z2 = tri::qnan();
    if (winner >= 0) {
      double R[9], t[3], P1[12], P2[12];
      tri::scene_motion(Rt, flags, R, t);
      tri::cameras(K, R, t, P1, P2);
      const float* m = matches + 4 * (long)i;
      s = tri::structure(P1, P2, R, t, (double)m[0], (double)m[1], (double)m[2], (double)m[3], has_scale ? (double)scale : 1.0,
                         (double)clamp);
    }
    for (int k = 0; k < 3; ++k) X[3 * (long)i + k] = (float)s.X[k];
    z1[i] = (float)s.z1;
    z2[i] = (float)s.z2;
  }
}

// one pair: X [n,3], Rt [12], K [9]; x [n,2], z [n], inside [n]
void emu_reproject(const float* X, const float* Rt, unsigned flags, const float* K, int n, float image_w, float image_h, float* x,
                   float* z, unsigned char* inside) {
  double R[9], t[3];
  tri::scene_motion(Rt, flags, R, t);
  for (int i = 0; i < n; ++i) {
    double u[3];
    tri::project(K, R, t, (double)X[3 * (long)i], (double)X[3 * (long)i + 1], (double)X[3 * (long)i + 2], u);
    const float xf = (float)(u[0] / u[2]), yf = (float)(u[1] / u[2]);
    x[2 * (long)i] = xf;
    x[2 * (long)i + 1] = yf;
    z[i] = (float)u[2];
    inside[i] = tri::within(xf, yf, image_w, image_h) ? 1 : 0;
  }
}
}
