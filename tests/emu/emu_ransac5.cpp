// Host build of csrc/ransac5_math.h (the per-lane arithmetic of the five-point RANSAC estimator) for tests/test_ransac5_cpu.py.
// Test infrastructure only: the product never loads it.
#include "ransac5_math.h"

extern "C" {

// iteration k's five indices
void emu_ransac5_sample(unsigned long long seed, int k, int N, int* idx) { r5::draw_sample(seed, k, N, idx); }

// pixels [n,4] and K [9] (float) -> normalised coordinates q [n,4] (double); returns the squared threshold in normalised units
double emu_ransac5_normalize(const float* pts, const float* K, int n, double threshold, double* q) {
  const r5::Cam cam = r5::cam_of(K);
  for (int i = 0; i < n; ++i) {
    q[4 * i] = r5::norm_x(cam, pts[4 * i]);
    q[4 * i + 1] = r5::norm_y(cam, pts[4 * i + 1]);
    q[4 * i + 2] = r5::norm_x(cam, pts[4 * i + 2]);
    q[4 * i + 3] = r5::norm_y(cam, pts[4 * i + 3]);
  }
  return r5::threshold2(cam, threshold);
}

// five-point solve of one sample in normalised coordinates q [5,4]; E [90]; returns the number of solutions
int emu_ransac5_five_point(const double* q, double* E) {
  double w[r5::kWork];
  double x1[5], y1[5], x2[5], y2[5];
  for (int i = 0; i < 5; ++i) { x1[i] = q[4 * i]; y1[i] = q[4 * i + 1]; x2[i] = q[4 * i + 2]; y2[i] = q[4 * i + 3]; }
  double* wp = w;
  const int n = r5::five_point(wp, x1, y1, x2, y2);
  for (int j = 0; j < 9 * n; ++j) E[j] = w[r5::kOffE + j];
  return n;
}

int emu_ransac5_update_num_iters(double p, double ep, int niters) { return r5::update_num_iters(p, ep, niters); }

// out = (best count, best k, best root, iterations consumed)
void emu_ransac5_select(const int* counts, int N, double confidence, int max_iters, int* out) {
  out[0] = r5::select_best(counts, N, confidence, max_iters, &out[1], &out[2], &out[3]);
}

// decisions of n correspondences q [n,4] for one E
void emu_ransac5_is_inlier(const double* E, const double* q, int n, double t2, unsigned char* out) {
  for (int i = 0; i < n; ++i) out[i] = r5::is_inlier(E, q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3], t2) ? 1 : 0;
}
}
