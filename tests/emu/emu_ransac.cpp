// Host build of csrc/ransac_math.h (the per-lane arithmetic of the RANSAC estimator) for tests/test_ransac_cpu.py.
// Test infrastructure only: the product never loads it.
#include "ransac_math.h"

namespace {
struct P4 {
  float x, y, z, w;
};
}  // namespace

extern "C" {

// the first `count` raw draws of iteration k's stream
void emu_ransac_stream(unsigned long long seed, int k, int N, int count, int* out) {
  rs::Stream s = rs::stream_of(seed, k);
  for (int i = 0; i < count; ++i) out[i] = rs::draw_index(s, N);
}

// iteration k's sample of the pair `pts` [N,4]; returns 1 (idx filled) or 0 (no sample within the attempts)
int emu_ransac_sample(unsigned long long seed, int k, int N, const float* pts, int* idx) {
  const P4* p = reinterpret_cast<const P4*>(pts);
  auto at = [&](int i) { return p[i]; };
  return rs::draw_sample(seed, k, N, at, idx) ? 1 : 0;
}

// 7-point solve of one sample given in pixels: x1, y1, x2, y2 [7] each; F [27]; returns the number of roots
int emu_ransac_seven_point(const float* x1, const float* y1, const float* x2, const float* y2, double* F) {
  return rs::seven_point(x1, y1, x2, y2, F);
}

int emu_ransac_update_num_iters(double p, double ep, int niters) { return rs::update_num_iters(p, ep, niters); }

// out = (best count, best k, best root, iterations consumed)
void emu_ransac_select(const int* counts, int N, double confidence, int max_iters, int* out) {
  out[0] = rs::select_best(counts, N, confidence, max_iters, &out[1], &out[2], &out[3]);
}

int emu_ransac_is_inlier(const double* F, double x1, double y1, double x2, double y2, double t2) {
  return rs::is_inlier(F, x1, y1, x2, y2, t2) ? 1 : 0;
}
}
