// Host build of csrc/lmeds_math.h (the per-lane arithmetic of the LMedS estimators) for tests/test_lmeds_cpu.py.
// Test infrastructure only: the product never loads it.
#include "lmeds_math.h"

namespace {

// lm::median_of's wavefront on the host: 64 lanes of R registers, the reductions as loops over the lanes.
template <int R>
struct HostWave {
  uint32_t v[64][R];
  template <class F>
  int sum(F f) const {
    int s = 0;
    for (int l = 0; l < 64; ++l) s += f(v[l]);
    return s;
  }
  template <class F>
  int max(F f) const {
    int m = f(v[0]);
    for (int l = 1; l < 64; ++l) {
      const int x = f(v[l]);
      m = x > m ? x : m;
    }
    return m;
  }
};

template <int R>
float median_r(const uint32_t* bits, int N) {
  static HostWave<R> w;  // 16 KiB at R = 64
  for (int l = 0; l < 64; ++l)
    for (int j = 0; j < R; ++j) {
      const int p = 64 * j + l;  // the device's layout: slot j of lane l is correspondence 64 j + l
      w.v[l][j] = p < N ? bits[p] : lm::kPadBits;
    }
  return lm::median_of<R>(w, N);
}

}  // namespace

extern "C" {

int emu_lmeds_regs_for(int N) { return lm::regs_for(N); }

// the median of N fp32 error patterns on the rung the device takes for N, or on the rung `force` (> 0)
float emu_lmeds_median(const uint32_t* bits, int N, int force) {
  switch (force > 0 ? force : lm::regs_for(N)) {
    case 1: return median_r<1>(bits, N);
    case 2: return median_r<2>(bits, N);
    case 4: return median_r<4>(bits, N);
    case 8: return median_r<8>(bits, N);
    case 16: return median_r<16>(bits, N);
    case 32: return median_r<32>(bits, N);
    default: return median_r<64>(bits, N);
  }
}

// fp32-rounded errors of n correspondences: pts [n,4] float pixels under F, q [n,4] double normalised under E
void emu_lmeds_f_errors(const double* F, const float* pts, int n, float* out) {
  for (int i = 0; i < n; ++i) out[i] = lm::err_float(lm::f_error(F, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], pts[4 * i + 3]));
}
void emu_lmeds_e_errors(const double* E, const double* q, int n, float* out) {
  for (int i = 0; i < n; ++i) out[i] = lm::err_float(lm::e_error(E, q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]));
}

double emu_lmeds_sigma(double min_median, int N, int model_points, float* bound) {
  const double s = lm::sigma_of(min_median, N, model_points);
  *bound = lm::inlier_bound(s);
  return s;
}

int emu_lmeds_num_iters(int model_points, double confidence, int max_iters) { return lm::num_iters(model_points, confidence, max_iters); }

// out = (min median, best k, best root, iterations)
void emu_lmeds_select(const double* med, int niters, int roots, double* out) {
  int bk, br, it;
  out[0] = roots == 3 ? lm::select_best<3>(med, niters, &bk, &br, &it) : lm::select_best<10>(med, niters, &bk, &br, &it);
  out[1] = bk;
  out[2] = br;
  out[3] = it;
}
}
