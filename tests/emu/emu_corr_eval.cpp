// Host build of csrc/corr_eval_math.h: the two launches of csrc/corr_eval.hip as plain loops with the arguments of the C ABI
// (include/dfepe.h) minus the stream, the refusals included.  tests/test_corr_eval_ref_cpu.py compiles it with g++ into a shared
// object, calls it through ctypes and holds the output to the same check() as the GPU.  The counts are integers, so walking the
// rows in index order gives what the kernel's per-wavefront ballots give; the mean adds the pairs in the kernel's order.
#include <cstddef>

#include "corr_eval_math.h"

extern "C" int emu_inlier_table(const float* matches, const double* F, const float* dist, const float* scores, const int* n_valid, int B,
                                int N, const double* inlier_thds, int Ti, const double* mask_thds, int Tm, int* cnt, int* num, double* ratio,
                                float* dist_out) {
  if (B < 0 || N < 0 || Ti < 1 || Ti > ce::kMaxThds || Tm < 1 || Tm > ce::kMaxThds) return -1;
  if (matches != nullptr && dist != nullptr) return -1;
  if (scores == nullptr && Tm != 1) return -1;
  if (B == 0) return 0;
  if (N > 0 && matches == nullptr && dist == nullptr) return -1;
  if (matches != nullptr && F == nullptr) return -1;
  if (!inlier_thds || (scores != nullptr && !mask_thds)) return -1;
  if (!cnt && !num && !ratio && !dist_out) return -1;
  for (size_t pair = 0; pair < (size_t)B; ++pair) {
    int n = N;
    if (n_valid != nullptr) {
      const int v = n_valid[pair];
      n = v < 0 ? 0 : (v > N ? N : v);
    }
    int tab[ce::kMaxThds][ce::kMaxThds + 1] = {};
    for (int i = 0; i < N; ++i) {
      const size_t at = pair * (size_t)N + i;
      if (i >= n) {
        if (dist_out != nullptr) dist_out[at] = 0.0f;
        continue;
      }
      double d;
      if (matches != nullptr) {
        const float* m = matches + at * 4;
        d = ce::epi_dist3(F + pair * 9, (double)m[0], (double)m[1], (double)m[2], (double)m[3]);
      } else {
        d = (double)dist[at];
      }
      const double s = (scores != nullptr) ? (double)scores[at] : 0.0;
      if (dist_out != nullptr) dist_out[at] = (float)d;
      for (int m = 0; m < Tm; ++m) {
        if (scores != nullptr && !ce::kept(s, mask_thds[m])) continue;
        ++tab[m][0];
        for (int t = 0; t < Ti; ++t) tab[m][1 + t] += ce::inlier(d, inlier_thds[t]) ? 1 : 0;
      }
    }
    for (int m = 0; m < Tm; ++m) {
      if (num != nullptr) num[pair * Tm + m] = tab[m][0];
      for (int t = 0; t < Ti; ++t) {
        const size_t o = (pair * Tm + m) * (size_t)Ti + t;
        if (cnt != nullptr) cnt[o] = tab[m][1 + t];
        if (ratio != nullptr) ratio[o] = ce::ratio_of(tab[m][1 + t], tab[m][0]);
      }
    }
  }
  return 0;
}

extern "C" int emu_inlier_table_mean(const double* ratio, const int* num, int B, int Tm, int Ti, double* mean, int* num_T) {
  if (B < 0 || Ti < 1 || Ti > ce::kMaxThds || Tm < 1 || Tm > ce::kMaxThds) return -1;
  if (!mean && !num_T) return -1;
  if (B > 0 && ((mean != nullptr && !ratio) || (num_T != nullptr && !num))) return -1;
  const int cells = Tm * Ti;
  if (mean != nullptr) {
    for (int c = 0; c < cells; ++c) mean[c] = ce::mean_of(ratio + c, cells, B);
  }
  if (num_T != nullptr) {
    for (int m = 0; m < Tm; ++m) {
      for (int b = 0; b < B; ++b) num_T[(size_t)m * B + b] = num[(size_t)b * Tm + m];
    }
  }
  return 0;
}
