// Host build of csrc/correct_matches_math.h (the per-lane arithmetic of dfepe_correct_matches) for
// tests/test_correct_matches_cpu.py.  Test infrastructure only: the product never loads it.
#include "correct_matches_math.h"

extern "C" {

int emu_correct_matches_max_candidates() { return cm::kMaxCand; }

// n points under one F [9]: p, q [n,2] as the kernel reads them (float); out [n,5] = corrected p, corrected q, cost, all fp64
// (before the kernel's rounding to float); cand [n, kMaxCand] the values of t that were evaluated (inf: t = infinity), ncand [n].
void emu_correct_matches(const double* F, const float* p, const float* q, int n, double* out, double* cand, int* ncand) {
  for (int i = 0; i < n; ++i) {
    const cm::Result r = cm::correct<true>(F, (double)p[2 * i], (double)p[2 * i + 1], (double)q[2 * i], (double)q[2 * i + 1],
                                           cand + (long)i * cm::kMaxCand, ncand + i);
    out[5 * i] = r.x1; out[5 * i + 1] = r.y1; out[5 * i + 2] = r.x2; out[5 * i + 3] = r.y2; out[5 * i + 4] = r.cost;
  }
}
}
