// robust_dev.h -- the device code the RANSAC estimators share (ransac.hip, ransac5.hip, homography.hip): the selection rule a
// wavefront at a time, and the inlier-mask kernel of the two epipolar estimators.  What they share with the host emulation of
// the tests (the rule's definition, the iteration bound, "solve iteration k") is in ransac_math.h and its two descendants.
#pragma once
#include "dfepe_common.h"
#include "ransac_math.h"

// rs::select_best<ROOTS, SAMPLE> (the sequential definition) with one wavefront per pair: the table is read 64 iterations at a
// time, one lane per iteration with its ROOTS counts, and the next model the sequential loop would take -- the first entry, in
// (k, root) order, past the last one taken, of an iteration the loop still reaches, whose count beats max(best, SAMPLE - 1), or
// the first iteration without a sample -- is found by a ballot.  The tests hold each estimator's outputs to its own Python
// restatement of the rule; one lane doing it alone spent ~400 us in dependent global loads (rocprofv3, 8 pairs x 1000
// iterations of the 7-point estimator).
// `k == bk` keeps the iteration being processed reached after its own model has lowered niters to k or below: the sequential
// loop looks at all of its roots.  With ROOTS = 1 that iteration has no entry past `done` = bk left, so reached-and-past-done
// reduces to k < niters && k > bk.
template <int ROOTS, int SAMPLE>
__device__ inline int select_wave(const int* __restrict__ tab, int N, double confidence, int max_iters, int* best_k, int* best_r,
                                  int* iters) {
  const int lane = threadIdx.x & 63;
  int best = 0, niters = max_iters, bk = -1, br = -1, done = -1, stop = -1;  // done: last entry (ROOTS k + r) taken
  for (int base = 0; base < max_iters && stop < 0; base += 64) {
    if (base >= niters) break;  // no iteration from here on is reached (bk < base)
    const int k = base + lane;
    const bool have = k < max_iters;
    int c[ROOTS];
#pragma unroll
    for (int r = 0; r < ROOTS; ++r) c[r] = have ? tab[ROOTS * k + r] : rs::kNoRoot;
    for (;;) {
      const int thr = best > SAMPLE - 1 ? best : SAMPLE - 1;
      const bool reached = have && (k < niters || k == bk);
      const bool nosample = reached && c[0] == rs::kNoSample && ROOTS * k > done;
      int r = -1, cr = 0;
      if (reached && !nosample) {
#pragma unroll
        for (int q = ROOTS - 1; q >= 0; --q)
          if (c[q] > thr && ROOTS * k + q > done) { r = q; cr = c[q]; }
      }
      const unsigned long long hit = __ballot(nosample || r >= 0);
      if (hit == 0ull) break;
      const int L = __ffsll((long long)hit) - 1;
      const int rL = __shfl(r, L, 64);
      if (rL < 0) {  // lane L's iteration drew no sample: the loop ends there
        stop = base + L;
        break;
      }
      best = __shfl(cr, L, 64);
      bk = base + L;
      br = rL;
      done = ROOTS * bk + br;
      niters = rs::update_num_iters<SAMPLE>(confidence, (double)(N - best) / N, niters);
    }
  }
  *best_k = bk;
  *best_r = br;
  *iters = stop >= 0 ? stop : (niters > bk + 1 ? niters : bk + 1);
  return best;
}

// One lane per correspondence: the winner's inlier mask, and optionally a copy of the matches with the other rows set to quiet
// NaN (the masked input of the unchanged cheirality kernel: a NaN row passes no depth test).  Model: what the test needs beside
// the winner Md[pair] -- model.is_inlier(M, pair, m) for the 3x3 M in fp64 and the correspondence m.
template <class Model>
__global__ void __launch_bounds__(256) mask_kernel(const float4* __restrict__ matches, int N, const double* __restrict__ Md,
                                                   const int* __restrict__ n_inliers, Model model, unsigned char* __restrict__ mask,
                                                   float4* __restrict__ masked) {
  const size_t pair = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  double M[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) M[j] = Md[pair * 9 + j];
  const float4 m = matches[pair * N + p];
  const bool in = n_inliers[pair] > 0 && model.is_inlier(M, pair, m);
  mask[pair * N + p] = in ? 1 : 0;
  if (masked != nullptr) {
    const float qn = __builtin_nanf("");
    masked[pair * N + p] = in ? m : make_float4(qn, qn, qn, qn);
  }
}
