// corr_eval -- the correspondence evaluation of the reference, batched over image pairs: the epipolar distance of every match
// under the ground-truth F (epi_dist_from_matches, deepFEPE/evaluation_epiDist.py:276-326 -> val_rt -> epi_distance_np,
// dsac_tools/utils_F.py:363-385) and Result_processor's table of inlier ratios by match score (inlier_ratio, get_mask,
// inlier_ratio_from_est, ap_inlier_thd: deepFEPE/utils/eval_tools.py:27-174).  The per-lane arithmetic is in corr_eval_math.h
// (shared with the host emulation of the tests); the contract is in include/dfepe.h.  The launches:
//   inlier_table  one 256-thread workgroup per pair strides over the pair's rows.  Each lane has one match's fp64 distance and
//                 score; per mask threshold and inlier threshold the wavefront counts its lanes with __ballot / __popcll and its
//                 first lane adds the count to the wavefront's own table in LDS (Tm (Ti + 1) integers: the kept matches, then the
//                 inliers among them).  After one barrier a lane per cell adds the four tables and stores the cell, so there is
//                 no atomic of any kind, every cell has one writer, and integer sums do not depend on an order.
//   table_mean    one workgroup: a lane per cell of the mean adds the B ratios in index order; num is transposed alongside.
#include "dfepe_common.h"
#include "corr_eval_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / WAVE;
constexpr int kCells = ce::kMaxThds * (ce::kMaxThds + 1);

__global__ void __launch_bounds__(kThreads) inlier_table_kernel(const float* __restrict__ matches, const double* __restrict__ F,
                                                                const float* __restrict__ dist, const float* __restrict__ scores,
                                                                const int* __restrict__ n_valid, int N, const double* __restrict__ inlier_thds,
                                                                int Ti, const double* __restrict__ mask_thds, int Tm, int* __restrict__ cnt,
                                                                int* __restrict__ num, double* __restrict__ ratio, float* __restrict__ dist_out) {
  __shared__ int tab[kWaves][kCells];
  __shared__ double ithd[ce::kMaxThds], mthd[ce::kMaxThds];
  const size_t pair = blockIdx.x;
  const int tid = threadIdx.x, wave = tid / WAVE;
  const int row = Ti + 1, cells = Tm * row;
  int n = N;
  if (n_valid != nullptr) {
    const int v = n_valid[pair];
    n = v < 0 ? 0 : (v > N ? N : v);
  }
  for (int c = tid; c < kWaves * kCells; c += kThreads) (&tab[0][0])[c] = 0;
  if (tid < Ti) ithd[tid] = inlier_thds[tid];
  if (tid < Tm) mthd[tid] = (mask_thds != nullptr) ? mask_thds[tid] : 0.0;  // read only where there are scores
  double Fm[9];
  if (matches != nullptr) {
#pragma unroll
    for (int j = 0; j < 9; ++j) Fm[j] = F[pair * 9 + j];
  }
  __syncthreads();
  for (int base = 0; base < N; base += kThreads) {  // the same trip count in every lane: the ballots below are wavefront-wide
    const int i = base + tid;
    const bool live = i < n;
    double d = 0.0, s = 0.0;
    if (live) {
      const size_t at = pair * (size_t)N + i;
      if (matches != nullptr) {
        const float4 m = reinterpret_cast<const float4*>(matches)[at];
        d = ce::epi_dist3(Fm, (double)m.x, (double)m.y, (double)m.z, (double)m.w);
      } else {
        d = (double)dist[at];
      }
      if (scores != nullptr) s = (double)scores[at];
    }
    if (dist_out != nullptr && i < N) dist_out[pair * (size_t)N + i] = live ? (float)d : 0.0f;
    if (base >= n) continue;  // uniform over the workgroup: only the zero fill of dist_out is left
    for (int m = 0; m < Tm; ++m) {
      const bool k = live && (scores == nullptr || ce::kept(s, mthd[m]));
      const int nk = __popcll(__ballot(k));
      if (nk == 0) continue;  // wavefront-uniform
      if ((tid & (WAVE - 1)) == 0) tab[wave][m * row] += nk;
      for (int t = 0; t < Ti; ++t) {
        const int ni = __popcll(__ballot(k && ce::inlier(d, ithd[t])));
        if ((tid & (WAVE - 1)) == 0) tab[wave][m * row + 1 + t] += ni;
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < cells; c += kThreads) {
    const int m = c / row, t = c % row;
    int v = 0, k = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      v += tab[w][c];
      k += tab[w][m * row];
    }
    if (t == 0) {
      if (num != nullptr) num[pair * Tm + m] = v;
    } else {
      const size_t o = (pair * Tm + m) * (size_t)Ti + (t - 1);
      if (cnt != nullptr) cnt[o] = v;
      if (ratio != nullptr) ratio[o] = ce::ratio_of(v, k);
    }
  }
}

__global__ void __launch_bounds__(kThreads) inlier_table_mean_kernel(const double* __restrict__ ratio, const int* __restrict__ num, int B, int Tm,
                                                                     int Ti, double* __restrict__ mean, int* __restrict__ num_T) {
  const int tid = threadIdx.x, cells = Tm * Ti;
  if (mean != nullptr) {
    for (int c = tid; c < cells; c += kThreads) mean[c] = ce::mean_of(ratio + c, cells, B);
  }
  if (num_T != nullptr) {
    const size_t total = (size_t)Tm * B;
    for (size_t c = tid; c < total; c += kThreads) {
      const size_t m = c / B, b = c % B;
      num_T[c] = num[b * Tm + m];
    }
  }
}

}  // namespace

extern "C" int dfepe_inlier_table(const float* matches, const double* F, const float* dist, const float* scores, const int* n_valid, int B,
                                  int N, const double* inlier_thds, int Ti, const double* mask_thds, int Tm, int* cnt, int* num,
                                  double* ratio, float* dist_out, void* stream) {
  if (B < 0 || N < 0 || Ti < 1 || Ti > ce::kMaxThds || Tm < 1 || Tm > ce::kMaxThds) return DFEPE_ERR_INVALID_ARG;
  if (matches != nullptr && dist != nullptr) return DFEPE_ERR_INVALID_ARG;
  if (scores == nullptr && Tm != 1) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (N > 0 && matches == nullptr && dist == nullptr) return DFEPE_ERR_INVALID_ARG;
  if (matches != nullptr && (F == nullptr || !aligned16(matches))) return DFEPE_ERR_INVALID_ARG;
  if (!inlier_thds || (scores != nullptr && !mask_thds)) return DFEPE_ERR_INVALID_ARG;
  if (!cnt && !num && !ratio && !dist_out) return DFEPE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(inlier_table_kernel, dim3(B), dim3(kThreads), 0, static_cast<hipStream_t>(stream), N > 0 ? matches : nullptr, F,
                     N > 0 ? dist : nullptr, scores, n_valid, N, inlier_thds, Ti, mask_thds, Tm, cnt, num, ratio, dist_out);
  return launched();
}

extern "C" int dfepe_inlier_table_mean(const double* ratio, const int* num, int B, int Tm, int Ti, double* mean, int* num_T, void* stream) {
  if (B < 0 || Ti < 1 || Ti > ce::kMaxThds || Tm < 1 || Tm > ce::kMaxThds) return DFEPE_ERR_INVALID_ARG;
  if (!mean && !num_T) return DFEPE_ERR_INVALID_ARG;
  if (B > 0 && ((mean != nullptr && !ratio) || (num_T != nullptr && !num))) return DFEPE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(inlier_table_mean_kernel, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), ratio, num, B, Tm, Ti, mean,
                     num_T);
  return launched();
}
