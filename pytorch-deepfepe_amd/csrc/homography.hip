// homography -- batched RANSAC homography estimator (OpenCV 3.4 findHomography(x1, x2, RANSAC), which the reference's front-end
// evaluation calls: evaluations/descriptor_evaluation.py:93, deepFEPE/evaluate_frontend.py:234) and the two measures that
// evaluation takes of a homography (getInliers, evaluate_frontend.py:210-228; the mean corner error, descriptor_evaluation.py:
// 104-123).  The per-lane arithmetic is in homography_math.h (shared with the host emulation of the tests); the contract is in
// include/dfepe.h.  The launch split follows ransac.hip:
//   count   one 256-thread workgroup per (pair, chunk of 64 iterations): the pair's correspondences are staged in LDS as the
//           float4 rows they arrive in (the sweep converts on the fly: four conversions against sixteen fp64 operations per row,
//           and half the LDS of staged doubles), one lane of wavefront 0 per iteration draws its sample and solves the 4-point
//           system in fp64, then the four wavefronts share the 64 hypotheses and sweep all correspondences for each (__ballot /
//           __popcll); the counts go to the [B, max_iters] table.  Every iteration is evaluated; select reads what the rule reads.
//   select  one wavefront per pair: the sequential rule over the table (select_wave, robust_dev.h, with one slot an iteration),
//           then lane 0 solves the winning iteration again by the two halves of the count launch's hg::solve_iteration (same H
//           bit for bit); a pair of exactly four points goes to the second half with its own points.
//   mask    one lane per correspondence: the winner's inlier mask.
//   refine  one wavefront per pair: runKernel over the inliers and the Levenberg-Marquardt refinement.  Lanes stride the
//           correspondences under the mask (no compaction); every sum is a wavefront reduction in fp64; the 9x9 and 8x8 Jacobi
//           decompositions run on lane 0 over matrices kept in LDS (profiles/homography.md).
#include "homography_math.h"
#include "robust_dev.h"

namespace {

constexpr int kChunk = 64;        // iterations per workgroup of the count launch (one hypothesis each)
constexpr int kMaxN = 4096;       // correspondences staged in LDS (16 B each)
constexpr unsigned kAllPoints = DFEPE_HOMOGRAPHY_ALL_POINTS, kNoRefine = DFEPE_HOMOGRAPHY_NO_REFINE;

__device__ inline int pair_count(const int* __restrict__ n_valid, size_t pair, int N) {
  if (n_valid == nullptr) return N;
  const int n = n_valid[pair];
  return n < 0 ? 0 : (n > N ? N : n);
}

__global__ void __launch_bounds__(256) homography_count_kernel(const float4* __restrict__ matches, const int* __restrict__ n_valid, int N,
                                                               int max_iters, double t2, unsigned long long seed,
                                                               int* __restrict__ table) {
  extern __shared__ float4 lds_pts[];  // [N], then the hypotheses (N * 16 bytes keeps them 16-byte aligned)
  double* hypH = reinterpret_cast<double*>(lds_pts + N);  // [kChunk][9]
  int* hcnt = reinterpret_cast<int*>(hypH + kChunk * 9);  // [kChunk]
  int* status = hcnt + kChunk;                            // [kChunk]: 1 model, 0 none, kNoSample
  const size_t pair = blockIdx.y;
  const int k0 = blockIdx.x * kChunk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = pair_count(n_valid, pair, N);
  if (n <= hg::kSample) {  // no sampling for this pair (uniform over the workgroup): the table says so
    if (tid < kChunk && k0 + tid < max_iters) table[pair * max_iters + k0 + tid] = rs::kNoSample;
    return;
  }
  const float4* mrow = matches + pair * (size_t)N;
  for (int i = tid; i < n; i += blockDim.x) lds_pts[i] = mrow[i];
  __syncthreads();
  if (wave == 0) {
    const int k = k0 + lane;
    int st = 0;
    if (k < max_iters) {
      auto pts = [&](int i) { return lds_pts[i]; };
      st = hg::solve_iteration(seed, k, n, pts, hypH + lane * 9);  // the model goes straight to its slot; read only where st == 1
    }
    status[lane] = st;
  }
  __syncthreads();
  const int nw = blockDim.x >> 6;
  for (int h = wave; h < kChunk; h += nw) {
    if (status[h] != 1) continue;  // uniform: no model / no sample / past max_iters
    double H[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) H[j] = hypH[h * 9 + j];
    int c = 0;
    for (int base = 0; base < n; base += 64) {
      const int p = base + lane;
      bool in = false;
      if (p < n) {
        const float4 m = lds_pts[p];
        in = hg::is_inlier(H, m.x, m.y, m.z, m.w, t2);
      }
      c += __popcll(__ballot(in));
    }
    if (lane == 0) hcnt[h] = c;
  }
  __syncthreads();
  if (tid < kChunk && k0 + tid < max_iters) {
    const int st = status[tid];
    table[pair * max_iters + k0 + tid] = (st == 1) ? hcnt[tid] : (st == 0 ? rs::kNoRoot : rs::kNoSample);
  }
}

__global__ void __launch_bounds__(256) homography_select_kernel(const float4* __restrict__ matches, const int* __restrict__ n_valid, int B,
                                                                int N, const int* __restrict__ table, double confidence, int max_iters,
                                                                unsigned long long seed, unsigned flags, double* __restrict__ Hd,
                                                                double* __restrict__ H_model, int* __restrict__ n_inliers,
                                                                int* __restrict__ iters_run, int* __restrict__ best_iter) {
  const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // one wavefront per pair
  if (b >= B) return;
  const int n = pair_count(n_valid, b, N);
  const bool sampled = n > hg::kSample && !(flags & kAllPoints);
  int bk = -1, br, it = 0, best = 0;  // br: the one slot, not reported
  if (sampled) best = select_wave<1, hg::kSample>(table + (size_t)b * max_iters, n, confidence, max_iters, &bk, &br, &it);
  if ((threadIdx.x & 63) != 0) return;
  double Hw[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) Hw[j] = 0.0;
  const float4* mrow = matches + (size_t)b * N;
  if (n == hg::kSample || (sampled && bk >= 0)) {
    auto pts = [&](int i) { return mrow[i]; };
    int idx[hg::kSample] = {0, 1, 2, 3};  // the pair's own four points, unless an iteration won:
    if (sampled) hg::draw_sample4(seed, bk, n, pts, idx);  // it gave a sample in the count launch: same stream, same sample
    double H[9];
    const bool ok = hg::solve_sample(pts, idx, H);  // the two halves of hg::solve_iteration, so that solve4 is inlined once
    if (ok) {
#pragma unroll
      for (int j = 0; j < 9; ++j) Hw[j] = H[j];
    }
    if (!sampled) best = ok ? hg::kSample : 0;
  } else if (n > hg::kSample && (flags & kAllPoints)) {
    best = n;  // the refine launch solves over all points, and takes this back if that gives no model
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    Hd[(size_t)b * 9 + j] = Hw[j];
    if (H_model != nullptr) H_model[(size_t)b * 9 + j] = Hw[j];
  }
  n_inliers[b] = best;
  iters_run[b] = it;
  if (best_iter != nullptr) best_iter[b] = bk;
}

__global__ void __launch_bounds__(256) homography_mask_kernel(const float4* __restrict__ matches, const int* __restrict__ n_valid, int N,
                                                              const double* __restrict__ Hd, const int* __restrict__ n_inliers, double t2,
                                                              unsigned flags, unsigned char* __restrict__ mask) {
  const size_t pair = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const int n = pair_count(n_valid, pair, N);
  bool in = false;
  if (p < n && n_inliers[pair] > 0) {
    if (n == hg::kSample || (flags & kAllPoints)) {
      in = true;
    } else {
      double H[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) H[j] = Hd[pair * 9 + j];
      const float4 m = matches[pair * N + p];
      in = hg::is_inlier(H, m.x, m.y, m.z, m.w, t2);
    }
  }
  mask[pair * N + p] = in ? 1 : 0;
}

// The sums of homography_math.h's drivers with one wavefront: lanes stride the pair's correspondences under the mask, a butterfly
// leaves the same totals in every lane, lane 0 puts them where the drivers read them.
struct WaveCtx {
  const float4* m;
  const unsigned char* mask;
  int n, lane;

  __device__ bool leader() const { return lane == 0; }
  __device__ void sync() const { __syncthreads(); }

  template <int KIND, int FIRST, int LAST, int NPAR>
  __device__ void run(const double* par, double* out) const {
    __syncthreads();
    double p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = (i < NPAR) ? par[i] : 0.0;
    double acc[hg::kRed];
#pragma unroll
    for (int i = 0; i < hg::kRed; ++i) acc[i] = 0.0;
    for (int i = lane; i < n; i += 64) {
      if (mask[i]) {
        const float4 q = m[i];
        hg::point_add<KIND>(p, (double)q.x, (double)q.y, (double)q.z, (double)q.w, acc);
      }
    }
#pragma unroll
    for (int i = FIRST; i < LAST; ++i) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(acc[i], o, 64);
        acc[i] = (i == 45) ? fmax(acc[i], other) : acc[i] + other;
      }
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int i = FIRST; i < LAST; ++i) out[i] = acc[i];
    }
    __syncthreads();
  }

  __device__ void reduce(int kind, const double* par, double* out) const {
    switch (kind) {
      case hg::kSum: run<hg::kSum, 0, 4, 0>(par, out); break;
      case hg::kAbs: run<hg::kAbs, 0, 4, 4>(par, out); break;
      case hg::kLtL: run<hg::kLtL, 0, 45, 8>(par, out); break;
      case hg::kLmFull: run<hg::kLmFull, 0, 46, 8>(par, out); break;
      default: run<hg::kLmRes, 44, 46, 8>(par, out); break;
    }
  }
};

__global__ void __launch_bounds__(64) homography_refine_kernel(const float4* __restrict__ matches, const int* __restrict__ n_valid, int N,
                                                               unsigned flags, const double* __restrict__ Hd, unsigned char* __restrict__ mask,
                                                               int* __restrict__ n_inliers, double* __restrict__ H_out,
                                                               double* __restrict__ H_model) {
  __shared__ hg::Work W;
  const size_t pair = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = pair_count(n_valid, pair, N);
  const int cnt = n_inliers[pair];
  if (cnt == 0 || n == hg::kSample) {  // no model (zeros), or the four points' own solution: nothing to refit
    if (lane < 9) H_out[pair * 9 + lane] = Hd[pair * 9 + lane];
    return;
  }
  WaveCtx ctx{matches + pair * (size_t)N, mask + pair * (size_t)N, n, lane};
  if (lane < 9) W.H[lane] = Hd[pair * 9 + lane];
  __syncthreads();
  const bool ok = hg::refit(ctx, W, cnt);
  if (flags & kAllPoints) {
    if (!ok) {  // runKernel over all points is the model here: without it the pair has none
      if (lane < 9) {
        H_out[pair * 9 + lane] = 0.0;
        if (H_model != nullptr) H_model[pair * 9 + lane] = 0.0;
      }
      for (int i = lane; i < n; i += 64) mask[pair * (size_t)N + i] = 0;
      if (lane == 0) n_inliers[pair] = 0;
      return;
    }
    if (H_model != nullptr && lane < 9) H_model[pair * 9 + lane] = W.H[lane];
  }
  if (!(flags & kNoRefine)) {
    if (lane < 8) W.h[lane] = W.H[lane];
    __syncthreads();
    double S0, S1;
    hg::lm_refine(ctx, W, static_cast<double*>(nullptr), &S0, &S1);
    if (lane < 8) W.H[lane] = W.h[lane];
    __syncthreads();
  }
  if (lane < 9) H_out[pair * 9 + lane] = W.H[lane];
}

__global__ void __launch_bounds__(256) homography_transfer_kernel(const double* __restrict__ H, const float4* __restrict__ matches,
                                                                  const int* __restrict__ n_valid, int N, double epi,
                                                                  float* __restrict__ dist, unsigned char* __restrict__ mask) {
  const size_t pair = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const int n = pair_count(n_valid, pair, N);
  double d = 0.0;
  bool in = false;
  if (p < n) {
    double Hh[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) Hh[j] = H[pair * 9 + j];
    const float4 m = matches[pair * N + p];
    d = hg::transfer_dist(Hh, m.x, m.y, m.z, m.w);
    in = d < epi;
  }
  if (dist != nullptr) dist[pair * N + p] = (float)d;
  if (mask != nullptr) mask[pair * N + p] = in ? 1 : 0;
}

__global__ void __launch_bounds__(256) homography_corners_kernel(const double* __restrict__ H_est, const double* __restrict__ H_gt, int B,
                                                                 int height, int width, const double* __restrict__ thresh, int T,
                                                                 double* __restrict__ mean_dist, unsigned char* __restrict__ correct) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double He[9], Hg[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) { He[j] = H_est[(size_t)b * 9 + j]; Hg[j] = H_gt[(size_t)b * 9 + j]; }
  const double md = hg::corner_mean_dist(He, Hg, height, width);
  if (mean_dist != nullptr) mean_dist[b] = md;
  for (int j = 0; j < T; ++j) correct[(size_t)b * T + j] = (md <= thresh[j]) ? 1 : 0;
}

}  // namespace

extern "C" size_t dfepe_homography_workspace_bytes(int B, int N, int max_iters) {
  (void)N;
  return robust_workspace_bytes(B, max_iters, 1, sizeof(int));
}

extern "C" int dfepe_ransac_homography(const float* matches, const int* n_valid, int B, int N, double threshold, double confidence,
                                       int max_iters, unsigned long long seed, unsigned flags, void* workspace, double* H_out,
                                       double* H_model, unsigned char* inlier_mask, int* n_inliers, int* iters_run, int* best_iter,
                                       int* hyp_counts, void* stream) {
  if (B < 0 || N < 1 || max_iters < 1 || threshold != threshold || !(confidence >= 0.0 && confidence <= 1.0)) return DFEPE_ERR_INVALID_ARG;
  if (flags & ~(kAllPoints | kNoRefine)) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (N > kMaxN || B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  if (!matches || !workspace || !H_out || !inlier_mask || !n_inliers || !iters_run) return DFEPE_ERR_INVALID_ARG;
  if (!aligned16(matches) || !aligned16(workspace)) return DFEPE_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!(threshold > 0.0)) threshold = 3.0;  // cv2's rule
  const double t2 = threshold * threshold;
  double* Hd = static_cast<double*>(workspace);
  int* table = hyp_counts ? hyp_counts : reinterpret_cast<int*>(Hd + (size_t)B * 9);
  const float4* m4 = reinterpret_cast<const float4*>(matches);
  if (!(flags & kAllPoints)) {
    const size_t lds = (size_t)N * sizeof(float4) + (size_t)kChunk * 9 * sizeof(double) + (size_t)2 * kChunk * sizeof(int);
    if (!opt_in_lds(homography_count_kernel, lds)) return DFEPE_ERR_HIP;
    hipLaunchKernelGGL(homography_count_kernel, dim3((max_iters + kChunk - 1) / kChunk, B), dim3(256), lds, s, m4, n_valid, N,
                       max_iters, t2, seed, table);
  }
  hipLaunchKernelGGL(homography_select_kernel, dim3((B + 3) / 4), dim3(256), 0, s, m4, n_valid, B, N, table, confidence, max_iters,
                     seed, flags, Hd, H_model, n_inliers, iters_run, best_iter);
  hipLaunchKernelGGL(homography_mask_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, m4, n_valid, N, Hd, n_inliers, t2, flags,
                     inlier_mask);
  hipLaunchKernelGGL(homography_refine_kernel, dim3(B), dim3(64), 0, s, m4, n_valid, N, flags, Hd, inlier_mask, n_inliers, H_out,
                     H_model);
  return launched();
}

extern "C" int dfepe_homography_transfer(const double* H, const float* matches, const int* n_valid, int B, int N, double epi,
                                         float* dist, unsigned char* mask, void* stream) {
  if (B < 0 || N < 0 || epi != epi) return DFEPE_ERR_INVALID_ARG;
  if (B == 0 || N == 0) return DFEPE_OK;
  if (B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  if (!H || !matches || (!dist && !mask) || !aligned16(matches)) return DFEPE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(homography_transfer_kernel, dim3((N + 255) / 256, B), dim3(256), 0, static_cast<hipStream_t>(stream), H,
                     reinterpret_cast<const float4*>(matches), n_valid, N, epi, dist, mask);
  return launched();
}

extern "C" int dfepe_homography_corners(const double* H_est, const double* H_gt, int B, int height, int width, const double* thresh,
                                        int T, double* mean_dist, unsigned char* correct, void* stream) {
  if (B < 0 || T < 0 || height < 1 || width < 1) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!H_est || !H_gt || (T > 0 && (!thresh || !correct)) || (T == 0 && !mean_dist)) return DFEPE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(homography_corners_kernel, dim3((B + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), H_est, H_gt, B,
                     height, width, thresh, T, mean_dist, correct);
  return launched();
}
