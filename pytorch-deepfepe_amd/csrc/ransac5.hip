// ransac5 -- batched RANSAC essential-matrix estimator with the five-point minimal solver (OpenCV 3.4 findEssentialMat(RANSAC),
// which the reference's validation baseline calls with five_point=True: dsac_tools/utils_opencv.py:147-151).  The per-lane
// arithmetic is in ransac5_math.h (shared with the host emulation of the tests); the contract is in include/dfepe.h.  The pose
// that follows goes through the unchanged dfepe_cheirality_ex / dfepe_ransac_in_front.
//
// The same three launches as ransac.hip:
//   count   one 256-thread workgroup per (pair, chunk of 16 iterations).  The pair's correspondences are staged in LDS; 16 lanes
//           of wavefront 0 each draw a sample and run the five-point solver in fp64.  The solver's 10x20 constraint matrix and its
//           other tables (r5::kWork doubles, 2368 bytes a lane) do not fit a lane's registers and are indexed at run time, so they
//           live in LDS, strided by lane so that the 16 lanes touch 16 consecutive doubles: no scratch memory.  16 lanes and not
//           64: 16 x 2368 B beside 4096 staged correspondences (64 KiB) stays inside the 160 KiB of a workgroup, small pairs keep
//           several workgroups on a CU, and a validation batch of a few pairs still spreads over the device (8 pairs x 1000
//           iterations are 504 workgroups).  The up to 10 solutions of a lane stay in its workspace; the four wavefronts then sweep
//           the correspondences -- each lane normalises one correspondence once (the divisions) and tests it against every
//           hypothesis of the chunk (__ballot / __popcll, integer LDS atomics: order-free) -- and the counts go to the
//           [B, max_iters, 10] table, the hypotheses optionally to hyp_E.
//   select  one wavefront per pair: the sequential rule over the table (select_wave, robust_dev.h), then the winning iteration
//           solved again by r5::solve_iteration (bit for bit the hypothesis the count launch scored).
//   mask    robust_dev.h's mask_kernel around r5::is_inlier on normalised coordinates.
#include "ransac5_math.h"
#include "robust_dev.h"

namespace {

constexpr int kChunk5 = 16;                          // iterations per workgroup of the count launch
constexpr int kHyps5 = kChunk5 * r5::kMaxRoots;      // hypotheses per workgroup
constexpr int kMaxN5 = 4096;                         // correspondences staged in LDS (16 B each)
constexpr int kMinN5 = 6;                            // with 5 OpenCV returns the stacked models of the one sample (not built)
constexpr int kSelectWaves = 4;                      // pairs per workgroup of the select launch

__global__ void __launch_bounds__(256) ransac5_count_kernel(const float4* __restrict__ matches, const float* __restrict__ K, int N,
                                                            int max_iters, double threshold, unsigned long long seed,
                                                            int* __restrict__ table, double* __restrict__ hyp_E) {
  extern __shared__ float4 lds_pts5[];  // [N], then the solver workspaces (N * 16 bytes keeps them 16-byte aligned)
  double* work = reinterpret_cast<double*>(lds_pts5 + N);       // [r5::kWork][kChunk5]
  int* hcnt = reinterpret_cast<int*>(work + r5::kWork * kChunk5);  // [kHyps5]
  int* nroots = hcnt + kHyps5;                                  // [kChunk5]
  const size_t pair = blockIdx.y;
  const int k0 = blockIdx.x * kChunk5;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float4* mrow = matches + pair * (size_t)N;
  for (int i = tid; i < N; i += blockDim.x) lds_pts5[i] = mrow[i];
  if (tid < kHyps5) hcnt[tid] = 0;
  const r5::Cam cam = r5::cam_of(K + pair * 9);
  const double t2 = r5::threshold2(cam, threshold);
  __syncthreads();
  if (tid < kChunk5) {
    const int k = k0 + tid;
    int n = 0;
    if (k < max_iters) {
      r5::LaneWork<kChunk5> w{work + tid};
      auto pts = [&](int i) { return lds_pts5[i]; };
      n = r5::solve_iteration(w, pts, cam, seed, k, N);
    }
    nroots[tid] = n;
  }
  __syncthreads();
  // wavefront w takes the correspondences [64 (w + 4 i), 64 (w + 4 i) + 64): one per lane, normalised once, against every
  // hypothesis of the chunk (the hypothesis is the same address for all lanes: an LDS broadcast)
  for (int base = wave * 64; base < N; base += 256) {
    const int p = base + lane;
    const bool valid = p < N;
    const float4 m = lds_pts5[valid ? p : 0];
    const double x1 = r5::norm_x(cam, m.x), y1 = r5::norm_y(cam, m.y), x2 = r5::norm_x(cam, m.z), y2 = r5::norm_y(cam, m.w);
    for (int li = 0; li < kChunk5; ++li) {
      const int n = nroots[li];
      for (int r = 0; r < n; ++r) {
        double E[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) E[j] = work[(r5::kOffE + 9 * r + j) * kChunk5 + li];
        const bool in = valid && r5::is_inlier(E, x1, y1, x2, y2, t2);
        const int c = __popcll(__ballot(in));
        if (lane == 0 && c != 0) atomicAdd(&hcnt[li * r5::kMaxRoots + r], c);
      }
    }
  }
  __syncthreads();
  if (tid < kHyps5) {
    const int li = tid / r5::kMaxRoots, r = tid - li * r5::kMaxRoots, k = k0 + li;
    if (k < max_iters) table[(pair * max_iters + k) * r5::kMaxRoots + r] = (r < nroots[li]) ? hcnt[tid] : r5::kNoRoot;
  }
  if (hyp_E != nullptr) {
    for (int e = tid; e < kHyps5 * 9; e += blockDim.x) {
      const int h = e / 9, j = e - 9 * h, li = h / r5::kMaxRoots, r = h - li * r5::kMaxRoots, k = k0 + li;
      if (k < max_iters)
        hyp_E[((pair * max_iters + k) * r5::kMaxRoots + r) * 9 + j] =
            (r < nroots[li]) ? work[(r5::kOffE + 9 * r + j) * kChunk5 + li] : 0.0;
    }
  }
}

__global__ void __launch_bounds__(64 * kSelectWaves) ransac5_select_kernel(
    const float4* __restrict__ matches, const float* __restrict__ K, int B, int N, const int* __restrict__ table, double confidence,
    int max_iters, unsigned long long seed, double* __restrict__ Ed, float* __restrict__ E_out, int* __restrict__ n_inliers,
    int* __restrict__ iters_run, int* __restrict__ best_hyp) {
  __shared__ double work[kSelectWaves][r5::kWork];
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kSelectWaves + wave;  // one wavefront per pair
  if (b >= B) return;
  int bk, br, it;
  const int best = select_wave<r5::kMaxRoots, r5::kSample>(table + (size_t)b * max_iters * r5::kMaxRoots, N, confidence, max_iters, &bk, &br, &it);
  if ((threadIdx.x & 63) != 0) return;
  double Ew[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) Ew[j] = 0.0;
  if (bk >= 0) {
    const float4* mrow = matches + (size_t)b * N;
    auto pts = [&](int i) { return mrow[i]; };
    r5::LaneWork<1> w{work[wave]};
    r5::solve_iteration(w, pts, r5::cam_of(K + (size_t)b * 9), seed, bk, N);  // same stream, same sample, same solutions
#pragma unroll
    for (int j = 0; j < 9; ++j) Ew[j] = w[r5::kOffE + 9 * br + j];
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    Ed[(size_t)b * 9 + j] = Ew[j];
    E_out[(size_t)b * 9 + j] = (float)Ew[j];
  }
  n_inliers[b] = best;
  iters_run[b] = it;
  if (best_hyp != nullptr) { best_hyp[2 * b] = bk; best_hyp[2 * b + 1] = br; }
}

struct MaskE {  // mask_kernel's Model
  const float* K;
  double threshold;
  __device__ bool is_inlier(const double* E, size_t pair, const float4& m) const {
    const r5::Cam cam = r5::cam_of(K + pair * 9);
    return r5::is_inlier(E, r5::norm_x(cam, m.x), r5::norm_y(cam, m.y), r5::norm_x(cam, m.z), r5::norm_y(cam, m.w),
                         r5::threshold2(cam, threshold));
  }
};

}  // namespace

extern "C" size_t dfepe_ransac5_workspace_bytes(int B, int N, int max_iters) {
  (void)N;
  return robust_workspace_bytes(B, max_iters, r5::kMaxRoots, sizeof(int));
}

extern "C" int dfepe_ransac_essential(const float* matches, const float* K, int B, int N, double threshold, double confidence,
                                      int max_iters, unsigned long long seed, void* workspace, float* E_out,
                                      unsigned char* inlier_mask, int* n_inliers, int* iters_run, int* best_hyp, int* hyp_counts,
                                      double* hyp_E, float* masked_matches, void* stream) {
  if (B < 0 || max_iters <= 0 || !(threshold >= 0.0) || !(confidence >= 0.0 && confidence <= 1.0)) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (N < kMinN5 || N > kMaxN5 || B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  if (!matches || !K || !workspace || !E_out || !inlier_mask || !n_inliers || !iters_run) return DFEPE_ERR_INVALID_ARG;
  if (!aligned16(matches) || !aligned16(workspace) || (masked_matches && !aligned16(masked_matches))) return DFEPE_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* Ed = static_cast<double*>(workspace);
  int* table = hyp_counts ? hyp_counts : reinterpret_cast<int*>(Ed + (size_t)B * 9);
  const float4* m4 = reinterpret_cast<const float4*>(matches);
  // 16 N + 38592 bytes: above 64 KiB (the attribute below) from N = 1685
  const size_t lds = (size_t)N * sizeof(float4) + (size_t)r5::kWork * kChunk5 * sizeof(double) + (size_t)(kHyps5 + kChunk5) * sizeof(int);
  if (!opt_in_lds(ransac5_count_kernel, lds)) return DFEPE_ERR_HIP;
  hipLaunchKernelGGL(ransac5_count_kernel, dim3((max_iters + kChunk5 - 1) / kChunk5, B), dim3(256), lds, s, m4, K, N, max_iters,
                     threshold, seed, table, hyp_E);
  hipLaunchKernelGGL(ransac5_select_kernel, dim3((B + kSelectWaves - 1) / kSelectWaves), dim3(64 * kSelectWaves), 0, s, m4, K, B, N,
                     table, confidence, max_iters, seed, Ed, E_out, n_inliers, iters_run, best_hyp);
  hipLaunchKernelGGL(mask_kernel<MaskE>, dim3((N + 255) / 256, B), dim3(256), 0, s, m4, N, Ed, n_inliers, MaskE{K, threshold},
                     inlier_mask, reinterpret_cast<float4*>(masked_matches));
  return launched();
}
