// ransac -- batched RANSAC fundamental-matrix estimator (OpenCV 3.4 findFundamentalMat(FM_RANSAC), which the reference's
// validation baseline calls: dsac_tools/utils_opencv.py:157) and the per-correspondence in-front mask of the pose that
// follows it (cv2.recoverPose's mask output, utils_opencv.py:177).  The per-lane arithmetic is in ransac_math.h (shared with
// the host emulation of the tests); the contract is in include/dfepe.h.
//
// Three launches for the estimator:
//   count   one 256-thread workgroup per (pair, chunk of 64 iterations): the pair's correspondences are staged in LDS, one
//           lane of wavefront 0 per iteration draws its sample and solves the 7-point system in fp64 (up to 3 hypotheses
//           into LDS), then the four wavefronts share the hypotheses and sweep all correspondences for each (fp64 inlier test,
//           __ballot / __popcll); the counts go to the [B, max_iters, 3] table.  Every iteration is evaluated, also those beyond
//           the stopping point the sequential rule will find: the select launch reads only what the rule reads.
//   select  one wavefront per pair: the sequential rule over the table (select_wave, robust_dev.h), then the winning iteration
//           solved again by rs::solve_iteration, as the count launch solved it (same F bit for bit, no hypothesis storage).
//   mask    robust_dev.h's mask_kernel around rs::is_inlier.
#include "cheirality_body.h"
#include "robust_dev.h"

namespace {

constexpr int kChunk = 64;                        // iterations per workgroup of the count launch
constexpr int kHyps = kChunk * rs::kMaxRoots;     // hypotheses per workgroup
constexpr int kMaxN = 4096;                       // correspondences staged in LDS (16 B each)
constexpr int kMinN = 15;                         // below: OpenCV switches to LMedS (lmeds.hip)

__global__ void __launch_bounds__(256) ransac_count_kernel(const float4* __restrict__ matches, int N, int max_iters, double t2,
                                                           unsigned long long seed, int* __restrict__ table) {
  extern __shared__ float4 lds_pts[];  // [N], then the hypotheses (N * 16 bytes keeps them 16-byte aligned)
  double* hypF = reinterpret_cast<double*>(lds_pts + N);        // [kHyps][9]
  int* hcnt = reinterpret_cast<int*>(hypF + kHyps * 9);         // [kHyps]
  int* nroots = hcnt + kHyps;                                   // [kChunk]: roots of the iteration, or kNoSample
  const size_t pair = blockIdx.y;
  const int k0 = blockIdx.x * kChunk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float4* mrow = matches + pair * (size_t)N;
  for (int i = tid; i < N; i += blockDim.x) lds_pts[i] = mrow[i];
  __syncthreads();
  if (wave == 0) {
    const int k = k0 + lane;
    int n = 0;
    if (k < max_iters) {
      auto pts = [&](int i) { return lds_pts[i]; };
      double F[9 * rs::kMaxRoots];
      n = rs::solve_iteration(seed, k, N, pts, F);
      if (n != rs::kNoSample) {
#pragma unroll
        for (int j = 0; j < 9 * rs::kMaxRoots; ++j) hypF[lane * 27 + j] = F[j];
      }
    }
    nroots[lane] = n;
  }
  __syncthreads();
  // wavefront w counts hypotheses w, w + 4, ... over all correspondences (not every hypothesis over a quarter of them: at N = 100
  // two of the four wavefronts would have no correspondence and the other two would walk all 192 hypotheses)
  const int nw = blockDim.x >> 6;
  for (int h = wave; h < kHyps; h += nw) {
    const int li = h / rs::kMaxRoots, r = h - li * rs::kMaxRoots;
    if (r >= nroots[li]) continue;  // uniform: no root / no sample / past max_iters
    double F[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) F[j] = hypF[h * 9 + j];
    int c = 0;
    for (int base = 0; base < N; base += 64) {
      const int p = base + lane;
      bool in = false;
      if (p < N) {
        const float4 m = lds_pts[p];
        in = rs::is_inlier(F, m.x, m.y, m.z, m.w, t2);
      }
      c += __popcll(__ballot(in));
    }
    if (lane == 0) hcnt[h] = c;
  }
  __syncthreads();
  if (tid < kHyps) {
    const int li = tid / rs::kMaxRoots, r = tid - li * rs::kMaxRoots, k = k0 + li;
    if (k < max_iters) {
      const int n = nroots[li];
      table[(pair * max_iters + k) * rs::kMaxRoots + r] = (n == rs::kNoSample) ? rs::kNoSample : (r < n ? hcnt[tid] : rs::kNoRoot);
    }
  }
}

__global__ void __launch_bounds__(256) ransac_select_kernel(const float4* __restrict__ matches, int B, int N, const int* __restrict__ table,
                                                            double confidence, int max_iters, unsigned long long seed, double* __restrict__ Fd,
                                                            float* __restrict__ F_out, int* __restrict__ n_inliers, int* __restrict__ iters_run,
                                                            int* __restrict__ best_hyp) {
  const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // one wavefront per pair
  if (b >= B) return;
  int bk, br, it;
  const int best = select_wave<rs::kMaxRoots, rs::kSample>(table + (size_t)b * max_iters * rs::kMaxRoots, N, confidence, max_iters, &bk, &br, &it);
  if ((threadIdx.x & 63) != 0) return;
  double Fw[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) Fw[j] = 0.0;
  if (bk >= 0) {
    const float4* mrow = matches + (size_t)b * N;
    auto pts = [&](int i) { return mrow[i]; };
    double F[9 * rs::kMaxRoots];
    rs::solve_iteration(seed, bk, N, pts, F);  // gave a sample in the count launch: same stream, same sample, same roots
#pragma unroll
    for (int r = 0; r < rs::kMaxRoots; ++r)
      if (r == br) {
#pragma unroll
        for (int j = 0; j < 9; ++j) Fw[j] = F[9 * r + j];
      }
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    Fd[(size_t)b * 9 + j] = Fw[j];
    F_out[(size_t)b * 9 + j] = (float)Fw[j];
  }
  n_inliers[b] = best;
  iters_run[b] = it;
  if (best_hyp != nullptr) { best_hyp[2 * b] = bk; best_hyp[2 * b + 1] = br; }
}

struct MaskF {  // mask_kernel's Model
  double t2;
  __device__ bool is_inlier(const double* F, size_t, const float4& m) const { return rs::is_inlier(F, m.x, m.y, m.z, m.w, t2); }
};

// The fp64 route of cheirality_pair (cheirality_body.h) for one correspondence and the rotation candidate RR: the same rows, the
// same normal matrix, the same eigenvector routines and depth tests, so that a correspondence is counted here exactly when the
// cheirality kernel counts it for that candidate.  Returns (in front for (R, t), in front for (R, -t)).
template <int RR>
__device__ inline void in_front_fp64(const double* prep, const float4& m, float depth_thres, bool* pos_out, bool* neg_out) {
  double Kd[9], P2[12];
#pragma unroll
  for (int k = 0; k < 9; ++k) Kd[k] = prep[kPrepK + k];
#pragma unroll
  for (int k = 0; k < 12; ++k) P2[k] = prep[kPrepP + 12 * RR + k];
  const double Rz[3] = {prep[kPrepR + 9 * RR + 6], prep[kPrepR + 9 * RR + 7], prep[kPrepR + 9 * RR + 8]};
  const double tz = prep[kPrepT + 2];
  double Sr[16];
  {
    double A1[6], A2[8];
    const double x1 = m.x, y1 = m.y;
#pragma unroll
    for (int c = 0; c < 3; ++c) { A1[c] = x1 * Kd[6 + c] - Kd[c]; A1[3 + c] = y1 * Kd[6 + c] - Kd[3 + c]; }
    const double x2 = m.z, y2 = m.w;
#pragma unroll
    for (int c = 0; c < 4; ++c) { A2[c] = x2 * P2[8 + c] - P2[c]; A2[4 + c] = y2 * P2[8 + c] - P2[4 + c]; }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = r; c < 4; ++c) Sr[4 * r + c] = A2[r] * A2[c] + A2[4 + r] * A2[4 + c];
    Sr[0] += A1[0] * A1[0] + A1[3] * A1[3]; Sr[1] += A1[0] * A1[1] + A1[3] * A1[4]; Sr[2] += A1[0] * A1[2] + A1[3] * A1[5];
    Sr[5] += A1[1] * A1[1] + A1[4] * A1[4]; Sr[6] += A1[1] * A1[2] + A1[4] * A1[5]; Sr[10] += A1[2] * A1[2] + A1[5] * A1[5];
  }
  const double itr = rcp_nr<1>(fmax(Sr[0] + Sr[5] + Sr[10] + Sr[15], 1e-30));
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = r; c < 4; ++c) Sr[4 * r + c] *= itr;
  float Sf[16], Xf[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = r; c < 4; ++c) { Sf[4 * r + c] = (float)Sr[4 * r + c]; Sf[4 * c + r] = Sf[4 * r + c]; }
  smallest_eigvec4_pk<float>(Sf, Xf);
  const double x0[4] = {(double)Xf[0], (double)Xf[1], (double)Xf[2], (double)Xf[3]};
  double X[4];
  rqi_refine4(Sr, x0, X);
  const double wq = X[3];
  const double z1n = X[2];
  const double z2n = Rz[0] * X[0] + Rz[1] * X[1] + Rz[2] * X[2] + tz * wq;
  const double thr = (double)depth_thres;
  const double aw = thr * fabs(wq);
  const bool inr = (fabs(z1n) < aw) && (fabs(z2n) < aw) && (wq != 0.0);
  const bool s1p = (z1n > 0.0) == (wq > 0.0), s2p = (z2n > 0.0) == (wq > 0.0);
  const bool nz = (z1n != 0.0) && (z2n != 0.0);
  *pos_out = inr && nz && s1p && s2p;
  *neg_out = inr && nz && !s1p && !s2p;
}

__global__ void __launch_bounds__(64) ransac_in_front_kernel(const float* __restrict__ E, const float* __restrict__ K,
                                                             const float4* __restrict__ matches, int N, float depth_thres,
                                                             const int* __restrict__ winner, unsigned char* __restrict__ mask) {
  const size_t pair = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const int win = winner[pair];
  bool in = false;
  if (win >= 0) {
    double prep[kCheirPrep];
    cheir_prepare(E + pair * 9, nullptr, K + pair * 9, prep);
    const float4 m = matches[pair * N + p];
    bool pos, neg;
    if (win >> 1) in_front_fp64<1>(prep, m, depth_thres, &pos, &neg);
    else in_front_fp64<0>(prep, m, depth_thres, &pos, &neg);
    in = (win & 1) ? neg : pos;
  }
  mask[pair * N + p] = in ? 1 : 0;
}

}  // namespace

extern "C" size_t dfepe_ransac_workspace_bytes(int B, int N, int max_iters) {
  (void)N;
  return robust_workspace_bytes(B, max_iters, rs::kMaxRoots, sizeof(int));
}

extern "C" int dfepe_ransac_fundamental(const float* matches, int B, int N, double threshold, double confidence, int max_iters,
                                        unsigned long long seed, void* workspace, float* F_out, unsigned char* inlier_mask,
                                        int* n_inliers, int* iters_run, int* best_hyp, int* hyp_counts, float* masked_matches,
                                        void* stream) {
  if (B < 0 || max_iters <= 0 || !(threshold >= 0.0) || !(confidence >= 0.0 && confidence <= 1.0)) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (N < kMinN || N > kMaxN || B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  if (!matches || !workspace || !F_out || !inlier_mask || !n_inliers || !iters_run) return DFEPE_ERR_INVALID_ARG;
  if (!aligned16(matches) || !aligned16(workspace) || (masked_matches && !aligned16(masked_matches))) return DFEPE_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const double t2 = threshold * threshold;
  double* Fd = static_cast<double*>(workspace);
  int* table = hyp_counts ? hyp_counts : reinterpret_cast<int*>(Fd + (size_t)B * 9);
  const float4* m4 = reinterpret_cast<const float4*>(matches);
  const size_t lds = (size_t)N * sizeof(float4) + (size_t)kHyps * 9 * sizeof(double) + (size_t)(kHyps + kChunk) * sizeof(int);
  if (!opt_in_lds(ransac_count_kernel, lds)) return DFEPE_ERR_HIP;
  hipLaunchKernelGGL(ransac_count_kernel, dim3((max_iters + kChunk - 1) / kChunk, B), dim3(256), lds, s, m4, N, max_iters, t2,
                     seed, table);
  hipLaunchKernelGGL(ransac_select_kernel, dim3((B + 3) / 4), dim3(256), 0, s, m4, B, N, table, confidence, max_iters, seed, Fd,
                     F_out, n_inliers, iters_run, best_hyp);
  hipLaunchKernelGGL(mask_kernel<MaskF>, dim3((N + 255) / 256, B), dim3(256), 0, s, m4, N, Fd, n_inliers, MaskF{t2}, inlier_mask,
                     reinterpret_cast<float4*>(masked_matches));
  return launched();
}

extern "C" int dfepe_ransac_in_front(const float* E, const float* K, const float* matches, int B, int N, float depth_thres,
                                     const int* winner, unsigned char* mask, void* stream) {
  if (B < 0 || N < 0) return DFEPE_ERR_INVALID_ARG;
  if (B == 0 || N == 0) return DFEPE_OK;
  if (!E || !K || !matches || !winner || !mask || !aligned16(matches)) return DFEPE_ERR_INVALID_ARG;
  if (B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(ransac_in_front_kernel, dim3((N + 63) / 64, B), dim3(64), 0, static_cast<hipStream_t>(stream), E, K,
                     reinterpret_cast<const float4*>(matches), N, depth_thres, winner, mask);
  return launched();
}
