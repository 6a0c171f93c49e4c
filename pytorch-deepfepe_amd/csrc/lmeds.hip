// lmeds -- batched least-median-of-squares estimators of the fundamental matrix (7-point models) and of the essential matrix
// (five-point models): OpenCV 3.4's LMeDSPointSetRegistrator::run, which cv2.findFundamentalMat(.., cv2.RANSAC, ..) runs instead
// of RANSAC on fewer than 15 correspondences (the reference's validation baseline, dsac_tools/utils_opencv.py:157) and which
// cv2.findEssentialMat runs for method LMEDS.  The per-lane arithmetic is in lmeds_math.h (shared with the host emulation of the
// tests) on top of ransac_math.h / ransac5_math.h; the contract is in include/dfepe.h.  The pose that follows goes through the
// unchanged dfepe_cheirality_ex / dfepe_ransac_in_front.
//
// Three launches, like ransac.hip:
//   median  one 256-thread workgroup per (pair, chunk of 16 iterations): the pair's correspondences are staged in LDS, 16 lanes of
//           wavefront 0 each draw a sample and solve it in fp64 (up to 3 resp. 10 models a lane, left in LDS), then every model
//           goes to one wavefront, which evaluates the N errors (fp64, rounded to fp32) into R = ceil(N / 64) registers per lane --
//           R from the ladder 1, 2, 4, .. 64 as a template argument, so that the registers are never indexed at run time -- and
//           finds the median by lm::median_of: the rank-N/2 pattern bit by bit, 31 rounds of R compares per lane and one butterfly
//           over the wavefront, no workgroup barrier, no LDS, no atomics.  The medians go to the [B, niters, 3 | 10] table, every
//           iteration's, also past an iteration without a sample: the select launch reads only what the rule reads.
//           16 iterations and not ransac.hip's 64: a model costs a selection here, not a count, and the validation's 8 pairs x 300
//           iterations are 152 workgroups this way instead of 40.
//   select  one wavefront per pair: the first strict minimum of the table in (iteration, root) order up to the first iteration
//           without a sample, the winning sample drawn and solved again by the same device functions, sigma, and the winner's
//           inlier count (fewer than the model size: no model).
//   mask    one lane per correspondence: the error against (float)sigma^2, and the NaN-masked copy of the matches.
#include "dfepe_common.h"
#include "lmeds_math.h"

namespace {

constexpr int kChunkL = 16;      // iterations per workgroup of the median launch
constexpr int kMaxNL = 4096;     // correspondences staged in LDS (16 B each); 64 lanes x 64 registers
constexpr int kMinNF = 8;        // N = 7 is OpenCV's direct 7-point path (not built)
constexpr int kMinNE = 6;        // N = 5: the stacked models of the one sample (not built)
constexpr int kSelectWavesL = 4;

__device__ inline int wave_sum(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return __builtin_amdgcn_readfirstlane(x);
}
__device__ inline int wave_max(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int y = __shfl_xor(x, o, 64);
    x = y > x ? y : x;
  }
  return __builtin_amdgcn_readfirstlane(x);
}

// lm::median_of's wavefront on the device: this lane's registers and the two reductions.
template <int R>
struct DevWave {
  uint32_t v[R];
  template <class F>
  __device__ int sum(F f) const { return wave_sum(f(v)); }
  template <class F>
  __device__ int max(F f) const { return wave_max(f(v)); }
};

struct ModelF {
  static constexpr int kRoots = rs::kMaxRoots;
  static constexpr int kPoints = rs::kSample;
};
struct ModelE {
  static constexpr int kRoots = r5::kMaxRoots;
  static constexpr int kPoints = r5::kSample;
};

// ---- median launch, fundamental matrix ------------------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(256) lmeds_median_f_kernel(const float4* __restrict__ matches, int N, int niters, unsigned long long seed,
                                                             double* __restrict__ table) {
  constexpr int kHyps = kChunkL * rs::kMaxRoots;
  extern __shared__ float4 lds_ptsl[];                            // [N], then the models (16 N bytes keep them aligned)
  double* hypF = reinterpret_cast<double*>(lds_ptsl + N);         // [kHyps][9]
  float* hmed = reinterpret_cast<float*>(hypF + kHyps * 9);       // [kHyps]
  int* nroots = reinterpret_cast<int*>(hmed + kHyps);             // [kChunkL]
  const size_t pair = blockIdx.y;
  const int k0 = blockIdx.x * kChunkL;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float4* mrow = matches + pair * (size_t)N;
  for (int i = tid; i < N; i += blockDim.x) lds_ptsl[i] = mrow[i];
  __syncthreads();
  if (tid < kChunkL) {
    const int k = k0 + tid;
    int n = 0;
    if (k < niters) {
      auto pts = [&](int i) { return lds_ptsl[i]; };
      double F[9 * rs::kMaxRoots];
      n = rs::solve_iteration(seed, k, N, pts, F);
      if (n != rs::kNoSample) {
#pragma unroll
        for (int j = 0; j < 9 * rs::kMaxRoots; ++j) hypF[tid * 9 * rs::kMaxRoots + j] = F[j];
      }
    }
    nroots[tid] = n;
  }
  __syncthreads();
  for (int h = wave; h < kHyps; h += 4) {
    const int li = h / rs::kMaxRoots, r = h - li * rs::kMaxRoots;
    if (r >= nroots[li]) continue;  // uniform: no root / no sample / past niters
    double F[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) F[j] = hypF[h * 9 + j];
    DevWave<R> w;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int p = 64 * j + lane;
      uint32_t e = lm::kPadBits;
      if (p < N) {
        const float4 m = lds_ptsl[p];
        e = lm::err_bits(lm::f_error(F, m.x, m.y, m.z, m.w));
      }
      w.v[j] = e;
    }
    const float med = lm::median_of<R>(w, N);
    if (lane == 0) hmed[h] = med;
  }
  __syncthreads();
  if (tid < kHyps) {
    const int li = tid / rs::kMaxRoots, r = tid - li * rs::kMaxRoots, k = k0 + li;
    if (k < niters) {
      const int n = nroots[li];
      table[(pair * niters + k) * rs::kMaxRoots + r] = (n == rs::kNoSample) ? lm::kNoSample : (r < n ? (double)hmed[tid] : lm::kNoRoot);
    }
  }
}

// ---- median launch, essential matrix --------------------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(256) lmeds_median_e_kernel(const float4* __restrict__ matches, const float* __restrict__ K, int N, int niters,
                                                             unsigned long long seed, double* __restrict__ table) {
  constexpr int kHyps = kChunkL * r5::kMaxRoots;
  extern __shared__ float4 lds_ptsl[];                               // [N], then the solver workspaces, lane-strided
  double* work = reinterpret_cast<double*>(lds_ptsl + N);            // [r5::kWork][kChunkL]
  float* hmed = reinterpret_cast<float*>(work + r5::kWork * kChunkL);  // [kHyps]
  int* nroots = reinterpret_cast<int*>(hmed + kHyps);                // [kChunkL]
  const size_t pair = blockIdx.y;
  const int k0 = blockIdx.x * kChunkL;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float4* mrow = matches + pair * (size_t)N;
  for (int i = tid; i < N; i += blockDim.x) lds_ptsl[i] = mrow[i];
  const r5::Cam cam = r5::cam_of(K + pair * 9);
  __syncthreads();
  if (tid < kChunkL) {
    const int k = k0 + tid;
    int n = 0;
    if (k < niters) {
      r5::LaneWork<kChunkL> w{work + tid};
      auto pts = [&](int i) { return lds_ptsl[i]; };
      n = r5::solve_iteration(w, pts, cam, seed, k, N);
    }
    nroots[tid] = n;
  }
  __syncthreads();
  for (int h = wave; h < kHyps; h += 4) {
    const int li = h / r5::kMaxRoots, r = h - li * r5::kMaxRoots;
    if (r >= nroots[li]) continue;  // uniform
    double E[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) E[j] = work[(r5::kOffE + 9 * r + j) * kChunkL + li];
    DevWave<R> w;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int p = 64 * j + lane;
      uint32_t e = lm::kPadBits;
      if (p < N) {
        const float4 m = lds_ptsl[p];
        e = lm::err_bits(lm::e_error(E, r5::norm_x(cam, m.x), r5::norm_y(cam, m.y), r5::norm_x(cam, m.z), r5::norm_y(cam, m.w)));
      }
      w.v[j] = e;
    }
    const float med = lm::median_of<R>(w, N);
    if (lane == 0) hmed[h] = med;
  }
  __syncthreads();
  if (tid < kHyps) {
    const int li = tid / r5::kMaxRoots, r = tid - li * r5::kMaxRoots, k = k0 + li;
    if (k < niters) table[(pair * niters + k) * r5::kMaxRoots + r] = (r < nroots[li]) ? (double)hmed[tid] : lm::kNoRoot;
  }
}

// ---- select launch --------------------------------------------------------------------------------------------------------
// lm::select_best with one wavefront per pair.  Lane l walks the iterations l, l + 64, ...: first the earliest iteration without
// a sample (the loop's end), then its own first strict minimum below that end; a butterfly takes the smaller median, and of equal
// medians the earlier (iteration, root): the first strict minimum of the sequential loop.
template <int ROOTS>
__device__ inline double select_wave_l(const double* __restrict__ med, int niters, int* best_k, int* best_r, int* iters) {
  const int lane = threadIdx.x & 63;
  int stop = niters;
  if (ROOTS == rs::kMaxRoots) {
    for (int k = lane; k < niters; k += 64)
      if (med[ROOTS * k] == lm::kNoSample) { stop = k; break; }
    stop = -wave_max(-stop);
  }
  double best = DBL_MAX;
  int at = 0x7FFFFFFF;
  for (int k = lane; k < stop; k += 64) {
#pragma unroll
    for (int r = 0; r < ROOTS; ++r) {
      const double m = med[ROOTS * k + r];
      if (m >= 0.0 && m < best) { best = m; at = ROOTS * k + r; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(at, o, 64);
    if (ob < best || (ob == best && oa < at)) { best = ob; at = oa; }
  }
  const bool have = best < DBL_MAX;
  *best_k = have ? at / ROOTS : -1;
  *best_r = have ? at % ROOTS : -1;
  *iters = stop;
  return best;
}

struct SelectOut {
  double* Md;          // [B,9] the winner in fp64 (workspace)
  float* bound;        // [B] (float)sigma^2 (workspace)
  float* M_out;
  int* n_inliers;
  int* iters_run;
  int* best_hyp;
  double* min_median;
  double* sigma;
};

// The common tail of the two select kernels: sigma, the inlier count of the winner M (uniform over the wavefront) and the outputs.
template <class Model, class Err>
__device__ inline void finish_select(const SelectOut& o, size_t b, int N, double best, int bk, int br, int it, const double* M, const Err& err) {
  const int lane = threadIdx.x & 63;
  const bool have = bk >= 0;
  const double sg = have ? lm::sigma_of(best, N, Model::kPoints) : 0.0;
  const float bound = lm::inlier_bound(sg);
  int c = 0;
  if (have)
    for (int p = lane; p < N; p += 64) c += (lm::err_float(err(M, p)) <= bound) ? 1 : 0;
  c = wave_sum(c);
  const bool model = have && c >= Model::kPoints;
  if (lane != 0) return;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    o.Md[b * 9 + j] = model ? M[j] : 0.0;
    o.M_out[b * 9 + j] = model ? (float)M[j] : 0.0f;
  }
  o.bound[b] = bound;
  o.n_inliers[b] = model ? c : 0;
  o.iters_run[b] = it;
  if (o.best_hyp != nullptr) { o.best_hyp[2 * b] = model ? bk : -1; o.best_hyp[2 * b + 1] = model ? br : -1; }
  if (o.min_median != nullptr) o.min_median[b] = best;
  if (o.sigma != nullptr) o.sigma[b] = sg;
}

__global__ void __launch_bounds__(64 * kSelectWavesL) lmeds_select_f_kernel(const float4* __restrict__ matches, int B, int N,
                                                                            const double* __restrict__ table, int niters,
                                                                            unsigned long long seed, SelectOut o) {
  const int b = blockIdx.x * kSelectWavesL + (threadIdx.x >> 6);  // one wavefront per pair
  if (b >= B) return;
  int bk, br, it;
  const double best = select_wave_l<rs::kMaxRoots>(table + (size_t)b * niters * rs::kMaxRoots, niters, &bk, &br, &it);
  const float4* mrow = matches + (size_t)b * N;
  double Fw[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) Fw[j] = 0.0;
  if (bk >= 0 && (threadIdx.x & 63) == 0) {
    auto pts = [&](int i) { return mrow[i]; };
    double F[9 * rs::kMaxRoots];
    rs::solve_iteration(seed, bk, N, pts, F);  // gave a sample in the median launch: same stream, same sample, same roots
#pragma unroll
    for (int r = 0; r < rs::kMaxRoots; ++r)
      if (r == br) {
#pragma unroll
        for (int j = 0; j < 9; ++j) Fw[j] = F[9 * r + j];
      }
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) Fw[j] = __shfl(Fw[j], 0, 64);
  auto err = [&](const double* F, int p) {
    const float4 m = mrow[p];
    return lm::f_error(F, m.x, m.y, m.z, m.w);
  };
  finish_select<ModelF>(o, (size_t)b, N, best, bk, br, it, Fw, err);
}

__global__ void __launch_bounds__(64 * kSelectWavesL) lmeds_select_e_kernel(const float4* __restrict__ matches, const float* __restrict__ K,
                                                                            int B, int N, const double* __restrict__ table, int niters,
                                                                            unsigned long long seed, SelectOut o) {
  __shared__ double work[kSelectWavesL][r5::kWork];
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kSelectWavesL + wave;  // one wavefront per pair
  if (b >= B) return;
  int bk, br, it;
  const double best = select_wave_l<r5::kMaxRoots>(table + (size_t)b * niters * r5::kMaxRoots, niters, &bk, &br, &it);
  const float4* mrow = matches + (size_t)b * N;
  const r5::Cam cam = r5::cam_of(K + (size_t)b * 9);
  double Ew[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) Ew[j] = 0.0;
  if (bk >= 0 && (threadIdx.x & 63) == 0) {
    auto pts = [&](int i) { return mrow[i]; };
    r5::LaneWork<1> w{work[wave]};
    r5::solve_iteration(w, pts, cam, seed, bk, N);  // same stream, same sample, same solutions
#pragma unroll
    for (int j = 0; j < 9; ++j) Ew[j] = w[r5::kOffE + 9 * br + j];
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) Ew[j] = __shfl(Ew[j], 0, 64);
  auto err = [&](const double* E, int p) {
    const float4 m = mrow[p];
    return lm::e_error(E, r5::norm_x(cam, m.x), r5::norm_y(cam, m.y), r5::norm_x(cam, m.z), r5::norm_y(cam, m.w));
  };
  finish_select<ModelE>(o, (size_t)b, N, best, bk, br, it, Ew, err);
}

// ---- mask launch ----------------------------------------------------------------------------------------------------------
template <bool ESSENTIAL>
__global__ void __launch_bounds__(256) lmeds_mask_kernel(const float4* __restrict__ matches, const float* __restrict__ K, int N,
                                                         const double* __restrict__ Md, const float* __restrict__ bound,
                                                         const int* __restrict__ n_inliers, unsigned char* __restrict__ mask,
                                                         float4* __restrict__ masked) {
  const size_t pair = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  double M[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) M[j] = Md[pair * 9 + j];
  const float4 m = matches[pair * N + p];
  double e;
  if (ESSENTIAL) {
    const r5::Cam cam = r5::cam_of(K + pair * 9);
    e = lm::e_error(M, r5::norm_x(cam, m.x), r5::norm_y(cam, m.y), r5::norm_x(cam, m.z), r5::norm_y(cam, m.w));
  } else {
    e = lm::f_error(M, m.x, m.y, m.z, m.w);
  }
  const bool in = n_inliers[pair] > 0 && lm::err_float(e) <= bound[pair];
  mask[pair * N + p] = in ? 1 : 0;
  if (masked != nullptr) {
    const float qn = __builtin_nanf("");
    masked[pair * N + p] = in ? m : make_float4(qn, qn, qn, qn);
  }
}

size_t lds_bytes(int N, bool essential) {
  const size_t models = essential ? (size_t)r5::kWork * kChunkL * sizeof(double) : (size_t)kChunkL * rs::kMaxRoots * 9 * sizeof(double);
  const size_t hyps = (size_t)kChunkL * (essential ? r5::kMaxRoots : rs::kMaxRoots);
  return (size_t)N * sizeof(float4) + models + hyps * sizeof(float) + (size_t)kChunkL * sizeof(int);
}

template <int R>
int launch_median(bool essential, const float4* m4, const float* K, int B, int N, int niters, unsigned long long seed, double* table,
                  hipStream_t s) {
  const size_t lds = lds_bytes(N, essential);
  const void* fn = essential ? reinterpret_cast<const void*>(lmeds_median_e_kernel<R>) : reinterpret_cast<const void*>(lmeds_median_f_kernel<R>);
  if (!opt_in_lds(fn, lds)) return DFEPE_ERR_HIP;
  const dim3 grid((niters + kChunkL - 1) / kChunkL, B);
  if (essential)
    hipLaunchKernelGGL(lmeds_median_e_kernel<R>, grid, dim3(256), lds, s, m4, K, N, niters, seed, table);
  else
    hipLaunchKernelGGL(lmeds_median_f_kernel<R>, grid, dim3(256), lds, s, m4, N, niters, seed, table);
  return DFEPE_OK;
}

int run_lmeds(bool essential, const float* matches, const float* K, int B, int N, double confidence, int max_iters, unsigned long long seed,
              void* workspace, float* M_out, unsigned char* inlier_mask, int* n_inliers, int* iters_run, int* best_hyp, double* min_median,
              double* sigma, double* hyp_medians, float* masked_matches, void* stream) {
  if (B < 0 || max_iters <= 0 || !(confidence >= 0.0 && confidence <= 1.0)) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (N < (essential ? kMinNE : kMinNF) || N > kMaxNL || B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  if (!matches || (essential && !K) || !workspace || !M_out || !inlier_mask || !n_inliers || !iters_run) return DFEPE_ERR_INVALID_ARG;
  if (!aligned16(matches) || !aligned16(workspace) || (masked_matches && !aligned16(masked_matches))) return DFEPE_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int niters = lm::num_iters(essential ? r5::kSample : rs::kSample, confidence, max_iters);
  double* Md = static_cast<double*>(workspace);
  float* bound = reinterpret_cast<float*>(Md + (size_t)B * 9);
  double* table = hyp_medians ? hyp_medians : Md + (size_t)B * 9 + ((size_t)B + 1) / 2;
  const float4* m4 = reinterpret_cast<const float4*>(matches);
  if (niters > 0) {
    int rc = DFEPE_OK;
    switch (lm::regs_for(N)) {
      case 1: rc = launch_median<1>(essential, m4, K, B, N, niters, seed, table, s); break;
      case 2: rc = launch_median<2>(essential, m4, K, B, N, niters, seed, table, s); break;
      case 4: rc = launch_median<4>(essential, m4, K, B, N, niters, seed, table, s); break;
      case 8: rc = launch_median<8>(essential, m4, K, B, N, niters, seed, table, s); break;
      case 16: rc = launch_median<16>(essential, m4, K, B, N, niters, seed, table, s); break;
      case 32: rc = launch_median<32>(essential, m4, K, B, N, niters, seed, table, s); break;
      default: rc = launch_median<64>(essential, m4, K, B, N, niters, seed, table, s); break;
    }
    if (rc != DFEPE_OK) return rc;
  }
  const SelectOut o{Md, bound, M_out, n_inliers, iters_run, best_hyp, min_median, sigma};
  const dim3 sgrid((B + kSelectWavesL - 1) / kSelectWavesL), sblock(64 * kSelectWavesL);
  float4* masked = reinterpret_cast<float4*>(masked_matches);
  if (essential) {
    hipLaunchKernelGGL(lmeds_select_e_kernel, sgrid, sblock, 0, s, m4, K, B, N, table, niters, seed, o);
    hipLaunchKernelGGL(lmeds_mask_kernel<true>, dim3((N + 255) / 256, B), dim3(256), 0, s, m4, K, N, Md, bound, n_inliers, inlier_mask, masked);
  } else {
    hipLaunchKernelGGL(lmeds_select_f_kernel, sgrid, sblock, 0, s, m4, B, N, table, niters, seed, o);
    hipLaunchKernelGGL(lmeds_mask_kernel<false>, dim3((N + 255) / 256, B), dim3(256), 0, s, m4, K, N, Md, bound, n_inliers, inlier_mask, masked);
  }
  return launched();
}

}  // namespace

extern "C" int dfepe_lmeds_num_iters(int model_points, double confidence, int max_iters) {
  if ((model_points != rs::kSample && model_points != r5::kSample) || max_iters <= 0 || !(confidence >= 0.0 && confidence <= 1.0))
    return DFEPE_ERR_INVALID_ARG;
  return lm::num_iters(model_points, confidence, max_iters);
}

extern "C" size_t dfepe_lmeds_workspace_bytes(int B, int model_points, double confidence, int max_iters) {
  if (B <= 0) return 0;
  const int niters = dfepe_lmeds_num_iters(model_points, confidence, max_iters);
  if (niters < 0) return 0;
  const size_t roots = model_points == rs::kSample ? rs::kMaxRoots : r5::kMaxRoots;
  return ((size_t)B * 9 + ((size_t)B + 1) / 2 + (size_t)B * niters * roots) * sizeof(double);
}

extern "C" int dfepe_lmeds_fundamental(const float* matches, int B, int N, double confidence, int max_iters, unsigned long long seed,
                                       void* workspace, float* F_out, unsigned char* inlier_mask, int* n_inliers, int* iters_run,
                                       int* best_hyp, double* min_median, double* sigma, double* hyp_medians, float* masked_matches,
                                       void* stream) {
  return run_lmeds(false, matches, nullptr, B, N, confidence, max_iters, seed, workspace, F_out, inlier_mask, n_inliers, iters_run, best_hyp,
                   min_median, sigma, hyp_medians, masked_matches, stream);
}

extern "C" int dfepe_lmeds_essential(const float* matches, const float* K, int B, int N, double confidence, int max_iters,
                                     unsigned long long seed, void* workspace, float* E_out, unsigned char* inlier_mask, int* n_inliers,
                                     int* iters_run, int* best_hyp, double* min_median, double* sigma, double* hyp_medians,
                                     float* masked_matches, void* stream) {
  return run_lmeds(true, matches, K, B, N, confidence, max_iters, seed, workspace, E_out, inlier_mask, n_inliers, iters_run, best_hyp,
                   min_median, sigma, hyp_medians, masked_matches, stream);
}
