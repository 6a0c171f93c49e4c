// odometry -- the reference's odometry evaluation on the device: relative poses -> trajectory (get_abs_poses, with the
// camera-to-body conjugation of Train_model_pipeline.py:1098-1108 folded in) and the snippet ATE / RE of pose_seq_ate
// (deepFEPE/utils/eval_tools.py:252-375).  The arithmetic is in odometry_math.h (shared with the host emulation of the tests);
// the contract is in include/dfepe.h.  All of it is fp64, there are no atomics, and no result depends on the order in which
// workgroups or wavefronts arrive: two runs give the same bits.
//
// pose_chain_kernel: an inclusive scan over a non-commutative group.  One workgroup per sequence walks the sequence in tiles of
// kChainThreads * kChainChunk poses:
//   1 lane t composes its kChainChunk consecutive poses in order, local = P_last ... P_first (the later operand on the left);
//   2 the lane totals are scanned across the wavefront with __shfl_up (Hillis-Steele, six steps: incl = incl . incl[lane - d]),
//     the wavefront totals go through LDS, and every lane forms  prefix = incl[lane - 1] . (W_{w-1} ... W_0 . carry);
//   3 the lane walks its chunk again, cur = P . cur from its prefix, and stores inv(cur);
//   4 carry = W_3 . W_2 . W_1 . W_0 . carry, the same value in every lane, for the next tile.
// A lane without poses contributes the identity, which affine_mul passes through bit for bit, so the first kChainChunk poses of
// a sequence are exactly the sequential result.
#include "dfepe_common.h"
#include "odometry_math.h"

namespace {

constexpr int kChainThreads = 256;  // _lib.POSE_CHAIN_THREADS
constexpr int kChainChunk = 8;      // _lib.POSE_CHAIN_CHUNK: poses per lane and tile
constexpr int kChainWaves = kChainThreads / WAVE;
constexpr int kChainTile = kChainThreads * kChainChunk;
constexpr int kSnipThreads = 256;
constexpr int kSnipMaxL = 64;

__device__ __forceinline__ odo::Aff shfl_up_aff(const odo::Aff& a, int d) {
  odo::Aff r;
#pragma unroll
  for (int k = 0; k < 12; ++k) r.m[k] = __shfl_up(a.m[k], (unsigned)d, WAVE);
  return r;
}

__device__ __forceinline__ odo::Aff chain_pose(const double* __restrict__ rel, const double* __restrict__ c2b, long c2b_stride,
                                               int j) {
  const odo::Aff M = odo::load(rel + 12L * j);
  if (c2b == nullptr) return M;
  return odo::conjugate(M, odo::load(c2b + c2b_stride * j));
}

__global__ void __launch_bounds__(kChainThreads) pose_chain_kernel(const double* __restrict__ rel, const int* __restrict__ lengths,
                                                                   const double* __restrict__ cam2body, long c2b_stride, int n_max,
                                                                   double* __restrict__ abs_out) {
  __shared__ double wtot[kChainWaves][12];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  int n = (lengths != nullptr) ? lengths[s] : n_max;
  n = min(max(n, 0), n_max);
  const double* R = rel + (long)s * n_max * 12;
  const double* C = (cam2body != nullptr) ? cam2body + (long)s * (c2b_stride != 0 ? 12L * n_max : 12L) : nullptr;
  double* A = abs_out + (long)s * (n_max + 1) * 12;
  if (tid == 0) odo::store(A, odo::identity());
  odo::Aff carry = odo::identity();
  for (int base = 0; base < n; base += kChainTile) {
    const int j0 = min(base + tid * kChainChunk, n), j1 = min(j0 + kChainChunk, n);
    odo::Aff incl = odo::identity();
    for (int j = j0; j < j1; ++j) incl = odo::affine_mul(chain_pose(R, C, c2b_stride, j), incl);
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const odo::Aff o = shfl_up_aff(incl, d);
      if (lane >= d) incl = odo::affine_mul(incl, o);
    }
    if (lane == WAVE - 1) odo::store(wtot[wave], incl);
    __syncthreads();
    odo::Aff prefix = carry;
#pragma unroll
    for (int w = 0; w < kChainWaves; ++w) {
      const odo::Aff t = odo::load(wtot[w]);
      if (w < wave) prefix = odo::affine_mul(t, prefix);
      carry = odo::affine_mul(t, carry);
    }
    const odo::Aff excl = shfl_up_aff(incl, 1);
    if (lane > 0) prefix = odo::affine_mul(excl, prefix);
    odo::Aff cur = prefix;
    for (int j = j0; j < j1; ++j) {
      cur = odo::affine_mul(chain_pose(R, C, c2b_stride, j), cur);
      odo::store(A + 12L * (j + 1), odo::affine_inv(cur));
    }
    __syncthreads();  // wtot is rewritten by the next tile
  }
}

// Sum of one value per thread in a fixed order (a binary tree over the thread index), the same in every thread afterwards.
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = kSnipThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// One workgroup per sequence, one lane per window (a lane takes windows tid, tid + 256, ...).  The statistics are a two-pass
// reduction over the float32-rounded errors: every lane adds its own windows in ascending order, block_sum adds the lanes.
__global__ void __launch_bounds__(kSnipThreads) snippet_errors_kernel(const double* __restrict__ est, const double* __restrict__ gt,
                                                                      const int* __restrict__ windows, int m_max, int W, int L,
                                                                      int compensate, float* __restrict__ errors,
                                                                      double* __restrict__ scale, double* __restrict__ aligned,
                                                                      double* __restrict__ compensated, double* __restrict__ stats) {
  __shared__ double red[kSnipThreads];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int nw = min(max(windows[s], 0), max(min(W, m_max - L + 1), 0));  // never past the buffers, whatever windows holds
  const double* E = est + (long)s * m_max * 12;
  const double* G = gt + (long)s * m_max * 12;
  double sum_a = 0.0, sum_r = 0.0;
  for (int w = tid; w < nw; w += kSnipThreads) {
    const long o = (long)s * W + w;
    const odo::Snippet r = odo::snippet(E + 12L * w, G + 12L * w, L, compensate != 0,
                                        compensated != nullptr ? compensated + o * L * 12 : nullptr);
    const float fa = (float)r.ate, fr = (float)r.re;
    errors[2 * o] = fa;
    errors[2 * o + 1] = fr;
    scale[o] = r.scale;
    odo::store(aligned + 12 * o, odo::aligned_pose(E + 12L * w, r.scale));
    sum_a = sum_a + (double)fa;
    sum_r = sum_r + (double)fr;
  }
  const double mean_a = block_sum(sum_a, red) / (double)nw;  // nw == 0: 0 / 0 = NaN, as numpy's mean of nothing
  const double mean_r = block_sum(sum_r, red) / (double)nw;
  double dev_a = 0.0, dev_r = 0.0;
  for (int w = tid; w < nw; w += kSnipThreads) {
    const long o = (long)s * W + w;
    const double da = (double)errors[2 * o] - mean_a, dr = (double)errors[2 * o + 1] - mean_r;  // this lane's own stores
    dev_a = dev_a + da * da;
    dev_r = dev_r + dr * dr;
  }
  const double var_a = block_sum(dev_a, red) / (double)nw;
  const double var_r = block_sum(dev_r, red) / (double)nw;
  if (tid == 0) {
    stats[4 * s] = mean_a;
    stats[4 * s + 1] = sqrt(var_a);
    stats[4 * s + 2] = mean_r;
    stats[4 * s + 3] = sqrt(var_r);
  }
}

}  // namespace

extern "C" int dfepe_pose_chain(void* stream, const double* rel, const int* lengths, const double* cam2body, long c2b_stride, int S,
                                int n_max, double* abs_out) {
  if (S < 0 || n_max < 0 || (c2b_stride != 0 && c2b_stride != 12)) return DFEPE_ERR_INVALID_ARG;
  if (S == 0) return DFEPE_OK;  // nothing to read or write: empty tensors have no address
  if (!abs_out || (n_max > 0 && !rel)) return DFEPE_ERR_INVALID_ARG;
  if (n_max > 0x7fffffff / 12 - 1) return DFEPE_ERR_UNSUPPORTED;  // 12 j is formed in int
  hipLaunchKernelGGL(pose_chain_kernel, dim3((unsigned)S), dim3(kChainThreads), 0, static_cast<hipStream_t>(stream), rel, lengths,
                     cam2body, c2b_stride, n_max, abs_out);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

extern "C" int dfepe_snippet_errors(void* stream, const double* est, const double* gt, const int* windows, int S, int m_max, int W,
                                    int L, int no_compensate, float* errors, double* scale, double* aligned, double* compensated,
                                    double* stats) {
  if (S < 0 || m_max < 0 || W < 0) return DFEPE_ERR_INVALID_ARG;
  if (L < 1 || L > kSnipMaxL) return DFEPE_ERR_UNSUPPORTED;
  if (S == 0) return DFEPE_OK;
  if (!windows || !stats) return DFEPE_ERR_INVALID_ARG;
  if (W > 0 && (!est || !gt || !errors || !scale || !aligned)) return DFEPE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(snippet_errors_kernel, dim3((unsigned)S), dim3(kSnipThreads), 0, static_cast<hipStream_t>(stream), est, gt,
                     windows, m_max, W, L, no_compensate ? 0 : 1, errors, scale, aligned, compensated, stats);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
