// correct_matches -- batched optimal correction of correspondences onto a given epipolar geometry (Hartley & Sturm; OpenCV's
// correctMatches, which the reference's loader calls per sample on its 10 x 10 grid of virtual points,
// dsac_tools/utils_misc.py:163-230).  The per-lane arithmetic is in correct_matches_math.h (shared with the host emulation of the
// tests); the contract is in include/dfepe.h.
//
// One lane per (pair, point) on a flat grid: the points share nothing but their pair's F (nine doubles, read through the cache by
// every lane), so there is no LDS and no wavefront operation.  All arithmetic is fp64; the points are read and written as fp32.
#include "dfepe_common.h"
#include "correct_matches_math.h"

namespace {

constexpr int kCmBlock = 256;

__global__ void __launch_bounds__(kCmBlock) correct_matches_kernel(const double* __restrict__ F, long f_stride,
                                                                   const float* __restrict__ p, const float* __restrict__ q,
                                                                   long total, int M, float* __restrict__ p_out,
                                                                   float* __restrict__ q_out, float* __restrict__ cost) {
  const long i = (long)blockIdx.x * kCmBlock + threadIdx.x;
  if (i >= total) return;
  const double* Fp = F + (i / M) * f_stride;
  double Fl[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) Fl[j] = Fp[j];
  const cm::Result r = cm::correct<false>(Fl, (double)p[2 * i], (double)p[2 * i + 1], (double)q[2 * i], (double)q[2 * i + 1],
                                          nullptr, nullptr);
  p_out[2 * i] = (float)r.x1;
  p_out[2 * i + 1] = (float)r.y1;
  q_out[2 * i] = (float)r.x2;
  q_out[2 * i + 1] = (float)r.y2;
  if (cost != nullptr) cost[i] = (float)r.cost;
}

}  // namespace

extern "C" int dfepe_correct_matches(void* stream, const double* F, long f_stride, const float* p, const float* q, int B, int M,
                                     float* p_out, float* q_out, float* cost) {
  if (B < 0 || M < 0 || (f_stride != 0 && f_stride != 9)) return DFEPE_ERR_INVALID_ARG;
  if (B == 0 || M == 0) return DFEPE_OK;  // nothing to read or write: empty tensors have no address
  if (!F || !p || !q || !p_out || !q_out) return DFEPE_ERR_INVALID_ARG;
  const long total = (long)B * M;
  const long blocks = (total + kCmBlock - 1) / kCmBlock;
  if (blocks > 0x7fffffffL) return DFEPE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(correct_matches_kernel, dim3((unsigned)blocks), dim3(kCmBlock), 0, static_cast<hipStream_t>(stream), F, f_stride,
                     p, q, total, M, p_out, q_out, cost);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
