// triangulate -- two-view structure: batched cv2.triangulatePoints, the points and depths of a recovered pose (the body of the
// reference's DeepFNet.get_depth, models/DeepFNet.py:406-427, after cv2.recoverPose) and the projection of points into an image
// (the numeric part of dsac_tools/utils_vis.reproj_and_scatter).  The per-lane arithmetic is in triangulate_math.h (shared with
// the host emulation of the tests); the contract is in include/dfepe.h.
//
// One lane per correspondence on a (ceil(N / 64), B) grid like ransac_in_front_kernel: a pair's matrices have a workgroup-uniform
// address and arrive through scalar loads, every lane forms the pair's cameras for itself (a few dozen fp64 operations next to
// the ~5 000 of the null vector), the match is one float4 load.  No LDS, no atomics, no scratch (profiles/triangulate.md).
#include "dfepe_common.h"
#include "triangulate_math.h"

namespace {

constexpr int kTriBlock = 64;

__global__ void __launch_bounds__(kTriBlock) triangulate_kernel(const float* __restrict__ P1, int p1_stride, const float* __restrict__ P2,
                                                                int p2_stride, const float4* __restrict__ matches, int N,
                                                                float4* __restrict__ Xh) {
  const size_t pair = blockIdx.y;
  const int p = blockIdx.x * kTriBlock + threadIdx.x;
  if (p >= N) return;
  const float* A = P1 + pair * p1_stride;
  const float* B = P2 + pair * p2_stride;
  double Ad[12], Bd[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) { Ad[k] = (double)A[k]; Bd[k] = (double)B[k]; }
  const float4 m = matches[pair * N + p];
  double X[4];
  const float qn = __builtin_nanf("");
  float4 out = make_float4(qn, qn, qn, qn);
  if (tri::null_vector(Ad, Bd, (double)m.x, (double)m.y, (double)m.z, (double)m.w, X))
    out = make_float4((float)X[0], (float)X[1], (float)X[2], (float)X[3]);
  Xh[pair * N + p] = out;
}

__global__ void __launch_bounds__(kTriBlock) two_view_structure_kernel(const float* __restrict__ Rt, unsigned flags, const float* __restrict__ K,
                                                                       const float4* __restrict__ matches, int N, const int* __restrict__ winner,
                                                                       const float* __restrict__ scale, float clamp, float* __restrict__ X,
                                                                       float* __restrict__ z1, float* __restrict__ z2) {
  const size_t pair = blockIdx.y;
  const int p = blockIdx.x * kTriBlock + threadIdx.x;
  if (p >= N) return;
  const size_t i = pair * N + p;
  tri::Structure s;
  s.X[0] = s.X[1] = s.X[2] = s.z1 = s.z2 = tri::qnan();
  if (winner == nullptr || winner[pair] >= 0) {
    double R[9], t[3], P1[12], P2[12];
    tri::scene_motion(Rt + pair * 12, flags, R, t);
    tri::cameras(K + pair * 9, R, t, P1, P2);
    const float4 m = matches[i];
    s = tri::structure(P1, P2, R, t, (double)m.x, (double)m.y, (double)m.z, (double)m.w,
                       scale != nullptr ? (double)scale[pair] : 1.0, (double)clamp);
  }
  if (X != nullptr) { X[3 * i] = (float)s.X[0]; X[3 * i + 1] = (float)s.X[1]; X[3 * i + 2] = (float)s.X[2]; }
  if (z1 != nullptr) z1[i] = (float)s.z1;
  if (z2 != nullptr) z2[i] = (float)s.z2;
}

__global__ void __launch_bounds__(kTriBlock) reproject_kernel(const float* __restrict__ X, const float* __restrict__ Rt, int rt_stride,
                                                              unsigned flags, const float* __restrict__ K, int k_stride, int M, float image_w,
                                                              float image_h, float* __restrict__ x, float* __restrict__ z,
                                                              unsigned char* __restrict__ inside) {
  const size_t pair = blockIdx.y;
  const int p = blockIdx.x * kTriBlock + threadIdx.x;
  if (p >= M) return;
  const size_t i = pair * M + p;
  double R[9], t[3], u[3];
  tri::scene_motion(Rt + pair * rt_stride, flags, R, t);
  tri::project(K + pair * k_stride, R, t, (double)X[3 * i], (double)X[3 * i + 1], (double)X[3 * i + 2], u);
  const float xf = (float)(u[0] / u[2]), yf = (float)(u[1] / u[2]);
  x[2 * i] = xf;
  x[2 * i + 1] = yf;
  if (z != nullptr) z[i] = (float)u[2];
  if (inside != nullptr) inside[i] = tri::within(xf, yf, image_w, image_h) ? 1 : 0;
}

bool stride_ok(int s, int row) { return s == 0 || s == row; }

}  // namespace

extern "C" int dfepe_triangulate(const float* P1, int p1_stride, const float* P2, int p2_stride, const float* matches, int B, int N,
                                 float* Xh, void* stream) {
  if (B < 0 || N < 0 || !stride_ok(p1_stride, 12) || !stride_ok(p2_stride, 12)) return DFEPE_ERR_INVALID_ARG;
  if (B == 0 || N == 0) return DFEPE_OK;
  if (!P1 || !P2 || !matches || !Xh || !aligned16(matches) || !aligned16(Xh)) return DFEPE_ERR_INVALID_ARG;
  if (B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(triangulate_kernel, dim3((N + kTriBlock - 1) / kTriBlock, B), dim3(kTriBlock), 0, static_cast<hipStream_t>(stream), P1,
                     p1_stride, P2, p2_stride, reinterpret_cast<const float4*>(matches), N, reinterpret_cast<float4*>(Xh));
  return launched();
}

extern "C" int dfepe_two_view_structure(const float* Rt, unsigned flags, const float* K, const float* matches, int B, int N,
                                        const int* winner, const float* scale, float clamp, float* X, float* z1, float* z2, void* stream) {
  if (B < 0 || N < 0 || (flags & ~DFEPE_POSE_CAMERA_MOTION) != 0u) return DFEPE_ERR_INVALID_ARG;
  if (B == 0 || N == 0) return DFEPE_OK;
  if (!Rt || !K || !matches || !aligned16(matches) || (!X && !z1 && !z2)) return DFEPE_ERR_INVALID_ARG;
  if (B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(two_view_structure_kernel, dim3((N + kTriBlock - 1) / kTriBlock, B), dim3(kTriBlock), 0, static_cast<hipStream_t>(stream),
                     Rt, flags, K, reinterpret_cast<const float4*>(matches), N, winner, scale, clamp, X, z1, z2);
  return launched();
}

extern "C" int dfepe_reproject(const float* X, const float* Rt, int rt_stride, unsigned flags, const float* K, int k_stride, int B, int M,
                               float image_w, float image_h, float* x, float* z, unsigned char* inside, void* stream) {
  if (B < 0 || M < 0 || (flags & ~DFEPE_POSE_CAMERA_MOTION) != 0u || !stride_ok(rt_stride, 12) || !stride_ok(k_stride, 9))
    return DFEPE_ERR_INVALID_ARG;
  if (B == 0 || M == 0) return DFEPE_OK;
  if (!X || !Rt || !K || !x) return DFEPE_ERR_INVALID_ARG;
  if (B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(reproject_kernel, dim3((M + kTriBlock - 1) / kTriBlock, B), dim3(kTriBlock), 0, static_cast<hipStream_t>(stream), X, Rt,
                     rt_stride, flags, K, k_stride, M, image_w, image_h, x, z, inside);
  return launched();
}
