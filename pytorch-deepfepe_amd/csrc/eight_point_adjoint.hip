// Adjoint of the textbook normalised eight-point solvers of dsac_tools.utils_F (_F_from_XY, _E_from_XY, _E_from_XY_batch;
// utils_F.py:104-275), i.e. of dfepe_w8pt_fwd with DFEPE_W8PT_SQRT2 | NO_ROWNORM: gradients to the points and to the weights.  The
// per-problem arithmetic is csrc/eight_point_adjoint_math.h, the contract include/dfepe.h.
//
// Layout.  A problem is one pair under one weight set; problem = set * B + pair.  One wavefront per problem, four problems per
// workgroup (the wavefronts of a workgroup never meet: no barrier).  A wavefront makes four passes over its correspondences, lane l
// taking n = l, l + 64, ... (float2 loads of consecutive points): the centroids, the mean distances, the 45 entries of M9 = A^T A,
// and, after the dense step, the per-point gradients.  Every sum is fp64, per lane in order and then across the wavefront with
// wave_sum (a balanced tree).  The dense step (9x9 Jacobi, 3x3 SVD, the rank-2 adjoint, u) runs once per problem, in lane 0, with
// its two 9x9 matrices in LDS: held per lane they would cost 324 VGPRs.
// With one weight set the point gradients are written at once.  With several, each problem writes its four doubles per
// correspondence to the workspace [S,B,N,4] and a second launch on the same stream adds the sets in ascending order and rounds once.
// No atomics: a problem's outputs are the same bits on every run and whatever else is in the batch.
#include "dfepe_common.h"

#include "eight_point_adjoint_math.h"

namespace {

constexpr int kThreads = e8::kProblemsPerBlock * WAVE;
constexpr unsigned kRequired = DFEPE_W8PT_SQRT2 | DFEPE_W8PT_NO_ROWNORM;
constexpr unsigned kAllowed = kRequired | DFEPE_W8PT_FORCE_110 | DFEPE_W8PT_NO_HARTLEY;
constexpr long long kMaxPoints = 2147483647LL;  // S * B * N

struct Args {
  const float *X, *Y, *w, *F_out, *g_F;
  float *g_X, *g_Y, *g_w;
  double* partial;  // [S,B,N,4], used when S > 1 and a point gradient is asked for
  int B, N, S;
  unsigned flags;
};

__global__ void __launch_bounds__(kThreads) eight_point_adjoint_kernel(Args p) {
  __shared__ double work[e8::kProblemsPerBlock][e8::kDenseDoubles];
  __shared__ double m45s[e8::kProblemsPerBlock][45];
  __shared__ double fu[e8::kProblemsPerBlock][18];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long problem = (long long)blockIdx.x * e8::kProblemsPerBlock + wave;
  if (problem >= (long long)p.S * p.B) return;  // wave-uniform
  const size_t pair = (size_t)(problem % p.B);
  const int N = p.N;
  const bool hartley = (p.flags & DFEPE_W8PT_NO_HARTLEY) == 0;
  const bool force110 = (p.flags & DFEPE_W8PT_FORCE_110) != 0;
  const float2* __restrict__ X = reinterpret_cast<const float2*>(p.X) + pair * N;
  const float2* __restrict__ Y = reinterpret_cast<const float2*>(p.Y) + pair * N;
  const float* __restrict__ w = p.w ? p.w + (size_t)problem * N : nullptr;

  e8::Norm t1 = {0.0, 0.0, 1.0}, t2 = {0.0, 0.0, 1.0};
  if (hartley) {
    double sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
    for (int n = lane; n < N; n += WAVE) {
      const float2 a = X[n], b = Y[n];
      sx1 += (double)a.x; sy1 += (double)a.y; sx2 += (double)b.x; sy2 += (double)b.y;
    }
    t1.cx = wave_sum(sx1) / (double)N; t1.cy = wave_sum(sy1) / (double)N;
    t2.cx = wave_sum(sx2) / (double)N; t2.cy = wave_sum(sy2) / (double)N;
    double d1 = 0.0, d2 = 0.0;
    for (int n = lane; n < N; n += WAVE) {
      const float2 a = X[n], b = Y[n];
      const double ax = (double)a.x - t1.cx, ay = (double)a.y - t1.cy, bx = (double)b.x - t2.cx, by = (double)b.y - t2.cy;
      d1 += sqrt(ax * ax + ay * ay);
      d2 += sqrt(bx * bx + by * by);
    }
    t1.s = sqrt(2.0) / (wave_sum(d1) / (double)N);
    t2.s = sqrt(2.0) / (wave_sum(d2) / (double)N);
  }

  double m[45];
#pragma unroll
  for (int k = 0; k < 45; ++k) m[k] = 0.0;
  for (int n = lane; n < N; n += WAVE) {
    const float2 a = X[n], b = Y[n];
    double p1[2], p2[2], r[9];
    e8::normalized(t1, hartley, (double)a.x, (double)a.y, p1);
    e8::normalized(t2, hartley, (double)b.x, (double)b.y, p2);
    e8::row(p1, p2, r);
    e8::accumulate(r, w ? (double)w[n] : 1.0, m);
  }
#pragma unroll
  for (int k = 0; k < 45; ++k) m[k] = wave_sum(m[k]);

  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 45; ++k) m45s[wave][k] = m[k];
    double Fo[9], gF[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      Fo[c] = (double)p.F_out[(size_t)problem * 9 + c];
      gF[c] = (double)p.g_F[(size_t)problem * 9 + c];
    }
    e8::dense_step(m45s[wave], t1, t2, hartley, force110, Fo, gF, work[wave], fu[wave], fu[wave] + 9);
  }
  wave_sync();
  double f[9], u[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    f[c] = fu[wave][c];
    u[c] = fu[wave][9 + c];
  }
  const double sc1 = hartley ? t1.s / e8::kDeHomo : 1.0, sc2 = hartley ? t2.s / e8::kDeHomo : 1.0;
  const bool want_pts = p.g_X != nullptr || p.g_Y != nullptr;
  const size_t prow = (size_t)problem * N;  // row of [S,B,N]
  for (int n = lane; n < N; n += WAVE) {
    const float2 a = X[n], b = Y[n];
    double p1[2], p2[2], gp[4], gw;
    e8::normalized(t1, hartley, (double)a.x, (double)a.y, p1);
    e8::normalized(t2, hartley, (double)b.x, (double)b.y, p2);
    e8::point_adjoint(p1, p2, w ? (double)w[n] : 1.0, f, u, sc1, sc2, N == 8, gp, &gw);
    if (p.g_w) p.g_w[prow + n] = (float)gw;
    if (p.S == 1) {
      if (p.g_X) reinterpret_cast<float2*>(p.g_X)[pair * N + n] = make_float2((float)gp[0], (float)gp[1]);
      if (p.g_Y) reinterpret_cast<float2*>(p.g_Y)[pair * N + n] = make_float2((float)gp[2], (float)gp[3]);
    } else if (want_pts) {
      double2* dst = reinterpret_cast<double2*>(p.partial) + (prow + n) * 2;
      dst[0] = make_double2(gp[0], gp[1]);
      dst[1] = make_double2(gp[2], gp[3]);
    }
  }
}

// g_X[b,n], g_Y[b,n] = the sets' partial gradients added in ascending set order, rounded once.
__global__ void __launch_bounds__(256) eight_point_set_sum_kernel(const double* __restrict__ partial, size_t points, int S,
                                                                  float* __restrict__ g_X, float* __restrict__ g_Y) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // pair * N + n
  if (i >= points) return;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int s = 0; s < S; ++s) {
    const double2* src = reinterpret_cast<const double2*>(partial) + ((size_t)s * points + i) * 2;
    const double2 u = src[0], v = src[1];
    a0 += u.x; a1 += u.y; a2 += v.x; a3 += v.y;
  }
  if (g_X) reinterpret_cast<float2*>(g_X)[i] = make_float2((float)a0, (float)a1);
  if (g_Y) reinterpret_cast<float2*>(g_Y)[i] = make_float2((float)a2, (float)a3);
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" size_t dfepe_eight_point_bwd_workspace_bytes(int B, int N, int n_weight_sets) {
  if (B <= 0 || N <= 0 || n_weight_sets <= 1) return 0;
  return (size_t)n_weight_sets * B * N * 4 * sizeof(double);
}

extern "C" int dfepe_eight_point_bwd(void* stream, const float* X, const float* Y, const float* w, int B, int N, int n_weight_sets,
                                     unsigned flags, const float* F_out, const float* g_F, float* g_X, float* g_Y, float* g_w,
                                     void* workspace) {
  const int S = n_weight_sets;
  if (B < 0 || N < 8 || S < 1) return DFEPE_ERR_INVALID_ARG;
  if ((flags & kRequired) != kRequired || (flags & ~kAllowed) != 0) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!X || !Y || !F_out || !g_F || (!g_X && !g_Y && !g_w)) return DFEPE_ERR_INVALID_ARG;
  if (!aligned8(X) || !aligned8(Y) || !aligned8(g_X) || !aligned8(g_Y)) return DFEPE_ERR_INVALID_ARG;
  const bool needs_ws = S > 1 && (g_X || g_Y);
  if (needs_ws && (!workspace || !aligned16(workspace))) return DFEPE_ERR_INVALID_ARG;
  if ((long long)S * B * N > kMaxPoints) return DFEPE_ERR_UNSUPPORTED;
  const Args a = {X, Y, w, F_out, g_F, g_X, g_Y, g_w, static_cast<double*>(workspace), B, N, S, flags};
  const long long problems = (long long)S * B;
  const unsigned grid = (unsigned)((problems + e8::kProblemsPerBlock - 1) / e8::kProblemsPerBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(eight_point_adjoint_kernel, dim3(grid), dim3(kThreads), 0, st, a);
  if (needs_ws) {
    const size_t points = (size_t)B * N;
    hipLaunchKernelGGL(eight_point_set_sum_kernel, dim3((unsigned)((points + 255) / 256)), dim3(256), 0, st,
                       static_cast<const double*>(workspace), points, S, g_X, g_Y);
  }
  return launched();
}
