// Adjoints of the epipolar distances of dsac_tools.utils_F (utils_F.py:291-361, 400-413): gradients to F and to the points, and the
// reduced loss form sum_n w e with its adjoint.  The per-point arithmetic is csrc/epi_adjoint_math.h, the contract include/dfepe.h.
//
// Layout.  One lane per correspondence.  A workgroup of 256 lanes owns a chunk of ea::kChunk consecutive points of ONE pair: block
// index = pair * chunks + chunk, so the pair's nine F values are wave-uniform loads, widened once.  Inside the chunk a wavefront
// walks slabs of 64 consecutive points (slab = 4 k + wave, k = 0 .. 3), so what it loads and stores at a time is one contiguous
// run: float2 per lane for [B,N,2] points; for the 12-byte homogeneous rows three dword accesses of 64 consecutive words each,
// turned into rows through a wave-private LDS strip (stride 3 words: no bank conflict).
// Reduction of the nine fp64 partial sums of g_F (and of the one of the loss), in a fixed order: per lane over its slabs in order,
// across the wavefront with wave_sum, the four wavefront totals in order through LDS; with one chunk per pair the workgroup writes
// the result itself, otherwise its doubles go to the caller's workspace slot [B, chunks, 9] and a second small launch on the same
// stream adds the chunks in ascending order.  No atomics: a pair's result is the same bits on every run and whatever else is in
// the batch.
#include "dfepe_common.h"

#include "epi_adjoint_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / WAVE;
constexpr int kSlabs = ea::kChunk / WAVE;  // slabs of 64 points per chunk
static_assert(ea::kChunk % kThreads == 0, "a chunk is a whole number of passes of the workgroup");

struct Args {
  const float *F, *X, *Y;
  const float* g_out;  // metrics: [B,N] or [3,B,N]
  const float* g_sum;  // loss: [B]
  const float* w;      // loss: [B,N] or null
  float *g_F, *g_X, *g_Y, *g_w, *sum_out;
  double* partial;  // [B, chunks, 9] (adjoint) or [B, chunks] (loss forward); used when chunks > 1
  int B, N, chunks, kind;
  float clamp_at, eps;
};

// The lane's point of the slab that starts at row `row0` (pair * N + first point); `nv` of its 64 points exist.
template <bool HOMO>
__device__ __forceinline__ void load_point(const float* __restrict__ P, size_t row0, int nv, int lane, float* strip, double* x) {
  if (HOMO) {
    const float* base = P + row0 * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int o = j * WAVE + lane;
      strip[o] = (o < 3 * nv) ? base[o] : 0.f;
    }
    wave_sync();
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = (double)strip[3 * lane + k];
    wave_sync();
  } else {
    float2 v = make_float2(0.f, 0.f);
    if (lane < nv) v = reinterpret_cast<const float2*>(P)[row0 + lane];
    x[0] = (double)v.x; x[1] = (double)v.y; x[2] = 1.0;
  }
}

template <bool HOMO>
__device__ __forceinline__ void store_point(float* __restrict__ P, size_t row0, int nv, int lane, float* strip, const double* g) {
  if (HOMO) {
#pragma unroll
    for (int k = 0; k < 3; ++k) strip[3 * lane + k] = (float)g[k];
    wave_sync();
    float* base = P + row0 * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int o = j * WAVE + lane;
      if (o < 3 * nv) base[o] = strip[o];
    }
    wave_sync();
  } else {
    if (lane < nv) reinterpret_cast<float2*>(P)[row0 + lane] = make_float2((float)g[0], (float)g[1]);
  }
}

// The NC partial sums of the workgroup, in the fixed order; all 256 lanes call it.
template <int NC>
__device__ __forceinline__ void block_reduce_write(double* acc, double (*red)[9], int wave, int lane, int chunks, size_t pair,
                                                   int chunk, float* out, double* partial) {
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = wave_sum(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) red[wave][c] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    const int c = threadIdx.x;
    const double tot = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
    if (chunks == 1) out[pair * NC + c] = (float)tot;
    else partial[(pair * chunks + chunk) * NC + c] = tot;
  }
}

// MODE 0: dfepe_epi_metrics_bwd (upstream g_out per point), 1: dfepe_epi_loss_bwd (upstream g_sum[pair] * w), 2: dfepe_epi_loss_fwd
template <bool HOMO, int MODE>
__global__ void __launch_bounds__(kThreads) epi_adjoint_kernel(Args p) {
  __shared__ float strips[kWaves][3 * WAVE];
  __shared__ double red[kWaves][9];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t pair = blockIdx.x / (unsigned)p.chunks;
  const int chunk = blockIdx.x % (unsigned)p.chunks;
  double f[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) f[c] = (double)p.F[pair * 9 + c];
  const int kind = p.kind;
  const double clamp_at = (double)p.clamp_at, eps = (double)p.eps;
  const double gs = (MODE == 1) ? (double)p.g_sum[pair] : 1.0;
  const size_t plane = (size_t)p.B * p.N;
  const bool want_F = (MODE == 2) || p.g_F != nullptr;
  double acc[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) acc[c] = 0.0;
  float* strip = strips[wave];
#pragma clang loop unroll(disable)
  for (int k = 0; k < kSlabs / kWaves; ++k) {
    const long long i0 = (long long)chunk * ea::kChunk + (k * kWaves + wave) * WAVE;  // wave-uniform; N may be close to 2^31
    if (i0 >= p.N) break;
    const int nv = (int)min((long long)WAVE, p.N - i0);
    const size_t row0 = pair * p.N + (size_t)i0;
    const bool valid = lane < nv;
    double x[3], y[3];
    load_point<HOMO>(p.X, row0, nv, lane, strip, x);
    load_point<HOMO>(p.Y, row0, nv, lane, strip, y);
    const ea::Terms t = ea::terms(f, x, y);
    double wgt = 1.0;
    if (MODE != 0 && p.w != nullptr && valid) wgt = (double)p.w[row0 + lane];
    if (MODE == 2) {
      const double e = wgt * ea::value(kind, t, clamp_at, eps);
      acc[0] += valid ? e : 0.0;
      continue;
    }
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    if (MODE == 0) {
      if (valid) {
        g0 = (double)p.g_out[row0 + lane];
        if (kind == 2) {
          g1 = (double)p.g_out[plane + row0 + lane];
          g2 = (double)p.g_out[2 * plane + row0 + lane];
        }
      }
    } else {
      g0 = gs * wgt;
      if (p.g_w != nullptr && valid) p.g_w[row0 + lane] = (float)(gs * ea::value(kind, t, clamp_at, eps));
    }
    double cs, cA, cQ, gF[9], gx[3], gy[3];
    ea::coeffs(kind, t, clamp_at, eps, g0, g1, g2, &cs, &cA, &cQ);
    ea::point_adjoint(f, x, y, t, cs, cA, cQ, gF, gx, gy);
    if (p.g_X != nullptr) store_point<HOMO>(p.g_X, row0, nv, lane, strip, gx);
    if (p.g_Y != nullptr) store_point<HOMO>(p.g_Y, row0, nv, lane, strip, gy);
    if (want_F) {
#pragma unroll
      for (int c = 0; c < 9; ++c) acc[c] += valid ? gF[c] : 0.0;
    }
  }
  if (MODE == 2) block_reduce_write<1>(acc, red, wave, lane, p.chunks, pair, chunk, p.sum_out, p.partial);
  else if (want_F) block_reduce_write<9>(acc, red, wave, lane, p.chunks, pair, chunk, p.g_F, p.partial);
}

// out[pair, c] = the chunks' partial sums added in ascending order, rounded once.
__global__ void __launch_bounds__(kThreads) epi_chunk_sum_kernel(const double* __restrict__ partial, size_t cells, int chunks, int nc,
                                                                 float* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;  // pair * nc + c
  if (idx >= cells) return;
  const size_t pair = idx / nc, c = idx % nc;
  double tot = 0.0;
  for (int k = 0; k < chunks; ++k) tot += partial[(pair * chunks + k) * nc + c];
  out[idx] = (float)tot;
}

__global__ void __launch_bounds__(kThreads) epi_residual_pts_kernel(const float* __restrict__ pts1, const float* __restrict__ pts2,
                                                                    const float* __restrict__ F, int N, int chunks, float clamp_at,
                                                                    const float* __restrict__ g_out, float* __restrict__ g_pts1,
                                                                    float* __restrict__ g_pts2) {
  __shared__ float strips[kWaves][3 * WAVE];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t pair = blockIdx.x / (unsigned)chunks;
  const int chunk = blockIdx.x % (unsigned)chunks;
  double f[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) f[c] = (double)F[pair * 9 + c];
  float* strip = strips[wave];
#pragma clang loop unroll(disable)
  for (int k = 0; k < kSlabs / kWaves; ++k) {
    const long long i0 = (long long)chunk * ea::kChunk + (k * kWaves + wave) * WAVE;
    if (i0 >= N) break;
    const int nv = (int)min((long long)WAVE, N - i0);
    const size_t row0 = pair * N + (size_t)i0;
    double x1[3], x2[3], g1[3], g2[3];
    load_point<true>(pts1, row0, nv, lane, strip, x1);
    load_point<true>(pts2, row0, nv, lane, strip, x2);
    const double g = (lane < nv) ? (double)g_out[row0 + lane] : 0.0;
    ea::residual_point_adjoint(f, x1, x2, (double)clamp_at, g, g1, g2);
    if (g_pts1 != nullptr) store_point<true>(g_pts1, row0, nv, lane, strip, g1);
    if (g_pts2 != nullptr) store_point<true>(g_pts2, row0, nv, lane, strip, g2);
  }
}

inline int chunks_of(int N) { return (int)(((long long)N + ea::kChunk - 1) / ea::kChunk); }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
constexpr long long kMaxPoints = 2147483647LL;  // B * N

// The refusals every entry shares, in the documented order.  > 0: nothing to do (return DFEPE_OK).
inline int common_checks(int kind, int B, int N, float clamp_at) {
  if (B < 0 || N < 0 || kind < 0 || (kind & ~DFEPE_EPI_HOMOGENEOUS) > 2) return DFEPE_ERR_INVALID_ARG;
  if ((kind & 7) != 0 && clamp_at >= 0.f) return DFEPE_ERR_INVALID_ARG;
  return (B == 0 || N == 0) ? 1 : DFEPE_OK;
}

template <int MODE>
int launch(const Args& a, bool needs_sum, hipStream_t stream) {
  const bool homo = (a.kind & DFEPE_EPI_HOMOGENEOUS) != 0;
  Args p = a;
  p.kind = a.kind & 7;
  const unsigned grid = (unsigned)((long long)a.B * a.chunks);
  if (homo) hipLaunchKernelGGL((epi_adjoint_kernel<true, MODE>), dim3(grid), dim3(kThreads), 0, stream, p);
  else hipLaunchKernelGGL((epi_adjoint_kernel<false, MODE>), dim3(grid), dim3(kThreads), 0, stream, p);
  if (needs_sum && a.chunks > 1) {
    const int nc = (MODE == 2) ? 1 : 9;
    const size_t cells = (size_t)a.B * nc;
    hipLaunchKernelGGL(epi_chunk_sum_kernel, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, a.partial,
                       cells, a.chunks, nc, (MODE == 2) ? a.sum_out : a.g_F);
  }
  return launched();
}

}  // namespace

extern "C" int dfepe_epi_adjoint_chunk(void) { return ea::kChunk; }

extern "C" size_t dfepe_epi_adjoint_workspace_bytes(int B, int N) {
  if (B <= 0 || N <= ea::kChunk) return 0;
  return (size_t)B * chunks_of(N) * 9 * sizeof(double);
}

extern "C" int dfepe_epi_metrics_bwd(void* stream, int kind, const float* F, const float* X, const float* Y, int B, int N, float clamp_at,
                                     float eps, const float* g_out, float* g_F, float* g_X, float* g_Y, void* workspace) {
  const int rc = common_checks(kind, B, N, clamp_at);
  if (rc != DFEPE_OK) return rc > 0 ? DFEPE_OK : rc;
  if (!F || !X || !Y || !g_out || (!g_F && !g_X && !g_Y)) return DFEPE_ERR_INVALID_ARG;
  const bool homo = (kind & DFEPE_EPI_HOMOGENEOUS) != 0;
  if (!homo && (!aligned8(X) || !aligned8(Y) || !aligned8(g_X) || !aligned8(g_Y))) return DFEPE_ERR_INVALID_ARG;
  const int chunks = chunks_of(N);
  if (g_F && chunks > 1 && (!workspace || !aligned8(workspace))) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * N > kMaxPoints) return DFEPE_ERR_UNSUPPORTED;
  Args a = {F, X, Y, g_out, nullptr, nullptr, g_F, g_X, g_Y, nullptr, nullptr, static_cast<double*>(workspace), B, N, chunks, kind,
            clamp_at, eps};
  return launch<0>(a, g_F != nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int dfepe_epi_loss_fwd(void* stream, int kind, const float* F, const float* X, const float* Y, const float* w, int B, int N,
                                  float clamp_at, float eps, float* sum_out, void* workspace) {
  const int rc = common_checks(kind, B, N, clamp_at);
  if (rc != DFEPE_OK) return rc > 0 ? DFEPE_OK : rc;
  if (!F || !X || !Y || !sum_out) return DFEPE_ERR_INVALID_ARG;
  const bool homo = (kind & DFEPE_EPI_HOMOGENEOUS) != 0;
  if (!homo && (!aligned8(X) || !aligned8(Y))) return DFEPE_ERR_INVALID_ARG;
  const int chunks = chunks_of(N);
  if (chunks > 1 && (!workspace || !aligned8(workspace))) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * N > kMaxPoints) return DFEPE_ERR_UNSUPPORTED;
  Args a = {F, X, Y, nullptr, nullptr, w, nullptr, nullptr, nullptr, nullptr, sum_out, static_cast<double*>(workspace), B, N, chunks, kind,
            clamp_at, eps};
  return launch<2>(a, true, static_cast<hipStream_t>(stream));
}

extern "C" int dfepe_epi_loss_bwd(void* stream, int kind, const float* F, const float* X, const float* Y, const float* w, int B, int N,
                                  float clamp_at, float eps, const float* g_sum, float* g_F, float* g_X, float* g_Y, float* g_w,
                                  void* workspace) {
  const int rc = common_checks(kind, B, N, clamp_at);
  if (rc != DFEPE_OK) return rc > 0 ? DFEPE_OK : rc;
  if (!F || !X || !Y || !g_sum || (!g_F && !g_X && !g_Y && !g_w)) return DFEPE_ERR_INVALID_ARG;
  const bool homo = (kind & DFEPE_EPI_HOMOGENEOUS) != 0;
  if (!homo && (!aligned8(X) || !aligned8(Y) || !aligned8(g_X) || !aligned8(g_Y))) return DFEPE_ERR_INVALID_ARG;
  const int chunks = chunks_of(N);
  if (g_F && chunks > 1 && (!workspace || !aligned8(workspace))) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * N > kMaxPoints) return DFEPE_ERR_UNSUPPORTED;
  Args a = {F, X, Y, nullptr, g_sum, w, g_F, g_X, g_Y, g_w, nullptr, static_cast<double*>(workspace), B, N, chunks, kind, clamp_at, eps};
  return launch<1>(a, g_F != nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int dfepe_epi_residual_bwd_pts(void* stream, const float* pts1, const float* pts2, const float* F, int B, int N,
                                          float clamp_at, const float* g_out, float* g_pts1, float* g_pts2) {
  if (B < 0 || N < 0) return DFEPE_ERR_INVALID_ARG;
  if (B == 0 || N == 0) return DFEPE_OK;
  if (!pts1 || !pts2 || !F || !g_out || (!g_pts1 && !g_pts2)) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * N > kMaxPoints) return DFEPE_ERR_UNSUPPORTED;
  const int chunks = chunks_of(N);
  hipLaunchKernelGGL(epi_residual_pts_kernel, dim3((unsigned)((long long)B * chunks)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     pts1, pts2, F, N, chunks, clamp_at, g_out, g_pts1, g_pts2);
  return launched();
}
