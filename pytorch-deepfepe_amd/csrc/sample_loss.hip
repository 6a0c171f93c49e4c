// The sample-loss branch of the reference (models/DeepFNetSampleLoss.py Fit.forward:364-436, train_good_utils.py:387-426) around the
// existing fit kernels: draw 100 multisets of 20 correspondences per pair in proportion to the weights, pick the top K, gather the
// sets into the layout dfepe_w8pt_fwd_shared takes, sum the clamped epipolar residual of every set's F over the pair's virtual
// points, and send the gradients of the gathered weights back to the correspondences.  The per-lane arithmetic is
// csrc/sample_loss_math.h, the contract include/dfepe.h, the algorithm DESIGN.md 3.22.
//
//   1  sl_scan_kernel          q and its exclusive prefix sums P[0..n] per pair, in the workspace layout of dfepe_sample_sets (the
//                              scan of csrc/sampler.hip with K in the place of S; integer sums, the order is free)
//   2  sl_draw_kernel          one lane per set, K independent draws, each stored as it is made
//   3  sl_topk_kernel          one wavefront per pair: K rounds of "the largest position below the last one"
//   4  sl_gather_kernel        one workgroup per pair: the copies cell by cell, the set products in fp64, their sum in a fixed tree
//   5  sl_floss_kernel<BWD>    one workgroup per pair: the virtual points go through T into LDS once, a wavefront per set
//   6  sl_scatter_kernel       one lane per correspondence walks the pair's H K cells (staged in LDS, read as broadcasts)
// No atomics, no allocation, no host synchronisation; every sum has a fixed order, so two runs agree bit for bit.
#include "dfepe_common.h"

#include "sample_loss_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLossThreads = 512;
constexpr long long kMaxCells = 2147483647LL;  // B * H * K
static_assert(kThreads == sm::kScanThreads && kThreads % WAVE == 0 && kLossThreads % WAVE == 0, "launch shapes of sample_loss.hip");

__host__ __device__ inline size_t pair_stride(int N) { return (size_t)N + 2; }  // as csrc/sampler.hip

__device__ __forceinline__ int valid_count(const int* __restrict__ n_valid, int b, int K, int N) {
  return n_valid ? sm::clamp_valid(n_valid[b], K, N) : N;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d, WAVE);
    v = o > v ? o : v;
  }
  return v;
}

// fixed-order sum of one double per thread of the workgroup; red has blockDim.x slots; every thread gets the total
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int d = blockDim.x / 2; d >= 1; d >>= 1) {
    if (tid < d) red[tid] = red[tid] + red[tid + d];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(kThreads) sl_scan_kernel(const float* __restrict__ weights, const int* __restrict__ n_valid, int N, int K,
                                                            unsigned long long* __restrict__ ws) {
  __shared__ unsigned long long sums[2][kThreads];
  __shared__ unsigned red[kThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = valid_count(n_valid, b, K, N);
  const unsigned* __restrict__ w = reinterpret_cast<const unsigned*>(weights) + (size_t)b * N;
  unsigned long long* __restrict__ P = ws + (size_t)b * pair_stride(N);

  unsigned m = 0u;
  for (int i = tid; i < n; i += kThreads) {
    const unsigned bits = w[i];
    if (sm::drawable(bits) && bits > m) m = bits;
  }
  red[tid] = m;
  __syncthreads();
  for (int d = kThreads / 2; d >= 1; d >>= 1) {
    if (tid < d) red[tid] = red[tid] > red[tid + d] ? red[tid] : red[tid + d];
    __syncthreads();
  }
  m = red[0];
  __syncthreads();
  const int e = m ? sm::frexp_exponent(m) : 0;

  unsigned long long carry = 0ull;
  unsigned positive = 0u;
  for (int base = 0; base < n; base += sm::kScanChunk) {
    const int i0 = base + tid * sm::kScanPerLane;
    unsigned q[sm::kScanPerLane];
    unsigned long long own = 0ull;
#pragma unroll
    for (int k = 0; k < sm::kScanPerLane; ++k) {
      q[k] = (i0 + k < n) ? sm::quantise(w[i0 + k], e) : 0u;
      own += q[k];
      positive += q[k] != 0u;
    }
    sums[0][tid] = own;
    __syncthreads();
    int src = 0;
    for (int d = 1; d < kThreads; d <<= 1) {
      const unsigned long long v = sums[src][tid] + (tid >= d ? sums[src][tid - d] : 0ull);
      sums[src ^ 1][tid] = v;
      __syncthreads();
      src ^= 1;
    }
    unsigned long long run = carry + (sums[src][tid] - own);  // exclusive
    carry += sums[src][kThreads - 1];
#pragma unroll
    for (int k = 0; k < sm::kScanPerLane; ++k) {
      if (i0 + k < n) P[i0 + k] = run;
      run += q[k];
    }
    __syncthreads();  // the next chunk writes sums[0]
  }
  red[tid] = positive;
  __syncthreads();
  for (int d = kThreads / 2; d >= 1; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  if (tid == 0) {
    P[n] = carry;
    P[(size_t)N + 1] = red[0];
  }
}

struct DrawArgs {
  unsigned long long seed;
  unsigned offset;
  const unsigned* counter;
  const unsigned long long* ws;  // null: uniform
  const int* n_valid;
  int* idx;
  int* fallback;
  int N, H, K;
  long long total;  // B * H
};

__global__ void __launch_bounds__(kThreads) sl_draw_kernel(DrawArgs a) {
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gid >= a.total) return;
  const int b = (int)(gid / a.H), h = (int)(gid - (long long)b * a.H);
  const unsigned off = a.offset + (a.counter ? *a.counter : 0u);
  const int n = valid_count(a.n_valid, b, a.K, a.N);
  sm::Stream s = sm::make_stream(a.seed, off, (unsigned)b, (unsigned)h);
  const unsigned long long* P = a.ws ? a.ws + (size_t)b * pair_stride(a.N) : nullptr;
  const bool fall = P && P[(size_t)a.N + 1] == 0ull;
  const uint64_t* Pd = (P && !fall) ? reinterpret_cast<const uint64_t*>(P) : nullptr;
  int* out = a.idx + gid * a.K;
  for (int j = 0; j < a.K; ++j) out[j] = sl::draw_one(s, j, Pd, n);
  if (h == 0 && a.fallback) a.fallback[b] = fall ? 1 : 0;
}

__global__ void __launch_bounds__(kThreads) sl_topk_kernel(const float* __restrict__ x, const int* __restrict__ n_valid, int B, int N, int K,
                                                            int* __restrict__ idx, float* __restrict__ values) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long b = (long long)blockIdx.x * (kThreads / WAVE) + (threadIdx.x / WAVE);
  if (b >= B) return;
  const int n = valid_count(n_valid, (int)b, K, N);
  const float* xb = x + (size_t)b * N;
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(xb);
  unsigned long long below = ~0ull;
  for (int k = 0; k < K; ++k) {
    below = wave_max_u64(sl::best_below(bits, n, lane, WAVE, below));  // n >= K: there is always one
    if (lane == 0) {
      const int i = below ? sl::position_index(below) : 0;
      idx[(size_t)b * K + k] = i;
      if (values) values[(size_t)b * K + k] = xb[i];
    }
  }
}

__global__ void __launch_bounds__(kThreads) sl_gather_kernel(const float* __restrict__ pts1, const float* __restrict__ pts2,
                                                              const float* __restrict__ weights, const int* __restrict__ idx, int N, int H, int K,
                                                              float* __restrict__ pts1_sel, float* __restrict__ pts2_sel, float* __restrict__ w_sel,
                                                              float* __restrict__ accu) {
  __shared__ double red[kThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t cell0 = (size_t)b * H * K;
  const int cells = H * K;
  const float* p1 = pts1 + (size_t)b * N * 3;
  const float* p2 = pts2 + (size_t)b * N * 3;
  const float* w = weights + (size_t)b * N;
  for (int c = tid; c < cells; c += kThreads) {
    const int i = sl::safe_index(idx[cell0 + c], N);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      pts1_sel[(cell0 + c) * 3 + d] = p1[(size_t)i * 3 + d];
      pts2_sel[(cell0 + c) * 3 + d] = p2[(size_t)i * 3 + d];
    }
    w_sel[cell0 + c] = w[i];
  }
  if (!accu) return;
  double own = 0.0;
  for (int h = tid; h < H; h += kThreads) own = own + sl::set_product(w, idx + cell0 + (size_t)h * K, K, N);
  const double total = block_sum(own, red) + 1e-10;
  for (int h = tid; h < H; h += kThreads) accu[(size_t)b * H + h] = (float)(sl::set_product(w, idx + cell0 + (size_t)h * K, K, N) / total);
}

template <bool BWD>
__global__ void __launch_bounds__(kLossThreads) sl_floss_kernel(const float* __restrict__ F_sel, int H, const float* __restrict__ T1,
                                                                 const float* __restrict__ T2, int t_stride, const float* __restrict__ virt1,
                                                                 const float* __restrict__ virt2, int M, float clamp_at,
                                                                 float* __restrict__ loss_sum, const float* __restrict__ g_loss_sum,
                                                                 float* __restrict__ g_F) {
  extern __shared__ float pts[];  // [M][6]: x1, x2 of every virtual point of the pair
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
  const float* t1 = T1 + (size_t)b * t_stride;
  const float* t2 = T2 + (size_t)b * t_stride;
  for (int i = tid; i < M; i += kLossThreads) {
    sl::eval_point(t1, virt1 + ((size_t)b * M + i) * 3, pts + 6 * i);
    sl::eval_point(t2, virt2 + ((size_t)b * M + i) * 3, pts + 6 * i + 3);
  }
  __syncthreads();
  const double clamp = (double)clamp_at;
  for (int h = wave; h < H; h += kLossThreads / WAVE) {
    const size_t bh = (size_t)b * H + h;
    double F[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) F[c] = (double)F_sel[bh * 9 + c];
    if (!BWD) {
      double acc = 0.0;
      for (int i = lane; i < M; i += WAVE) acc = acc + sl::residual(F, pts + 6 * i, pts + 6 * i + 3, clamp);
      acc = wave_sum(acc);
      if (lane == 0) loss_sum[bh] = (float)acc;
    } else {
      double g[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) g[c] = 0.0;
      for (int i = lane; i < M; i += WAVE) sl::residual_adjoint_F(F, pts + 6 * i, pts + 6 * i + 3, clamp, g);
      const double up = (double)g_loss_sum[bh];
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const double t = wave_sum(g[c]);
        if (lane == 0) g_F[bh * 9 + c] = (float)(up * t);
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads) sl_scatter_kernel(const float* __restrict__ g_w_sel, const float* __restrict__ g_accu,
                                                               const float* __restrict__ weights, const float* __restrict__ accu,
                                                               const int* __restrict__ idx, int N, int H, int K, float* __restrict__ g_w) {
  __shared__ double red[kThreads];
  __shared__ int s_idx[sl::kScatterChunk];
  __shared__ float s_direct[sl::kScatterChunk];
  __shared__ double s_accu[sl::kScatterChunk];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = blockIdx.x * kThreads + tid;
  const size_t cell0 = (size_t)b * H * K;
  const int cells = H * K;
  double G = 0.0;
  if (g_accu) {
    double own = 0.0;
    for (int h = tid; h < H; h += kThreads) own = own + (double)g_accu[(size_t)b * H + h] * (double)accu[(size_t)b * H + h];
    G = block_sum(own, red);
  }
  double direct = 0.0, through = 0.0;
  for (int base = 0; base < cells; base += sl::kScatterChunk) {
    const int here = cells - base < sl::kScatterChunk ? cells - base : sl::kScatterChunk;
    for (int c = tid; c < here; c += kThreads) {
      const size_t cell = cell0 + base + c;
      s_idx[c] = idx[cell];
      s_direct[c] = g_w_sel ? g_w_sel[cell] : 0.0f;
      const size_t bh = (size_t)b * H + (size_t)(base + c) / K;
      s_accu[c] = g_accu ? sl::cell_accu((double)accu[bh], (double)g_accu[bh], G) : 0.0;
    }
    __syncthreads();
    for (int c = 0; c < here; ++c) {
      if (s_idx[c] == n) {
        direct = direct + (double)s_direct[c];
        through = through + s_accu[c];
      }
    }
    __syncthreads();  // the next chunk overwrites the stage
  }
  if (n < N) g_w[(size_t)b * N + n] = sl::scatter_finish(direct, through, g_accu ? weights[(size_t)b * N + n] : 1.0f);
}

}  // namespace

extern "C" int dfepe_sample_loss_max_virt(void) { return sl::kMaxVirt; }
extern "C" int dfepe_sample_scatter_chunk(void) { return sl::kScatterChunk; }

extern "C" int dfepe_sample_multisets(void* stream, int B, int N, int H, int K, unsigned long long seed, unsigned offset,
                                      const unsigned* counter, const float* weights, const int* n_valid, int* idx, int* fallback,
                                      void* workspace) {
  if (B < 0 || N < 0 || H < 1) return DFEPE_ERR_INVALID_ARG;
  if (K < sl::kMinDraws || K > sl::kMaxDraws || N < K) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!idx) return DFEPE_ERR_INVALID_ARG;
  if (weights && (!workspace || !aligned16(workspace))) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * H * K > kMaxCells) return DFEPE_ERR_UNSUPPORTED;
  if (weights && N > sm::kMaxWeightedN) return DFEPE_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* ws = weights ? static_cast<unsigned long long*>(workspace) : nullptr;
  if (weights) {
    hipLaunchKernelGGL(sl_scan_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, weights, n_valid, N, K, ws);
    const int rc = launched();
    if (rc != DFEPE_OK) return rc;
  }
  const long long total = (long long)B * H;
  DrawArgs a = {seed, offset, counter, ws, n_valid, idx, fallback, N, H, K, total};
  hipLaunchKernelGGL(sl_draw_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
  return launched();
}

extern "C" int dfepe_topk_select(void* stream, const float* x, const int* n_valid, int B, int N, int K, int* idx, float* values) {
  if (B < 0 || N < 1 || K < 1 || K > N) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!x || !idx) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * K > kMaxCells) return DFEPE_ERR_UNSUPPORTED;
  const int per = kThreads / WAVE;
  hipLaunchKernelGGL(sl_topk_kernel, dim3((unsigned)((B + per - 1) / per)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, n_valid, B,
                     N, K, idx, values);
  return launched();
}

extern "C" int dfepe_sample_gather(void* stream, const float* pts1, const float* pts2, const float* weights, const int* idx, int B, int N,
                                   int H, int K, float* pts1_sel, float* pts2_sel, float* w_sel, float* accu) {
  if (B < 0 || N < 1 || H < 1 || K < 1) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!pts1 || !pts2 || !weights || !idx || !pts1_sel || !pts2_sel || !w_sel) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * H * K > kMaxCells) return DFEPE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sl_gather_kernel, dim3((unsigned)B), dim3(kThreads), 0, static_cast<hipStream_t>(stream), pts1, pts2, weights, idx, N, H,
                     K, pts1_sel, pts2_sel, w_sel, accu);
  return launched();
}

namespace {

int floss_check(const float* F_sel, int B, int H, const float* T1, const float* T2, int t_stride, const float* virt1, const float* virt2,
                int M, const void* out, const void* extra) {
  if (B < 0 || H < 1 || M < 1) return DFEPE_ERR_INVALID_ARG;
  if (t_stride != 0 && t_stride != 9) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!F_sel || !T1 || !T2 || !virt1 || !virt2 || !out || !extra) return DFEPE_ERR_INVALID_ARG;
  if (M > sl::kMaxVirt || (long long)B * H > kMaxCells) return DFEPE_ERR_UNSUPPORTED;
  return DFEPE_OK;
}

}  // namespace

extern "C" int dfepe_sample_floss_fwd(void* stream, const float* F_sel, int B, int H, const float* T1, const float* T2, int t_stride,
                                      const float* virt1, const float* virt2, int M, float clamp_at, float* loss_sum) {
  const int rc = floss_check(F_sel, B, H, T1, T2, t_stride, virt1, virt2, M, loss_sum, loss_sum);
  if (rc != DFEPE_OK || B == 0) return rc;
  hipLaunchKernelGGL((sl_floss_kernel<false>), dim3((unsigned)B), dim3(kLossThreads), (size_t)M * 6 * sizeof(float),
                     static_cast<hipStream_t>(stream), F_sel, H, T1, T2, t_stride, virt1, virt2, M, clamp_at, loss_sum, nullptr, nullptr);
  return launched();
}

extern "C" int dfepe_sample_floss_bwd(void* stream, const float* F_sel, int B, int H, const float* T1, const float* T2, int t_stride,
                                      const float* virt1, const float* virt2, int M, float clamp_at, const float* g_loss_sum, float* g_F) {
  const int rc = floss_check(F_sel, B, H, T1, T2, t_stride, virt1, virt2, M, g_F, g_loss_sum);
  if (rc != DFEPE_OK || B == 0) return rc;
  hipLaunchKernelGGL((sl_floss_kernel<true>), dim3((unsigned)B), dim3(kLossThreads), (size_t)M * 6 * sizeof(float),
                     static_cast<hipStream_t>(stream), F_sel, H, T1, T2, t_stride, virt1, virt2, M, clamp_at, nullptr, g_loss_sum, g_F);
  return launched();
}

extern "C" int dfepe_sample_scatter_bwd(void* stream, const float* g_w_sel, const float* g_accu, const float* weights, const float* accu,
                                        const int* idx, int B, int N, int H, int K, float* g_w) {
  if (B < 0 || N < 1 || H < 1 || K < 1) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!idx || !g_w) return DFEPE_ERR_INVALID_ARG;
  if (g_accu && (!weights || !accu)) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * H * K > kMaxCells || B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sl_scatter_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), g_w_sel, g_accu, weights, accu, idx, N, H, K, g_w);
  return launched();
}
