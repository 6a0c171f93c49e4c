// dfepe_sample_sets -- the minimal sets of the DSAC loop drawn on the device: Philox4x32-10 streams, uniform (Floyd's subset
// algorithm) or in proportion to per-correspondence weights (successive sampling over quantised prefix sums).  The per-lane
// arithmetic is csrc/sampler_math.h, the contract include/dfepe.h, the algorithm DESIGN.md 3.21.
//
//   1  sampler_scan_kernel   weighted mode only.  One workgroup per pair: the largest drawable weight among the first n (a max over
//                            words), then q and its exclusive prefix sums P[0..n] in chunks of sm::kScanChunk with a carry, and the
//                            number of q > 0.  Integer sums: the order is free.
//   2  sampler_draw_kernel   one lane per hypothesis.  A lane reads nothing but its pair's n, P and count; a grid tail is a lane
//                            that draws nothing.  A wavefront passes its sets through 4 KiB of LDS of its own so that idx is written
//                            as consecutive words (no workgroup barrier: wavefronts do not depend on each other).
//
// dfepe_sampler_advance is a one-thread launch that adds to the counter the draw reads, so that a captured draw + advance samples
// the next offset on every replay.  No atomics, no allocation, no host synchronisation; one linear chain of launches.
#include "dfepe_common.h"

#include "sampler_math.h"

namespace {

constexpr int kThreads = 256;
constexpr long long kMaxCells = 2147483647LL;  // B * H * S
static_assert(kThreads == sm::kScanThreads && kThreads % WAVE == 0, "launch shapes of sampler.hip");

// per pair: P[0 .. N] and, behind them, the number of q > 0
__host__ __device__ inline size_t pair_stride(int N) { return (size_t)N + 2; }

__device__ __forceinline__ int valid_count(const int* __restrict__ n_valid, int b, int S, int N) {
  return n_valid ? sm::clamp_valid(n_valid[b], S, N) : N;
}

__global__ void __launch_bounds__(kThreads) sampler_scan_kernel(const float* __restrict__ weights, const int* __restrict__ n_valid, int N,
                                                                 int S, unsigned long long* __restrict__ ws) {
  __shared__ unsigned long long sums[2][kThreads];
  __shared__ unsigned red[kThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = valid_count(n_valid, b, S, N);
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
  const unsigned long long* ws;  // null: uniform mode
  const int* n_valid;
  int* idx;
  int* fallback;
  int N, H, S;
  long long total;  // B * H
};

__global__ void __launch_bounds__(kThreads) sampler_draw_kernel(DrawArgs a) {
  __shared__ int stage[kThreads / WAVE][WAVE * sm::kMaxSample];
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const long long first = gid - lane;  // the wavefront's first hypothesis
  if (first >= a.total) return;        // a whole wavefront of the tail
  const bool live = gid < a.total;
  int out[sm::kMaxSample];
#pragma unroll
  for (int i = 0; i < sm::kMaxSample; ++i) out[i] = 0;
  if (live) {
    const int b = (int)(gid / a.H), h = (int)(gid - (long long)b * a.H);
    const unsigned off = a.offset + (a.counter ? *a.counter : 0u);
    const int n = valid_count(a.n_valid, b, a.S, a.N);
    sm::Stream s = sm::make_stream(a.seed, off, (unsigned)b, (unsigned)h);
    const unsigned long long* P = a.ws ? a.ws + (size_t)b * pair_stride(a.N) : nullptr;
    const bool fall = P && P[(size_t)a.N + 1] < (unsigned long long)a.S;
    if (P && !fall) sm::weighted_set(s, reinterpret_cast<const uint64_t*>(P), n, a.S, out);
    else sm::uniform_set(s, n, a.S, out);
    if (h == 0 && a.fallback) a.fallback[b] = fall ? 1 : 0;
  }
  int* st = stage[wave];
#pragma unroll
  for (int i = 0; i < sm::kMaxSample; ++i)
    if (live && i < a.S) st[lane * a.S + i] = out[i];
  wave_sync();
  const long long rest = a.total - first;
  const int cells = (int)(rest < WAVE ? rest : WAVE) * a.S;
  int* dst = a.idx + first * a.S;
  for (int k = lane; k < cells; k += WAVE) dst[k] = st[k];
}

__global__ void sampler_advance_kernel(unsigned* counter, unsigned by) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *counter = *counter + by;
}

}  // namespace

extern "C" int dfepe_sampler_scan_chunk(void) { return sm::kScanChunk; }

extern "C" size_t dfepe_sample_sets_workspace_bytes(int B, int N, int weighted) {
  if (!weighted || B <= 0 || N <= 0) return 0;
  return (((size_t)B * pair_stride(N) * sizeof(unsigned long long)) + 15) & ~(size_t)15;
}

extern "C" int dfepe_sample_sets(void* stream, int B, int N, int H, int S, unsigned long long seed, unsigned offset, const unsigned* counter,
                                 const float* weights, const int* n_valid, int* idx, int* fallback, void* workspace) {
  if (B < 0 || N < 0 || H < 1) return DFEPE_ERR_INVALID_ARG;
  if (S < sm::kMinSample || S > sm::kMaxSample || N < S) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!idx) return DFEPE_ERR_INVALID_ARG;
  if (weights && (!workspace || !aligned16(workspace))) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * H * S > kMaxCells) return DFEPE_ERR_UNSUPPORTED;
  if (weights && N > sm::kMaxWeightedN) return DFEPE_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* ws = weights ? static_cast<unsigned long long*>(workspace) : nullptr;
  if (weights) {
    hipLaunchKernelGGL(sampler_scan_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, weights, n_valid, N, S, ws);
    const int rc = launched();
    if (rc != DFEPE_OK) return rc;
  }
  const long long total = (long long)B * H;
  DrawArgs a = {seed, offset, counter, ws, n_valid, idx, fallback, N, H, S, total};
  hipLaunchKernelGGL(sampler_draw_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
  return launched();
}

extern "C" int dfepe_sampler_advance(void* stream, unsigned* counter, unsigned by) {
  if (!counter) return DFEPE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(sampler_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), counter, by);
  return launched();
}
