// est_planes -- what surrounds the weight estimator's products (precision and plane layout: est_common.h): fp32 -> 16-bit planes
// (est_split*, est_input_split for the estimator's input, est_wprep_* for every layer's weights in two launches, est_absmax for
// the power-of-two scale of a layer's fp16 weight planes) and the fixed-order column sums of a backward (est_colsum).
#include "est_common.h"

namespace {

// fp32 [rows][C] (ld = src_ld, first C_src columns used, the rest zero) -> NP K-blocked planes [C/32][rows][32]
template <int NP>
__global__ void __launch_bounds__(256)
est_split_kernel(const float* __restrict__ src, long rows, int C_src, int src_ld, int C, bf16_t* __restrict__ planes, size_t plane_stride) {
  const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
  if (e >= rows * C) return;
  const long r = e / C;
  const int ch = (int)(e - r * C);
  const float x = (ch < C_src) ? src[r * src_ld + ch] : 0.f, y = (ch + 1 < C_src) ? src[r * src_ld + ch + 1] : 0.f;
  unsigned p0, p1, p2;
  split3(x, y, p0, p1, p2);
  const size_t at = kb_index((size_t)r, ch, (size_t)rows);
  *reinterpret_cast<unsigned*>(planes + at) = p0;
  if (NP > 1) *reinterpret_cast<unsigned*>(planes + plane_stride + at) = p1;
  if (NP > 2) *reinterpret_cast<unsigned*>(planes + 2 * plane_stride + at) = p2;
}

// the same into two fp16 planes, optionally scaled by the layer's power of two (weights: see wscale)
__global__ void __launch_bounds__(256)
est_split_f16_kernel(const float* __restrict__ src, long rows, int C_src, int src_ld, int C, const unsigned* __restrict__ absmax,
                     bf16_t* __restrict__ planes, size_t plane_stride) {
  const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
  if (e >= rows * C) return;
  const float sc = absmax ? wscale(*absmax, false) : 1.0f;
  const long r = e / C;
  const int ch = (int)(e - r * C);
  const float x = (ch < C_src) ? src[r * src_ld + ch] * sc : 0.f, y = (ch + 1 < C_src) ? src[r * src_ld + ch + 1] * sc : 0.f;
  unsigned p0, p1;
  split2h(x, y, p0, p1);
  const size_t at = kb_index((size_t)r, ch, (size_t)rows);
  *reinterpret_cast<unsigned*>(planes + at) = p0;
  *reinterpret_cast<unsigned*>(planes + plane_stride + at) = p1;
}
// *word = max(*word, bits of max |src[i]|)  (non-negative floats order like their bit patterns; NaN / inf sort above: the clamp in
// wscale keeps the scale finite and the NaN travels in the data)
__global__ void __launch_bounds__(256)
est_absmax_kernel(const float* __restrict__ src, long n, unsigned* __restrict__ word) {
  unsigned m = 0u;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const unsigned b = __float_as_uint(src[i]) & 0x7fffffffu;
    m = b > m ? b : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o, 64); m = t > m ? t : m; }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(word, m);
}

// ---- table-driven launches (round 5): at the reference's batch sizes (4-32 pairs) one estimator call is ~75 launches of which ~60
// are a few microseconds of bookkeeping each -- per layer a maximum, a split, a transposed split, three reductions, three fills.  These
// kernels do a call's worth of each in ONE launch, the per-layer pointers travelling in the kernel arguments.
struct WprepTab {
  int n;
  const float* W[kTabMax];   // [Co][Ci] fp32
  int Co[kTabMax], Ci[kTabMax], K[kTabMax];  // K = Ci rounded up to 32
  bf16_t* pf[kTabMax];       // two fp16 planes of W * s, [K/32][Co][32] each
  bf16_t* pt[kTabMax];       // two bf16 planes of W^T (rows = K, channels = Co: [Co/32][K][32]) for the data gradient, or null
  unsigned* words;           // [n] bit patterns of max |W|
};
// kAbsBlocks workgroups per layer leave their partial maxima in part[layer][block] (no atomics, no zeroing beforehand); the split
// kernel merges them (and its first workgroup of a layer publishes words[layer] for the GEMM epilogues that follow)
constexpr int kAbsBlocks = 64;  // (a wavefront merges them with shuffles: <= 64)
__global__ void __launch_bounds__(256) est_wprep_absmax_kernel(const WprepTab T, unsigned* __restrict__ part) {
  __shared__ unsigned red[4];
  const int layer = (int)blockIdx.y;
  const float* W = T.W[layer];
  const long n = (long)T.Co[layer] * T.Ci[layer];
  unsigned m = 0u;
  constexpr long kStride = (long)kAbsBlocks * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * kStride < n; i += 4 * kStride) {  // four loads in flight
    const unsigned b0 = __float_as_uint(W[i]) & 0x7fffffffu, b1 = __float_as_uint(W[i + kStride]) & 0x7fffffffu,
                   b2 = __float_as_uint(W[i + 2 * kStride]) & 0x7fffffffu, b3 = __float_as_uint(W[i + 3 * kStride]) & 0x7fffffffu;
    const unsigned c0 = b0 > b1 ? b0 : b1, c1 = b2 > b3 ? b2 : b3, c = c0 > c1 ? c0 : c1;
    m = c > m ? c : m;
  }
  for (; i < n; i += kStride) {
    const unsigned b = __float_as_uint(W[i]) & 0x7fffffffu;
    m = b > m ? b : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o, 64); m = t > m ? t : m; }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
    part[layer * kAbsBlocks + blockIdx.x] = m;
  }
}
__global__ void __launch_bounds__(256) est_wprep_split_kernel(const WprepTab T, const unsigned* __restrict__ part) {
  const int layer = (int)blockIdx.y;
  const float* W = T.W[layer];
  const int Co = T.Co[layer], Ci = T.Ci[layer], K = T.K[layer];
  unsigned mx = part[layer * kAbsBlocks + (threadIdx.x & (kAbsBlocks - 1))];
#pragma unroll
  for (int o = kAbsBlocks / 2; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)mx, o, 64); mx = t > mx ? t : mx; }
  if (blockIdx.x == 0 && threadIdx.x == 0) T.words[layer] = mx;
  const float sc = wscale(mx, false);
  const long nf = (long)Co * K / 2, nt = T.pt[layer] ? (long)K * Co / 2 : 0;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < nf + nt; idx += (long)gridDim.x * 256) {
    unsigned p0, p1;
    if (idx < nf) {  // the forward's operand: row = output channel, channel = input channel
      const long e = idx * 2;
      const int r = (int)(e / K), ch = (int)(e - (long)r * K);
      const float x = (ch < Ci) ? W[(size_t)r * Ci + ch] * sc : 0.f, y = (ch + 1 < Ci) ? W[(size_t)r * Ci + ch + 1] * sc : 0.f;
      split2h(x, y, p0, p1);
      const size_t at = kb_index((size_t)r, ch, (size_t)Co);
      *reinterpret_cast<unsigned*>(T.pf[layer] + at) = p0;
      *reinterpret_cast<unsigned*>(T.pf[layer] + (size_t)Co * K + at) = p1;
    } else {         // the data gradient's: row = input channel (zero rows up to K), channel = output channel
      const long e = (idx - nf) * 2;
      const int r = (int)(e / Co), ch = (int)(e - (long)r * Co);
      const float x = (r < Ci) ? W[(size_t)ch * Ci + r] : 0.f, y = (r < Ci) ? W[(size_t)(ch + 1) * Ci + r] : 0.f;
      split2(x, y, p0, p1);
      const size_t at = kb_index((size_t)r, ch, (size_t)K);
      *reinterpret_cast<unsigned*>(T.pt[layer] + at) = p0;
      *reinterpret_cast<unsigned*>(T.pt[layer] + (size_t)K * Co + at) = p1;
    }
  }
}

// dst[c] = sum over r < rows of src[r * cols + c] for up to kSegMax independent segments (rows = 0: zeros): every reduction of one
// backward -- per-pair d gamma / d beta partials, split-K partials of the weight gradients, the head's -- and the exact-zero
// gradients of the cancelled convolution biases.  Fixed order of additions.  Two shapes of segment: TALL (rows > 32: the per-pair
// partials, thousands of rows x <= 1024 columns): a workgroup = 64 columns x 16 row groups, thread (column, group g) adds rows g,
// g + 16, ... and the sixteen partial sums are added in order; WIDE (rows <= 32: split-K partials, up to 2^19 columns): a workgroup
// = 1024 columns, a thread adds its column's rows in order.
struct ColSumTab {
  int n;
  const float* src[kSegMax];
  float* dst[kSegMax];
  int rows[kSegMax], cols[kSegMax];
  int ld_src[kSegMax], ld_dst[kSegMax];  // ld_dst > 0: the sums are a [cols / ld_src][ld_src] matrix of which the first ld_dst columns are kept, densely
                                         // (the first layer's weight gradient without its zero-padded input channels; round 6: was a launch of its own)
  int first_block[kSegMax + 1];  // prefix sums of the segments' workgroup counts
};
__device__ __forceinline__ void colsum_store(const ColSumTab& T, int seg, int c, float v) {
  const int ls = T.ld_src[seg], ld = T.ld_dst[seg];
  if (ld <= 0) { T.dst[seg][c] = v; return; }
  const int r = c / ls, k = c - r * ls;
  if (k < ld) T.dst[seg][(size_t)r * ld + k] = v;
}
__host__ __device__ inline int colsum_blocks(int rows, int cols) { return rows > 32 ? (cols + 63) / 64 : (cols + 1023) / 1024; }
__global__ void __launch_bounds__(1024) est_colsum_kernel(const ColSumTab T) {
  __shared__ float red[16][64];
  int seg = 0;
  while (seg + 1 < T.n && (int)blockIdx.x >= T.first_block[seg + 1]) ++seg;
  const int rows = T.rows[seg], cols = T.cols[seg], blk = (int)blockIdx.x - T.first_block[seg];
  const float* src = T.src[seg];
  if (rows <= 32) {  // WIDE (uniform per workgroup)
    const int c = blk * 1024 + (int)threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += src[(size_t)r * cols + c];
    colsum_store(T, seg, c, s);
    return;
  }
  const int c = blk * 64 + (int)(threadIdx.x & 63), g = (int)(threadIdx.x >> 6);
  float s = 0.f;
  if (c < cols) {
    int r = g;
    for (; r + 48 < rows; r += 64) {  // four loads in flight
      const float a0 = src[(size_t)r * cols + c], a1 = src[(size_t)(r + 16) * cols + c], a2 = src[(size_t)(r + 32) * cols + c],
                  a3 = src[(size_t)(r + 48) * cols + c];
      s = (((s + a0) + a1) + a2) + a3;
    }
    for (; r < rows; r += 16) s += src[(size_t)r * cols + c];
  }
  red[g][threadIdx.x & 63] = s;
  __syncthreads();
  if (g == 0 && c < cols) {
    float t = red[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < 16; ++q) t += red[q][threadIdx.x];
    colsum_store(T, seg, c, t);
  }
}

// x [B][C0][N] fp32 (element (b, c, n) at b * x_sb + c * x_sc + n: dense, or a view of the channel-major [C0][B][N] buffer) -> planes [cols = B N][K0]: two fp16 (what the first layer multiplies by) and, if wanted, two bf16 (what its
// weight gradient multiplies by); channels C0..K0 zero.  A thread = one column x one block of 32 channels: its reads of x run along n
// with its neighbours' (coalesced), its 64 bytes per plane are contiguous with theirs.
__global__ void __launch_bounds__(256)
est_input_split_kernel(const float* __restrict__ x, long x_sb, long x_sc, long B, int C0, int N, int K0, bf16_t* __restrict__ ph, size_t h_stride,
                       bf16_t* __restrict__ pb, size_t b_stride) {
  const long cols = B * (long)N;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;  // (channel block, column), column fastest
  const long col = t % cols;
  const int cb = (int)(t / cols) * 32;
  if (cb >= K0) return;
  const long b = col / N, n = col - b * N;
  unsigned h0[16], h1[16], q0[16], q1[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int ch = cb + 2 * i;
    const float v0 = (ch < C0) ? x[(size_t)b * x_sb + (size_t)ch * x_sc + n] : 0.f, v1 = (ch + 1 < C0) ? x[(size_t)b * x_sb + (size_t)(ch + 1) * x_sc + n] : 0.f;
    split2h(v0, v1, h0[i], h1[i]);
    split2(v0, v1, q0[i], q1[i]);
  }
  const size_t at = kb_index((size_t)col, cb, (size_t)cols);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    *reinterpret_cast<uint4*>(ph + at + 8 * i) = make_uint4(h0[4 * i], h0[4 * i + 1], h0[4 * i + 2], h0[4 * i + 3]);
    *reinterpret_cast<uint4*>(ph + h_stride + at + 8 * i) = make_uint4(h1[4 * i], h1[4 * i + 1], h1[4 * i + 2], h1[4 * i + 3]);
  }
  if (pb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<uint4*>(pb + at + 8 * i) = make_uint4(q0[4 * i], q0[4 * i + 1], q0[4 * i + 2], q0[4 * i + 3]);
      *reinterpret_cast<uint4*>(pb + b_stride + at + 8 * i) = make_uint4(q1[4 * i], q1[4 * i + 1], q1[4 * i + 2], q1[4 * i + 3]);
    }
  }
}

}  // namespace

extern "C" int dfepe_est_absmax(const float* src, long n, unsigned* word, void* stream) {
  if (!src || !word || n < 0) return DFEPE_ERR_INVALID_ARG;
  if (n == 0) return DFEPE_OK;
  long blocks = (n + 2047) / 2048;
  blocks = blocks > 256 ? 256 : blocks;
  hipLaunchKernelGGL(est_absmax_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), src, n, word);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

// every layer's weights in two launches: the maxima (one workgroup per layer), then the two fp16 planes of W * s for the forward
// and -- where planes_wt[l] is given -- the two bf16 planes of W^T the data gradient multiplies by
extern "C" size_t dfepe_est_wprep_workspace_bytes(int n_layers) { return (size_t)(n_layers > 0 ? n_layers : 0) * kAbsBlocks * sizeof(unsigned); }

extern "C" int dfepe_est_wprep(int n_layers, const float* const* W, const int* Co, const int* Ci, void* const* planes_f16,
                               void* const* planes_wt, unsigned* words, void* workspace, void* stream) {
  if (n_layers <= 0 || n_layers > kTabMax || !W || !Co || !Ci || !planes_f16 || !words || !workspace) return DFEPE_ERR_INVALID_ARG;
  WprepTab T{};
  T.n = n_layers; T.words = words;
  for (int l = 0; l < n_layers; ++l) {
    if (!W[l] || !planes_f16[l] || Co[l] <= 0 || Ci[l] <= 0) return DFEPE_ERR_INVALID_ARG;
    if (planes_wt && planes_wt[l] && (Co[l] & 31)) return DFEPE_ERR_INVALID_ARG;
    T.W[l] = W[l]; T.Co[l] = Co[l]; T.Ci[l] = Ci[l]; T.K[l] = (Ci[l] + 31) / 32 * 32;
    T.pf[l] = static_cast<bf16_t*>(planes_f16[l]); T.pt[l] = planes_wt ? static_cast<bf16_t*>(planes_wt[l]) : nullptr;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned* part = static_cast<unsigned*>(workspace);
  hipLaunchKernelGGL(est_wprep_absmax_kernel, dim3(kAbsBlocks, n_layers), dim3(256), 0, st, T, part);
  hipLaunchKernelGGL(est_wprep_split_kernel, dim3(256, n_layers), dim3(256), 0, st, T, static_cast<const unsigned*>(part));
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

int dfepe_est_detail::input_split_launch(const float* x, long x_sb, long x_sc, long B, int C0, int N, int K0, void* ph, size_t h_stride,
                                         void* pb, size_t b_stride, void* stream) {
  const long threads = B * (long)N * (K0 / 32);
  hipLaunchKernelGGL(est_input_split_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, x_sb, x_sc,
                     B, C0, N, K0, static_cast<bf16_t*>(ph), h_stride, static_cast<bf16_t*>(pb), b_stride);
  return launched();
}

int dfepe_est_detail::colsum_launch(int n_seg, const float* const* src, const int* rows, const int* cols, float* const* dst, const int* ld_src,
                                    const int* ld_dst, void* stream) {
  if (n_seg <= 0 || n_seg > kSegMax || !src || !rows || !cols || !dst) return DFEPE_ERR_INVALID_ARG;
  ColSumTab T{};
  T.n = n_seg;
  int blocks = 0;
  for (int s = 0; s < n_seg; ++s) {
    if (rows[s] < 0 || cols[s] <= 0 || !dst[s] || (rows[s] > 0 && !src[s])) return DFEPE_ERR_INVALID_ARG;
    T.src[s] = src[s]; T.dst[s] = dst[s]; T.rows[s] = rows[s]; T.cols[s] = cols[s];
    T.ld_src[s] = ld_src ? ld_src[s] : 0; T.ld_dst[s] = ld_dst ? ld_dst[s] : 0;
    if (T.ld_dst[s] > 0 && (T.ld_src[s] < T.ld_dst[s] || cols[s] % T.ld_src[s])) return DFEPE_ERR_INVALID_ARG;
    T.first_block[s] = blocks;
    blocks += colsum_blocks(rows[s], cols[s]);
  }
  T.first_block[n_seg] = blocks;
  hipLaunchKernelGGL(est_colsum_kernel, dim3(blocks), dim3(1024), 0, static_cast<hipStream_t>(stream), T);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
extern "C" int dfepe_est_colsum(int n_seg, const float* const* src, const int* rows, const int* cols, float* const* dst, void* stream) {
  return dfepe_est_detail::colsum_launch(n_seg, src, rows, cols, dst, nullptr, nullptr, stream);
}

extern "C" int dfepe_est_split_f16(const float* src, long rows, int C_src, int src_ld, int C, const unsigned* absmax, void* planes,
                                   size_t plane_stride, void* stream) {
  if (!src || !planes || rows < 0 || C <= 0 || (C & 31) || C_src <= 0 || C_src > C) return DFEPE_ERR_INVALID_ARG;
  if (rows == 0) return DFEPE_OK;
  const unsigned blocks = (unsigned)((rows * C / 2 + 255) / 256);
  hipLaunchKernelGGL(est_split_f16_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), src, rows, C_src, src_ld, C, absmax,
                     static_cast<bf16_t*>(planes), plane_stride);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

extern "C" int dfepe_est_split(const float* src, long rows, int C_src, int src_ld, int C, int n_planes, void* planes, size_t plane_stride,
                               void* stream) {
  if (!src || !planes || rows < 0 || C <= 0 || (C & 31) || C_src <= 0 || C_src > C || n_planes < 1 || n_planes > 3) return DFEPE_ERR_INVALID_ARG;
  if (rows == 0) return DFEPE_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)((rows * C / 2 + 255) / 256);
  bf16_t* P = static_cast<bf16_t*>(planes);
  if (n_planes == 3) hipLaunchKernelGGL((est_split_kernel<3>), dim3(blocks), dim3(256), 0, st, src, rows, C_src, src_ld, C, P, plane_stride);
  else if (n_planes == 2) hipLaunchKernelGGL((est_split_kernel<2>), dim3(blocks), dim3(256), 0, st, src, rows, C_src, src_ld, C, P, plane_stride);
  else hipLaunchKernelGGL((est_split_kernel<1>), dim3(blocks), dim3(256), 0, st, src, rows, C_src, src_ld, C, P, plane_stride);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
