// est_common -- what the estimator's translation units share: est_gemm.hip (the matrix-core products), est_norm.hip (normalisation,
// adjoints, head), est_planes.hip (plane making and reductions) and est_pass.hip (one estimator pass per call, host only).
//
// The per-correspondence weight estimator on the matrix cores.
// Replaces: the Conv1d(k=1) -> InstanceNorm1d(affine) -> LeakyReLU stack of ErrorEstimator
// (deepFEPE/models/ErrorEstimators.py:47-64), called depth times per step (deepFEPE/models/DeepFNet.py:441,510), forward and
// backward.  Every 1x1 convolution is a GEMM  Y[C_out, cols] = W[C_out, C_in] X[C_in, cols]  over cols = pairs x N points.
//
// Precision: the reference trains this stack in fp32.  16-bit MFMA is 16x the fp32 MFMA rate, so every fp32 operand is carried as a
// sum of 16-bit PLANES, exact remainders of each other.
//   forward (round 5): TWO fp16 planes, a = a0 + a1 (a0 = fp16(a), a1 = fp16(a - a0): 22 mantissa bits), a product = a0 b0 + a0 b1 +
//     a1 b0 -- three MFMAs, fp32 accumulate, error ~2^-22 per product: the fp32 class (scripts/proto_split_fp16.py: logits 1e-6 from
//     the fp64 truth against 2.4-3.5e-6 for stock fp32; measured on the GPU 2.0-2.4e-6 with the fp32 accumulation).  Rounds 3-4 used
//     three bf16 planes and six products for the same accuracy: twice the matrix work, 6 instead of 4 bytes per element read.  fp16's
//     narrow exponent is handled where it bites: weights (1 / sqrt(fan-in): their low plane would be subnormal) are split scaled by a
//     power of two found on the device (est_absmax_kernel, wscale) and the accumulators scaled back; activations are O(1) behind an
//     InstanceNorm, |a| <= |gamma| sqrt(N - 1) + |beta| must stay below 65504 (beyond it the result is inf / NaN, loudly).
//   backward: two bf16 planes (i + j <= 1, three MFMAs, ~2^-16): gradients need far less than the activations the next fit is
//     sensitive to, and bf16 keeps fp32's exponent range -- no loss scaling.  A forward that will be differentiated therefore also
//     leaves each activation as two bf16 planes (est_in_bwd / est_gemm_tn read those); one that will not skips them.
//
// Layout: activations POINT-major and K-BLOCKED:  P[plane][C/32][col][32]  (the 32 channels of a K step are contiguous per
// column, and the columns of a K step are contiguous: the 208 x 32 operand tile of a block is ONE contiguous 13 KB run, so
// every LDS-DMA instruction moves a full contiguous KiB -- row-major [col][C] made each instruction touch 64 different lines
// and the address unit, not the matrix cores, set the pace), weights W[plane][C_in/32][C_out][32] alike.
#pragma once
#include "dfepe_common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef unsigned short bf16_t;  // storage type of a plane element (bf16 or fp16 bits)
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(8))) short frag8;  // an MFMA operand fragment: eight 16-bit values of either format
enum { FMT_BF16 = 0, FMT_F16 = 1 };

template <int FMT>
__device__ __forceinline__ f32x4 mfma16(const frag8& a, const frag8& b, const f32x4& c) {
  if constexpr (FMT == FMT_F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

#define DFEPE_GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define DFEPE_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

constexpr int kPts = 100;          // points per pair the fused epilogues are built for (N of BASELINE configs 2-4)
constexpr int BM = 128;            // channels per block tile
constexpr int NT = 13;             // 16-column tiles per block: 2 pairs = 200 columns + 8
constexpr int BN = NT * 16;        // 208
constexpr int BSTEP = 2 * kPts;    // columns a block owns
constexpr int BK = 32;             // K step = one MFMA 16x16x32

// table-driven launches (round 5): a call's worth of per-layer bookkeeping in ONE launch, the per-layer pointers travelling in the
// kernel arguments
constexpr int kTabMax = 8;      // hidden layers per table (the reference's estimator has five)
constexpr int kSegMax = 40;     // reduction segments per launch (>= 2 + 4 kTabMax: one backward never needs a second launch)
constexpr int kFixMaxN = 4096;  // points per pair the gamma == 0 fix (est_dgamma_zero_kernel) holds in LDS

__device__ __forceinline__ float row16_sum(float v) {  // sum over the 16 lanes of a DPP row, in every lane
  v += dpp_f32<0xB1>(v);
  v += dpp_f32<0x4E>(v);
  v += dpp_f32<0x141>(v);
  v += dpp_f32<0x140>(v);
  return v;
}

// fp32 -> three bf16 planes (round-to-nearest-even each, remainders exact in fp32), two values at a time
__device__ __forceinline__ void split3(float x, float y, unsigned& p0, unsigned& p1, unsigned& p2) {
  f32x2 v = {x, y};
  const bf16x2 h = __builtin_convertvector(v, bf16x2);
  v -= __builtin_convertvector(h, f32x2);
  const bf16x2 m = __builtin_convertvector(v, bf16x2);
  v -= __builtin_convertvector(m, f32x2);
  const bf16x2 l = __builtin_convertvector(v, bf16x2);
  p0 = __builtin_bit_cast(unsigned, h); p1 = __builtin_bit_cast(unsigned, m); p2 = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ void split2(float x, float y, unsigned& p0, unsigned& p1) {
  f32x2 v = {x, y};
  const bf16x2 h = __builtin_convertvector(v, bf16x2);
  v -= __builtin_convertvector(h, f32x2);
  const bf16x2 m = __builtin_convertvector(v, bf16x2);
  p0 = __builtin_bit_cast(unsigned, h); p1 = __builtin_bit_cast(unsigned, m);
}
// fp32 -> two fp16 planes (round-to-nearest-even each; 22 mantissa bits while the low plane stays in fp16's normal range,
// an absolute 2^-25 below it; |x| > 65504 overflows to inf / NaN -- loudly)
__device__ __forceinline__ void split2h(float x, float y, unsigned& p0, unsigned& p1) {
  f32x2 v = {x, y};
  const f16x2 h = __builtin_convertvector(v, f16x2);
  v -= __builtin_convertvector(h, f32x2);
  const f16x2 m = __builtin_convertvector(v, f16x2);
  p0 = __builtin_bit_cast(unsigned, h); p1 = __builtin_bit_cast(unsigned, m);
}
__device__ __forceinline__ float f16_lo(unsigned u) { return (float)__builtin_bit_cast(f16x2, u)[0]; }
__device__ __forceinline__ float f16_hi(unsigned u) { return (float)__builtin_bit_cast(f16x2, u)[1]; }
// The forward products run on fp16 planes.  Weights are small (1 / sqrt(fan-in)): unscaled, their low plane would sit in fp16's
// subnormal range and lose bits, so a layer's weights are split as W * s with s the power of two that brings max |W| into [8, 16)
// (exact), and the product's accumulators are scaled back before anything else reads them.  `bits` = the fp32 bit pattern of max |W|
// (est_absmax_kernel); exponent clamped so that s and 1 / s^2 stay normal fp32 numbers.
__device__ __forceinline__ float wscale(unsigned bits, bool inverse) {
  int eb = (int)((bits >> 23) & 255u);
  eb = eb < 100 ? 100 : (eb > 150 ? 150 : eb);
  return __uint_as_float((unsigned)(inverse ? eb - 3 : 257 - eb) << 23);
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// element (row, ch) of a K-blocked plane with `rows` rows
__device__ __forceinline__ size_t kb_index(size_t row, int ch, size_t rows) { return ((size_t)(ch >> 5) * rows + row) * 32 + (ch & 31); }
// chunk permutation of the staged [row][4 chunks] image: rows 4r..4r+3 of a 16-row tile hold chunk kg at position kg ^ f(r),
// f = (0, 2, 3, 1): each of the four 16-lane service groups of a ds_read_b128 then covers all 16 slots of the bank row
__device__ __forceinline__ int chunk_swz(int rowgroup) { return (0x78 >> (2 * (rowgroup & 3))) & 3; }

}  // namespace

// The two launches est_pass.hip needs beyond the exported entry points (both defined in est_planes.hip)
namespace dfepe_est_detail {

// dst[s][c] = sum_r src[s][r][c] for n_seg <= kSegMax segments in one launch (rows[s] = 0: zeros; src[s] may then be null); ld_src / ld_dst
// (null: plain): segment s is a [cols / ld_src][ld_src] matrix of which the first ld_dst columns are stored densely
int colsum_launch(int n_seg, const float* const* src, const int* rows, const int* cols, float* const* dst, const int* ld_src,
                  const int* ld_dst, void* stream);

// x [B][C0][N] fp32 (element (b, c, n) at b * x_sb + c * x_sc + n) -> planes [cols = B N][K0]: two fp16 planes `ph` and, unless null,
// two bf16 planes `pb` (h_stride / b_stride elements between a pair of planes); channels C0..K0 zero
int input_split_launch(const float* x, long x_sb, long x_sc, long B, int C0, int N, int K0, void* ph, size_t h_stride, void* pb,
                       size_t b_stride, void* stream);

}  // namespace dfepe_est_detail
