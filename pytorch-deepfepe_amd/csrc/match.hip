// nn_match — two-way nearest-neighbour matching of unit-norm descriptors, the step that PRODUCES the (B,N,4)
// correspondences of the solver.
//
// Replaces, per image pair, the host/numpy loop of get_matches_from_SP (deepFEPE/train_good_utils.py:683-716):
//   matching_mask = SP_tracker.nn_match_two_way(desc1.T, desc2.T, nn_thresh)      (:687-691)
//   xs / offsets / quality gathered through crop_or_pad_choice                     (:693-716, utils_misc.py:139-161)
// nn_match_two_way lives in the un-vendored `superpoint` package (eric-yyjau/pytorch-superpoint,
// models/model_wrap.py, PointTracker; README.md:37-40 installs it unpinned); its published algorithm (Magic Leap's
// SuperPoint demo) is restated in oracle/deepf_oracle.py:nn_match_two_way:
//   dmat = sqrt(2 - 2 clip(desc1^T desc2, -1, 1)); idx = argmin_j dmat[i,j]; keep = dmat[i,idx] < nn_thresh and
//   argmin_i dmat[i,idx[i]] == i; matches = (i, idx[i], dmat[i,idx[i]]) for the kept i in increasing order.
//
// Kernel 1 (nn_match_tile): the only GEMM-shaped op of the whole path, so it runs on the matrix cores in exact fp32
// (v_mfma_f32_32x32x2_f32: the descriptors are fp32 and the arg-min decisions must not see bf16 rounding).  One
// 256-thread workgroup per 128x128 tile of dmat; the tile itself (placement, LDS staging, the double-buffered MFMA
// loop) is mfma_dot_tile of match_tile.h, which knn_match.hip runs too.  dmat never reaches HBM:
// the epilogue turns the accumulators into squared distances and folds them into per-row and per-column minima, packed
// as (value bits << 32 | index) so that one 64-bit atomicMin per row/column realises numpy's first-occurrence argmin.
// Kernel 2 (nn_match_finish): threshold + mutual check + order-preserving compaction (ballot / popcount).
// Kernel 3 (gather_matches): the crop/pad gather into xs [B,N,4], offsets [B,N,4], quality [B,N].
#include "match_tile.h"

namespace {

// Squared distance of two unit descriptors from their dot product: t = 2 - 2 clip(dot, -1, 1), bit-identical to the
// reference's fp32 expression under the square root (one rounding).  The minima are taken over t; the reference takes
// them over sqrt(t), which is the same arg-min except when two DIFFERENT t round to the same square root and the larger
// one comes first -- a 1-ulp near-tie that already depends on the summation order of the BLAS behind np.dot.  Exact
// ties (duplicated descriptors, dots clipped at 1) keep numpy's first-occurrence rule.  The score is sqrtf(t_min).
__device__ __forceinline__ float dot_to_t(float dot) { return fmaf(-2.0f, __builtin_amdgcn_fmed3f(dot, -1.0f, 1.0f), 2.0f); }

// One step of a transposing min-reduction over the 32 lanes of a half: CNT keys per lane -> CNT/2; the lane with the
// decision bit set keeps the upper half of its array and hands the lower half to its partner (any partner on the other
// side of the bit works: lane^16, row_mirror, row_half_mirror, quad_perm xor 2 / xor 1).  After the five steps lane j
// holds the minimum over the half of key number j: 31 exchanges instead of 32 x 5.
template <int CNT, int CTRL>
__device__ __forceinline__ void halve_min(u64* a, bool upper) {
  constexpr int H = CNT / 2;
#pragma unroll
  for (int k = 0; k < H; ++k) {
    const u64 lo = a[k], hi = a[k + H];
    const u64 got = exchange_u64<CTRL>(upper ? lo : hi);
    const u64 keep = upper ? hi : lo;
    a[k] = (got < keep) ? got : keep;
  }
}

__global__ void __launch_bounds__(256, 4)
nn_match_tile_kernel(const float* __restrict__ desc1, const float* __restrict__ desc2, int N1, int N2, int D,
                     u64* __restrict__ rowkey, u64* __restrict__ colkey) {
  __shared__ float lds[2][2][TK][TM];  // [buffer][image][k][row]: 32 KiB
  f32x16 acc[2][2];
  const auto [b, m0, n0, wr, wc, h, jl] = mfma_dot_tile(desc1, desc2, N1, N2, D, lds, acc, [](const float4(&)[TK / 4]) {});
  const int lane = threadIdx.x & 63;

  // ---- epilogue: C/D layout of the 32x32 tile: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) ----------
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = dot_to_t(acc[i][j][r]);

  const int cg0 = n0 + wc * 64 + jl;  // global column of my element in column tile 0 (tile 1: +32)
  const int rbase = m0 + wr * 64 + 4 * h;
  const bool c0ok = cg0 < N2, c1ok = cg0 + 32 < N2;
  // column minima first (they read the accumulators in place): in-lane over my 32 rows, visited in increasing order so
  // that strict < keeps the first row, then the two halves through one 64-bit exchange
  u64 colk[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    unsigned bestv = kNoVal, bestr = kNoVal;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rg = rbase + rt * 32 + (r & 3) + 8 * (r >> 2);
        const unsigned k = (rg < N1) ? __float_as_uint(acc[rt][ct][r]) : kNoVal;
        if (k < bestv) { bestv = k; bestr = (unsigned)rg; }
      }
    }
    const u64 key = ((u64)bestv << 32) | bestr;
    const u64 other = (u64)__shfl_xor((long long)key, 32, 64);
    colk[ct] = (other < key) ? other : key;
  }
  {
    const u64 mycol = h ? colk[1] : colk[0];
    const int cg = cg0 + 32 * h;
    if (cg < N2 && (unsigned)(mycol >> 32) != kNoVal) atomicMin(&colkey[(size_t)b * N2 + cg], mycol);
  }
  // row minima: in-lane over the two column tiles (ties keep the smaller column), then the transposing reduction over
  // the 32 lanes of the half; key number q = 16 rt + r ends up in lane q of the half
  u64 rk[32];
#pragma unroll
  for (int q = 0; q < 32; ++q) {
    const unsigned k0 = c0ok ? __float_as_uint(acc[q >> 4][0][q & 15]) : kNoVal;
    const unsigned k1 = c1ok ? __float_as_uint(acc[q >> 4][1][q & 15]) : kNoVal;
    const unsigned cb = (k1 < k0) ? (unsigned)(cg0 + 32) : (unsigned)cg0;
    rk[q] = ((u64)min(k0, k1) << 32) | cb;
  }
  halve_min<32, 0>(rk, (lane & 16) != 0);
  halve_min<16, 0x140>(rk, (lane & 8) != 0);  // row_mirror
  halve_min<8, 0x141>(rk, (lane & 4) != 0);   // row_half_mirror
  halve_min<4, 0x4E>(rk, (lane & 2) != 0);    // quad_perm [2,3,0,1]
  halve_min<2, 0xB1>(rk, (lane & 1) != 0);    // quad_perm [1,0,3,2]
  {
    const int r = jl & 15;
    const int rg = rbase + (jl >> 4) * 32 + (r & 3) + 8 * (r >> 2);
    if (rg < N1 && (unsigned)(rk[0] >> 32) != kNoVal) atomicMin(&rowkey[(size_t)b * N1 + rg], rk[0]);
  }
}

__global__ void __launch_bounds__(1024)
nn_match_finish_kernel(const u64* __restrict__ rowkey, const u64* __restrict__ colkey, int N1, int N2, float nn_thresh,
                       int* __restrict__ m_idx1, int* __restrict__ m_idx2, float* __restrict__ score,
                       int* __restrict__ count) {
  __shared__ int wsum[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  int base = 0;
  for (int i0 = 0; i0 < N1; i0 += 1024) {  // one pass for up to 1024 keypoints: a single memory latency per pair
    const int i = i0 + tid;
    bool keep = false;
    unsigned j = 0;
    float d = 0.0f;
    if (i < N1) {
      const u64 key = rowkey[(size_t)b * N1 + i];
      if ((unsigned)(key >> 32) != kNoVal) {
        j = (unsigned)key;
        d = sqrtf(__uint_as_float((unsigned)(key >> 32)));  // the keys carry t = 2 - 2 clip(dot); the score is the distance
        // scores < nn_thresh, and the nearest neighbour of j in image 1 is i again
        keep = (d < nn_thresh) && ((unsigned)colkey[(size_t)b * N2 + j] == (unsigned)i);
      }
    }
    const size_t p = (size_t)b * N1 + compact_slot<16>(keep, wsum, base);
    if (keep) {
      m_idx1[p] = i;
      m_idx2[p] = (int)j;
      score[p] = d;
    }
  }
  if (tid == 0) count[b] = base;
}

__global__ void __launch_bounds__(256)
gather_matches_kernel(const float* __restrict__ pts1, const float* __restrict__ pts2, const float* __restrict__ off1,
                      const float* __restrict__ off2, int B, int N1, int N2, const int* __restrict__ m_idx1,
                      const int* __restrict__ m_idx2, const float* __restrict__ score, const int* __restrict__ choice,
                      int n_out, float* __restrict__ xs, float* __restrict__ offsets, float* __restrict__ quality) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * n_out) return;
  const size_t b = t / n_out;
  const int c = choice[t];
  const int i = m_idx1[b * N1 + c], j = m_idx2[b * N1 + c];
  const float2 p1 = reinterpret_cast<const float2*>(pts1)[b * N1 + i];
  const float2 p2 = reinterpret_cast<const float2*>(pts2)[b * N2 + j];
  reinterpret_cast<float4*>(xs)[t] = make_float4(p1.x, p1.y, p2.x, p2.y);
  if (offsets != nullptr) {
    const float2 o1 = reinterpret_cast<const float2*>(off1)[b * N1 + i];
    const float2 o2 = reinterpret_cast<const float2*>(off2)[b * N2 + j];
    reinterpret_cast<float4*>(offsets)[t] = make_float4(o1.x, o1.y, o2.x, o2.y);
  }
  if (quality != nullptr) quality[t] = score[b * N1 + c];
}

// The adjoint of the offsets output of gather_matches_kernel: row t of g_offsets belongs to keypoint m_idx1[choice[t]] of image 1
// (its first two columns) and m_idx2[choice[t]] of image 2 (the last two).  Padding repeats choices, so rows collide: one lane per
// source keypoint (blockIdx.z: the image) walks the n_out rows in ascending order, their sources staged in LDS in tiles, and adds
// its own in fp64 -- no atomics, one writer per cell, the same bits on every run.
constexpr int kGatherTile = 1024;
__global__ void __launch_bounds__(256)
gather_offsets_bwd_kernel(const float* __restrict__ g_offsets, int N1, int N2, const int* __restrict__ m_idx1,
                          const int* __restrict__ m_idx2, const int* __restrict__ choice, int n_out, float* __restrict__ g_off1,
                          float* __restrict__ g_off2) {
  __shared__ int src[kGatherTile];
  const size_t b = blockIdx.y;
  const int second = blockIdx.z, tid = threadIdx.x;
  const int N = second ? N2 : N1;
  if ((int)(blockIdx.x * 256) >= N) return;  // uniform over the workgroup, before any barrier
  const int i = blockIdx.x * 256 + tid;
  const int* m = (second ? m_idx2 : m_idx1) + b * N1;
  const float* g = g_offsets + b * (size_t)n_out * 4 + (second ? 2 : 0);
  double ax = 0.0, ay = 0.0;
  for (int t0 = 0; t0 < n_out; t0 += kGatherTile) {
    const int cnt = (n_out - t0 < kGatherTile) ? n_out - t0 : kGatherTile;
    __syncthreads();
    for (int j = tid; j < cnt; j += 256) {
      const int c = choice[b * n_out + t0 + j];
      src[j] = (c >= 0 && c < N1) ? m[c] : -1;
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      if (src[j] == i) {  // every lane reads the same cell: a broadcast
        ax += (double)g[(size_t)(t0 + j) * 4];
        ay += (double)g[(size_t)(t0 + j) * 4 + 1];
      }
    }
  }
  if (i < N) reinterpret_cast<float2*>(second ? g_off2 : g_off1)[b * N + i] = make_float2((float)ax, (float)ay);
}

}  // namespace

extern "C" size_t dfepe_nn_match_workspace_bytes(int B, int N1, int N2) {
  if (B <= 0 || N1 < 0 || N2 < 0) return 0;
  return (size_t)B * ((size_t)N1 + (size_t)N2) * sizeof(u64);
}

extern "C" int dfepe_nn_match_two_way(const float* desc1, const float* desc2, int B, int N1, int N2, int D, float nn_thresh,
                                      void* workspace, int* m_idx1, int* m_idx2, float* score, int* count, void* stream) {
  if (B < 0 || N1 < 0 || N2 < 0 || D <= 0) return DFEPE_ERR_INVALID_ARG;
  if (!(nn_thresh >= 0.0f)) return DFEPE_ERR_INVALID_ARG;  // the reference raises ValueError for a negative threshold
  if (B == 0) return DFEPE_OK;
  if (!count) return DFEPE_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (N1 == 0 || N2 == 0) {  // np.zeros((3, 0)): no matches
    return (hipMemsetAsync(count, 0, (size_t)B * sizeof(int), st) == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
  }
  if (!desc1 || !desc2 || !workspace || !m_idx1 || !m_idx2 || !score) return DFEPE_ERR_INVALID_ARG;
  unsigned tiles;
  if (const int rc = match_tile_plan(desc1, desc2, workspace, B, N1, N2, D, &tiles)) return rc;
  u64* rowkey = static_cast<u64*>(workspace);
  u64* colkey = rowkey + (size_t)B * N1;
  if (hipMemsetAsync(workspace, 0xff, dfepe_nn_match_workspace_bytes(B, N1, N2), st) != hipSuccess) return DFEPE_ERR_HIP;
  hipLaunchKernelGGL(nn_match_tile_kernel, dim3(tiles), dim3(256), 0, st, desc1, desc2, N1, N2, D, rowkey, colkey);
  hipLaunchKernelGGL(nn_match_finish_kernel, dim3(B), dim3(1024), 0, st, rowkey, colkey, N1, N2, nn_thresh, m_idx1, m_idx2,
                     score, count);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

extern "C" int dfepe_gather_matches(const float* pts1, const float* pts2, const float* off1, const float* off2, int B, int N1,
                                    int N2, const int* m_idx1, const int* m_idx2, const float* score, const int* choice,
                                    int n_out, float* xs, float* offsets, float* quality, void* stream) {
  if (B < 0 || N1 <= 0 || N2 <= 0 || n_out < 0) return DFEPE_ERR_INVALID_ARG;
  if (B == 0 || n_out == 0) return DFEPE_OK;
  if (!pts1 || !pts2 || !m_idx1 || !m_idx2 || !choice || !xs) return DFEPE_ERR_INVALID_ARG;
  if (offsets && (!off1 || !off2)) return DFEPE_ERR_INVALID_ARG;
  if (quality && !score) return DFEPE_ERR_INVALID_ARG;
  const size_t n = (size_t)B * n_out;
  hipLaunchKernelGGL(gather_matches_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     pts1, pts2, off1, off2, B, N1, N2, m_idx1, m_idx2, score, choice, n_out, xs, offsets, quality);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

extern "C" int dfepe_gather_offsets_bwd(const float* g_offsets, int B, int N1, int N2, const int* m_idx1, const int* m_idx2,
                                        const int* choice, int n_out, float* g_off1, float* g_off2, void* stream) {
  if (B < 0 || N1 <= 0 || N2 <= 0 || n_out < 0) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (B > 65535) return DFEPE_ERR_UNSUPPORTED;
  if (!g_off1 || !g_off2 || !m_idx1 || !m_idx2) return DFEPE_ERR_INVALID_ARG;
  if (n_out > 0 && (!g_offsets || !choice)) return DFEPE_ERR_INVALID_ARG;
  const int nmax = N1 > N2 ? N1 : N2;
  hipLaunchKernelGGL(gather_offsets_bwd_kernel, dim3((unsigned)((nmax + 255) / 256), B, 2), dim3(256), 0,
                     static_cast<hipStream_t>(stream), g_offsets, N1, N2, m_idx1, m_idx2, choice, n_out, g_off1, g_off2);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
