// knn_match — k = 2 nearest-neighbour search over general (not unit-norm) descriptors with Lowe's ratio test: the correspondence
// source of every SIFT-based config.
//
// Replaces, per image pair, KNN_match of deepFEPE/dsac_tools/utils_opencv.py:39-90 (if_BF=True):
//   matches = cv2.BFMatcher(normType=cv2.NORM_L2).knnMatch(des1, des2, k=2)          (:44-45)
//   for m, n in matches: all_m.append(m); if m.distance < 0.8 * n.distance: good.append(m)   (:63-67)
// OpenCV's k-best insertion visits the columns in increasing order with a strict <, so the two neighbours of a query are
// its two smallest (distance, column) pairs; the ratio line is Python: float64(m.distance) < ratio * float64(n.distance).
//
// Kernel 1 (knn_match_tile): the fp32 MFMA tile of match.hip, shared with it as mfma_dot_tile of match_tile.h -- one
// 256-thread workgroup per 128x128 tile, 2x2 wavefronts of 64x64, K = D in chunks of 16 staged K-major in LDS,
// double-buffered, XCD-aware tile order.  Its own:
//   * squared norms: every loader thread streams one whole descriptor row, so the callable it hands to the tile accumulates
//     that row's sum of squares, one fmaf per component in increasing k, and the kernel leaves it in LDS (1 KiB) for the
//     epilogue.  Bitwise-equal rows therefore have bitwise-equal norms in every tile;
//   * epilogue: t = fma(-2, dot, n1 + n2), a non-positive t becomes +0.0f (not fmaxf: it may return -0.0f, whose bits
//     would sort last as an unsigned key); columns >= N2 carry the kNoVal key;
//   * per row the TWO smallest (t bits << 32 | column) keys: in-lane over the two column tiles, then the transposing
//     reduction of match.hip over pairs (best = min(a1, b1), second = min(max(a1, b1), min(a2, b2))).  The two 32-row
//     halves (rt = 0, 1) are reduced one after the other: 16 rows x 2 keys x 64 bit = 64 VGPRs at a time next to the 64
//     accumulators;
//   * no column side and no atomics: a top-2 list cannot be merged by a 64-bit atomicMin, so every 64-column wavefront
//     strip writes its pair of keys per row to a slot of its own in the workspace [B, N1, slots, 2], slots =
//     2 ceil(N2 / 128).  Every slot is written by exactly one wavefront: no memset, no launch-order dependence.
// Kernel 2 (knn_match_finish): one block per pair: merge the row's slots, dist = sqrtf(t), the ratio decision in double,
// order-preserving compaction (ballot / popcount) in passes of 1024 rows.  The compacted list has the layout of
// dfepe_nn_match_two_way, so dfepe_gather_matches takes it unchanged.
#include "match_tile.h"

#include <math.h>

namespace {

// Squared L2 distance from the dot product and the sum of the two squared norms; <= 0 (and -0.0f) -> +0.0f.
__device__ __forceinline__ float dot_to_t(float dot, float nsum) {
  const float t = fmaf(-2.0f, dot, nsum);
  return (t > 0.0f) ? t : 0.0f;
}

// The two smallest of {a1 <= a2} and {b1 <= b2}, all four distinct (every key carries its own column).
__device__ __forceinline__ void merge2(u64& a1, u64& a2, u64 b1, u64 b2) {
  const u64 lo = (b1 < a1) ? b1 : a1, hi = (b1 < a1) ? a1 : b1;
  const u64 s = (b2 < a2) ? b2 : a2;
  a1 = lo;
  a2 = (s < hi) ? s : hi;
}
// One step of the transposing reduction of match.hip (halve_min) over pairs of keys: CNT pairs per lane -> CNT/2; the lane
// with the decision bit set keeps the upper half of its arrays and hands the lower half to its partner.
template <int CNT, int CTRL>
__device__ __forceinline__ void halve_min2(u64* a1, u64* a2, bool upper) {
  constexpr int H = CNT / 2;
#pragma unroll
  for (int k = 0; k < H; ++k) {
    const u64 g1 = exchange_u64<CTRL>(upper ? a1[k] : a1[k + H]);
    const u64 g2 = exchange_u64<CTRL>(upper ? a2[k] : a2[k + H]);
    u64 k1 = upper ? a1[k + H] : a1[k], k2 = upper ? a2[k + H] : a2[k];
    merge2(k1, k2, g1, g2);
    a1[k] = k1;
    a2[k] = k2;
  }
}

__global__ void __launch_bounds__(256, 4)
knn_match_tile_kernel(const float* __restrict__ desc1, const float* __restrict__ desc2, int N1, int N2, int D, int slots,
                      u64* __restrict__ ws) {
  __shared__ float lds[2][2][TK][TM];  // [buffer][image][k][row]: 32 KiB
  __shared__ __attribute__((aligned(16))) float nrm[2][TM];  // [image][row]: squared norms of the tile's descriptors
  f32x16 acc[2][2];
  float nsq = 0.0f;  // sum of squares of my loader row, one fmaf per component in increasing k
  const auto [b, m0, n0, wr, wc, h, jl] = mfma_dot_tile(desc1, desc2, N1, N2, D, lds, acc, [&nsq](const float4(&pre)[TK / 4]) {
#pragma unroll
    for (int q = 0; q < TK / 4; ++q) {
      nsq = fmaf(pre[q].x, pre[q].x, nsq);
      nsq = fmaf(pre[q].y, pre[q].y, nsq);
      nsq = fmaf(pre[q].z, pre[q].z, nsq);
      nsq = fmaf(pre[q].w, pre[q].w, nsq);
    }
  });
  const int tid = threadIdx.x, lane = tid & 63;
  nrm[tid >> 7][tid & 127] = nsq;  // the loader's image and row; rows beyond N1 / N2 loaded zeros: norm 0
  __syncthreads();

  // ---- epilogue: C/D layout of the 32x32 tile: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) ----------
  const int cl0 = wc * 64 + jl;        // my column inside the tile, column tile 0 (tile 1: +32)
  const int cg0 = n0 + cl0;            // global
  const int rl0 = wr * 64 + 4 * h;     // my first row inside the tile
  const bool c0ok = cg0 < N2, c1ok = cg0 + 32 < N2;
  const float nc0 = nrm[1][cl0], nc1 = nrm[1][cl0 + 32];
  const u64 none0 = ((u64)kNoVal << 32) | (unsigned)cg0, none1 = ((u64)kNoVal << 32) | (unsigned)(cg0 + 32);
  // per row the two smallest keys: in-lane over the two column tiles, then over the 32 lanes of the half.  The two 32-row
  // halves go one after the other; key number r of half rt ends up in the lanes with (lane & 15) == r, and the lanes with
  // ((lane & 31) >> 4) == rt keep it.
  u64 best = ~0ull, second = ~0ull;
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    u64 p1[16], p2[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 nr = *reinterpret_cast<const float4*>(&nrm[0][rl0 + rt * 32 + 8 * g]);
      const float nrow[4] = {nr.x, nr.y, nr.z, nr.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        const float t0 = dot_to_t(acc[rt][0][r], nrow[e] + nc0);
        const float t1 = dot_to_t(acc[rt][1][r], nrow[e] + nc1);
        const u64 k0 = c0ok ? (((u64)__float_as_uint(t0) << 32) | (unsigned)cg0) : none0;
        const u64 k1 = c1ok ? (((u64)__float_as_uint(t1) << 32) | (unsigned)(cg0 + 32)) : none1;
        p1[r] = (k1 < k0) ? k1 : k0;
        p2[r] = (k1 < k0) ? k0 : k1;
      }
    }
    halve_min2<16, 0x140>(p1, p2, (lane & 8) != 0);  // row_mirror
    halve_min2<8, 0x141>(p1, p2, (lane & 4) != 0);   // row_half_mirror
    halve_min2<4, 0x4E>(p1, p2, (lane & 2) != 0);    // quad_perm [2,3,0,1]
    halve_min2<2, 0xB1>(p1, p2, (lane & 1) != 0);    // quad_perm [1,0,3,2]
    const u64 g1 = exchange_u64<0>(p1[0]), g2 = exchange_u64<0>(p2[0]);  // the other 16-lane row of the half: a plain merge
    merge2(p1[0], p2[0], g1, g2);
    if ((jl >> 4) == rt) { best = p1[0]; second = p2[0]; }
  }
  {
    const int r = jl & 15;
    const int rg = m0 + rl0 + (jl >> 4) * 32 + (r & 3) + 8 * (r >> 2);
    if (rg < N1) {
      u64* dst = ws + (((size_t)b * N1 + rg) * slots + (size_t)((n0 / TM) * 2 + wc)) * 2;
      dst[0] = best;
      dst[1] = second;
    }
  }
}

__global__ void __launch_bounds__(1024)
knn_match_finish_kernel(const u64* __restrict__ ws, int N1, int slots, double ratio, int ratio_test, int* __restrict__ nn1,
                        int* __restrict__ nn2, float* __restrict__ dist1, float* __restrict__ dist2, int* __restrict__ m_idx1,
                        int* __restrict__ m_idx2, float* __restrict__ score, int* __restrict__ count) {
  __shared__ int wsum[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  int base = 0;
  for (int i0 = 0; i0 < N1; i0 += 1024) {
    const int i = i0 + tid;
    bool keep = false;
    unsigned j = 0;
    float d = 0.0f;
    if (i < N1) {
      const u64* p = ws + ((size_t)b * N1 + i) * slots * 2;
      u64 k1 = p[0], k2 = p[1];
      for (int s = 1; s < slots; ++s) merge2(k1, k2, p[2 * s], p[2 * s + 1]);
      j = (unsigned)k1;
      d = sqrtf(__uint_as_float((unsigned)(k1 >> 32)));
      const float d2 = sqrtf(__uint_as_float((unsigned)(k2 >> 32)));  // N2 >= 2: the second key is a real column
      const size_t o = (size_t)b * N1 + i;
      nn1[o] = (int)j;
      nn2[o] = (int)(unsigned)k2;
      dist1[o] = d;
      dist2[o] = d2;
      // m.distance < ratio * n.distance as Python evaluates it: both distances widened to double, the product in double
      keep = !ratio_test || ((double)d < ratio * (double)d2);
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

inline size_t knn_slots(int N2) { return 2 * (size_t)((N2 + TM - 1) / TM); }

}  // namespace

extern "C" size_t dfepe_knn_match_workspace_bytes(int B, int N1, int N2) {
  if (B <= 0 || N1 < 0 || N2 < 0) return 0;
  return (size_t)B * (size_t)N1 * knn_slots(N2) * 2 * sizeof(u64);
}

extern "C" int dfepe_knn_match(const float* desc1, const float* desc2, int B, int N1, int N2, int D, double ratio, int ratio_test,
                               void* workspace, int* nn1, int* nn2, float* dist1, float* dist2, int* m_idx1, int* m_idx2,
                               float* score, int* count, void* stream) {
  if (B < 0 || N1 < 0 || N2 < 0 || D <= 0) return DFEPE_ERR_INVALID_ARG;
  if (ratio_test && isnan(ratio)) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!count) return DFEPE_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (N1 == 0) {  // no query: empty outputs
    return (hipMemsetAsync(count, 0, (size_t)B * sizeof(int), st) == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
  }
  if (N2 < 2) return DFEPE_ERR_INVALID_ARG;  // no second neighbour: the reference's `for m, n in matches` raises ValueError
  if (!desc1 || !desc2 || !workspace || !nn1 || !nn2 || !dist1 || !dist2 || !m_idx1 || !m_idx2 || !score)
    return DFEPE_ERR_INVALID_ARG;
  unsigned tiles;
  if (const int rc = match_tile_plan(desc1, desc2, workspace, B, N1, N2, D, &tiles)) return rc;
  const int slots = (int)knn_slots(N2);
  u64* ws = static_cast<u64*>(workspace);
  hipLaunchKernelGGL(knn_match_tile_kernel, dim3(tiles), dim3(256), 0, st, desc1, desc2, N1, N2, D, slots, ws);
  hipLaunchKernelGGL(knn_match_finish_kernel, dim3(B), dim3(1024), 0, st, ws, N1, slots, ratio, ratio_test, nn1, nn2, dist1, dist2,
                     m_idx1, m_idx2, score, count);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
