// The fp32 MFMA dot-product tile of the two descriptor matchers (match.hip: nn_match_tile, knn_match.hip: knn_match_tile), with
// what both build around it: the packed-key exchange of their transposing reductions and the host-side refusals of their entry
// points.  The epilogues (what a dot product becomes and which minima are kept) stay with their kernels.
#pragma once
#include "dfepe_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int TM = 128;  // tile edge (rows of image 1 x rows of image 2)
constexpr int TK = 16;   // K chunk: 2 x 2 x 16 x 128 floats = 32 KiB of LDS per workgroup, so four workgroups share a CU and one
                         // workgroup's epilogue / prologue overlaps the others' MFMA phases
constexpr unsigned kNoVal = 0xffffffffu;

template <int CTRL>
__device__ __forceinline__ u64 exchange_u64(u64 v) {
  union { u64 k; int i[2]; } a, r;
  a.k = v;
  if constexpr (CTRL == 0) {  // lane ^ 16: crosses the 16-lane DPP rows
    r.i[0] = __shfl_xor(a.i[0], 16, 64);
    r.i[1] = __shfl_xor(a.i[1], 16, 64);
  } else {
    r.i[0] = __builtin_amdgcn_update_dpp(a.i[0], a.i[0], CTRL, 0xf, 0xf, false);
    r.i[1] = __builtin_amdgcn_update_dpp(a.i[1], a.i[1], CTRL, 0xf, 0xf, false);
  }
  return r.k;
}

// Where a workgroup's tile lies and which part of it a lane holds: pair b, first row m0 (image 1) and n0 (image 2) of the tile,
// wavefront (wr, wc) of the 2 x 2, half h and lane-in-half jl of the wavefront.
struct TileAt {
  int b, m0, n0, wr, wc, h, jl;
};

// One 256-thread workgroup per 128x128 tile of desc1 desc2^T, 2x2 wavefronts of 64x64 (2x2 MFMA tiles of 32x32, 64 accumulator
// VGPRs), K = D in chunks of TK staged K-major in LDS ([k][row]: a lane's MFMA operand A[i=l&31][k=l>>5] is then a conflict-free
// ds_read_b32), double-buffered with the next chunk prefetched into registers.  staged(pre) sees every chunk of the loader
// thread's own row (threadIdx.x >> 7: the image, & 127: the row of the tile) once, in increasing k, as it goes to LDS.
template <class Staged>
__device__ __forceinline__ TileAt mfma_dot_tile(const float* __restrict__ desc1, const float* __restrict__ desc2, int N1, int N2, int D,
                                                float (&lds)[2][2][TK][TM], f32x16 (&acc)[2][2], Staged staged) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  // XCD-aware tile order: workgroup w runs on XCD w % 8 (round-robin dispatch), and each XCD has its own 4 MiB L2.  The
  // tiles of one image pair share its 2 x N x D descriptors, so every XCD is given whole pairs: the workgroups an XCD
  // has in flight (32 CUs x 4) then cover ~2 pairs = ~4 MiB of descriptors instead of a slice of 16 different pairs.
  const int tn = (N2 + TM - 1) / TM, tm = (N1 + TM - 1) / TM;
  const unsigned total = gridDim.x;
  unsigned w = blockIdx.x;
  if ((total & 7u) == 0u) w = (w & 7u) * (total >> 3) + (w >> 3);
  const int b = (int)(w / (unsigned)(tm * tn));
  const int trem = (int)(w % (unsigned)(tm * tn));
  const int m0 = (trem / tn) * TM, n0 = (trem % tn) * TM;

  // loader role: threads 0..127 stream one descriptor of image 1 each (64 contiguous bytes per chunk), 128..255 image 2
  const int img = tid >> 7, lr = tid & 127;
  const int grow = (img ? n0 : m0) + lr;
  const bool rvalid = grow < (img ? N2 : N1);
  const float* src = (img ? desc2 + (size_t)b * N2 * D : desc1 + (size_t)b * N1 * D) + (size_t)(rvalid ? grow : 0) * D;
  float4 pre[TK / 4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int q = 0; q < TK / 4; ++q)
      pre[q] = rvalid ? reinterpret_cast<const float4*>(src + k0)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto lstore = [&](int buf) {
    float* dst = &lds[buf][img][0][lr];
#pragma unroll
    for (int q = 0; q < TK / 4; ++q) {
      dst[(4 * q + 0) * TM] = pre[q].x;
      dst[(4 * q + 1) * TM] = pre[q].y;
      dst[(4 * q + 2) * TM] = pre[q].z;
      dst[(4 * q + 3) * TM] = pre[q].w;
    }
    staged(pre);
  };

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int h = lane >> 5, jl = lane & 31;
  gload(0);
  lstore(0);
  __syncthreads();
  const int nk = D / TK;
  for (int c = 0; c < nk; ++c) {
    const int buf = c & 1;
    if (c + 1 < nk) gload((c + 1) * TK);
    const float* Ab = &lds[buf][0][h][wr * 64 + jl];
    const float* Bb = &lds[buf][1][h][wc * 64 + jl];
#pragma unroll
    for (int kk = 0; kk < TK / 2; ++kk) {
      const float a0 = Ab[2 * kk * TM], a1 = Ab[2 * kk * TM + 32];
      const float b0 = Bb[2 * kk * TM], b1 = Bb[2 * kk * TM + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (c + 1 < nk) lstore(buf ^ 1);
    __syncthreads();
  }
  return {b, m0, n0, wr, wc, h, jl};
}

// The refusals the two entry points share once their pointers are known to be set, in the order their C-ABI tests pin.  tiles:
// the grid of the tile kernel.
inline int match_tile_plan(const float* desc1, const float* desc2, const void* workspace, int B, int N1, int N2, int D, unsigned* tiles) {
  if (D % 32 != 0) return DFEPE_ERR_UNSUPPORTED;  // K is consumed in 16-float chunks, two per 128-byte line (SuperPoint: D = 256, SIFT: 128)
  if (((uintptr_t)desc1 | (uintptr_t)desc2) & 15u) return DFEPE_ERR_INVALID_ARG;
  if (((uintptr_t)workspace) & 7u) return DFEPE_ERR_INVALID_ARG;
  const size_t n = (size_t)((N2 + TM - 1) / TM) * ((N1 + TM - 1) / TM) * B;
  if (n > 0x7fffffffu) return DFEPE_ERR_UNSUPPORTED;
  *tiles = (unsigned)n;
  return DFEPE_OK;
}
