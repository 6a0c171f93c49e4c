// est_gemm -- the two matrix-core products of the weight estimator (precision and plane layout: est_common.h).
//   est_gemm_nt   C[m][n] = sum_terms A_i[m][:] . B_j[n][:]   (both operands K-contiguous), 128 x 208 block tile = 128 channels
//                 x two whole pairs (N = 100: 2 x 100 columns + 8 of the next block, recomputed there), K step 32, operands staged
//                 by LDS-DMA (global_load_lds_dwordx4) as [plane][row][4 chunks of 8 k] with the chunk order XOR-permuted per group
//                 of four rows (on the SOURCE address: the LDS image of a DMA is lane-linear), so that an MFMA fragment is one
//                 conflict-free ds_read_b128; single LDS stage, two workgroups per CU overlap each other's load and MFMA phases
//                 (the small-grid build: two LDS stages, one workgroup per CU).
//                 Epilogues: EPI_F32 (plain fp32 store, the data-gradient GEMM and the plain product of any N), EPI_IN (forward:
//                 InstanceNorm statistics of each (channel, pair) straight from the accumulators -- a pair's 100 columns sit in
//                 the 16 lanes of a DPP row across 7 column tiles --, affine, LeakyReLU, split into two fp16 planes and, for a
//                 forward that will be differentiated, two bf16 planes, 8-byte stores; the convolution bias cancels in the
//                 normalisation) and EPI_INBWD (since round 5 the InstanceNorm + LeakyReLU adjoint of the layer below is the
//                 data-gradient GEMM's epilogue: dA stays in the accumulators, the layer's output planes are read twice -- sums,
//                 then dY -- 228 registers, no scratch; round 3's first attempt held x^ and spilled.  dA never reaches memory: 8
//                 of the 20 bytes per element.  Only the layer under the head and any N != 100 run est_norm.hip's adjoint
//                 kernels as launches of their own).
//   est_gemm_tn   dW[co][ci] = sum_cols dY[col][co] X[col][ci]: both operands are K-major here, fragments come from
//                 ds_read_b64_tr_b16 (the LDS transpose read) of an XOR-swizzled [k][128 channels] image, split-K over columns.
// K-loop and tile-walk variants that were measured and retired: DESIGN.md §3.6, "variants tried and retired".
#include "est_common.h"

namespace {

enum { EPI_F32 = 0, EPI_IN = 1, EPI_INBWD = 2 };
#ifndef DFEPE_NT2_BLOCKS
#define DFEPE_NT2_BLOCKS 3  // workgroups per CU the two-plane (data-gradient) product is compiled for
#endif
#ifndef DFEPE_INBWD_DEPTH
#define DFEPE_INBWD_DEPTH 4  // column tiles of the layer's output in flight in the fused adjoint's two passes
#endif
#ifndef DFEPE_FWD_BLOCKS
#define DFEPE_FWD_BLOCKS 3  // workgroups per CU the two-plane forward layer (fused epilogue) is compiled for: 168 registers, 43 KB of LDS each;
                            // measured at B = 4096: forward 2.49 ms against 2.67 with two (one fragment set then, fetched per tile, like the data gradient)
#endif

// -DDFEPE_EST_PHASE_CLOCKS (scripts/ubench/est_phases.hip only): lane 0 of every wavefront stamps the shader clock at the phase
// boundaries of est_gemm_nt_kernel and sums its waits in the K loop
#ifdef DFEPE_EST_PHASE_CLOCKS
__device__ unsigned long long* g_est_phase_clk;  // [workgroup * 4 + wavefront][8]
#define EST_STAMP(slot)                                                                                                  \
  do {                                                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                                                   \
    const unsigned long long t_ = __builtin_readcyclecounter();                                                          \
    if ((threadIdx.x & 63u) == 0u)                                                                                       \
      g_est_phase_clk[((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6)) * 8 + (slot)] = t_;      \
    __builtin_amdgcn_sched_barrier(0);                                                                                   \
  } while (0)
#else
#define EST_STAMP(slot) do {} while (0)
#endif

struct EpiArgs {
  // EPI_F32: out[col][m] fp32, ld = ldc; with gridDim.z = S > 1 (split-K) slice z of the K steps goes to out + z * split_stride
  float* out;
  int ldc;
  size_t split_stride;
  // EPI_F32, gx != null: the product is the gradient w.r.t. the estimator's input -- stored as gx[pair][ch][n], ch < gx_C0, col = pair * gx_N + n
  float* gx;
  int gx_C0, gx_N;
  long gx_sb, gx_sc;  // element strides of gx between pairs / channels (points are contiguous): [pairs][C0][N] dense, or the channel-major
                      // [C0][pairs][N] buffer the model keeps its estimator inputs in
  // EPI_IN
  const float* gamma;
  const float* beta;
  float eps, slope;
  bf16_t* planes;        // [2][ncols][M] fp16: the next layer's operand
  size_t plane_stride;   // elements between planes
  float* rstd;           // [npairs][M]
  // FMT_F16
  const unsigned* absmax;  // bits of max |W| (the weights were split scaled, see wscale); null: unscaled
  bf16_t* planes_bwd;      // [2][ncols][M] bf16: what the backward reads (est_in_bwd, est_gemm_tn); null: not kept (no gradient wanted)
  size_t bwd_stride;
  // EPI_INBWD (the data gradient dA = dY_next W_next stays in the accumulators and goes straight through the InstanceNorm + LeakyReLU
  // adjoint of the layer below): gamma, beta, slope as above; planes / plane_stride = dY out [2][ncols][M] bf16
  const bf16_t* aout;      // that layer's output as the backward reads it, [2][ncols][M] bf16
  size_t aout_stride;
  const float* rstd_in;    // [npairs][M]
  float* dgamma_part;      // [npairs][M] each
  float* dbeta_part;
};

// C[m][n] = sum over plane pairs (i, j), i + j <= ORDER, of A_i[m][:] . B_j[n][:]
//   A: [NPA][M][K] (a_plane elements between planes), B: [NPB][ncols][K]; K % 32 == 0, M % 4 == 0.
// Block (bx, by): columns [200 bx, 200 bx + 208), channels [128 by, 128 by + 128); 4 wavefronts, wavefront w owns channels
// 32 w .. 32 w + 31 (two 16-row MFMA tiles) x all 13 column tiles: 26 accumulator tiles = 104 registers.
// One LDS stage, two workgroups per CU: while one multiplies, the other waits for its LDS-DMA.  Measured alternatives at
// B = 4096 (1024 -> 512 layer, 2.16 ms as built): two LDS stages with one workgroup per CU (DMA of step k + 1 under the MFMAs of
// step k) 2.68 ms -- a lone wavefront per SIMD issues its 16 DMA instructions, 45 fragment reads and 156 MFMAs in order;
// weights straight from global memory into a second register set + two LDS stages of the activations only, still two workgroups
// per CU: 1.47 vs 1.43 ms with two planes (206 registers), spills with three.  The step is bound by instruction issue around the
// MFMAs (DMA setup, fragment reads, barriers), not by an exposed load latency.
// AHEAD: column tiles whose B fragments are fetched ahead of the MFMAs that consume them.  -1: what the (planes, epilogue) combination
// is tuned for at a full grid -- 0 for the two-plane products compiled for three workgroups per CU (the third wavefront on the SIMD
// covers the LDS latency), 1 otherwise.  2: the build for SMALL grids (the reference's batch sizes: 16-64 workgroups on 256 CUs):
// a wavefront alone on its SIMD sees every LDS round trip (13 tiles x ~120 cycles against 96 cycles of MFMAs per tile with AHEAD = 0).
constexpr int nt_blocks(int NPA, int NPB, int EPI, int AHEAD) {
  return (AHEAD >= 0) ? 2 : ((NPA == 2 && NPB == 2 && EPI == EPI_F32) ? DFEPE_NT2_BLOCKS : ((NPA == 2 && NPB == 2 && EPI == EPI_IN) ? DFEPE_FWD_BLOCKS : 2));
}
template <int NPA, int NPB, int ORDER, int EPI, int FMT = FMT_BF16, int AHEAD = -1>
__global__ void __launch_bounds__(256, nt_blocks(NPA, NPB, EPI, AHEAD))
est_gemm_nt_kernel(const bf16_t* __restrict__ A, size_t a_plane, const bf16_t* __restrict__ B, size_t b_plane, int M, int ncols, int K,
                   const EpiArgs E) {
  constexpr int kABytes = NPA * BM * 64, kBBytes = NPB * BN * 64;
  static_assert(EPI != EPI_IN || FMT == FMT_F16, "the forward epilogue writes fp16 planes");
  // the small-grid builds (AHEAD = 2: at most one workgroup per CU) own their CU: TWO stages (86 KB), the next K step's DMA under the
  // whole MFMA phase of this one
  constexpr bool kTwoStage = (AHEAD == 2);
  __shared__ __attribute__((aligned(16))) unsigned char lds_all[(kTwoStage ? 2 : 1) * (kABytes + kBBytes)];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  // XCD-aware order: consecutive workgroup ids go round-robin to the 8 XCDs; the channel blocks of one column block share its
  // activation tile, so they are given consecutive slots of ONE XCD (its L2 then serves the re-reads)
  const int mblocks = (int)gridDim.y, cblocks = (int)gridDim.x;
  int bx = (int)blockIdx.x, by = (int)blockIdx.y;
  if ((cblocks & 7) == 0) {
    const int id = by * cblocks + bx;  // linear dispatch order (x fastest)
    const int xcd = id & 7, s = id >> 3;
    by = s % mblocks;
    bx = (s / mblocks) * 8 + xcd;
  }
  const int m0 = by * BM, n0 = bx * BSTEP;

  f32x4 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- staging tasks of this wavefront: one contiguous KiB (16 rows x 64 B of one plane's K block) per LDS-DMA instruction ----
  constexpr int kATasks = NPA * (BM / 16), kBTasks = NPB * NT, kTasks = kATasks + kBTasks;
  constexpr int kPerWave = (kTasks + 3) / 4;
  const int drow = lane >> 2, dchunk = (lane & 3) ^ chunk_swz(lane >> 4);  // DMA role: row within the instruction, source chunk
  const int fsw = chunk_swz(c >> 2);                                       // fragment role: this lane's rows sit in row group c >> 2
  // Row i of the wavefront's A tile mt holds channel 8 (i >> 2) + 4 mt + (i & 3) of its 32 (not 16 mt + i): an accumulator lane
  // (row group g) then owns the EIGHT consecutive channels 8 g .. 8 g + 7 across its two tiles, so the epilogue stores 16 bytes per
  // lane and plane, 64 contiguous bytes per column, one contiguous KiB per store instruction
  const int fswA[2] = {chunk_swz(2 * (c >> 2)), chunk_swz(2 * (c >> 2) + 1)};
  // split-K (EPI_F32 only): workgroup z of gridDim.z walks the K steps [ks_begin, ks_end)
  const int nk_all = K / BK, kz = (int)blockIdx.z, nz = (int)gridDim.z;
  const int ks_begin = (nk_all * kz) / nz, nk = (nk_all * (kz + 1)) / nz;
  auto issue_task_a = [&](int ks, unsigned char* lds, int t) {
    const int p = t / (BM / 16), rb = t % (BM / 16);
    int row = m0 + rb * 16 + drow;
    row = (row < M) ? row : M - 1;
    const bf16_t* src = A + (size_t)p * a_plane + ((size_t)ks * M + row) * 32 + dchunk * 8;
    unsigned char* dst = lds + (p * BM + rb * 16) * 64;
    __builtin_amdgcn_global_load_lds(DFEPE_GLOBAL_PTR(src), DFEPE_LDS_PTR(dst), 16, 0, 0);
  };
  auto issue_task_b = [&](int ks, unsigned char* lds, int p, int rb) {
    int row = n0 + rb * 16 + drow;
    row = (row < ncols) ? row : ncols - 1;
    const bf16_t* src = B + (size_t)p * b_plane + ((size_t)ks * ncols + row) * 32 + dchunk * 8;
    unsigned char* dst = lds + kABytes + (p * BN + rb * 16) * 64;
    __builtin_amdgcn_global_load_lds(DFEPE_GLOBAL_PTR(src), DFEPE_LDS_PTR(dst), 16, 0, 0);
  };
  auto stage_issue = [&](int ks, unsigned char* lds) {
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
      const int t = wave + 4 * i;  // wave-uniform
      if (t < kATasks) issue_task_a(ks, lds, t);
      else if (t < kTasks) issue_task_b(ks, lds, (t - kATasks) / NT, (t - kATasks) % NT);
    }
  };
  auto a_from_lds = [&](const unsigned char* lds, frag8 (&a)[2][NPA]) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int p = 0; p < NPA; ++p)
        a[mt][p] = *reinterpret_cast<const frag8*>(lds + ((p * BM + wave * 32 + 8 * (c >> 2) + 4 * mt + (c & 3)) * 4 + (g ^ fswA[mt])) * 16);
  };
  auto mfma_phase = [&](const unsigned char* lds, const frag8 (&a)[2][NPA]) {
    // the column tile's B fragments are fetched one tile ahead of the MFMAs that consume them (two register sets): the LDS
    // latency of tile nt + 1 hides behind the twelve MFMAs of tile nt instead of stalling every tile
    // (the two-plane product compiled for three workgroups per CU has 168 registers: one fragment set, fetched per tile -- the
    // third wavefront on the SIMD covers the LDS latency the second set would)
    constexpr int kD = (AHEAD >= 0) ? AHEAD : ((nt_blocks(NPA, NPB, EPI, AHEAD) > 2) ? 0 : 1);  // tiles fetched ahead
    frag8 b[kD + 1][NPB];
    auto fetch_b = [&](int nt, frag8 (&dst)[NPB]) {
#pragma unroll
      for (int p = 0; p < NPB; ++p) dst[p] = *reinterpret_cast<const frag8*>(lds + kABytes + ((p * BN + nt * 16 + c) * 4 + (g ^ fsw)) * 16);
    };
#pragma unroll
    for (int d = 0; d < kD; ++d) fetch_b(d, b[d]);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (nt + kD < NT) fetch_b(nt + kD, b[(nt + kD) % (kD + 1)]);
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of this tile's MFMAs (the scheduler would sink it to its first use)
      // smallest terms first; the two row tiles alternate, so that no MFMA waits for the one issued just before it
#pragma unroll
      for (int ord = ORDER; ord >= 0; --ord)
#pragma unroll
        for (int i = 0; i <= ord; ++i) {
          const int j = ord - i;
          if (i < NPA && j < NPB) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
              acc[mt][nt] = mfma16<FMT>(a[mt][i], b[nt % (kD + 1)][j], acc[mt][nt]);
          }
        }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  EST_STAMP(0);
#ifdef DFEPE_EST_PHASE_CLOCKS
  unsigned long long wait_cycles = 0, mfma_cycles = 0;
#endif
  if constexpr (kTwoStage) {
    constexpr int kStage = kABytes + kBBytes;
    stage_issue(ks_begin, lds_all);
    for (int ks = ks_begin; ks < nk; ++ks) {
      unsigned char* cur = lds_all + ((ks - ks_begin) & 1) * kStage;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this step's stage
      __syncthreads();                                  // ... everyone's, and everyone is done reading the other buffer (step ks - 1)
      if (ks + 1 < nk) stage_issue(ks + 1, lds_all + ((ks + 1 - ks_begin) & 1) * kStage);
      frag8 a[2][NPA];
      a_from_lds(cur, a);
      mfma_phase(cur, a);
    }
  } else {  // one stage: issue / wait / multiply (the other workgroups of the CU cover the wait)
    for (int ks = ks_begin; ks < nk; ++ks) {
#ifdef DFEPE_EST_PHASE_CLOCKS
      const unsigned long long t0_ = __builtin_readcyclecounter();
#endif
      stage_issue(ks, lds_all);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
#ifdef DFEPE_EST_PHASE_CLOCKS
      const unsigned long long t1_ = __builtin_readcyclecounter();
#endif
      frag8 a[2][NPA];
      a_from_lds(lds_all, a);
      mfma_phase(lds_all, a);
#ifdef DFEPE_EST_PHASE_CLOCKS
      const unsigned long long t2_ = __builtin_readcyclecounter();
      wait_cycles += t1_ - t0_; mfma_cycles += t2_ - t1_;
#endif
      __syncthreads();
    }
  }
  EST_STAMP(1);
#ifdef DFEPE_EST_PHASE_CLOCKS
  if ((threadIdx.x & 63u) == 0u) {
    unsigned long long* q = g_est_phase_clk + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6)) * 8;
    q[5] = wait_cycles; q[6] = mfma_cycles;
  }
#endif

  // ---- epilogue: lane holds, per column n0 + 16 nt + c, channels ch8 + 4 mt + r (mt = 0, 1; r = 0..3): eight in a row --------
  const int ch8 = m0 + wave * 32 + 8 * g;
  const bool chok = ch8 < M;  // M % 8 == 0
  float unscale = 1.0f;  // FMT_F16: the weights were split scaled by a power of two
  if constexpr (FMT == FMT_F16) unscale = E.absmax ? wscale(*E.absmax, true) : 1.0f;
  if constexpr (EPI == EPI_F32) {
    if (E.gx != nullptr) {  // (uniform) the input gradient, channel-major per pair like x itself: 16 consecutive points per channel and store
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int cl = nt * 16 + c, col = n0 + cl;
        if (cl < BSTEP && col < ncols) {
          const int pr = col / E.gx_N, pt = col - pr * E.gx_N;
          float* dst = E.gx + (size_t)pr * E.gx_sb + (size_t)ch8 * E.gx_sc + pt;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (ch8 + j < E.gx_C0) dst[(size_t)j * E.gx_sc] = acc[j >> 2][nt][j & 3] * unscale;
        }
      }
      return;
    }
    float* const out_z = E.out + (size_t)kz * E.split_stride;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int cl = nt * 16 + c, col = n0 + cl;
      if (cl < BSTEP && col < ncols && chok) {
        float* dst = out_z + (size_t)col * E.ldc + ch8;
        if constexpr (FMT == FMT_F16) {
          *reinterpret_cast<f32x4*>(dst) = acc[0][nt] * unscale;
          *reinterpret_cast<f32x4*>(dst + 4) = acc[1][nt] * unscale;
        } else {
          *reinterpret_cast<f32x4*>(dst) = acc[0][nt];
          *reinterpret_cast<f32x4*>(dst + 4) = acc[1][nt];
        }
      }
    }
  } else if constexpr (EPI == EPI_INBWD) {
    // The accumulators hold dA[col][ch] of TWO whole pairs x this lane's eight channels: est_in_bwd_kernel's arithmetic on them in
    // place.  Pass A: a = the layer's output (two bf16 planes, one 16-byte load per plane and column tile), dz = dA lrelu'(a) written
    // back into the accumulator, x^ = (z - beta) / gamma recovered from a, the two sums per (channel, pair) accumulated over the
    // pair's column tiles and then over the 16 lanes of the DPP row.  Pass B: x^ recomputed from the same planes (L2), dY = rstd gamma
    // (dz - mean(dz) - x^ mean(dz x^)), two bf16 planes, 16-byte stores.  dA never reaches memory.
    const bool t6p0 = c < 4, t12ok = c < 8;
    const int npairs = ncols / kPts;
    const int pair0 = 2 * bx, pair1 = (pair0 + 1 < npairs) ? pair0 + 1 : pair0;
    const int chc = chok ? ch8 : 0;
    const float islope = 1.0f / E.slope;
    // z from a = lrelu(z) without a compare (a mask per element kept for a second use is what spilled the first build of this
    // epilogue): a slope below one makes the pre-activation the smaller of a and a / slope, one above it the larger
    // (the median of a, a / slope and -inf resp. +inf: one instruction)
    const float med_lim = (E.slope <= 1.0f) ? -__builtin_inff() : __builtin_inff();
    auto unrelu = [&](float a) { return __builtin_amdgcn_fmed3f(a, a * islope, med_lim); };
    float ig[8], bt[8];
    {
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(E.gamma + chc), g1 = *reinterpret_cast<const f32x4*>(E.gamma + chc + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(E.beta + chc), b1 = *reinterpret_cast<const f32x4*>(E.beta + chc + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gj = j < 4 ? g0[j & 3] : g1[j & 3];
        ig[j] = (fabsf(gj) > 1e-30f) ? 1.0f / gj : 0.0f;
        bt[j] = j < 4 ? b0[j & 3] : b1[j & 3];
      }
    }
    // the raw words of one column tile (two planes x 16 bytes), fetched one tile ahead of their use; the scheduling barriers keep the
    // compiler from hoisting all thirteen tiles' loads (104 registers) above the loop
    struct Raw { uint4 u0, u1; };
    size_t plane_at = kb_index(0, chc, (size_t)ncols);  // of this lane's channel group, column 0
    auto fetch = [&](int nt) {
      int cc = c;
      asm volatile("" : "+v"(cc));  // the address arithmetic stays with its tile (hoisted, the 26 addresses are 52 registers)
      int col = n0 + nt * 16 + cc;
      col = (col < ncols) ? col : ncols - 1;
      const size_t at = plane_at + (size_t)col * 32;
      Raw r;
      r.u0 = *reinterpret_cast<const uint4*>(E.aout + at);
      r.u1 = *reinterpret_cast<const uint4*>(E.aout + E.aout_stride + at);
      return r;
    };
    auto unpack = [&](const Raw& r, float (&a)[8]) {
      const unsigned w0[4] = {r.u0.x, r.u0.y, r.u0.z, r.u0.w}, w1[4] = {r.u1.x, r.u1.y, r.u1.z, r.u1.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[2 * q] = bf16_lo(w0[q]) + bf16_lo(w1[q]);
        a[2 * q + 1] = bf16_hi(w0[q]) + bf16_hi(w1[q]);
      }
    };
    float s1[2][8], s2[2][8];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int j = 0; j < 8; ++j) { s1[p][j] = 0.f; s2[p][j] = 0.f; }
    // kDepth tiles in flight: one iteration is ~80 vector instructions, a miss to HBM an order of magnitude more
    constexpr int kDepth = DFEPE_INBWD_DEPTH;
    Raw ring[kDepth];
#pragma unroll
    for (int i = 0; i < kDepth; ++i) ring[i] = fetch(i);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const Raw cur = ring[nt % kDepth];
      if (nt + kDepth < NT) ring[nt % kDepth] = fetch(nt + kDepth);
      __builtin_amdgcn_sched_barrier(0);
      float a[8];
      unpack(cur, a);
      const bool live = (nt < 12) || t12ok;  // lanes 8..15 of tile 12 belong to the next block
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = acc[j >> 2][nt][j & 3];
        const float e = live ? ((a[j] > 0.f) ? d : d * E.slope) : 0.f;
        const float x = unrelu(a[j]);  // z; x^ = (z - beta) / gamma is affine in it: sum dz x^ = (sum dz z - beta sum dz) / gamma, below
        acc[j >> 2][nt][j & 3] = e;
        if (nt < 6) { s1[0][j] += e; s2[0][j] = fmaf(e, x, s2[0][j]); }
        else if (nt > 6) { s1[1][j] += e; s2[1][j] = fmaf(e, x, s2[1][j]); }
        else {
          const float e0 = t6p0 ? e : 0.f, e1 = t6p0 ? 0.f : e;
          s1[0][j] += e0; s2[0][j] = fmaf(e0, x, s2[0][j]);
          s1[1][j] += e1; s2[1][j] = fmaf(e1, x, s2[1][j]);
        }
      }
      // pin the sums to this iteration: left free, instruction selection orders the pure accumulation chains after ALL thirteen
      // tiles' x^ (104 more live values), and the scheduling barriers then keep them there
#pragma unroll
      for (int p = 0; p < 2; ++p)
        if ((p == 0 && nt <= 6) || (p == 1 && nt >= 6))
          asm volatile("" : "+v"(s1[p][0]), "+v"(s1[p][1]), "+v"(s1[p][2]), "+v"(s1[p][3]), "+v"(s1[p][4]), "+v"(s1[p][5]), "+v"(s1[p][6]), "+v"(s1[p][7]),
                            "+v"(s2[p][0]), "+v"(s2[p][1]), "+v"(s2[p][2]), "+v"(s2[p][3]), "+v"(s2[p][4]), "+v"(s2[p][5]), "+v"(s2[p][6]), "+v"(s2[p][7]));
      __builtin_amdgcn_sched_barrier(0);
    }
    EST_STAMP(2);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s1[p][j] = row16_sum(s1[p][j]);
        s2[p][j] = (row16_sum(s2[p][j]) - bt[j] * s1[p][j]) * ig[j];  // sum dz x^  (0 where gamma == 0, like est_in_bwd)
      }
    if (chok && c == 0) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int pr = pair0 + p;
        if (pr < npairs) {
          float* db = E.dbeta_part + (size_t)pr * M + ch8;
          float* dg = E.dgamma_part + (size_t)pr * M + ch8;
          *reinterpret_cast<f32x4*>(db) = f32x4{s1[p][0], s1[p][1], s1[p][2], s1[p][3]};
          *reinterpret_cast<f32x4*>(db + 4) = f32x4{s1[p][4], s1[p][5], s1[p][6], s1[p][7]};
          *reinterpret_cast<f32x4*>(dg) = f32x4{s2[p][0], s2[p][1], s2[p][2], s2[p][3]};
          *reinterpret_cast<f32x4*>(dg + 4) = f32x4{s2[p][4], s2[p][5], s2[p][6], s2[p][7]};
        }
      }
    }
    float kk[2][8];
    {
      const float inv_n = 1.0f / (float)kPts;
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(E.gamma + chc), g1 = *reinterpret_cast<const f32x4*>(E.gamma + chc + 4);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const float* rp = E.rstd_in + (size_t)(p ? pair1 : pair0) * M + chc;
        const f32x4 r0 = *reinterpret_cast<const f32x4*>(rp), r1 = *reinterpret_cast<const f32x4*>(rp + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          // dY = k (dz - m1 - x^ m2), x^ = (z - beta) / gamma:  dY = k dz + c1 z + c0 -- two FMAs per element in pass B
          const float k = (j < 4 ? r0[j & 3] : r1[j & 3]) * (j < 4 ? g0[j & 3] : g1[j & 3]);
          const float m1 = s1[p][j] * inv_n, m2g = s2[p][j] * inv_n * ig[j];
          kk[p][j] = k;
          s2[p][j] = -k * m2g;                   // c1
          s1[p][j] = k * (m2g * bt[j] - m1);     // c0
        }
      }
    }
    // the planes are read AGAIN for pass B (L2): without the compiler barrier the second loads are merged with the first and all
    // 104 values of a stay live across the row sums (the first build spilled 130 registers that way)
    EST_STAMP(3);
    asm volatile("" : "+v"(plane_at) :: "memory");  // (and the addresses formed again: kept, they were 52 registers, spilled)
#pragma unroll
    for (int i = 0; i < kDepth; ++i) ring[i] = fetch(i);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const Raw cur = ring[nt % kDepth];
      if (nt + kDepth < NT) ring[nt % kDepth] = fetch(nt + kDepth);
      __builtin_amdgcn_sched_barrier(0);
      float a[8];
      unpack(cur, a);
      const bool first = (nt < 6) || (nt == 6 && t6p0);
      float y[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c0 = first ? s1[0][j] : s1[1][j], c1 = first ? s2[0][j] : s2[1][j], k = first ? kk[0][j] : kk[1][j];
        y[j] = fmaf(k, acc[j >> 2][nt][j & 3], fmaf(c1, unrelu(a[j]), c0));
      }
      unsigned pl[2][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) split2(y[2 * q], y[2 * q + 1], pl[0][q], pl[1][q]);
      const int cl = nt * 16 + c, col = n0 + cl;
      if (cl < BSTEP && col < ncols && chok) {
        bf16_t* dst = E.planes + kb_index((size_t)col, ch8, (size_t)ncols);
        *reinterpret_cast<uint4*>(dst) = make_uint4(pl[0][0], pl[0][1], pl[0][2], pl[0][3]);
        *reinterpret_cast<uint4*>(dst + E.plane_stride) = make_uint4(pl[1][0], pl[1][1], pl[1][2], pl[1][3]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    EST_STAMP(4);
  } else {
    // pair 0 = columns 0..99 (tiles 0..5 and lanes 0..3 of tile 6), pair 1 = 100..199 (lanes 4..15 of tile 6, tiles 7..11,
    // lanes 0..7 of tile 12); lanes 8..15 of tile 12 belong to the next block
    const float inv_n = 1.0f / (float)kPts;
    const float inv_n2 = inv_n * unscale * unscale;
    const bool t6p0 = c < 4, t12ok = c < 8;
    const int pair0 = 2 * bx;
    const int chc = chok ? ch8 : 0;
    f32x4 gam[2], bet[2], mean0[2], mean1[2], rs0[2], rs1[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      gam[mt] = *reinterpret_cast<const f32x4*>(E.gamma + chc + 4 * mt);
      bet[mt] = *reinterpret_cast<const f32x4*>(E.beta + chc + 4 * mt);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int nt = 0; nt < 6; ++nt) s0 += acc[mt][nt][r];
        s0 += t6p0 ? acc[mt][6][r] : 0.f;
        s1 += t6p0 ? 0.f : acc[mt][6][r];
#pragma unroll
        for (int nt = 7; nt < 12; ++nt) s1 += acc[mt][nt][r];
        s1 += t12ok ? acc[mt][12][r] : 0.f;
        const float mu0 = row16_sum(s0) * inv_n, mu1 = row16_sum(s1) * inv_n;
        float q0 = 0.f, q1 = 0.f;
#pragma unroll
        for (int nt = 0; nt < 6; ++nt) { const float d = acc[mt][nt][r] - mu0; q0 = fmaf(d, d, q0); }
        { const float d = acc[mt][6][r] - (t6p0 ? mu0 : mu1); const float dd = d * d; q0 += t6p0 ? dd : 0.f; q1 += t6p0 ? 0.f : dd; }
#pragma unroll
        for (int nt = 7; nt < 12; ++nt) { const float d = acc[mt][nt][r] - mu1; q1 = fmaf(d, d, q1); }
        { const float d = acc[mt][12][r] - mu1; q1 += t12ok ? d * d : 0.f; }
        mean0[mt][r] = mu0; mean1[mt][r] = mu1;
        // biased variance, like F.instance_norm.  FMT_F16: the accumulators are s x the product (s a power of two: mean and
        // deviations scale exactly), so the variance is q / s^2 and the normalised value (acc - mean) (rstd / s)
        rs0[mt][r] = 1.0f / sqrtf(row16_sum(q0) * inv_n2 + E.eps);
        rs1[mt][r] = 1.0f / sqrtf(row16_sum(q1) * inv_n2 + E.eps);
      }
      if (chok && c == 0) {
        if ((size_t)(pair0) * kPts < (size_t)ncols) *reinterpret_cast<f32x4*>(E.rstd + (size_t)pair0 * M + ch8 + 4 * mt) = rs0[mt];
        if ((size_t)(pair0 + 1) * kPts < (size_t)ncols) *reinterpret_cast<f32x4*>(E.rstd + (size_t)(pair0 + 1) * M + ch8 + 4 * mt) = rs1[mt];
      }
      // z = (v - mean) * (rstd gamma) + beta  (the difference first: no cancellation against a large mean)
#pragma unroll
      for (int r = 0; r < 4; ++r) { rs0[mt][r] *= gam[mt][r] * unscale; rs1[mt][r] *= gam[mt][r] * unscale; }
    }
    EST_STAMP(2);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const bool first = (nt < 6) || (nt == 6 && t6p0);
      const int cl = nt * 16 + c, col = n0 + cl;
      unsigned pl[4][4];  // two fp16 planes (forward) + two bf16 planes (backward)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float z = fmaf(acc[mt][nt][r] - (first ? mean0[mt][r] : mean1[mt][r]), first ? rs0[mt][r] : rs1[mt][r], bet[mt][r]);
          v[r] = (z > 0.f) ? z : z * E.slope;
        }
        split2h(v[0], v[1], pl[0][2 * mt], pl[1][2 * mt]);
        split2h(v[2], v[3], pl[0][2 * mt + 1], pl[1][2 * mt + 1]);
        if (E.planes_bwd) {  // uniform
          split2(v[0], v[1], pl[2][2 * mt], pl[3][2 * mt]);
          split2(v[2], v[3], pl[2][2 * mt + 1], pl[3][2 * mt + 1]);
        }
      }
      if (cl < BSTEP && col < ncols && chok) {
        const size_t at = kb_index((size_t)col, ch8, (size_t)ncols);
        bf16_t* dst = E.planes + at;
#pragma unroll
        for (int p = 0; p < 2; ++p) *reinterpret_cast<uint4*>(dst + p * E.plane_stride) = make_uint4(pl[p][0], pl[p][1], pl[p][2], pl[p][3]);
        if (E.planes_bwd) {
          bf16_t* bw = E.planes_bwd + at;
#pragma unroll
          for (int p = 0; p < 2; ++p) *reinterpret_cast<uint4*>(bw + p * E.bwd_stride) = make_uint4(pl[2 + p][0], pl[2 + p][1], pl[2 + p][2], pl[2 + p][3]);
        }
      }
    }
    EST_STAMP(4);
  }
}

// ---- dW[co][ci] = sum_cols dY[col][co] X[col][ci], two planes each (three products) ------------------------------------------
// Block: 128 x 128 output tile (2 x 2 wavefronts of 64 x 64 = 4 x 4 MFMA tiles), one slice of the columns (split-K); the partial
// product goes to part[slice][co][ci] (summed by the caller: deterministic, no floating-point atomics).
// LDS image per (operand, plane): [4 channel blocks][32 k][4 chunks of 8 channels] = the K-blocked global layout as it is (each
// LDS-DMA instruction copies one contiguous KiB: 16 columns of one channel block); chunk position q of column k holds channel
// chunk q ^ 2 ((k >> 2) & 1)  (the swizzle lives on the SOURCE address, the image itself is lane-linear), so that the eight
// columns a ds_read_b64_tr_b16 half-wave touches fall on all 64 banks.
// (the body is shared by the one-problem launch and the table-driven one of round 6: `id` = the workgroup's linear index among the
// nx * ny * nslices of its problem)
__device__ __forceinline__ void est_gemm_tn_body(const bf16_t* __restrict__ dY, size_t dy_plane, int Cout, const bf16_t* __restrict__ X,
                                                 size_t x_plane, int Cin, int ncols, int cols_per_slice, float* __restrict__ part, int id,
                                                 int nx, int ny, int nslices) {
  constexpr int kOpBytes = 2 * BK * 256;  // two planes of [32][256 B]
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kOpBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  // XCD-aware order: consecutive workgroup ids go round-robin to the 8 XCDs; all output tiles of one column slice
  // stream the same columns of dY and X, so a slice's tiles are given consecutive slots of ONE XCD and its L2 serves the re-reads
  // (in launch order the eight Cout tiles of a (Cin tile, slice) sat on eight different XCDs: X crossed the fabric eight times)
  int bx = id % nx, by = (id / nx) % ny, slice = id / (nx * ny);
  if ((nslices & 7) == 0) {
    const int tiles = nx * ny;
    const int xcd = id & 7, j = id >> 3, t = j % tiles;
    slice = (j / tiles) * 8 + xcd;
    bx = t % nx; by = t / nx;
  }
  const int m0 = bx * 128, n0 = by * 128;
  const int kbeg = slice * cols_per_slice;
  int kend = kbeg + cols_per_slice;
  kend = (kend < ncols) ? kend : ncols;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int dcol = lane >> 2, dq = (lane & 3) ^ (2 * ((lane >> 4) & 1));  // DMA role: column within the instruction, source chunk
  const int c = lane & 15, g = lane >> 4;
  const int tr_row = (c >> 2), tr_piece = c & 3;  // ds_read_tr role inside the 16-lane group
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    // 2 operands x 2 planes x 4 channel blocks x 2 column halves = 32 DMA instructions per stage, 8 per wavefront
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int t = wave * 8 + i;  // wave-uniform: operand = t >> 4, plane = (t >> 3) & 1, channel block = (t >> 1) & 3, half = t & 1
      const int op = t >> 4, p = (t >> 3) & 1, cb = (t >> 1) & 3, half = t & 1;
      int col = k0 + half * 16 + dcol;
      col = (col < kend) ? col : kend - 1;  // past the slice: a copy of the last column, zeroed below
      const int C = op ? Cin : Cout, base = op ? n0 : m0;
      int ch = base + cb * 32;
      ch = (ch < C) ? ch : 0;  // channel blocks past the operand: any valid address, masked at the store
      const bf16_t* src = (op ? X + (size_t)p * x_plane : dY + (size_t)p * dy_plane) + kb_index((size_t)col, ch, (size_t)ncols) + dq * 8;
      unsigned char* dst = lds + op * kOpBytes + p * (BK * 256) + cb * (BK * 64) + half * 16 * 64;
      __builtin_amdgcn_global_load_lds(DFEPE_GLOBAL_PTR(src), DFEPE_LDS_PTR(dst), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (k0 + BK > kend) {  // ragged last step of the slice: rows past the end hold a copy of the last column -- zero them
      for (int e = tid; e < 2 * kOpBytes / 16; e += 256) {
        const int k = (e >> 2) & (BK - 1);  // image [operand][plane][channel block][32 columns][4 chunks]
        if (k0 + k >= kend) reinterpret_cast<uint4*>(lds)[e] = make_uint4(0, 0, 0, 0);
      }
      __syncthreads();
    }
    // one 16-channel fragment (8 k-values per lane: rows 4g..4g+3 and 16+4g..16+4g+3 of the stage) through the transposing read
    auto frag = [&](int op, int p, int t) {
      typedef __attribute__((ext_vector_type(8))) short s16x8;
      // 16-channel tile t: channel block t >> 1, chunks 2 (t & 1), 2 (t & 1) + 1 of the column's 64 bytes
      const unsigned char* base = lds + op * kOpBytes + p * (BK * 256) + (t >> 1) * (BK * 64) + tr_piece * 8;
      const int ka = 4 * g + tr_row, kb = 16 + 4 * g + tr_row;
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(base + ka * 64 + (((2 * (t & 1)) ^ (2 * ((ka >> 2) & 1))) * 16)));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(base + kb * 64 + (((2 * (t & 1)) ^ (2 * ((kb >> 2) & 1))) * 16)));
      return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
    bf16x8 a[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int p = 0; p < 2; ++p) a[mt][p] = frag(0, p, wr * 4 + mt);
    bf16x8 b[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p) b[0][p] = frag(1, p, wc * 4);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      if (nt + 1 < 4) {
#pragma unroll
        for (int p = 0; p < 2; ++p) b[(nt + 1) & 1][p] = frag(1, p, wc * 4 + nt + 1);
      }
      __builtin_amdgcn_sched_barrier(0);  // the next tile's fragments stay ahead of this tile's MFMAs
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][1], b[nt & 1][0], acc[mt][nt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][0], b[nt & 1][1], acc[mt][nt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][0], b[nt & 1][0], acc[mt][nt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
  }
  float* dst = part + (size_t)slice * Cout * Cin;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int ci = n0 + wc * 64 + nt * 16 + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = m0 + wr * 64 + mt * 16 + 4 * g + r;
        if (co < Cout && ci < Cin) dst[(size_t)co * Cin + ci] = acc[mt][nt][r];
      }
    }
}
__global__ void __launch_bounds__(256, 2)
est_gemm_tn_kernel(const bf16_t* __restrict__ dY, size_t dy_plane, int Cout, const bf16_t* __restrict__ X, size_t x_plane, int Cin,
                   int ncols, int cols_per_slice, float* __restrict__ part) {
  const int nx = (int)gridDim.x, ny = (int)gridDim.y;
  est_gemm_tn_body(dY, dy_plane, Cout, X, x_plane, Cin, ncols, cols_per_slice, part, (int)blockIdx.x + nx * ((int)blockIdx.y + ny * (int)blockIdx.z),
                   nx, ny, (int)gridDim.z);
}
// every layer's weight gradient of one backward in ONE launch (round 6): over few columns a backward keeps all its dY alive to the end
// anyway (the gamma == 0 fix), and five launches of 1-32 tiles each become one grid that fills the chip
struct TnTab {
  int n;
  const bf16_t* dY[8]; const bf16_t* X[8];
  size_t dy_plane[8], x_plane[8];
  int Cout[8], Cin[8], nx[8], ny[8], slices[8], cps[8];
  float* part[8];
  int first_block[9];  // multiples of 8: a problem's linear ids keep their XCD phase
};
__global__ void __launch_bounds__(256, 2) est_gemm_tn_multi_kernel(const TnTab T, int ncols) {
  int l = 0;
  while (l + 1 < T.n && (int)blockIdx.x >= T.first_block[l + 1]) ++l;
  const int id = (int)blockIdx.x - T.first_block[l];
  if (id >= T.nx[l] * T.ny[l] * T.slices[l]) return;  // padding up to the next multiple of 8
  est_gemm_tn_body(T.dY[l], T.dy_plane[l], T.Cout[l], T.X[l], T.x_plane[l], T.Cin[l], ncols, T.cps[l], T.part[l], id, T.nx[l], T.ny[l], T.slices[l]);
}

}  // namespace

extern "C" int dfepe_est_points(void) { return kPts; }

// at most one workgroup per CU: a wavefront is alone on its SIMD and the GEMM kernels take their AHEAD = 2 build (B fragments two
// column tiles ahead of the MFMAs, two LDS stages); DFEPE_EST_SMALL_GRID=0 / 1 forces the choice (A/B timing)
static bool small_grid(const dim3& grid) {
  static const char* force = getenv("DFEPE_EST_SMALL_GRID");
  if (force) return force[0] == '1';
  return (size_t)grid.x * grid.y * grid.z <= 256;  // one workgroup per CU at most: the two-stage build's 86 KB of LDS admit no second one
}

// one est_gemm_nt_kernel launch: the small-grid (AHEAD = 2) build or the one tuned for full grids
template <int NPA, int NPB, int ORDER, int EPI, int FMT>
static int launch_nt(const dim3& grid, void* stream, const void* A, size_t a_plane, const void* B, size_t b_plane, int M, int ncols, int K,
                     const EpiArgs& E) {
  const auto kernel = small_grid(grid) ? est_gemm_nt_kernel<NPA, NPB, ORDER, EPI, FMT, 2> : est_gemm_nt_kernel<NPA, NPB, ORDER, EPI, FMT>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(A), a_plane,
                     static_cast<const bf16_t*>(B), b_plane, M, ncols, K, E);
  return launched();
}

// forward layer: planes_out[2][ncols][M] (fp16) = split(lrelu(IN(W X))) for the next layer, planes_bwd[2][ncols][M] (bf16, or
// null) = the same activation as the backward reads it, rstd[npairs][M].  W, X: two fp16 planes each (three products); W split
// scaled with `absmax` (dfepe_est_absmax + dfepe_est_split_f16), or unscaled with absmax = null.
extern "C" int dfepe_est_layer_fwd(const void* W, size_t w_plane, const void* X, size_t x_plane, int M, int ncols, int K,
                                   const unsigned* absmax, const float* gamma, const float* beta, float eps, float slope,
                                   void* planes_out, size_t out_plane, void* planes_bwd, size_t bwd_plane, float* rstd, void* stream) {
  if (!W || !X || !gamma || !beta || !planes_out || !rstd || M <= 0 || (M & 31) || ncols <= 0 || (ncols % kPts) || K <= 0 || (K % BK))
    return DFEPE_ERR_INVALID_ARG;
  if (!(slope > 0.f)) return DFEPE_ERR_UNSUPPORTED;  // the backward inverts the activation
  EpiArgs E{};
  E.gamma = gamma; E.beta = beta; E.eps = eps; E.slope = slope; E.planes = static_cast<bf16_t*>(planes_out); E.plane_stride = out_plane;
  E.rstd = rstd; E.absmax = absmax; E.planes_bwd = static_cast<bf16_t*>(planes_bwd); E.bwd_stride = bwd_plane;
  const dim3 grid((ncols + BSTEP - 1) / BSTEP, (M + BM - 1) / BM);
  return launch_nt<2, 2, 1, EPI_IN, FMT_F16>(grid, stream, W, w_plane, X, x_plane, M, ncols, K, E);
}

// the forward's plain product (any number of points per pair): out[col][m] fp32 = (1 / s) sum_terms A_i[m][:] . B_j[col][:] on two
// fp16 planes each, A split scaled by s (absmax as above, or null).  splits = S > 1 (round 6): S workgroups share a tile's K steps and leave
// S partial products out[z][col][m], z < S, split_stride floats apart -- summed by dfepe_est_norm_fwd_r
static int nt_f16_launch(const void* A, size_t a_plane, const void* B, size_t b_plane, int M, int ncols, int K, const unsigned* absmax,
                         float* out, int ldc, int splits, size_t split_stride, void* stream) {
  if (!A || !B || !out || M <= 0 || (M & 7) || ncols <= 0 || K <= 0 || (K % BK) || ldc < M || (ldc & 3)) return DFEPE_ERR_INVALID_ARG;
  if (splits < 1 || splits > K / BK || (splits > 1 && split_stride < (size_t)ncols * ldc)) return DFEPE_ERR_INVALID_ARG;
  EpiArgs E{};
  E.out = out; E.ldc = ldc; E.absmax = absmax; E.split_stride = split_stride;
  const dim3 grid((ncols + BSTEP - 1) / BSTEP, (M + BM - 1) / BM, splits);
  return launch_nt<2, 2, 1, EPI_F32, FMT_F16>(grid, stream, A, a_plane, B, b_plane, M, ncols, K, E);
}
extern "C" int dfepe_est_gemm_nt_f16(const void* A, size_t a_plane, const void* B, size_t b_plane, int M, int ncols, int K,
                                     const unsigned* absmax, float* out, int ldc, void* stream) {
  return nt_f16_launch(A, a_plane, B, b_plane, M, ncols, K, absmax, out, ldc, 1, 0, stream);
}
extern "C" int dfepe_est_gemm_nt_f16_splitk(const void* A, size_t a_plane, const void* B, size_t b_plane, int M, int ncols, int K,
                                            const unsigned* absmax, float* out, int ldc, int splits, size_t split_stride, void* stream) {
  return nt_f16_launch(A, a_plane, B, b_plane, M, ncols, K, absmax, out, ldc, splits, split_stride, stream);
}

// plain product: out[col][m] (fp32, ld = ldc) = sum_terms A_i[m][:] . B_j[col][:]; n_planes = 2 (three products) or 3 (six); splits as above
// (two planes only); gx != null (two planes, splits = 1): the product is the gradient w.r.t. the estimator's input and is stored as
// gx[pair * gx_sb + ch * gx_sc + n], ch < gx_C0, col = pair * gx_N + n, instead of out (round 6: was a transposing launch of its own)
static int nt_bf16_launch(const void* A, size_t a_plane, const void* B, size_t b_plane, int M, int ncols, int K, int n_planes, float* out,
                          int ldc, int splits, size_t split_stride, float* gx, int gx_C0, int gx_N, long gx_sb, long gx_sc, void* stream) {
  if (!A || !B || (!out && !gx) || M <= 0 || (M & 7) || ncols <= 0 || K <= 0 || (K % BK)) return DFEPE_ERR_INVALID_ARG;
  if (!gx && (ldc < M || (ldc & 3))) return DFEPE_ERR_INVALID_ARG;
  if (gx && (gx_C0 <= 0 || gx_C0 > M || gx_N <= 0 || (ncols % gx_N) || splits != 1 || n_planes != 2 || gx_sb <= 0 || gx_sc <= 0)) return DFEPE_ERR_INVALID_ARG;
  if (n_planes != 2 && n_planes != 3) return DFEPE_ERR_INVALID_ARG;
  if (splits < 1 || splits > K / BK || (splits > 1 && (n_planes != 2 || split_stride < (size_t)ncols * ldc))) return DFEPE_ERR_INVALID_ARG;
  EpiArgs E{};
  E.out = out; E.ldc = ldc; E.split_stride = split_stride; E.gx = gx; E.gx_C0 = gx_C0; E.gx_N = gx_N; E.gx_sb = gx_sb; E.gx_sc = gx_sc;
  const dim3 grid((ncols + BSTEP - 1) / BSTEP, (M + BM - 1) / BM, splits);
  if (n_planes == 2) return launch_nt<2, 2, 1, EPI_F32, FMT_BF16>(grid, stream, A, a_plane, B, b_plane, M, ncols, K, E);
  // three planes, six products: one build, tuned for full grids
  hipLaunchKernelGGL((est_gemm_nt_kernel<3, 3, 2, EPI_F32>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(A),
                     a_plane, static_cast<const bf16_t*>(B), b_plane, M, ncols, K, E);
  return launched();
}
extern "C" int dfepe_est_gemm_nt(const void* A, size_t a_plane, const void* B, size_t b_plane, int M, int ncols, int K, int n_planes,
                                 float* out, int ldc, void* stream) {
  return nt_bf16_launch(A, a_plane, B, b_plane, M, ncols, K, n_planes, out, ldc, 1, 0, nullptr, 0, 0, 0, 0, stream);
}
extern "C" int dfepe_est_gemm_nt_splitk(const void* A, size_t a_plane, const void* B, size_t b_plane, int M, int ncols, int K, float* out,
                                        int ldc, int splits, size_t split_stride, void* stream) {
  return nt_bf16_launch(A, a_plane, B, b_plane, M, ncols, K, 2, out, ldc, splits, split_stride, nullptr, 0, 0, 0, 0, stream);
}
extern "C" int dfepe_est_gemm_nt_gx(const void* A, size_t a_plane, const void* B, size_t b_plane, int M, int ncols, int K, float* gx, int C0,
                                    int N, long gx_stride_pair, long gx_stride_ch, void* stream) {
  return nt_bf16_launch(A, a_plane, B, b_plane, M, ncols, K, 2, nullptr, 0, 1, 0, gx, C0, N, gx_stride_pair, gx_stride_ch, stream);
}

// data gradient + the adjoint of the layer below in one launch (N = dfepe_est_points()):
//   dA[col][m] = sum_k WT[m][k] dY_next[col][k]  (two bf16 planes each, three products; never written),
//   dY[2][ncols][M] = InstanceNorm + LeakyReLU adjoint of the layer whose output planes are `aout`, and its per-pair d gamma / d beta
extern "C" int dfepe_est_dgrad_in_bwd(const void* WT, size_t wt_plane, const void* dY_next, size_t dyn_plane, int M, int ncols, int K,
                                      const void* aout, size_t aout_plane, const float* rstd, const float* gamma, const float* beta,
                                      float slope, void* dY, size_t dy_plane, float* dgamma_part, float* dbeta_part, void* stream) {
  if (!WT || !dY_next || !aout || !rstd || !gamma || !beta || !dY || !dgamma_part || !dbeta_part) return DFEPE_ERR_INVALID_ARG;
  if (M <= 0 || (M & 31) || ncols <= 0 || (ncols % kPts) || K <= 0 || (K % BK) || !(slope > 0.f)) return DFEPE_ERR_INVALID_ARG;
  EpiArgs E{};
  E.gamma = gamma; E.beta = beta; E.slope = slope; E.planes = static_cast<bf16_t*>(dY); E.plane_stride = dy_plane;
  E.aout = static_cast<const bf16_t*>(aout); E.aout_stride = aout_plane; E.rstd_in = rstd; E.dgamma_part = dgamma_part; E.dbeta_part = dbeta_part;
  const dim3 grid((ncols + BSTEP - 1) / BSTEP, (M + BM - 1) / BM);
  return launch_nt<2, 2, 1, EPI_INBWD, FMT_BF16>(grid, stream, WT, wt_plane, dY_next, dyn_plane, M, ncols, K, E);
}

// weight gradient partials: part[slices][Cout][Cin]
extern "C" int dfepe_est_gemm_tn(const void* dY, size_t dy_plane, int Cout, const void* X, size_t x_plane, int Cin, int ncols,
                                 int slices, float* part, void* stream) {
  if (!dY || !X || !part || Cout <= 0 || Cin <= 0 || (Cout & 31) || (Cin & 31) || ncols <= 0 || slices <= 0) return DFEPE_ERR_INVALID_ARG;
  int cps = (ncols + slices - 1) / slices;
  cps = ((cps + BK - 1) / BK) * BK;
  const dim3 grid((Cout + 127) / 128, (Cin + 127) / 128, slices), block(256);
  hipLaunchKernelGGL(est_gemm_tn_kernel, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(dY), dy_plane, Cout,
                     static_cast<const bf16_t*>(X), x_plane, Cin, ncols, cps, part);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

// the weight-gradient partials of n_layers <= 8 layers over the same ncols columns in ONE launch (host arrays indexed by layer)
extern "C" int dfepe_est_gemm_tn_multi(int n_layers, const void* const* dY, const size_t* dy_plane, const int* Cout, const void* const* X,
                                       const size_t* x_plane, const int* Cin, int ncols, const int* slices, float* const* part, void* stream) {
  if (n_layers <= 0 || n_layers > 8 || !dY || !dy_plane || !Cout || !X || !x_plane || !Cin || !slices || !part || ncols <= 0)
    return DFEPE_ERR_INVALID_ARG;
  TnTab T{};
  T.n = n_layers;
  int blocks = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (!dY[l] || !X[l] || !part[l] || Cout[l] <= 0 || Cin[l] <= 0 || (Cout[l] & 31) || (Cin[l] & 31) || slices[l] <= 0) return DFEPE_ERR_INVALID_ARG;
    int cps = (ncols + slices[l] - 1) / slices[l];
    cps = ((cps + BK - 1) / BK) * BK;
    T.dY[l] = static_cast<const bf16_t*>(dY[l]); T.X[l] = static_cast<const bf16_t*>(X[l]); T.dy_plane[l] = dy_plane[l]; T.x_plane[l] = x_plane[l];
    T.Cout[l] = Cout[l]; T.Cin[l] = Cin[l]; T.nx[l] = (Cout[l] + 127) / 128; T.ny[l] = (Cin[l] + 127) / 128; T.slices[l] = slices[l]; T.cps[l] = cps;
    T.part[l] = part[l];
    T.first_block[l] = blocks;
    blocks += (T.nx[l] * T.ny[l] * slices[l] + 7) / 8 * 8;
  }
  T.first_block[n_layers] = blocks;
  hipLaunchKernelGGL(est_gemm_tn_multi_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), T, ncols);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
