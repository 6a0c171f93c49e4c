// est_norm -- the weight estimator's normalisation, its adjoints and the head (precision and plane layout: est_common.h), in
// three generations that all remain in use:
//   est_in_bwd    InstanceNorm + LeakyReLU adjoint in the point-major layout at N = 100 (x^ and the activation sign recovered from
//                 the stored planes), writes dY as two planes; streams at 5 TB/s.  Since round 5 only the layer under the head runs
//                 it as a launch of its own: below that the adjoint is the data-gradient GEMM's epilogue (est_gemm.hip, EPI_INBWD).
//   est_norm_fwd_n / est_in_bwd_n   (round 4) the normalisation + activation + split of the fused forward epilogue, and its
//                 adjoint, for ANY number of points per pair behind the plain product (EPI_F32): a workgroup per (pair, 64
//                 channels) striding the pair's columns, or the pair's rows over several workgroups in two launches when a dozen
//                 pairs would not fill the chip.  What serves N > 2048.
//   est_norm_fwd_r / est_in_bwd_r   (round 6) the same with the pair's block resident in registers (N <= 2048), summing the plain
//                 product's split-K partials on the way in: one launch, one read.
//   est_head_*    the last Conv1d(256 -> O) and its adjoint pieces (a GEMV per output channel: VALU, HBM-bound).
//   est_dgamma_zero   d gamma of a channel whose gamma is exactly zero, where the adjoints above cannot recover x^.
#include "est_common.h"

namespace {

// ---- InstanceNorm + LeakyReLU adjoint, point-major ----------------------------------------------------------------------------
// One workgroup = one pair (100 columns) x 64 channels: 32 channel pairs x 8 row groups of 13 columns.  Inputs: the upstream
// gradient dA [cols][C] fp32 -- or, for the layer under the head, its rank-one form dlogit[col] * w_head[c] --, the layer's
// output planes (a = lrelu(z), z = gamma x^ + beta: z and x^ are recovered from them -- from the two leading planes, 2^-17 of a: the
// third would be 2 of the 14 bytes per element this HBM-bound kernel moves, for digits the two-plane products downstream drop),
// rstd, gamma, beta.  Outputs: dY as two planes, and the pair's contributions to d gamma / d beta ([pair][C] each, summed by the caller).
__global__ void __launch_bounds__(256)
est_in_bwd_kernel(const float* __restrict__ dA, const float* __restrict__ dlogit, const float* __restrict__ w_head,
                  const bf16_t* __restrict__ planes, size_t plane_stride, const float* __restrict__ rstd,
                  const float* __restrict__ gamma, const float* __restrict__ beta, float slope, int C, int ncols,
                  bf16_t* __restrict__ dYp, size_t dy_plane, float* __restrict__ dgamma_part, float* __restrict__ dbeta_part) {
  __shared__ float red[2][8][64];
  const int pair = (int)blockIdx.x, cb = (int)blockIdx.y * 64;
  const int cp = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int ch = cb + 2 * cp;
  const bool chok = ch < C;
  const int chc = chok ? ch : 0;
  const float g0 = gamma[chc], g1 = gamma[chc + 1], b0 = beta[chc], b1 = beta[chc + 1];
  const float ig0 = (fabsf(g0) > 1e-30f) ? 1.0f / g0 : 0.0f, ig1 = (fabsf(g1) > 1e-30f) ? 1.0f / g1 : 0.0f;
  const float islope = 1.0f / slope;
  const float r0 = rstd[(size_t)pair * C + chc], r1 = rstd[(size_t)pair * C + chc + 1];
  constexpr int RPG = 13;  // 8 x 13 >= 100
  float dz0[RPG], dz1[RPG], xh0[RPG], xh1[RPG];
  float s10 = 0.f, s11 = 0.f, s20 = 0.f, s21 = 0.f;
#pragma unroll
  for (int i = 0; i < RPG; ++i) {
    const int rl = rg * RPG + i;
    const bool live = rl < kPts;
    const size_t col = (size_t)pair * kPts + (live ? rl : 0);
    const size_t at = kb_index(col, chc, (size_t)ncols);
    const unsigned u0 = *reinterpret_cast<const unsigned*>(planes + at);
    const unsigned u1 = *reinterpret_cast<const unsigned*>(planes + plane_stride + at);
    // two planes: a to 2^-17, the class of the two-plane products this gradient feeds; the sign of a is its leading plane's
    const float a0 = bf16_lo(u0) + bf16_lo(u1), a1 = bf16_hi(u0) + bf16_hi(u1);
    float d0, d1;
    if (dA != nullptr) {
      const f32x2 d = *reinterpret_cast<const f32x2*>(dA + col * C + chc);
      d0 = d[0]; d1 = d[1];
    } else {
      const float dl = dlogit[col];
      d0 = dl * w_head[chc]; d1 = dl * w_head[chc + 1];
    }
    const float z0 = (a0 > 0.f) ? a0 : a0 * islope, z1 = (a1 > 0.f) ? a1 : a1 * islope;
    const float e0 = live ? ((a0 > 0.f) ? d0 : d0 * slope) : 0.f, e1 = live ? ((a1 > 0.f) ? d1 : d1 * slope) : 0.f;
    const float x0 = (z0 - b0) * ig0, x1 = (z1 - b1) * ig1;
    dz0[i] = e0; dz1[i] = e1; xh0[i] = x0; xh1[i] = x1;
    s10 += e0; s11 += e1; s20 = fmaf(e0, x0, s20); s21 = fmaf(e1, x1, s21);
  }
  red[0][rg][2 * cp] = s10; red[0][rg][2 * cp + 1] = s11;
  red[1][rg][2 * cp] = s20; red[1][rg][2 * cp + 1] = s21;
  __syncthreads();
  float S10 = 0.f, S11 = 0.f, S20 = 0.f, S21 = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    S10 += red[0][q][2 * cp]; S11 += red[0][q][2 * cp + 1];
    S20 += red[1][q][2 * cp]; S21 += red[1][q][2 * cp + 1];
  }
  if (rg == 0 && chok) {
    dbeta_part[(size_t)pair * C + ch] = S10; dbeta_part[(size_t)pair * C + ch + 1] = S11;
    dgamma_part[(size_t)pair * C + ch] = S20; dgamma_part[(size_t)pair * C + ch + 1] = S21;
  }
  const float inv_n = 1.0f / (float)kPts;
  const float k0 = r0 * g0, k1 = r1 * g1;
  const float m10 = S10 * inv_n, m11 = S11 * inv_n, m20 = S20 * inv_n, m21 = S21 * inv_n;
#pragma unroll
  for (int i = 0; i < RPG; ++i) {
    const int rl = rg * RPG + i;
    if (rl < kPts && chok) {
      const size_t col = (size_t)pair * kPts + rl;
      const float y0 = k0 * (dz0[i] - m10 - xh0[i] * m20), y1 = k1 * (dz1[i] - m11 - xh1[i] * m21);
      unsigned p0, p1;
      split2(y0, y1, p0, p1);
      const size_t at = kb_index(col, ch, (size_t)ncols);
      *reinterpret_cast<unsigned*>(dYp + at) = p0;
      *reinterpret_cast<unsigned*>(dYp + dy_plane + at) = p1;
    }
  }
}

// ---- any number of points per pair: InstanceNorm + LeakyReLU + split behind the plain product, and its adjoint ---------------
// The fused epilogue above is built around 100 points per pair.  For another N (the reference's SIFT configurations carry up to
// 2000 correspondences, deepFEPE/configs/*.yaml, at batch sizes of 4-12) a layer is the plain product est_gemm_nt<EPI_F32>
// followed by this kernel: one workgroup = one pair x 64 channels, 32 channel pairs x 32 row groups striding the pair's columns,
// four independent rows in flight per thread (with a dozen pairs the grid is a few hundred workgroups at most: the time is the
// chain of dependent load latencies, so the rows are spread over 1024 threads and the loads unrolled).  Three passes over the
// pair's fp32 block (mean; squared deviations from it -- the same two-pass variance as the epilogue --; normalise + activate +
// split): N x 64 x 4 bytes, L2-resident between the passes.
constexpr int kRG = 32;   // row groups of a workgroup
constexpr int kRU = 4;    // rows a thread has in flight

__device__ __forceinline__ void pair_reduce2(float (&red)[kRG][64], int rg, int cp, float a, float b, float& A, float& B) {
  __syncthreads();  // the previous reduction's readers are done
  red[rg][2 * cp] = a; red[rg][2 * cp + 1] = b;
  __syncthreads();
  A = 0.f; B = 0.f;
#pragma unroll
  for (int q = 0; q < kRG; ++q) { A += red[q][2 * cp]; B += red[q][2 * cp + 1]; }
}

// MODE 0: the whole pair in one workgroup (grid.z = 1).  With a dozen pairs that is too few workgroups, so the pair's rows can be
// split over grid.z = S workgroups and two launches: MODE 1 leaves each split's mean and sum of squared deviations from it in
// part[pair][split][2][C], MODE 2 merges the S partials (Chan's pairwise formula: M2 = sum M2_s + sum n_s (m_s - m)^2, as accurate
// as the two-pass form) and normalises its own rows.
template <int MODE>
__global__ void __launch_bounds__(1024)
est_norm_fwd_n_kernel(const float* __restrict__ Y, int ldy, int C, int N, size_t ncols, const float* __restrict__ gamma,
                      const float* __restrict__ beta, float eps, float slope, bf16_t* __restrict__ planes, size_t plane_stride,
                      bf16_t* __restrict__ planes_bwd, size_t bwd_stride, float* __restrict__ rstd, float* __restrict__ part) {
  __shared__ float red[kRG][64];
  const int pair = (int)blockIdx.x, cb = (int)blockIdx.y * 64;
  const int S = (int)gridDim.z, sp = (int)blockIdx.z;
  const int R = (N + S - 1) / S;
  const int r0 = sp * R, r1 = (r0 + R < N) ? r0 + R : N;  // this workgroup's rows (possibly none in the last split)
  const int cp = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int ch = cb + 2 * cp;
  const bool chok = ch < C;
  const int chc = chok ? ch : 0;
  const size_t col0 = (size_t)pair * N;
  const float* Yc = Y + col0 * ldy + chc;
  float mu0, mu1, Q0, Q1;
  if (MODE != 2) {
    const float inv_n = 1.0f / (float)((r1 > r0) ? r1 - r0 : 1);
    float s0 = 0.f, s1 = 0.f;
    for (int rb = r0 + rg; rb < r1; rb += kRG * kRU) {
      f32x2 y[kRU];
#pragma unroll
      for (int u = 0; u < kRU; ++u) { const int rl = rb + kRG * u; y[u] = *reinterpret_cast<const f32x2*>(Yc + (size_t)(rl < r1 ? rl : rb) * ldy); }
#pragma unroll
      for (int u = 0; u < kRU; ++u) { const bool live = rb + kRG * u < r1; s0 += live ? y[u][0] : 0.f; s1 += live ? y[u][1] : 0.f; }
    }
    float S0, S1;
    pair_reduce2(red, rg, cp, s0, s1, S0, S1);
    mu0 = S0 * inv_n; mu1 = S1 * inv_n;
    float q0 = 0.f, q1 = 0.f;
    for (int rb = r0 + rg; rb < r1; rb += kRG * kRU) {
      f32x2 y[kRU];
#pragma unroll
      for (int u = 0; u < kRU; ++u) { const int rl = rb + kRG * u; y[u] = *reinterpret_cast<const f32x2*>(Yc + (size_t)(rl < r1 ? rl : rb) * ldy); }
#pragma unroll
      for (int u = 0; u < kRU; ++u) {
        const bool live = rb + kRG * u < r1;
        const float d0 = y[u][0] - mu0, d1 = y[u][1] - mu1;
        q0 += live ? d0 * d0 : 0.f; q1 += live ? d1 * d1 : 0.f;
      }
    }
    pair_reduce2(red, rg, cp, q0, q1, Q0, Q1);
    if (MODE == 1) {
      if (rg == 0 && chok) {
        float* P = part + ((size_t)pair * S + sp) * 2 * C + ch;
        P[0] = mu0; P[1] = mu1; P[C] = Q0; P[C + 1] = Q1;
      }
      return;
    }
  } else {
    const float* P = part + (size_t)pair * S * 2 * C + chc;
    float a0 = 0.f, a1 = 0.f;
    for (int t = 0; t < S; ++t) {
      const int n_t = ((t + 1) * R < N ? (t + 1) * R : N) - t * R;
      if (n_t > 0) { a0 = fmaf((float)n_t, P[(size_t)t * 2 * C], a0); a1 = fmaf((float)n_t, P[(size_t)t * 2 * C + 1], a1); }
    }
    mu0 = a0 / (float)N; mu1 = a1 / (float)N;
    Q0 = 0.f; Q1 = 0.f;
    for (int t = 0; t < S; ++t) {
      const int n_t = ((t + 1) * R < N ? (t + 1) * R : N) - t * R;
      if (n_t > 0) {
        const float d0 = P[(size_t)t * 2 * C] - mu0, d1 = P[(size_t)t * 2 * C + 1] - mu1;
        Q0 += P[(size_t)t * 2 * C + C] + (float)n_t * d0 * d0; Q1 += P[(size_t)t * 2 * C + C + 1] + (float)n_t * d1 * d1;
      }
    }
  }
  const float inv_N = 1.0f / (float)N;
  const float rs0 = 1.0f / sqrtf(Q0 * inv_N + eps), rs1 = 1.0f / sqrtf(Q1 * inv_N + eps);  // biased variance, like F.instance_norm
  if (rg == 0 && sp == 0 && chok) { rstd[(size_t)pair * C + ch] = rs0; rstd[(size_t)pair * C + ch + 1] = rs1; }
  const float k0 = rs0 * gamma[chc], k1 = rs1 * gamma[chc + 1], b0 = beta[chc], b1 = beta[chc + 1];
  if (!chok) return;
  for (int rb = r0 + rg; rb < r1; rb += kRG * kRU) {
    f32x2 y[kRU];
#pragma unroll
    for (int u = 0; u < kRU; ++u) { const int rl = rb + kRG * u; y[u] = *reinterpret_cast<const f32x2*>(Yc + (size_t)(rl < r1 ? rl : rb) * ldy); }
#pragma unroll
    for (int u = 0; u < kRU; ++u) {
      const int rl = rb + kRG * u;
      if (rl >= r1) break;
      const float z0 = fmaf(y[u][0] - mu0, k0, b0), z1 = fmaf(y[u][1] - mu1, k1, b1);
      const float a0 = (z0 > 0.f) ? z0 : z0 * slope, a1 = (z1 > 0.f) ? z1 : z1 * slope;
      unsigned p0, p1;
      split2h(a0, a1, p0, p1);  // two fp16 planes: the next layer's operand
      const size_t at = kb_index(col0 + rl, ch, ncols);
      *reinterpret_cast<unsigned*>(planes + at) = p0;
      *reinterpret_cast<unsigned*>(planes + plane_stride + at) = p1;
      if (planes_bwd) {  // two bf16 planes: what the backward reads
        split2(a0, a1, p0, p1);
        *reinterpret_cast<unsigned*>(planes_bwd + at) = p0;
        *reinterpret_cast<unsigned*>(planes_bwd + bwd_stride + at) = p1;
      }
    }
  }
}

// The adjoint for any N: est_in_bwd_kernel's arithmetic with the pair's columns strided instead of held in registers -- one pass
// for the two sums, one that recomputes d z and x^ from the same inputs and writes dY.  MODE as above: 1 leaves the split's two
// sums in part[pair][split][2][C], 2 adds the S partials up and writes its own rows.
template <int MODE>
__global__ void __launch_bounds__(1024)
est_in_bwd_n_kernel(const float* __restrict__ dA, const float* __restrict__ dlogit, const float* __restrict__ w_head,
                    const bf16_t* __restrict__ planes, size_t plane_stride, const float* __restrict__ rstd,
                    const float* __restrict__ gamma, const float* __restrict__ beta, float slope, int C, int N, size_t ncols,
                    bf16_t* __restrict__ dYp, size_t dy_plane, float* __restrict__ dgamma_part, float* __restrict__ dbeta_part,
                    float* __restrict__ part) {
  __shared__ float red[kRG][64];
  const int pair = (int)blockIdx.x, cb = (int)blockIdx.y * 64;
  const int S = (int)gridDim.z, sp = (int)blockIdx.z;
  const int R = (N + S - 1) / S;
  const int r0 = sp * R, r1 = (r0 + R < N) ? r0 + R : N;
  const int cp = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int ch = cb + 2 * cp;
  const bool chok = ch < C;
  const int chc = chok ? ch : 0;
  const float g0 = gamma[chc], g1 = gamma[chc + 1], b0 = beta[chc], b1 = beta[chc + 1];
  const float ig0 = (fabsf(g0) > 1e-30f) ? 1.0f / g0 : 0.0f, ig1 = (fabsf(g1) > 1e-30f) ? 1.0f / g1 : 0.0f;
  const float islope = 1.0f / slope;
  const float wh0 = dA ? 0.f : w_head[chc], wh1 = dA ? 0.f : w_head[chc + 1];
  const size_t col0 = (size_t)pair * N;
  struct Raw { unsigned u0, u1; float d0, d1; };
  auto load = [&](int rl) {
    const size_t col = col0 + rl;
    const size_t at = kb_index(col, chc, ncols);
    Raw r;
    r.u0 = *reinterpret_cast<const unsigned*>(planes + at);
    r.u1 = *reinterpret_cast<const unsigned*>(planes + plane_stride + at);
    if (dA != nullptr) {
      const f32x2 d = *reinterpret_cast<const f32x2*>(dA + col * C + chc);
      r.d0 = d[0]; r.d1 = d[1];
    } else {
      const float dl = dlogit[col];
      r.d0 = dl * wh0; r.d1 = dl * wh1;
    }
    return r;
  };
  auto item = [&](const Raw& r, float& e0, float& e1, float& x0, float& x1) {
    // (+ 0.0f: where a third plane used to be added; it turns a sum of -0 into +0 and stays so that the kernel's code does not change)
    const float a0 = (bf16_lo(r.u0) + bf16_lo(r.u1)) + 0.0f, a1 = (bf16_hi(r.u0) + bf16_hi(r.u1)) + 0.0f;
    const float z0 = (a0 > 0.f) ? a0 : a0 * islope, z1 = (a1 > 0.f) ? a1 : a1 * islope;
    e0 = (a0 > 0.f) ? r.d0 : r.d0 * slope; e1 = (a1 > 0.f) ? r.d1 : r.d1 * slope;
    x0 = (z0 - b0) * ig0; x1 = (z1 - b1) * ig1;
  };
  float S10, S11, S20, S21;
  if (MODE != 2) {
    float s10 = 0.f, s11 = 0.f, s20 = 0.f, s21 = 0.f;
    for (int rb = r0 + rg; rb < r1; rb += kRG * kRU) {
      Raw r[kRU];
#pragma unroll
      for (int u = 0; u < kRU; ++u) { const int rl = rb + kRG * u; r[u] = load(rl < r1 ? rl : rb); }
#pragma unroll
      for (int u = 0; u < kRU; ++u) {
        float e0, e1, x0, x1;
        item(r[u], e0, e1, x0, x1);
        if (rb + kRG * u >= r1) { e0 = 0.f; e1 = 0.f; }
        s10 += e0; s11 += e1; s20 = fmaf(e0, x0, s20); s21 = fmaf(e1, x1, s21);
      }
    }
    pair_reduce2(red, rg, cp, s10, s11, S10, S11);
    pair_reduce2(red, rg, cp, s20, s21, S20, S21);
    if (MODE == 1) {
      if (rg == 0 && chok) {
        float* P = part + ((size_t)pair * S + sp) * 2 * C + ch;
        P[0] = S10; P[1] = S11; P[C] = S20; P[C + 1] = S21;
      }
      return;
    }
  } else {
    const float* P = part + (size_t)pair * S * 2 * C + chc;
    S10 = 0.f; S11 = 0.f; S20 = 0.f; S21 = 0.f;
    for (int t = 0; t < S; ++t) {
      S10 += P[(size_t)t * 2 * C]; S11 += P[(size_t)t * 2 * C + 1];
      S20 += P[(size_t)t * 2 * C + C]; S21 += P[(size_t)t * 2 * C + C + 1];
    }
  }
  if (!chok) return;
  if (rg == 0 && sp == 0) {
    dbeta_part[(size_t)pair * C + ch] = S10; dbeta_part[(size_t)pair * C + ch + 1] = S11;
    dgamma_part[(size_t)pair * C + ch] = S20; dgamma_part[(size_t)pair * C + ch + 1] = S21;
  }
  const float inv_n = 1.0f / (float)N;
  const float k0 = rstd[(size_t)pair * C + ch] * g0, k1 = rstd[(size_t)pair * C + ch + 1] * g1;
  const float m10 = S10 * inv_n, m11 = S11 * inv_n, m20 = S20 * inv_n, m21 = S21 * inv_n;
  for (int rb = r0 + rg; rb < r1; rb += kRG * kRU) {
    Raw r[kRU];
#pragma unroll
    for (int u = 0; u < kRU; ++u) { const int rl = rb + kRG * u; r[u] = load(rl < r1 ? rl : rb); }
#pragma unroll
    for (int u = 0; u < kRU; ++u) {
      const int rl = rb + kRG * u;
      if (rl >= r1) break;
      float e0, e1, x0, x1;
      item(r[u], e0, e1, x0, x1);
      unsigned p0, p1;
      split2(k0 * (e0 - m10 - x0 * m20), k1 * (e1 - m11 - x1 * m21), p0, p1);
      const size_t at = kb_index(col0 + rl, ch, ncols);
      *reinterpret_cast<unsigned*>(dYp + at) = p0;
      *reinterpret_cast<unsigned*>(dYp + dy_plane + at) = p1;
    }
  }
}

// ---- round 6: the same two kernels with the pair's block RESIDENT IN REGISTERS, summing split-K partials on the way in ----------
// What the reference's own configurations need (N = 1000-2000 points, 4-12 pairs per batch, deepFEPE/configs/kitti_corr_baseline.yaml:
// 12-13) and what the K-heavy layers need at ANY N once a batch is so small that one 128 x 208 tile per workgroup leaves most CUs idle:
// the product is the plain GEMM (EPI_F32), optionally split over S slices of K (S partial products [S][cols][ld] fp32), and ONE more
// launch does everything else.  A workgroup = one pair x 32 channels (one K block of the plane layout) = 16 channel pairs x 64 row
// groups; thread (cp, rg) owns rows rg, rg + 64, ... (RPT = ceil(N / 64) of them, template: N <= 128 / 512 / 1024 / 2048) of its two
// channels: ONE pass over the fp32 block -- the partials added in slice order --, the values stay in registers for the two-pass
// statistics (mean, then squared deviations: the same arithmetic as the fused epilogue and est_norm_fwd_n) and the normalise +
// activate + split.  Against est_norm_fwd_n (three passes, two launches when the pair's rows are spread): one launch, one read.
// Geometry: CP channel pairs x RG = 1024 / CP row groups per workgroup; RPT rows per thread.  (CP, RPT) = (16, 2 / 8 / 16) serves
// N <= 128 / 512 / 1024 with 32 channels per workgroup; N <= 2048 takes (8, 16): 16 channels, because 1024 threads hold 128 registers
// each and the adjoint keeps four values per (row, channel pair).
// sums over the workgroup's row groups of NV values per thread (each channel pair's own): a wavefront holds 64 / CP row groups --
// cross-lane exchanges --, then sixteen partials per channel pair through LDS
template <int NV, int CP>
__device__ __forceinline__ void rg_all_sum(float (&red)[16][NV][CP], float (&v)[NV]) {
  const int cp = threadIdx.x & (CP - 1), w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int o = CP; o < 64; o <<= 1) v[i] += __shfl_xor(v[i], o, 64);
  }
  __syncthreads();  // the previous reduction's readers are done
  if ((threadIdx.x & 63) < CP) {
#pragma unroll
    for (int i = 0; i < NV; ++i) red[w][i][cp] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    float t = red[0][i][cp];
#pragma unroll
    for (int q = 1; q < 16; ++q) t += red[q][i][cp];
    v[i] = t;
  }
}

template <int RPT, int CP>
__global__ void __launch_bounds__(1024)
est_norm_fwd_r_kernel(const float* __restrict__ Y, int ldy, size_t split_stride, int S, int C, int N, size_t ncols,
                      const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float slope, bf16_t* __restrict__ planes,
                      size_t plane_stride, bf16_t* __restrict__ planes_bwd, size_t bwd_stride, float* __restrict__ rstd) {
  constexpr int RG = 1024 / CP;
  __shared__ float red[16][2][CP];
  const int pair = (int)blockIdx.x, cb = (int)blockIdx.y * (2 * CP);
  const int cp = threadIdx.x & (CP - 1), rg = threadIdx.x / CP;
  const int ch = cb + 2 * cp;  // C % 32 == 0: every channel of the workgroup exists
  const size_t col0 = (size_t)pair * N;
  const float* Yc = Y + col0 * ldy + ch;
  f32x2 v[RPT];
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int rl = rg + RG * i;
    v[i] = *reinterpret_cast<const f32x2*>(Yc + (size_t)(rl < N ? rl : 0) * ldy);
  }
  for (int s = 1; s < S; ++s) {
    const float* Ys = Yc + (size_t)s * split_stride;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int rl = rg + RG * i;
      v[i] += *reinterpret_cast<const f32x2*>(Ys + (size_t)(rl < N ? rl : 0) * ldy);
    }
  }
  const float inv_N = 1.0f / (float)N;
  float a[2] = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < RPT; ++i) { const bool live = rg + RG * i < N; a[0] += live ? v[i][0] : 0.f; a[1] += live ? v[i][1] : 0.f; }
  rg_all_sum<2, CP>(red, a);
  const float mu0 = a[0] * inv_N, mu1 = a[1] * inv_N;
  float q[2] = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const bool live = rg + RG * i < N;
    const float d0 = v[i][0] - mu0, d1 = v[i][1] - mu1;
    q[0] += live ? d0 * d0 : 0.f; q[1] += live ? d1 * d1 : 0.f;
  }
  rg_all_sum<2, CP>(red, q);
  const float rs0 = 1.0f / sqrtf(q[0] * inv_N + eps), rs1 = 1.0f / sqrtf(q[1] * inv_N + eps);  // biased variance, like F.instance_norm
  if (rg == 0) { rstd[(size_t)pair * C + ch] = rs0; rstd[(size_t)pair * C + ch + 1] = rs1; }
  const float k0 = rs0 * gamma[ch], k1 = rs1 * gamma[ch + 1], b0 = beta[ch], b1 = beta[ch + 1];
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int rl = rg + RG * i;
    if (rl < N) {
      const float z0 = fmaf(v[i][0] - mu0, k0, b0), z1 = fmaf(v[i][1] - mu1, k1, b1);
      const float a0 = (z0 > 0.f) ? z0 : z0 * slope, a1 = (z1 > 0.f) ? z1 : z1 * slope;
      unsigned p0, p1;
      split2h(a0, a1, p0, p1);  // two fp16 planes: the next layer's operand
      const size_t at = kb_index(col0 + rl, ch, ncols);
      *reinterpret_cast<unsigned*>(planes + at) = p0;
      *reinterpret_cast<unsigned*>(planes + plane_stride + at) = p1;
      if (planes_bwd) {  // two bf16 planes: what the backward reads
        split2(a0, a1, p0, p1);
        *reinterpret_cast<unsigned*>(planes_bwd + at) = p0;
        *reinterpret_cast<unsigned*>(planes_bwd + bwd_stride + at) = p1;
      }
    }
  }
}

// the adjoint, same geometry: dz and x^ of the thread's rows stay in registers between the two sums and the dY they feed (the rows come
// in four at a time: with all of a thread's raw words in flight at once the 128 registers of a 1024-thread workgroup spill)
template <int RPT, int CP>
__global__ void __launch_bounds__(1024)
est_in_bwd_r_kernel(const float* __restrict__ dA, int ldd, size_t split_stride, int S, const float* __restrict__ dlogit,
                    const float* __restrict__ w_head, const bf16_t* __restrict__ planes, size_t plane_stride, const float* __restrict__ rstd,
                    const float* __restrict__ gamma, const float* __restrict__ beta, float slope, int C, int N, size_t ncols,
                    bf16_t* __restrict__ dYp, size_t dy_plane, float* __restrict__ dgamma_part, float* __restrict__ dbeta_part) {
  constexpr int RG = 1024 / CP;
  constexpr int CHUNK = RPT < 4 ? RPT : 4;
  __shared__ float red[16][4][CP];
  const int pair = (int)blockIdx.x, cb = (int)blockIdx.y * (2 * CP);
  const int cp = threadIdx.x & (CP - 1), rg = threadIdx.x / CP;
  const int ch = cb + 2 * cp;
  const size_t col0 = (size_t)pair * N;
  const float g0 = gamma[ch], g1 = gamma[ch + 1], b0 = beta[ch], b1 = beta[ch + 1];
  const float ig0 = (fabsf(g0) > 1e-30f) ? 1.0f / g0 : 0.0f, ig1 = (fabsf(g1) > 1e-30f) ? 1.0f / g1 : 0.0f;
  const float islope = 1.0f / slope;
  const float wh0 = dA ? 0.f : w_head[ch], wh1 = dA ? 0.f : w_head[ch + 1];
  // RPT >= 16: x^ is not kept but formed again from a second read of the planes (L2) for the output pass -- dz alone is 32 registers
  constexpr bool kKeepX = RPT < 16;
  f32x2 dz[RPT], xh[kKeepX ? RPT : 1];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i0 = 0; i0 < RPT; i0 += CHUNK) {
    unsigned u0[CHUNK], u1[CHUNK];
    f32x2 d[CHUNK];
    int rgx = rg;
    asm volatile("" : "+v"(rgx));  // the address arithmetic stays with its chunk (hoisted, the thread's 3 x RPT addresses are what spills)
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) {
      const int rl = rgx + RG * (i0 + k);
      const size_t col = col0 + (rl < N ? rl : 0);
      const size_t at = kb_index(col, ch, ncols);
      u0[k] = *reinterpret_cast<const unsigned*>(planes + at);
      u1[k] = *reinterpret_cast<const unsigned*>(planes + plane_stride + at);
      if (dA != nullptr) d[k] = *reinterpret_cast<const f32x2*>(dA + col * ldd + ch);
      else { const float dl = dlogit[col]; d[k] = f32x2{dl * wh0, dl * wh1}; }
    }
    if (dA != nullptr)
      for (int s = 1; s < S; ++s) {
        const float* Ds = dA + (size_t)s * split_stride;
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) {
          const int rl = rgx + RG * (i0 + k);
          d[k] += *reinterpret_cast<const f32x2*>(Ds + (col0 + (rl < N ? rl : 0)) * ldd + ch);
        }
      }
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) {
      const bool live = rg + RG * (i0 + k) < N;
      const float a0 = bf16_lo(u0[k]) + bf16_lo(u1[k]), a1 = bf16_hi(u0[k]) + bf16_hi(u1[k]);
      const float z0 = (a0 > 0.f) ? a0 : a0 * islope, z1 = (a1 > 0.f) ? a1 : a1 * islope;
      const float e0 = live ? ((a0 > 0.f) ? d[k][0] : d[k][0] * slope) : 0.f, e1 = live ? ((a1 > 0.f) ? d[k][1] : d[k][1] * slope) : 0.f;
      dz[i0 + k] = f32x2{e0, e1};
      const float x0 = (z0 - b0) * ig0, x1 = (z1 - b1) * ig1;
      if constexpr (kKeepX) xh[i0 + k] = f32x2{x0, x1};
      s[0] += e0; s[1] += e1;
      s[2] = fmaf(e0, x0, s[2]); s[3] = fmaf(e1, x1, s[3]);
    }
    __builtin_amdgcn_sched_barrier(0);  // one chunk's raw words at a time
  }
  rg_all_sum<4, CP>(red, s);
  if (rg == 0) {
    dbeta_part[(size_t)pair * C + ch] = s[0]; dbeta_part[(size_t)pair * C + ch + 1] = s[1];
    dgamma_part[(size_t)pair * C + ch] = s[2]; dgamma_part[(size_t)pair * C + ch + 1] = s[3];
  }
  const float inv_n = 1.0f / (float)N;
  const float k0 = rstd[(size_t)pair * C + ch] * g0, k1 = rstd[(size_t)pair * C + ch + 1] * g1;
  const float m10 = s[0] * inv_n, m11 = s[1] * inv_n, m20 = s[2] * inv_n, m21 = s[3] * inv_n;
#pragma unroll
  for (int i0 = 0; i0 < RPT; i0 += CHUNK) {
    f32x2 x[CHUNK];
    int rgx = rg;
    asm volatile("" : "+v"(rgx));
    if constexpr (kKeepX) {
#pragma unroll
      for (int k = 0; k < CHUNK; ++k) x[k] = xh[i0 + k];
    } else {
      unsigned u0[CHUNK], u1[CHUNK];
#pragma unroll
      for (int k = 0; k < CHUNK; ++k) {
        const int rl = rgx + RG * (i0 + k);
        const size_t at = kb_index(col0 + (rl < N ? rl : 0), ch, ncols);
        u0[k] = *reinterpret_cast<const unsigned*>(planes + at);
        u1[k] = *reinterpret_cast<const unsigned*>(planes + plane_stride + at);
      }
#pragma unroll
      for (int k = 0; k < CHUNK; ++k) {
        const float a0 = bf16_lo(u0[k]) + bf16_lo(u1[k]), a1 = bf16_hi(u0[k]) + bf16_hi(u1[k]);
        const float z0 = (a0 > 0.f) ? a0 : a0 * islope, z1 = (a1 > 0.f) ? a1 : a1 * islope;
        x[k] = f32x2{(z0 - b0) * ig0, (z1 - b1) * ig1};
      }
    }
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) {
      const int rl = rgx + RG * (i0 + k);
      if (rl < N) {
        unsigned p0, p1;
        split2(k0 * (dz[i0 + k][0] - m10 - x[k][0] * m20), k1 * (dz[i0 + k][1] - m11 - x[k][1] * m21), p0, p1);
        const size_t at = kb_index(col0 + rl, ch, ncols);
        *reinterpret_cast<unsigned*>(dYp + at) = p0;
        *reinterpret_cast<unsigned*>(dYp + dy_plane + at) = p1;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- head: logits[col] = sum_c w[c] a[col][c] + b (Conv1d(256 -> 1)); one 16-lane row per column ----------------------------
__global__ void __launch_bounds__(256)
est_head_fwd_kernel(const bf16_t* __restrict__ planes, size_t plane_stride, int C, int ncols, const float* __restrict__ w,
                    const float* __restrict__ bias, float* __restrict__ logits) {
  const int col = (int)blockIdx.x * 16 + (int)(threadIdx.x >> 4), l = threadIdx.x & 15;
  const int cc = (col < ncols) ? col : ncols - 1;
  float s = 0.f;
  for (int ch = 2 * l; ch < C; ch += 32) {
    const size_t at = kb_index((size_t)cc, ch, (size_t)ncols);
    const unsigned u0 = *reinterpret_cast<const unsigned*>(planes + at);
    const unsigned u1 = *reinterpret_cast<const unsigned*>(planes + plane_stride + at);
    s = fmaf(f16_lo(u0) + f16_lo(u1), w[ch], s);  // the forward's two fp16 planes
    s = fmaf(f16_hi(u0) + f16_hi(u1), w[ch + 1], s);
  }
  s = row16_sum(s);
  if (l == 0 && col < ncols) logits[col] = s + (bias ? bias[0] : 0.f);
}
// d w_head partials: part[block][c] = sum over the block's columns of dlogit[col] a[col][c].  Thread = (channel pair, one of
// eight column groups): the 16 channel pairs of a K block read one contiguous 64-byte row per column.
__global__ void __launch_bounds__(256)
est_head_dw_kernel(const bf16_t* __restrict__ planes, size_t plane_stride, int C, int ncols, int cols_per_block,
                   const float* __restrict__ dlogit, float* __restrict__ part, float* __restrict__ bias_part) {
  __shared__ float red[8][64];
  __shared__ float redb[8];
  float sd = 0.f;  // bias_part[block] = sum of dlogit over the block's columns (the head bias gradient's partials; round 6: was a launch of its own)
  const int c0 = (int)blockIdx.x * cols_per_block;
  int c1 = c0 + cols_per_block;
  c1 = (c1 < ncols) ? c1 : ncols;
  const int cp = threadIdx.x & 31, cg = threadIdx.x >> 5;
  for (int cb = 0; cb < C; cb += 64) {
    const int ch = cb + 2 * cp;
    float s0 = 0.f, s1 = 0.f;
    if (ch < C) {
      // two leading planes (a to 2^-17: a gradient), four columns in flight per thread
      int col = c0 + cg;
      for (; col + 24 < c1; col += 32) {
        unsigned u0[4], u1[4];
        float d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const size_t at = kb_index((size_t)(col + 8 * u), ch, (size_t)ncols);
          u0[u] = *reinterpret_cast<const unsigned*>(planes + at);
          u1[u] = *reinterpret_cast<const unsigned*>(planes + plane_stride + at);
          d[u] = dlogit[col + 8 * u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          s0 = fmaf(bf16_lo(u0[u]) + bf16_lo(u1[u]), d[u], s0);
          s1 = fmaf(bf16_hi(u0[u]) + bf16_hi(u1[u]), d[u], s1);
        }
        if (cb == 0) sd += (d[0] + d[1]) + (d[2] + d[3]);
      }
      for (; col < c1; col += 8) {
        const size_t at = kb_index((size_t)col, ch, (size_t)ncols);
        const unsigned u0 = *reinterpret_cast<const unsigned*>(planes + at);
        const unsigned u1 = *reinterpret_cast<const unsigned*>(planes + plane_stride + at);
        const float d = dlogit[col];
        s0 = fmaf(bf16_lo(u0) + bf16_lo(u1), d, s0);
        s1 = fmaf(bf16_hi(u0) + bf16_hi(u1), d, s1);
        if (cb == 0) sd += d;
      }
    }
    red[cg][2 * cp] = s0; red[cg][2 * cp + 1] = s1;
    if (cb == 0 && cp == 0) redb[cg] = sd;  // (C >= 32: channel pair 0 exists and saw every column of its group)
    __syncthreads();
    if (cb == 0 && bias_part != nullptr && threadIdx.x == 0)
      bias_part[blockIdx.x] = ((redb[0] + redb[1]) + (redb[2] + redb[3])) + ((redb[4] + redb[5]) + (redb[6] + redb[7]));
    if (threadIdx.x < 64 && cb + (int)threadIdx.x < C) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) t += red[q][threadIdx.x];
      part[(size_t)blockIdx.x * C + cb + threadIdx.x] = t;
    }
    __syncthreads();
  }
}

// ---- d gamma of a channel whose gamma is EXACTLY zero (ADVICE r3 / VERDICT r4 7d) ---------------------------------------------------
// The adjoints above recover x^ from the stored activation as (z - beta) / gamma.  With gamma = 0 the activation is the constant
// lrelu(beta) and x^ is gone: they take it as 0, which leaves d beta and dY right (dY = 0 there anyway) and d gamma = sum dz x^ wrong.
// This kernel -- one workgroup per channel, leaving at once unless |gamma| < 1e-30, i.e. a handful of idle workgroups in any trained
// network -- recomputes that channel's pre-normalisation product y = W[ch] . x from the layer's INPUT planes and fp32 weights, forms
// x^ = (y - mean) rstd per pair and overwrites the channel's per-pair d gamma.  Slow (a serial GEMV per pair) and rare by construction.
struct ZeroFix {  // one layer's arguments
  const float* dA; const float* dlogit; const float* w_head;
  const bf16_t* out_planes; size_t out_stride;
  const bf16_t* in_planes; size_t in_stride;
  const float* W; int ldw, Ci;
  const float* rstd; const float* gamma;
  int C;
  float* dgamma_part;
  const bf16_t* dYn; size_t dyn_stride; const float* Wn; int ldwn, Cn;
};
struct ZeroFixTab { int n; float slope; int N; long n_pairs; ZeroFix L[kTabMax]; };
// grid (max C, layers): a launch covers every layer of a backward when their dY are still alive (few columns), one layer otherwise
__global__ void __launch_bounds__(256) est_dgamma_zero_kernel(const ZeroFixTab T) {
  const ZeroFix& A = T.L[blockIdx.y];
  const int ch = (int)blockIdx.x;
  if (ch >= A.C || fabsf(A.gamma[ch]) > 1e-30f) return;
  const float slope = T.slope;
  const int N = T.N, C = A.C, Ci = A.Ci;
  const long n_pairs = T.n_pairs;
  __shared__ float y[kFixMaxN];
  __shared__ float red[4];
  const int t = (int)threadIdx.x;
  const size_t ncols = (size_t)n_pairs * N;
  auto plane2 = [&](const bf16_t* P, size_t stride, size_t at) {  // the backward's two bf16 planes (2^-17: a gradient)
    return __uint_as_float((unsigned)P[at] << 16) + __uint_as_float((unsigned)P[stride + at] << 16);
  };
  auto block_sum = [&](float v) {
    v = wave_sum(v);
    __syncthreads();
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
  };
  for (long pair = 0; pair < n_pairs; ++pair) {
    const size_t col0 = (size_t)pair * N;
    float s = 0.f;
    for (int r = t; r < N; r += 256) {
      float acc = 0.f;
      for (int k = 0; k < Ci; ++k) acc = fmaf(A.W[(size_t)ch * A.ldw + k], plane2(A.in_planes, A.in_stride, kb_index(col0 + r, k, ncols)), acc);
      y[r] = acc;
      s += acc;
    }
    const float mean = block_sum(s) / (float)N;
    const float rs = A.rstd[(size_t)pair * C + ch];
    float g = 0.f;
    for (int r = t; r < N; r += 256) {
      const size_t col = col0 + r;
      const size_t at = kb_index(col, ch, ncols);
      const float a = __uint_as_float((unsigned)A.out_planes[at] << 16) + __uint_as_float((unsigned)A.out_planes[A.out_stride + at] << 16);
      float d;
      if (A.dA != nullptr) d = A.dA[col * C + ch];
      else if (A.dlogit != nullptr) d = A.dlogit[col] * A.w_head[ch];
      else {  // the fused data gradient never wrote dA: this channel's column of dY_next W_next again (Cn terms per point)
        d = 0.f;
        for (int k = 0; k < A.Cn; ++k) d = fmaf(plane2(A.dYn, A.dyn_stride, kb_index(col, k, ncols)), A.Wn[(size_t)k * A.ldwn + ch], d);
      }
      const float dz = (a > 0.f) ? d : d * slope;
      g = fmaf(dz, (y[r] - mean) * rs, g);
    }
    const float G = block_sum(g);
    if (t == 0) A.dgamma_part[(size_t)pair * C + ch] = G;
  }
}

}  // namespace

static int zero_fix_fill(ZeroFix& Z, const float* dA, const float* dlogit, const float* w_head, const void* out_planes, size_t out_plane,
                         const void* in_planes, size_t in_plane, const float* W, int ldw, int Ci, const float* rstd, const float* gamma, int C,
                         float* dgamma_part, const void* dY_next, size_t dyn_plane, const float* W_next, int ldw_next, int C_next) {
  const bool from_next = dY_next && W_next && C_next > 0 && ldw_next >= C;
  if ((!dA && !(dlogit && w_head) && !from_next) || !out_planes || !in_planes || !W || !rstd || !gamma || !dgamma_part) return DFEPE_ERR_INVALID_ARG;
  if (C <= 0 || Ci <= 0 || ldw < Ci) return DFEPE_ERR_INVALID_ARG;
  Z.dA = dA; Z.dlogit = dlogit; Z.w_head = w_head; Z.out_planes = static_cast<const bf16_t*>(out_planes); Z.out_stride = out_plane;
  Z.in_planes = static_cast<const bf16_t*>(in_planes); Z.in_stride = in_plane; Z.W = W; Z.ldw = ldw; Z.Ci = Ci; Z.rstd = rstd; Z.gamma = gamma;
  Z.C = C; Z.dgamma_part = dgamma_part; Z.dYn = static_cast<const bf16_t*>(dY_next); Z.dyn_stride = dyn_plane; Z.Wn = W_next; Z.ldwn = ldw_next;
  Z.Cn = C_next;
  return DFEPE_OK;
}

extern "C" int dfepe_est_dgamma_zero(const float* dA, const float* dlogit, const float* w_head, const void* out_planes, size_t out_plane,
                                     const void* in_planes, size_t in_plane, const float* W, int ldw, int Ci, const float* rstd,
                                     const float* gamma, float slope, int C, int N, long n_pairs, float* dgamma_part,
                                     const void* dY_next, size_t dyn_plane, const float* W_next, int ldw_next, int C_next, void* stream) {
  if (N <= 0 || N > kFixMaxN || n_pairs < 0 || !(slope > 0.f)) return DFEPE_ERR_INVALID_ARG;
  ZeroFixTab T{};
  T.n = 1; T.slope = slope; T.N = N; T.n_pairs = n_pairs;
  const int rc = zero_fix_fill(T.L[0], dA, dlogit, w_head, out_planes, out_plane, in_planes, in_plane, W, ldw, Ci, rstd, gamma, C, dgamma_part,
                               dY_next, dyn_plane, W_next, ldw_next, C_next);
  if (rc != DFEPE_OK) return rc;
  if (n_pairs == 0) return DFEPE_OK;
  hipLaunchKernelGGL(est_dgamma_zero_kernel, dim3(C, 1), dim3(256), 0, static_cast<hipStream_t>(stream), T);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

// the same for n_layers <= 8 layers in one launch (arrays indexed by layer; ldw = Ci, ldw_next = C): what a backward over few columns
// does, where keeping every layer's dY alive to the end costs nothing
extern "C" int dfepe_est_dgamma_zero_multi(int n_layers, const float* const* dA, const float* const* dlogit, const float* const* w_head,
                                           const void* const* out_planes, const size_t* out_plane, const void* const* in_planes,
                                           const size_t* in_plane, const float* const* W, const int* Ci, const float* const* rstd,
                                           const float* const* gamma, const int* C, float* const* dgamma_part, const void* const* dY_next,
                                           const size_t* dyn_plane, const float* const* W_next, const int* C_next, float slope, int N,
                                           long n_pairs, void* stream) {
  if (n_layers <= 0 || n_layers > kTabMax || N <= 0 || N > kFixMaxN || n_pairs < 0 || !(slope > 0.f)) return DFEPE_ERR_INVALID_ARG;
  if (!dA || !dlogit || !w_head || !out_planes || !out_plane || !in_planes || !in_plane || !W || !Ci || !rstd || !gamma || !C || !dgamma_part ||
      !dY_next || !dyn_plane || !W_next || !C_next)
    return DFEPE_ERR_INVALID_ARG;
  ZeroFixTab T{};
  T.n = n_layers; T.slope = slope; T.N = N; T.n_pairs = n_pairs;
  int cmax = 0;
  for (int l = 0; l < n_layers; ++l) {
    const int rc = zero_fix_fill(T.L[l], dA[l], dlogit[l], w_head[l], out_planes[l], out_plane[l], in_planes[l], in_plane[l], W[l], Ci[l], Ci[l],
                                 rstd[l], gamma[l], C[l], dgamma_part[l], dY_next[l], dyn_plane[l], W_next[l], C[l], C_next[l]);
    if (rc != DFEPE_OK) return rc;
    cmax = C[l] > cmax ? C[l] : cmax;
  }
  if (n_pairs == 0) return DFEPE_OK;
  hipLaunchKernelGGL(est_dgamma_zero_kernel, dim3(cmax, n_layers), dim3(256), 0, static_cast<hipStream_t>(stream), T);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

extern "C" int dfepe_est_in_bwd(const float* dA, const float* dlogit, const float* w_head, const void* planes, size_t plane_stride,
                                const float* rstd, const float* gamma, const float* beta, float slope, int C, int ncols, void* dY,
                                size_t dy_plane, float* dgamma_part, float* dbeta_part, void* stream) {
  if ((!dA && !(dlogit && w_head)) || !planes || !rstd || !gamma || !beta || !dY || !dgamma_part || !dbeta_part) return DFEPE_ERR_INVALID_ARG;
  if (C <= 0 || (C & 31) || ncols <= 0 || (ncols % kPts) || !(slope > 0.f)) return DFEPE_ERR_INVALID_ARG;
  const dim3 grid(ncols / kPts, (C + 63) / 64), block(256);
  hipLaunchKernelGGL(est_in_bwd_kernel, grid, block, 0, static_cast<hipStream_t>(stream), dA, dlogit, w_head,
                     static_cast<const bf16_t*>(planes), plane_stride, rstd, gamma, beta, slope, C, ncols, static_cast<bf16_t*>(dY), dy_plane,
                     dgamma_part, dbeta_part);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

// InstanceNorm + LeakyReLU + split of a plain product, N points per pair (any N >= 1): Y fp32 [n_pairs * N][ldy].  splits = 1:
// one launch, a workgroup per (pair, 64 channels); splits = 2..64 (few pairs): the pair's rows over `splits` workgroups, two
// launches, part = workspace of n_pairs * splits * 2 * C floats.
extern "C" int dfepe_est_norm_fwd(const float* Y, int ldy, int C, long n_pairs, int N, const float* gamma, const float* beta, float eps,
                                  float slope, void* planes_out, size_t out_plane, void* planes_bwd, size_t bwd_plane, float* rstd,
                                  int splits, float* part, void* stream) {
  if (!Y || !gamma || !beta || !planes_out || !rstd || C <= 0 || (C & 31) || ldy < C || (ldy & 1) || n_pairs < 0 || N <= 0)
    return DFEPE_ERR_INVALID_ARG;
  if (splits < 1 || splits > 64 || (splits > 1 && !part)) return DFEPE_ERR_INVALID_ARG;
  if (!(slope > 0.f)) return DFEPE_ERR_UNSUPPORTED;  // the backward inverts the activation
  if (n_pairs == 0) return DFEPE_OK;
  if (n_pairs > 0x7fffffffL) return DFEPE_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)n_pairs, (C + 63) / 64, splits), block(kRG * 32);
  const size_t ncols = (size_t)n_pairs * N;
  bf16_t* P = static_cast<bf16_t*>(planes_out);
  bf16_t* Q = static_cast<bf16_t*>(planes_bwd);
  if (splits == 1) {
    hipLaunchKernelGGL(est_norm_fwd_n_kernel<0>, grid, block, 0, st, Y, ldy, C, N, ncols, gamma, beta, eps, slope, P, out_plane, Q, bwd_plane, rstd, part);
  } else {
    hipLaunchKernelGGL(est_norm_fwd_n_kernel<1>, grid, block, 0, st, Y, ldy, C, N, ncols, gamma, beta, eps, slope, P, out_plane, Q, bwd_plane, rstd, part);
    hipLaunchKernelGGL(est_norm_fwd_n_kernel<2>, grid, block, 0, st, Y, ldy, C, N, ncols, gamma, beta, eps, slope, P, out_plane, Q, bwd_plane, rstd, part);
  }
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

// dfepe_est_in_bwd for N points per pair (any N >= 1; ncols = n_pairs * N); splits / part as in dfepe_est_norm_fwd
extern "C" int dfepe_est_in_bwd_n(const float* dA, const float* dlogit, const float* w_head, const void* planes, size_t plane_stride,
                                  const float* rstd, const float* gamma, const float* beta, float slope, int C, long n_pairs, int N, void* dY,
                                  size_t dy_plane, float* dgamma_part, float* dbeta_part, int splits, float* part, void* stream) {
  if ((!dA && !(dlogit && w_head)) || !planes || !rstd || !gamma || !beta || !dY || !dgamma_part || !dbeta_part) return DFEPE_ERR_INVALID_ARG;
  if (C <= 0 || (C & 31) || n_pairs < 0 || N <= 0 || !(slope > 0.f)) return DFEPE_ERR_INVALID_ARG;
  if (splits < 1 || splits > 64 || (splits > 1 && !part)) return DFEPE_ERR_INVALID_ARG;
  if (n_pairs == 0) return DFEPE_OK;
  if (n_pairs > 0x7fffffffL) return DFEPE_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)n_pairs, (C + 63) / 64, splits), block(kRG * 32);
  const size_t ncols = (size_t)n_pairs * N;
  const bf16_t* P = static_cast<const bf16_t*>(planes);
  bf16_t* D = static_cast<bf16_t*>(dY);
  if (splits == 1) {
    hipLaunchKernelGGL(est_in_bwd_n_kernel<0>, grid, block, 0, st, dA, dlogit, w_head, P, plane_stride, rstd, gamma, beta, slope, C, N, ncols, D,
                       dy_plane, dgamma_part, dbeta_part, part);
  } else {
    hipLaunchKernelGGL(est_in_bwd_n_kernel<1>, grid, block, 0, st, dA, dlogit, w_head, P, plane_stride, rstd, gamma, beta, slope, C, N, ncols, D,
                       dy_plane, dgamma_part, dbeta_part, part);
    hipLaunchKernelGGL(est_in_bwd_n_kernel<2>, grid, block, 0, st, dA, dlogit, w_head, P, plane_stride, rstd, gamma, beta, slope, C, N, ncols, D,
                       dy_plane, dgamma_part, dbeta_part, part);
  }
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

// round 6: InstanceNorm + LeakyReLU + split of a plain product held in registers (N <= 2048), the product given as `splits` partials
// Y[z][n_pairs * N][ldy] (split_stride floats apart; splits = 1: the plain product).  One launch, one read of Y.
extern "C" int dfepe_est_norm_fwd_r(const float* Y, int ldy, int splits, size_t split_stride, int C, long n_pairs, int N, const float* gamma,
                                    const float* beta, float eps, float slope, void* planes_out, size_t out_plane, void* planes_bwd,
                                    size_t bwd_plane, float* rstd, void* stream) {
  if (!Y || !gamma || !beta || !planes_out || !rstd || C <= 0 || (C & 31) || ldy < C || (ldy & 1) || n_pairs < 0 || N <= 0 || N > 2048)
    return DFEPE_ERR_INVALID_ARG;
  if (splits < 1 || splits > 64) return DFEPE_ERR_INVALID_ARG;
  if (!(slope > 0.f)) return DFEPE_ERR_UNSUPPORTED;
  if (n_pairs == 0) return DFEPE_OK;
  if (n_pairs > 0x7fffffffL) return DFEPE_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)n_pairs, N <= 1024 ? C / 32 : C / 16), block(1024);
  const size_t ncols = (size_t)n_pairs * N;
  bf16_t* P = static_cast<bf16_t*>(planes_out);
  bf16_t* Q = static_cast<bf16_t*>(planes_bwd);
#define DFEPE_NORM_R(R, CP) hipLaunchKernelGGL((est_norm_fwd_r_kernel<R, CP>), grid, block, 0, st, Y, ldy, split_stride, splits, C, N, ncols, gamma, beta, eps, slope, P, out_plane, Q, bwd_plane, rstd)
  if (N <= 128) DFEPE_NORM_R(2, 16);
  else if (N <= 512) DFEPE_NORM_R(8, 16);
  else if (N <= 1024) DFEPE_NORM_R(16, 16);
  else DFEPE_NORM_R(16, 8);
#undef DFEPE_NORM_R
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
// ... and its adjoint: dA given as `splits` partials [z][n_pairs * N][ldd] (or the head's rank-one form: dA null)
extern "C" int dfepe_est_in_bwd_r(const float* dA, int ldd, int splits, size_t split_stride, const float* dlogit, const float* w_head,
                                  const void* planes, size_t plane_stride, const float* rstd, const float* gamma, const float* beta,
                                  float slope, int C, long n_pairs, int N, void* dY, size_t dy_plane, float* dgamma_part, float* dbeta_part,
                                  void* stream) {
  if ((!dA && !(dlogit && w_head)) || !planes || !rstd || !gamma || !beta || !dY || !dgamma_part || !dbeta_part) return DFEPE_ERR_INVALID_ARG;
  if (C <= 0 || (C & 31) || n_pairs < 0 || N <= 0 || N > 2048 || !(slope > 0.f)) return DFEPE_ERR_INVALID_ARG;
  if (dA && (ldd < C || (ldd & 1) || splits < 1 || splits > 64)) return DFEPE_ERR_INVALID_ARG;
  if (n_pairs == 0) return DFEPE_OK;
  if (n_pairs > 0x7fffffffL) return DFEPE_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)n_pairs, N <= 1024 ? C / 32 : C / 16), block(1024);
  const size_t ncols = (size_t)n_pairs * N;
  const bf16_t* P = static_cast<const bf16_t*>(planes);
  bf16_t* D = static_cast<bf16_t*>(dY);
#define DFEPE_INBWD_R(R, CP) hipLaunchKernelGGL((est_in_bwd_r_kernel<R, CP>), grid, block, 0, st, dA, ldd, split_stride, splits, dlogit, w_head, P, plane_stride, rstd, gamma, beta, slope, C, N, ncols, D, dy_plane, dgamma_part, dbeta_part)
  if (N <= 128) DFEPE_INBWD_R(2, 16);
  else if (N <= 512) DFEPE_INBWD_R(8, 16);
  else if (N <= 1024) DFEPE_INBWD_R(16, 16);
  else DFEPE_INBWD_R(16, 8);
#undef DFEPE_INBWD_R
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

extern "C" int dfepe_est_head_fwd(const void* planes, size_t plane_stride, int C, int ncols, const float* w, const float* bias,
                                  float* logits, void* stream) {
  if (!planes || !w || !logits || C <= 0 || (C & 31) || ncols <= 0) return DFEPE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(est_head_fwd_kernel, dim3((ncols + 15) / 16), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(planes), plane_stride, C, ncols, w, bias, logits);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

extern "C" int dfepe_est_head_dw(const void* planes, size_t plane_stride, int C, int ncols, int blocks, const float* dlogit, float* part,
                                 float* bias_part, void* stream) {
  if (!planes || !dlogit || !part || C <= 0 || (C & 31) || ncols <= 0 || blocks <= 0) return DFEPE_ERR_INVALID_ARG;
  const int cpb = (ncols + blocks - 1) / blocks;
  hipLaunchKernelGGL(est_head_dw_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(planes),
                     plane_stride, C, ncols, cpb, dlogit, part, bias_part);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
