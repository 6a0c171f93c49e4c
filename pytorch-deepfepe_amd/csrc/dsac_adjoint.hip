// dfepe_dsac_bwd -- the adjoint of the DSAC hypothesis loop (csrc/dsac.hip): gradients of E_sample, score, E_refit, loss, quality
// and exp_loss to the pixel points, in eight launches whatever B and H are (seven with H = 1).  The per-lane arithmetic is csrc/dsac_adjoint_math.h, the
// contract include/dfepe.h.
//
//   1    dsac_bwd_prep_kernel       the K^-1 points [B,N,2] x 2 and the gathered samples [B H,S,2] x 2 (the 8-byte layout the fit
//                                   adjoint reads), the refit's weights sqrt(soft) [H,B,N], E_refit as [H,B,9], and in fp64
//                                   F_h = K^-T E_sample K^-1 and M_h (E_refit, or K^-T E_refit K^-1 with loss_kind 2)
//   2    dsac_bwd_head_kernel       t_loss, t_score [B,H]: a wavefront per pair
//   3    dsac_bwd_hyp_kernel<true>  t_E_refit [B,H,9] and [H,B,9]: a wavefront per hypothesis, launch 5 of the forward
//   4-5  dfepe_eight_point_bwd      the refits' adjoint: H weight sets of the B pairs -> t_w [H,B,N], the K^-1 point gradients
//   6    dsac_bwd_hyp_kernel<false> t_E_sample [B,H,9]: launch 3 of the forward
//   7    dfepe_eight_point_bwd      the sample fits' adjoint: B H problems of S points
//   8    dsac_bwd_points_kernel     g_X, g_Y: one lane per correspondence and quarter of the hypotheses
//
// Launches 3 and 6: a lane walks the correspondences lane, lane + 64, ... and adds its nine matrix entries in that order; the 64
// partial sums of each entry are added by wave_sum, the forward's fixed tree.
// Launch 8: a workgroup of 256 lanes owns da::kPointLanes = 64 consecutive correspondences of one pair; wavefront v adds, for its
// correspondence, the hypotheses [v Hq, (v + 1) Hq), Hq = ceil(H / 4), in ascending order: per hypothesis first the sample-fit
// gradient of every slot j (ascending) that names the correspondence, then the score's pixel term, then the loss's.  The four
// partial sums go through LDS and wavefront 0 adds them in wavefront order: the K^-1 gradient is ((((refit + P0) + P1) + P2) + P3),
// the pixel terms ((D0 + D1) + D2) + D3, and the output is the K^-1 gradient through the Jacobian of _de_homo(K^-1 .) plus D.
// The index list of a hypothesis is the same for every lane of a wavefront, so it is read through the scalar cache; no tile is
// staged in LDS as the vote does, because here the wavefronts of a workgroup walk different hypotheses.
// No atomics, no allocation, no host synchronisation: a pair's gradients are the same bits on every run and in every batch.
#include "dfepe_common.h"

#include "dsac_adjoint_math.h"

namespace {

constexpr int kThreads = 256;
constexpr unsigned kFitFlags = DFEPE_W8PT_SQRT2 | DFEPE_W8PT_NO_ROWNORM | DFEPE_W8PT_FORCE_110;
constexpr long long kMaxCells = 2147483647LL;  // B * H * N
static_assert(kThreads / WAVE == ds::kHypsPerBlock && WAVE == ds::kLanes, "launch shapes of dsac_adjoint.hip");
static_assert(da::kPointLanes == WAVE && da::kPointWaves * WAVE == kThreads, "launch shape of the points kernel");

inline size_t round4(size_t floats) { return (floats + 3) & ~(size_t)3; }  // every section starts 16-byte aligned

struct Workspace {  // offsets in floats
  size_t pn1, pn2, g1, g2, wts, E_hb, tE_hb, t_score, t_loss, t_E_refit, t_w, t_E_sample, gpn1, gpn2, gg1, gg2, Fd, Md, fit, total;
};
inline Workspace layout(int B, int N, int H, int S) {
  const size_t bn = (size_t)B * N, bh = (size_t)B * H;
  Workspace w;
  size_t o = 0;
  w.pn1 = o; o += round4(bn * 2);
  w.pn2 = o; o += round4(bn * 2);
  w.g1 = o; o += round4(bh * S * 2);
  w.g2 = o; o += round4(bh * S * 2);
  w.wts = o; o += round4(bh * N);
  w.E_hb = o; o += round4(bh * 9);
  w.tE_hb = o; o += round4(bh * 9);
  w.t_score = o; o += round4(bh);
  w.t_loss = o; o += round4(bh);
  w.t_E_refit = o; o += round4(bh * 9);
  w.t_w = o; o += round4(bh * N);
  w.t_E_sample = o; o += round4(bh * 9);
  w.gpn1 = o; o += round4(bn * 2);
  w.gpn2 = o; o += round4(bn * 2);
  w.gg1 = o; o += round4(bh * S * 2);
  w.gg2 = o; o += round4(bh * S * 2);
  w.Fd = o; o += round4(bh * 18);   // fp64
  w.Md = o; o += round4(bh * 18);   // fp64
  w.fit = o; o += round4(dfepe_eight_point_bwd_workspace_bytes(B, N, H) / sizeof(float));
  w.total = o;
  return w;
}

__device__ __forceinline__ void load9(const float* __restrict__ p, double* m) {
#pragma unroll
  for (int c = 0; c < 9; ++c) m[c] = (double)p[c];
}
__device__ __forceinline__ void load9(const double* __restrict__ p, double* m) {
#pragma unroll
  for (int c = 0; c < 9; ++c) m[c] = p[c];
}
__device__ __forceinline__ void pair_Ki(const float* __restrict__ K, size_t b, double* Ki) {
  double Km[9];
  load9(K + b * 9, Km);
  ds::inv3(Km, Ki);
}

struct PrepArgs {
  const float2 *X, *Y;
  const float *K, *soft, *E_sample, *E_refit;
  const int* idx;
  float2 *pn1, *pn2, *g1, *g2;
  float *wts, *E_hb;
  double *Fd, *Md;
  int B, N, H, S, loss_kind;
};

// t runs over four ranges: the B N correspondences, the B H S sample slots, the B H N weights, the B H hypotheses.
__global__ void __launch_bounds__(kThreads) dsac_bwd_prep_kernel(PrepArgs p) {
  size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t bn = (size_t)p.B * p.N, bh = (size_t)p.B * p.H, slots = bh * p.S, cells = bh * p.N;
  double Ki[9];
  float o[2];
  if (t < bn) {
    pair_Ki(p.K, t / p.N, Ki);
    const float2 x = p.X[t], y = p.Y[t];
    ds::normalized_point(Ki, (double)x.x, (double)x.y, o);
    p.pn1[t] = make_float2(o[0], o[1]);
    ds::normalized_point(Ki, (double)y.x, (double)y.y, o);
    p.pn2[t] = make_float2(o[0], o[1]);
    return;
  }
  t -= bn;
  if (t < slots) {
    const size_t b = t / ((size_t)p.H * p.S);
    int n = p.idx[t];
    n = n < 0 ? 0 : (n >= p.N ? p.N - 1 : n);  // as the forward's gather: an index outside is never followed out of the pair
    pair_Ki(p.K, b, Ki);
    const float2 x = p.X[b * p.N + n], y = p.Y[b * p.N + n];
    ds::normalized_point(Ki, (double)x.x, (double)x.y, o);
    p.g1[t] = make_float2(o[0], o[1]);
    ds::normalized_point(Ki, (double)y.x, (double)y.y, o);
    p.g2[t] = make_float2(o[0], o[1]);
    return;
  }
  t -= slots;
  if (t < cells) {
    const size_t q = t / p.N, n = t % p.N, b = q / p.H, h = q % p.H;
    p.wts[(h * p.B + b) * p.N + n] = ds::refit_weight(p.soft[t]);
    return;
  }
  t -= cells;
  if (t >= bh) return;
  const size_t b = t / p.H, h = t % p.H, hb = h * p.B + b;
  double E[9], M[9];
  pair_Ki(p.K, b, Ki);
  load9(p.E_sample + t * 9, E);
  ds::e_to_f(Ki, E, M);
#pragma unroll
  for (int c = 0; c < 9; ++c) p.Fd[t * 9 + c] = M[c];
  load9(p.E_refit + t * 9, E);
#pragma unroll
  for (int c = 0; c < 9; ++c) p.E_hb[hb * 9 + c] = (float)E[c];
  if (p.loss_kind == 2) ds::e_to_f(Ki, E, M);
#pragma unroll
  for (int c = 0; c < 9; ++c) p.Md[t * 9 + c] = (p.loss_kind == 2) ? M[c] : E[c];
}

struct HeadArgs {
  const int* idx;
  const float *score, *loss, *counts, *g_score, *g_loss, *g_quality, *g_exp_loss;
  float alpha;
  float *t_score, *t_loss;
  int N, H, S;
};

// One wavefront per pair.  p and Lbar as the vote forms them: max-subtracted, lane l adds h = l, l + 64, ..., wave_sum.
__global__ void __launch_bounds__(WAVE) dsac_bwd_head_kernel(HeadArgs p) {
  const size_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const float* __restrict__ score = p.score + b * p.H;
  const float* __restrict__ loss = p.loss + b * p.H;
  const double alpha = (double)p.alpha;
  double m = 0.0, Z = 1.0, Lbar = 0.0, ge = 0.0;
  if (p.g_exp_loss != nullptr) {
    ge = (double)p.g_exp_loss[b];
    m = -INFINITY;
    for (int h = lane; h < p.H; h += WAVE) m = fmax(m, alpha * (double)score[h]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    double z = 0.0, num = 0.0;
    for (int h = lane; h < p.H; h += WAVE) {
      const double e = exp(alpha * (double)score[h] - m);
      z += e;
      num += e * (double)loss[h];
    }
    Z = wave_sum(z);
    Lbar = wave_sum(num) / Z;
  }
  for (int h = lane; h < p.H; h += WAVE) {
    const size_t bh = b * p.H + h;
    double tl = p.g_loss != nullptr ? (double)p.g_loss[bh] : 0.0;
    double ts = p.g_score != nullptr ? (double)p.g_score[bh] : 0.0;
    if (p.g_exp_loss != nullptr) {
      const double ph = exp(alpha * (double)score[h] - m) / Z;
      tl = da::head_loss(tl, ge, ph);
      ts = ts + da::head_score_exp(ge, alpha, ph, (double)loss[h], Lbar);
    }
    if (p.g_quality != nullptr) {
      for (int j = 0; j < p.S; ++j) {  // slot order
        const int n = p.idx[bh * p.S + j];
        if (n >= 0 && n < p.N) ts = ts + da::head_vote((double)p.g_quality[b * p.N + n], (double)p.counts[b * p.N + n]);
      }
    }
    p.t_loss[bh] = (float)tl;
    p.t_score[bh] = (float)ts;
  }
}

struct HypArgs {
  const float2 *X, *Y;
  const float *K, *g_E;       // g_E: the upstream on E_refit (loss) or E_sample (score), [B,H,9] or NULL
  const double* Md;           // M_h (loss) or F_h (score), [B,H,9]
  const float *t_head;        // t_loss or t_score [B,H]
  const float *soft, *wts, *t_w;  // score only: [B,H,N], [H,B,N], [H,B,N]
  float beta;
  int loss_kind;
  float *t_E, *t_E_hb;        // [B,H,9]; loss only: also [H,B,9]
  int B, N, H;
};

// LOSS true: launch 3 (t_E_refit).  LOSS false: launch 6 (t_E_sample).
template <bool LOSS>
__global__ void __launch_bounds__(kThreads) dsac_bwd_hyp_kernel(HypArgs p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned tiles = (unsigned)((p.H + ds::kHypsPerBlock - 1) / ds::kHypsPerBlock);
  const size_t b = blockIdx.x / tiles;
  const int h = (int)(blockIdx.x % tiles) * ds::kHypsPerBlock + wave;
  if (h >= p.H) return;  // wave-uniform; the kernel has no workgroup barrier
  const size_t bh = b * p.H + h, hb = (size_t)h * p.B + b;
  double tE[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) tE[c] = 0.0;
  if (!LOSS || p.loss_kind != 0) {
    double M[9], acc[9], gM[9], gx[2], gy[2];
    load9(p.Md + bh * 9, M);
#pragma unroll
    for (int c = 0; c < 9; ++c) acc[c] = 0.0;
    const double th = (double)p.t_head[bh], beta = (double)p.beta;
    const float2* __restrict__ X = p.X + b * p.N;
    const float2* __restrict__ Y = p.Y + b * p.N;
#pragma clang loop unroll(disable)
    for (long long n = lane; n < p.N; n += WAVE) {
      const float2 x = X[n], y = Y[n];
      double g0 = 1.0;
      if (!LOSS) {
        const double s = (double)p.soft[bh * p.N + n], w = (double)p.wts[hb * p.N + n], tw = (double)p.t_w[hb * p.N + n];
        g0 = da::score_coeff(beta, s, w, th, tw);
      }
      da::sampson_adjoint(M, (double)x.x, (double)x.y, (double)y.x, (double)y.y, g0, gM, gx, gy);
#pragma unroll
      for (int c = 0; c < 9; ++c) acc[c] += gM[c];
    }
    double tM[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) tM[c] = wave_sum(acc[c]);
    if (LOSS) {
      const double k = th / (double)p.N;
#pragma unroll
      for (int c = 0; c < 9; ++c) tM[c] = k * tM[c];
    }
    if (!LOSS || p.loss_kind == 2) {
      double Ki[9];
      pair_Ki(p.K, b, Ki);
      da::f_to_e_adjoint(Ki, tM, tE);
    } else {
#pragma unroll
      for (int c = 0; c < 9; ++c) tE[c] = tM[c];
    }
  }
  // lane c < 9 writes entry c (a select over registers: tE is not indexed by the lane)
  double mine = 0.0;
#pragma unroll
  for (int c = 0; c < 9; ++c) mine = (lane == c) ? tE[c] : mine;
  if (lane < 9) {
    const double up = p.g_E != nullptr ? (double)p.g_E[bh * 9 + lane] : 0.0;
    const float v = (float)(up + mine);
    p.t_E[bh * 9 + lane] = v;
    if (LOSS) p.t_E_hb[hb * 9 + lane] = v;
  }
}

struct PointArgs {
  const float2 *X, *Y;
  const float* K;
  const int* idx;
  const float *soft, *wts, *t_w, *t_score, *t_loss;
  const double *Fd, *Md;
  const float2 *gpn1, *gpn2, *gg1, *gg2;
  float beta;
  int loss_kind;
  float2 *g_X, *g_Y;
  int B, N, H, S, chunks;
};

__global__ void __launch_bounds__(kThreads) dsac_bwd_points_kernel(PointArgs p) {
  __shared__ double part[da::kPointWaves - 1][8][da::kPointLanes];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t b = blockIdx.x / (unsigned)p.chunks;
  const long long n = (long long)(blockIdx.x % (unsigned)p.chunks) * da::kPointLanes + lane;
  const bool live = n < p.N;
  const int me = live ? (int)n : -2;  // a lane past the pair's end takes part in the barrier and matches nothing
  const int Hq = (p.H + da::kPointWaves - 1) / da::kPointWaves;
  const int h_end = (wave + 1) * Hq < p.H ? (wave + 1) * Hq : p.H;
  const double beta = (double)p.beta, inv_n = 1.0 / (double)p.N;
  float2 x = make_float2(0.f, 0.f), y = x;
  if (live) {
    x = p.X[b * p.N + n];
    y = p.Y[b * p.N + n];
  }
  double P[4] = {0.0, 0.0, 0.0, 0.0}, D[4] = {0.0, 0.0, 0.0, 0.0};  // K^-1 gradient (x, y of image 1, then 2); pixel terms likewise
#pragma clang loop unroll(disable)
  for (int h = wave * Hq; h < h_end; ++h) {
    const size_t bh = b * p.H + h, hb = (size_t)h * p.B + b;
    const int* __restrict__ list = p.idx + bh * p.S;
    for (int j = 0; j < p.S; ++j) {
      if (list[j] == me) {
        const float2 a1 = p.gg1[bh * p.S + j], a2 = p.gg2[bh * p.S + j];
        P[0] += (double)a1.x; P[1] += (double)a1.y; P[2] += (double)a2.x; P[3] += (double)a2.y;
      }
    }
    if (!live) continue;
    double M[9], gM[9], gx[2], gy[2];
    load9(p.Fd + bh * 9, M);
    const double s = (double)p.soft[bh * p.N + n], w = (double)p.wts[hb * p.N + n], tw = (double)p.t_w[hb * p.N + n];
    const double c = da::score_coeff(beta, s, w, (double)p.t_score[bh], tw);
    da::sampson_adjoint(M, (double)x.x, (double)x.y, (double)y.x, (double)y.y, c, gM, gx, gy);
    D[0] += gx[0]; D[1] += gx[1]; D[2] += gy[0]; D[3] += gy[1];
    if (p.loss_kind != 0) {
      load9(p.Md + bh * 9, M);
      da::sampson_adjoint(M, (double)x.x, (double)x.y, (double)y.x, (double)y.y, (double)p.t_loss[bh] * inv_n, gM, gx, gy);
      D[0] += gx[0]; D[1] += gx[1]; D[2] += gy[0]; D[3] += gy[1];
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      part[wave - 1][k][lane] = P[k];
      part[wave - 1][4 + k][lane] = D[k];
    }
  }
  __syncthreads();
  if (wave > 0 || !live) return;
  const float2 r1 = p.gpn1[b * p.N + n], r2 = p.gpn2[b * p.N + n];
  double G[4] = {(double)r1.x + P[0], (double)r1.y + P[1], (double)r2.x + P[2], (double)r2.y + P[3]};
#pragma unroll
  for (int v = 0; v < da::kPointWaves - 1; ++v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      G[k] += part[v][k][lane];
      D[k] += part[v][4 + k][lane];
    }
  }
  double Ki[9], pix[2];
  pair_Ki(p.K, b, Ki);
  if (p.g_X != nullptr) {
    da::pixel_from_normalized(Ki, (double)x.x, (double)x.y, G, pix);
    p.g_X[b * p.N + n] = make_float2((float)(pix[0] + D[0]), (float)(pix[1] + D[1]));
  }
  if (p.g_Y != nullptr) {
    da::pixel_from_normalized(Ki, (double)y.x, (double)y.y, G + 2, pix);
    p.g_Y[b * p.N + n] = make_float2((float)(pix[0] + D[2]), (float)(pix[1] + D[3]));
  }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" size_t dfepe_dsac_bwd_workspace_bytes(int B, int N, int H, int S) {
  if (B <= 0 || N <= 0 || H <= 0 || S < ds::kMinSample || S > ds::kMaxSample) return 0;
  return layout(B, N, H, S).total * sizeof(float);
}

extern "C" int dfepe_dsac_bwd(void* stream, const float* X, const float* Y, const float* K, const int* idx, int B, int N, int H, int S,
                              float inlier_thresh, float inlier_beta, float inlier_alpha, int loss_kind, const float* E_sample,
                              const float* soft, const float* score, const float* E_refit, const float* loss, const float* counts,
                              const float* g_E_sample, const float* g_score, const float* g_E_refit, const float* g_loss,
                              const float* g_quality, const float* g_exp_loss, float* g_X, float* g_Y, float* t_score, float* t_loss,
                              float* t_E_refit, float* t_w, float* t_E_sample, void* workspace) {
  (void)inlier_thresh;  // the soft weights are read as written, not recomputed
  if (B < 0 || N < 0 || H < 1) return DFEPE_ERR_INVALID_ARG;
  if (S < ds::kMinSample || S > ds::kMaxSample || N < S) return DFEPE_ERR_INVALID_ARG;
  if (loss_kind < 0 || loss_kind > 2) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!X || !Y || !K || !idx || !E_sample || !soft || !score || !E_refit || !loss || !counts || !workspace) return DFEPE_ERR_INVALID_ARG;
  if (!g_E_sample && !g_score && !g_E_refit && !g_loss && !g_quality && !g_exp_loss) return DFEPE_ERR_INVALID_ARG;
  if (!g_X && !g_Y) return DFEPE_ERR_INVALID_ARG;
  if (!aligned8(X) || !aligned8(Y) || !aligned8(g_X) || !aligned8(g_Y) || !aligned16(workspace)) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * H * N > kMaxCells) return DFEPE_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Workspace w = layout(B, N, H, S);
  float* ws = static_cast<float*>(workspace);
  const float2* X2 = reinterpret_cast<const float2*>(X);
  const float2* Y2 = reinterpret_cast<const float2*>(Y);
  if (!t_score) t_score = ws + w.t_score;
  if (!t_loss) t_loss = ws + w.t_loss;
  if (!t_E_refit) t_E_refit = ws + w.t_E_refit;
  if (!t_w) t_w = ws + w.t_w;
  if (!t_E_sample) t_E_sample = ws + w.t_E_sample;
  double* Fd = reinterpret_cast<double*>(ws + w.Fd);
  double* Md = reinterpret_cast<double*>(ws + w.Md);
  float2* pn1 = reinterpret_cast<float2*>(ws + w.pn1);
  float2* pn2 = reinterpret_cast<float2*>(ws + w.pn2);
  float2* g1 = reinterpret_cast<float2*>(ws + w.g1);
  float2* g2 = reinterpret_cast<float2*>(ws + w.g2);

  const size_t bh = (size_t)B * H;
  const size_t prep = (size_t)B * N + bh * S + bh * N + bh;
  const PrepArgs pa = {X2, Y2, K, soft, E_sample, E_refit, idx, pn1, pn2, g1, g2, ws + w.wts, ws + w.E_hb, Fd, Md, B, N, H, S, loss_kind};
  hipLaunchKernelGGL(dsac_bwd_prep_kernel, dim3((unsigned)((prep + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, pa);
  int rc = launched();
  if (rc != DFEPE_OK) return rc;

  const HeadArgs ha = {idx, score, loss, counts, g_score, g_loss, g_quality, g_exp_loss, inlier_alpha, t_score, t_loss, N, H, S};
  hipLaunchKernelGGL(dsac_bwd_head_kernel, dim3((unsigned)B), dim3(WAVE), 0, st, ha);
  rc = launched();
  if (rc != DFEPE_OK) return rc;

  const unsigned tiles = (unsigned)((H + ds::kHypsPerBlock - 1) / ds::kHypsPerBlock);
  const unsigned hyp_grid = (unsigned)B * tiles;
  HypArgs a = {X2, Y2, K, g_E_refit, Md, t_loss, nullptr, nullptr, nullptr, inlier_beta, loss_kind, t_E_refit, ws + w.tE_hb, B, N, H};
  hipLaunchKernelGGL(dsac_bwd_hyp_kernel<true>, dim3(hyp_grid), dim3(kThreads), 0, st, a);
  rc = launched();
  if (rc != DFEPE_OK) return rc;
  rc = dfepe_eight_point_bwd(stream, ws + w.pn1, ws + w.pn2, ws + w.wts, B, N, H, kFitFlags, ws + w.E_hb, ws + w.tE_hb, ws + w.gpn1,
                             ws + w.gpn2, t_w, ws + w.fit);
  if (rc != DFEPE_OK) return rc;

  a.g_E = g_E_sample;
  a.Md = Fd;
  a.t_head = t_score;
  a.soft = soft;
  a.wts = ws + w.wts;
  a.t_w = t_w;
  a.t_E = t_E_sample;
  a.t_E_hb = nullptr;
  hipLaunchKernelGGL(dsac_bwd_hyp_kernel<false>, dim3(hyp_grid), dim3(kThreads), 0, st, a);
  rc = launched();
  if (rc != DFEPE_OK) return rc;
  rc = dfepe_eight_point_bwd(stream, ws + w.g1, ws + w.g2, nullptr, B * H, S, 1, kFitFlags, E_sample, t_E_sample, ws + w.gg1, ws + w.gg2,
                             nullptr, nullptr);
  if (rc != DFEPE_OK) return rc;

  const int chunks = (int)(((long long)N + da::kPointLanes - 1) / da::kPointLanes);
  const PointArgs q = {X2, Y2, K, idx, soft, ws + w.wts, t_w, t_score, t_loss, Fd, Md,
                       reinterpret_cast<const float2*>(ws + w.gpn1), reinterpret_cast<const float2*>(ws + w.gpn2),
                       reinterpret_cast<const float2*>(ws + w.gg1), reinterpret_cast<const float2*>(ws + w.gg2), inlier_beta, loss_kind,
                       reinterpret_cast<float2*>(g_X), reinterpret_cast<float2*>(g_Y), B, N, H, S, chunks};
  hipLaunchKernelGGL(dsac_bwd_points_kernel, dim3((unsigned)B * (unsigned)chunks), dim3(kThreads), 0, st, q);
  return launched();
}
