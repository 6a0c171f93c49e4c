// dfepe_dsac -- the DSAC hypothesis loop of dsac_tools/dsac.py (:37-92, :138-176, :194) for a whole batch of pairs and all their
// hypotheses in six launches, whatever B and H are.  The per-lane arithmetic is csrc/dsac_math.h, the contract include/dfepe.h.
//
//   1  dsac_prep_kernel    K^-1 points of every correspondence [B,N,3] x 2, and the gathered K^-1 points of every sample [B H,S,3] x 2
//   2  dfepe_w8pt_fwd      the sample fits: B H problems of N = S (sqrt(2) Hartley, un-normalised rows, singular values (1,1,0))
//   3  dsac_score_kernel   F = K^-T E K^-1, Sampson distances, soft weights, the ordered score, the refit's weights [H,B,N]
//   4  dfepe_w8pt_fwd      the refits: H weightings (n_weight_sets) of the same B pairs
//   5  dsac_loss_kernel    E_refit [H,B] -> [B,H], the loss of every hypothesis
//   6  dsac_vote_kernel    quality and counts per correspondence, best / exp_loss / top_loss per pair
//
// Launches 3 and 5: a workgroup of 256 lanes owns ds::kHypsPerBlock hypotheses of ONE pair, a wavefront each, so the pair's points
// are read by its four wavefronts at about the same time and by the other workgroups of the pair out of L2.  A lane walks the
// correspondences lane, lane + 64, ... and adds in that order; the wavefront's 64 partial sums are added by wave_sum, a fixed tree.
// Launch 6: one lane per correspondence scans the pair's H S indices, staged through LDS ds::kVoteTile hypotheses at a time, and adds
// the float32 scores in hypothesis order, exactly the reference's sequential `+=`; the first wavefront of the pair's first workgroup
// then reduces the H scores.
// No atomics, no allocation, no host synchronisation: a pair's outputs are the same bits on every run and in every batch.
#include "dfepe_common.h"

#include "dsac_math.h"

namespace {

constexpr int kThreads = 256;
constexpr unsigned kFitFlags = DFEPE_W8PT_SQRT2 | DFEPE_W8PT_NO_ROWNORM | DFEPE_W8PT_FORCE_110;
constexpr long long kMaxCells = 2147483647LL;  // B * H * max(N, S)
static_assert(kThreads / WAVE == ds::kHypsPerBlock && kThreads == ds::kVoteChunk && WAVE == ds::kLanes, "launch shapes of dsac.hip");
static_assert(ds::kVoteTile * ds::kMaxSample == kThreads && ds::kMaxSample % 4 == 0, "one LDS entry of the vote's tile per lane");

inline size_t round4(size_t floats) { return (floats + 3) & ~(size_t)3; }  // every section starts 16-byte aligned

struct Workspace {  // offsets in floats
  size_t pn1, pn2, g1, g2, ones, res_s, wts, res_r, E_hb, total;
};
inline Workspace layout(int B, int N, int H, int S) {
  const size_t bn = (size_t)B * N, bh = (size_t)B * H;
  Workspace w;
  size_t o = 0;
  w.pn1 = o; o += round4(bn * 3);
  w.pn2 = o; o += round4(bn * 3);
  w.g1 = o; o += round4(bh * S * 3);
  w.g2 = o; o += round4(bh * S * 3);
  w.ones = o; o += round4(bh * S);
  w.res_s = o; o += round4(bh * S);
  w.wts = o; o += round4(bh * N);
  w.res_r = o; o += round4(bh * N);
  w.E_hb = o; o += round4(bh * 9);
  w.total = o;
  return w;
}

__device__ __forceinline__ void load9(const float* __restrict__ p, double* m) {
#pragma unroll
  for (int c = 0; c < 9; ++c) m[c] = (double)p[c];
}

__device__ __forceinline__ void write_point(float* __restrict__ dst, const double* Ki, float2 v) {
  float o[2];
  ds::normalized_point(Ki, (double)v.x, (double)v.y, o);
  dst[0] = o[0]; dst[1] = o[1]; dst[2] = 1.0f;
}

// t < B N: correspondence t of the batch.  Above: slot q = t - B N of the samples, q = (b H + h) S + s.
__global__ void __launch_bounds__(kThreads) dsac_prep_kernel(const float2* __restrict__ X, const float2* __restrict__ Y,
                                                             const float* __restrict__ K, const int* __restrict__ idx, int B, int N,
                                                             int H, int S, float* __restrict__ pn1, float* __restrict__ pn2,
                                                             float* __restrict__ g1, float* __restrict__ g2, float* __restrict__ ones) {
  const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t bn = (size_t)B * N, slots = (size_t)B * H * S;
  if (t >= bn + slots) return;
  double Km[9], Ki[9];
  if (t < bn) {
    load9(K + (t / N) * 9, Km);
    ds::inv3(Km, Ki);
    write_point(pn1 + t * 3, Ki, X[t]);
    write_point(pn2 + t * 3, Ki, Y[t]);
    return;
  }
  const size_t q = t - bn;
  const size_t b = q / ((size_t)H * S);
  int n = idx[q];
  n = n < 0 ? 0 : (n >= N ? N - 1 : n);  // the contract is 0 <= idx < N; an index outside is never followed out of the pair
  load9(K + b * 9, Km);
  ds::inv3(Km, Ki);
  write_point(g1 + q * 3, Ki, X[b * N + n]);
  write_point(g2 + q * 3, Ki, Y[b * N + n]);
  ones[q] = 1.0f;
}

struct HypArgs {
  const float2 *X, *Y;
  const float *K, *E;  // E: [B,H,9] (score) or [H,B,9] (loss)
  float thresh, beta;
  int loss_kind;
  float *soft, *sampson, *score, *wts;  // score kernel
  float *E_out, *loss;                  // loss kernel
  int B, N, H;
};

// LOSS false: launch 3.  LOSS true: launch 5.
template <bool LOSS>
__global__ void __launch_bounds__(kThreads) dsac_hyp_kernel(HypArgs p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned tiles = (unsigned)((p.H + ds::kHypsPerBlock - 1) / ds::kHypsPerBlock);
  const size_t b = blockIdx.x / tiles;
  const int h = (int)(blockIdx.x % tiles) * ds::kHypsPerBlock + wave;
  if (h >= p.H) return;  // wave-uniform; the kernel has no workgroup barrier
  const size_t bh = b * p.H + h, hb = (size_t)h * p.B + b;
  double Km[9], Ki[9], E[9], M[9];
  load9(p.E + (LOSS ? hb : bh) * 9, E);
  const bool pixel_F = !LOSS || p.loss_kind == 2;
  if (pixel_F) {
    load9(p.K + b * 9, Km);
    ds::inv3(Km, Ki);
    ds::e_to_f(Ki, E, M);
  } else {
#pragma unroll
    for (int c = 0; c < 9; ++c) M[c] = E[c];
  }
  if (LOSS && lane < 9) p.E_out[bh * 9 + lane] = (float)E[lane];
  if (LOSS && p.loss_kind == 0) {
    if (lane == 0) p.loss[bh] = 0.0f;
    return;
  }
  const double thresh = (double)p.thresh, beta = (double)p.beta;
  const float2* __restrict__ X = p.X + b * p.N;
  const float2* __restrict__ Y = p.Y + b * p.N;
  double acc = 0.0;
#pragma clang loop unroll(disable)
  for (long long n = lane; n < p.N; n += WAVE) {
    const float2 x = X[n], y = Y[n];
    const double d = ds::sampson(M, (double)x.x, (double)x.y, (double)y.x, (double)y.y);
    if (LOSS) {
      acc += d;
    } else {
      const double s = ds::soft_inlier(d, thresh, beta);
      const float sf = (float)s;
      if (p.soft != nullptr) p.soft[bh * p.N + n] = sf;
      if (p.sampson != nullptr) p.sampson[bh * p.N + n] = (float)d;
      p.wts[hb * p.N + n] = ds::refit_weight(sf);
      acc += s;
    }
  }
  const double tot = wave_sum(acc);
  if (lane == 0) {
    if (LOSS) p.loss[bh] = (float)(tot / (double)p.N);
    else p.score[bh] = (float)tot;
  }
}

struct VoteArgs {
  const int* idx;
  const float *score, *loss;
  float alpha;
  float *quality, *counts, *exp_loss, *top_loss;
  int* best;
  int N, H, S, chunks;
};

__global__ void __launch_bounds__(kThreads) dsac_vote_kernel(VoteArgs p) {
  const size_t b = blockIdx.x / (unsigned)p.chunks;
  const int chunk = blockIdx.x % (unsigned)p.chunks;
  const long long n = (long long)chunk * ds::kVoteChunk + threadIdx.x;
  const float* __restrict__ score = p.score + b * p.H;
  const int* __restrict__ idx = p.idx + b * p.H * p.S;
  // The pair's index lists go through LDS a tile of ds::kVoteTile hypotheses at a time, one entry per lane: slot s < S of
  // hypothesis h0 + t, the slots S .. 15 and the hypotheses past H padded with -1, which equals no correspondence.  A lane then
  // reads a hypothesis as four 16-byte words that every lane of the wavefront reads too (a broadcast, no bank conflict).  The
  // next tile's entry is loaded before the current one is scanned, so its latency is hidden behind the scan.
  __shared__ __attribute__((aligned(16))) int tile_idx[ds::kVoteTile * ds::kMaxSample];
  __shared__ float tile_score[ds::kVoteTile];
  const int th = threadIdx.x / ds::kMaxSample, ts = threadIdx.x % ds::kMaxSample;
  auto entry = [&](int h0) { return (h0 + th < p.H && ts < p.S) ? idx[(size_t)(h0 + th) * p.S + ts] : -1; };
  auto score_of = [&](int h0) { return (threadIdx.x < ds::kVoteTile && h0 + (int)threadIdx.x < p.H) ? score[h0 + threadIdx.x] : 0.f; };
  int next_idx = entry(0);
  float next_score = score_of(0);
  const int me = (n < p.N) ? (int)n : -2;  // a lane past the pair's end takes part in the barriers and matches nothing
  float ns = 0.f, nc = 0.f;
#pragma clang loop unroll(disable)
  for (int h0 = 0; h0 < p.H; h0 += ds::kVoteTile) {
    __syncthreads();  // the scan of the tile before is over
    tile_idx[threadIdx.x] = next_idx;
    if (threadIdx.x < ds::kVoteTile) tile_score[threadIdx.x] = next_score;
    __syncthreads();
    next_idx = entry(h0 + ds::kVoteTile);
    next_score = score_of(h0 + ds::kVoteTile);
#pragma unroll
    for (int t = 0; t < ds::kVoteTile; ++t) {
      int hit = 0;  // `|`, not `||`: the four reads of a hypothesis are issued together, not one behind a branch on the other
#pragma unroll
      for (int q = 0; q < ds::kMaxSample / 4; ++q) {
        const int4 v = reinterpret_cast<const int4*>(tile_idx)[t * (ds::kMaxSample / 4) + q];
        hit |= (int)(v.x == me) | (int)(v.y == me) | (int)(v.z == me) | (int)(v.w == me);
      }
      // the indices of one hypothesis are distinct: one `+=` per hypothesis, in hypothesis order (dsac.py:163-165)
      const float sc = tile_score[t];
      ns = hit ? ns + sc : ns;
      nc = hit ? nc + 1.0f : nc;
    }
  }
  if (n < p.N) {
    p.quality[b * p.N + n] = ds::quality(ns, nc);
    p.counts[b * p.N + n] = nc;
  }
  if (chunk != 0 || threadIdx.x >= WAVE) return;
  // the pair's H scores: the first hypothesis whose score is the strict maximum above 0 (dsac.py:130, :168), and the expectation
  // the reference leaves commented out (:178-190)
  const int lane = threadIdx.x;
  float bv = 0.f;
  int bi = -1;
  for (int h = lane; h < p.H; h += WAVE) {
    const float sc = score[h];
    if (sc > bv) { bv = sc; bi = h; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    if (ov > bv || (ov == bv && oi >= 0 && (bi < 0 || oi < bi))) { bv = ov; bi = oi; }
  }
  if (lane == 0) {
    p.best[b] = bi;
    if (p.top_loss != nullptr) p.top_loss[b] = bi >= 0 ? p.loss[b * p.H + bi] : 0.0f;
  }
  if (p.exp_loss == nullptr) return;
  const double alpha = (double)p.alpha;
  double m = -INFINITY;
  for (int h = lane; h < p.H; h += WAVE) m = fmax(m, alpha * (double)score[h]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off));
  double Z = 0.0, num = 0.0;
  for (int h = lane; h < p.H; h += WAVE) {
    const double e = exp(alpha * (double)score[h] - m);
    Z += e;
    num += e * (double)p.loss[b * p.H + h];
  }
  Z = wave_sum(Z);
  num = wave_sum(num);
  if (lane == 0) p.exp_loss[b] = (float)(num / Z);
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int dfepe_dsac_hyps_per_block(void) { return ds::kHypsPerBlock; }
extern "C" int dfepe_dsac_vote_chunk(void) { return ds::kVoteChunk; }
extern "C" int dfepe_dsac_vote_tile(void) { return ds::kVoteTile; }

extern "C" size_t dfepe_dsac_workspace_bytes(int B, int N, int H, int S) {
  if (B <= 0 || N <= 0 || H <= 0 || S < ds::kMinSample || S > ds::kMaxSample) return 0;
  return layout(B, N, H, S).total * sizeof(float);
}

extern "C" int dfepe_dsac(void* stream, const float* X, const float* Y, const float* K, const int* idx, int B, int N, int H, int S,
                          float inlier_thresh, float inlier_beta, float inlier_alpha, int loss_kind, float* E_sample, float* soft,
                          float* sampson, float* score, float* E_refit, float* loss, float* quality, float* counts, int* best,
                          float* exp_loss, float* top_loss, void* workspace) {
  if (B < 0 || N < 0 || H < 1) return DFEPE_ERR_INVALID_ARG;
  if (S < ds::kMinSample || S > ds::kMaxSample || N < S) return DFEPE_ERR_INVALID_ARG;
  if (loss_kind < 0 || loss_kind > 2) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!X || !Y || !K || !idx || !E_sample || !score || !E_refit || !loss || !quality || !counts || !best || !workspace)
    return DFEPE_ERR_INVALID_ARG;
  if (!aligned8(X) || !aligned8(Y) || !aligned16(workspace)) return DFEPE_ERR_INVALID_ARG;
  if ((long long)B * H * N > kMaxCells) return DFEPE_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Workspace w = layout(B, N, H, S);
  float* ws = static_cast<float*>(workspace);
  const float2* X2 = reinterpret_cast<const float2*>(X);
  const float2* Y2 = reinterpret_cast<const float2*>(Y);

  const size_t prep = (size_t)B * N + (size_t)B * H * S;
  hipLaunchKernelGGL(dsac_prep_kernel, dim3((unsigned)((prep + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, X2, Y2, K, idx, B, N, H, S,
                     ws + w.pn1, ws + w.pn2, ws + w.g1, ws + w.g2, ws + w.ones);
  int rc = launched();
  if (rc != DFEPE_OK) return rc;
  rc = dfepe_w8pt_fwd(ws + w.g1, ws + w.g2, ws + w.ones, B * H, S, 1, kFitFlags, 0.f, 0.f, 0.5f, E_sample, ws + w.res_s, nullptr, nullptr,
                      nullptr, stream);
  if (rc != DFEPE_OK) return rc;

  const unsigned tiles = (unsigned)((H + ds::kHypsPerBlock - 1) / ds::kHypsPerBlock);
  const unsigned hyp_grid = (unsigned)B * tiles;
  HypArgs a = {X2, Y2, K, E_sample, inlier_thresh, inlier_beta, loss_kind, soft, sampson, score, ws + w.wts, nullptr, nullptr, B, N, H};
  hipLaunchKernelGGL(dsac_hyp_kernel<false>, dim3(hyp_grid), dim3(kThreads), 0, st, a);
  rc = launched();
  if (rc != DFEPE_OK) return rc;
  rc = dfepe_w8pt_fwd(ws + w.pn1, ws + w.pn2, ws + w.wts, B, N, H, kFitFlags, 0.f, 0.f, 0.5f, ws + w.E_hb, ws + w.res_r, nullptr, nullptr,
                      nullptr, stream);
  if (rc != DFEPE_OK) return rc;

  a.E = ws + w.E_hb;
  a.E_out = E_refit;
  a.loss = loss;
  hipLaunchKernelGGL(dsac_hyp_kernel<true>, dim3(hyp_grid), dim3(kThreads), 0, st, a);
  rc = launched();
  if (rc != DFEPE_OK) return rc;

  const int chunks = (int)(((long long)N + ds::kVoteChunk - 1) / ds::kVoteChunk);
  VoteArgs v = {idx, score, loss, inlier_alpha, quality, counts, exp_loss, top_loss, best, N, H, S, chunks};
  hipLaunchKernelGGL(dsac_vote_kernel, dim3((unsigned)B * (unsigned)chunks), dim3(kThreads), 0, st, v);
  return launched();
}
