// est_pass -- one estimator pass per call (round 5), host code only: dfepe_est_forward / dfepe_est_backward run the whole Conv1d ->
// InstanceNorm -> LeakyReLU stack and its head (one output channel) through the exported entry points of est_gemm.hip, est_norm.hip and
// est_planes.hip (and the two launches of dfepe_est_detail).  Why: at the reference's batch sizes the HOST is the limiter of the eager
// training step (Python spent ~0.27 ms per forward and more per backward on ~30 launches, ~40 allocations and their bookkeeping: more than
// the GPU needs for the whole model's step).  The caller brings three buffers -- `saved` (what the backward reads: the layers' bf16
// planes, reciprocal deviations, transposed weight planes), a transient workspace per pass, the outputs -- whose sizes the *_bytes
// functions give; nothing is allocated here.
//
// Round 6 -- the step a train_good.py user runs (N = 1000-2000 points, 4-12 pairs: deepFEPE/configs/kitti_corr_baseline.yaml:12-13):
//   * every layer has a PLAN (fwd_plan / dgrad_plan): the fused epilogue (N = 100, grid large enough), or the plain product -- split over
//     S slices of K where a batch of a few pairs leaves a K-heavy layer on a dozen workgroups -- followed by ONE register-resident
//     normalisation launch that adds the slices (est_norm_fwd_r / est_in_bwd_r: N <= 2048; beyond, the strided kernels of round 4);
//   * `prep` (dfepe_est_prepare): the weights' planes made ONCE per model forward for an estimator that is called several times in it
//     (DeepFNet.update_weights: depth - 1 calls, deepFEPE/models/DeepFNet.py:510) instead of once per call;
//   * over few columns (all dY of a backward alive together: the gamma == 0 fix already wanted that) the five weight-gradient GEMMs are
//     ONE table-driven launch at the end (est_gemm_tn_multi);
//   * the head bias partials ride in est_head_dw, the first layer's cropped weight gradient in est_colsum, the input gradient's
//     transposition in its GEMM's epilogue: three launches per call gone.
#include "est_common.h"

namespace {

constexpr size_t kAlign = 256;
inline size_t up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }
inline int pad32(int c) { return (c + 31) / 32 * 32; }

struct PassDims {
  int n;              // hidden layers
  int Co[kTabMax], Ci[kTabMax], K[kTabMax];
  long B; int N; long cols;
  int C0, K0, Cmax, Kmax;
  bool fusable;       // N == kPts: the fused epilogues exist
  bool resident;      // N <= 2048: the register-resident normalisation kernels serve the plain products
};
int pass_dims(PassDims& D, int n_hidden, const int* Co, const int* Ci, long B, int C0, int N) {
  if (n_hidden <= 0 || n_hidden > kTabMax || !Co || !Ci || B <= 0 || N < 2 || C0 <= 0 || B * (long)N >= (1L << 31)) return DFEPE_ERR_INVALID_ARG;
  D.n = n_hidden; D.B = B; D.N = N; D.cols = B * (long)N; D.C0 = C0; D.K0 = pad32(C0); D.Cmax = 0; D.Kmax = 0;
  D.fusable = (N == kPts); D.resident = (N <= 2048);
  for (int l = 0; l < n_hidden; ++l) {
    if (Co[l] <= 0 || (Co[l] & 31) || Ci[l] != (l ? Co[l - 1] : C0)) return DFEPE_ERR_INVALID_ARG;
    D.Co[l] = Co[l]; D.Ci[l] = Ci[l]; D.K[l] = pad32(Ci[l]);
    D.Cmax = Co[l] > D.Cmax ? Co[l] : D.Cmax; D.Kmax = D.K[l] > D.Kmax ? D.K[l] : D.Kmax;
  }
  return DFEPE_OK;
}
int row_splits(long pairs, int c, int n) {  // estimator.py: _row_splits
  const long blocks = pairs * ((c + 63) / 64);
  if (blocks >= 512 || n < 256) return 1;
  long s = (1024 + blocks - 1) / blocks;
  s = s < n / 128 ? s : n / 128;
  s = s < 64 ? s : 64;
  return (int)(s > 1 ? s : 1);
}
int slices_for(int cout, int cin, long cols) {  // estimator.py: _slices_for (TN_BLOCKS = 768)
  const int tiles = ((cout + 127) / 128) * ((cin + 127) / 128);
  long s = 768 / tiles;
  s = s < 512 ? s : 512;
  s = s < cols / 256 ? s : cols / 256;
  s = s > 1 ? s : 1;
  return (int)(s >= 8 ? s - s % 8 : s);
}

// How one GEMM of a pass runs: through its fused epilogue, or as S partial products + a normalisation launch.
// DFEPE_EST_SPLITK = 0: fused wherever it exists and never split (round 5's behaviour); 2: the plain product wherever it can serve (A/B timing)
struct Plan { bool fused; int S; };
int splitk_mode() {
  static const char* e = getenv("DFEPE_EST_SPLITK");
  return e ? (e[0] - '0') : 1;
}
Plan gemm_plan(const PassDims& D, int M, int K, bool fusable) {
  const long tiles = ((D.cols + BSTEP - 1) / BSTEP) * ((M + BM - 1) / BM);
  const int nk = K / BK, mode = splitk_mode();
  Plan P{fusable, 1};
  if (!D.resident || mode == 0) return P;  // the strided kernels of round 4 take one plain product
  // a K-heavy product on a few workgroups is a chain of K steps with most of the chip idle: slices of >= 4 K steps each, up to ~256
  // workgroups, at most eight partials for the normalisation launch to add
  long S = 1;
  if (tiles < 128 && nk >= 8) {
    S = 256 / tiles;
    S = S < nk / 4 ? S : nk / 4;
    S = S < 8 ? S : 8;
    S = S > 1 ? S : 1;
  }
  if (fusable && mode != 2 && !(tiles <= 64 && nk >= 8)) return P;  // the fused epilogue: one launch, nothing written twice
  P.fused = false; P.S = (int)S;
  return P;
}
Plan fwd_plan(const PassDims& D, int l) { return gemm_plan(D, D.Co[l], D.K[l], D.fusable); }
// the data gradient of layer l (>= 1) = the upstream gradient of layer l - 1: M = K[l] rows (= Co[l - 1]), contraction over Co[l]
Plan dgrad_plan(const PassDims& D, int l) { return gemm_plan(D, D.K[l], D.Co[l], D.fusable && D.Ci[l] == D.K[l]); }

// the weights' planes of one estimator, made once and shared by its calls: words | fp16 planes per layer | transposed bf16 planes per layer
struct PrepLayout { size_t words, absws, wf[kTabMax], wt[kTabMax], total; };
PrepLayout prep_layout(int n, const int* Co, const int* Ci) {
  PrepLayout P{};
  size_t at = 0;
  P.words = at; at += up(sizeof(unsigned) * kTabMax);
  P.absws = at; at += up(dfepe_est_wprep_workspace_bytes(n));
  for (int l = 0; l < n; ++l) { P.wf[l] = at; at += up((size_t)2 * Co[l] * pad32(Ci[l]) * 2); }
  for (int l = 0; l < n; ++l) { P.wt[l] = at; at += up((size_t)2 * pad32(Ci[l]) * Co[l] * 2); }
  P.total = at;
  return P;
}

// what the backward reads, laid out in `saved`
struct SavedLayout {
  size_t words, act[kTabMax + 1], rstd[kTabMax], wt[kTabMax], total;
};
SavedLayout saved_layout(const PassDims& D, bool need_gx) {
  SavedLayout S{};
  size_t at = 0;
  S.words = at; at += up(sizeof(unsigned) * kTabMax);
  S.act[0] = at; at += up((size_t)2 * D.cols * D.K0 * 2);
  for (int l = 0; l < D.n; ++l) { S.act[l + 1] = at; at += up((size_t)2 * D.cols * D.Co[l] * 2); }
  for (int l = 0; l < D.n; ++l) { S.rstd[l] = at; at += up((size_t)D.B * D.Co[l] * 4); }
  (void)need_gx;  // the first layer's transposed planes (a few KB) are always there: the layout must not depend on what the caller
  for (int l = 0; l < D.n; ++l) { S.wt[l] = at; at += up((size_t)2 * D.K[l] * D.Co[l] * 2); }  // later asks the backward for
  S.total = at;
  return S;
}
struct FwdLayout {
  size_t absws, wf[kTabMax], xh, ping, pong, rstd_scratch, Y, npart, words, total;
};
FwdLayout fwd_layout(const PassDims& D, bool keep) {
  FwdLayout F{};
  size_t at = 0;
  F.absws = at; at += up(dfepe_est_wprep_workspace_bytes(D.n));
  F.words = at; at += up(sizeof(unsigned) * kTabMax);  // used when nothing is kept (no `saved`)
  for (int l = 0; l < D.n; ++l) { F.wf[l] = at; at += up((size_t)2 * D.Co[l] * D.K[l] * 2); }
  F.xh = at; at += up((size_t)2 * D.cols * D.K0 * 2);
  int c_even = 0, c_odd = 0;  // the layers' fp16 outputs take turns in two buffers: even layers in one, odd ones in the other
  for (int l = 0; l < D.n; ++l) { int& c = (l & 1) ? c_odd : c_even; c = D.Co[l] > c ? D.Co[l] : c; }
  F.ping = at; at += up((size_t)2 * D.cols * c_even * 2);
  F.pong = at; at += up((size_t)2 * D.cols * c_odd * 2);
  F.rstd_scratch = at; if (!keep) at += up((size_t)D.B * D.Cmax * 4);
  size_t ybytes = 0;  // the largest plain product of the pass, its split-K partials included
  for (int l = 0; l < D.n; ++l) {
    const Plan P = fwd_plan(D, l);
    if (!P.fused) { const size_t b = (size_t)P.S * D.cols * D.Co[l] * 4; ybytes = b > ybytes ? b : ybytes; }
  }
  F.Y = at; at += up(ybytes);
  F.npart = at; if (!D.resident) at += up((size_t)D.B * 64 * 2 * D.Cmax * 4);
  F.total = at;
  return F;
}
struct BwdLayout {
  size_t hpart, bpart, dY[kTabMax], dg[kTabMax], db[kTabMax], partw[kTabMax], dA, npart, total;
  int slices[kTabMax];
  bool keep_all;  // every layer's dY stays alive to the end of the backward: one gamma == 0 launch and one weight-gradient launch there
};
BwdLayout bwd_layout(const PassDims& D, bool need_gx) {
  BwdLayout L{};
  size_t at = 0;
  L.hpart = at; at += up((size_t)512 * D.Co[D.n - 1] * 4);
  L.bpart = at; at += up((size_t)512 * 4);
  size_t dy_total = 0;
  for (int l = 0; l < D.n; ++l) dy_total += (size_t)D.cols * D.Co[l] * 4;
  L.keep_all = dy_total <= ((size_t)64 << 20);
  if (const char* e = getenv("DFEPE_EST_KEEP_ALL")) L.keep_all = e[0] == '1';  // tests: both branches at any size
  if (L.keep_all) {
    for (int l = 0; l < D.n; ++l) { L.dY[l] = at; at += up((size_t)2 * D.cols * D.Co[l] * 2); }
  } else {  // two buffers taking turns: dY of layer l is read while dY of layer l - 1 is written
    int ca = 0, cb = 0;
    for (int l = D.n - 1, k = 0; l >= 0; --l, ++k) { int& c = (k & 1) ? cb : ca; c = D.Co[l] > c ? D.Co[l] : c; }
    const size_t a = at, b = at + up((size_t)2 * D.cols * ca * 2);
    at = b + up((size_t)2 * D.cols * cb * 2);
    for (int l = D.n - 1, k = 0; l >= 0; --l, ++k) L.dY[l] = (k & 1) ? b : a;
  }
  for (int l = 0; l < D.n; ++l) {
    L.dg[l] = at; at += up((size_t)D.B * D.Co[l] * 4);
    L.db[l] = at; at += up((size_t)D.B * D.Co[l] * 4);
    L.slices[l] = slices_for(D.Co[l], D.K[l], D.cols);
    L.partw[l] = at; at += up((size_t)L.slices[l] * D.Co[l] * D.K[l] * 4);
  }
  size_t dabytes = 0;  // the largest data gradient that is written (not fused, not the input's: that one goes straight to gx)
  for (int l = 1; l < D.n; ++l) {
    const Plan P = dgrad_plan(D, l);
    if (!P.fused) { const size_t b = (size_t)P.S * D.cols * D.K[l] * 4; dabytes = b > dabytes ? b : dabytes; }
  }
  (void)need_gx;
  L.dA = at; at += up(dabytes);
  L.npart = at; if (!D.resident) at += up((size_t)D.B * 64 * 2 * D.Cmax * 4);
  L.total = at;
  return L;
}

}  // namespace

#define EST_TRY(call) do { const int rc_ = (call); if (rc_ != DFEPE_OK) return rc_; } while (0)

extern "C" size_t dfepe_est_saved_bytes(int n_hidden, const int* Co, const int* Ci, long B, int C0, int N, int need_gx) {
  PassDims D;
  if (pass_dims(D, n_hidden, Co, Ci, B, C0, N) != DFEPE_OK) return 0;
  return saved_layout(D, need_gx != 0).total;
}
extern "C" size_t dfepe_est_forward_workspace_bytes(int n_hidden, const int* Co, const int* Ci, long B, int C0, int N, int keep) {
  PassDims D;
  if (pass_dims(D, n_hidden, Co, Ci, B, C0, N) != DFEPE_OK) return 0;
  return fwd_layout(D, keep != 0).total;
}
extern "C" size_t dfepe_est_backward_workspace_bytes(int n_hidden, const int* Co, const int* Ci, long B, int C0, int N, int need_gx) {
  PassDims D;
  if (pass_dims(D, n_hidden, Co, Ci, B, C0, N) != DFEPE_OK) return 0;
  return bwd_layout(D, need_gx != 0).total;
}
extern "C" size_t dfepe_est_prep_bytes(int n_hidden, const int* Co, const int* Ci) {
  if (n_hidden <= 0 || n_hidden > kTabMax || !Co || !Ci) return 0;
  for (int l = 0; l < n_hidden; ++l)
    if (Co[l] <= 0 || (Co[l] & 31) || Ci[l] <= 0) return 0;
  return prep_layout(n_hidden, Co, Ci).total;
}
// the weights' planes (scales, scaled fp16 planes for the forward, transposed bf16 planes for the data gradients) of one estimator into
// `prep` (dfepe_est_prep_bytes, 16-byte aligned): two launches, once per model forward; dfepe_est_forward / _backward given `prep`
// read them instead of making their own.  The weights must not change between this call and the last backward that is handed `prep`.
extern "C" int dfepe_est_prepare(int n_hidden, const float* const* W, const int* Co, const int* Ci, void* prep, void* stream) {
  if (n_hidden <= 0 || n_hidden > kTabMax || !W || !Co || !Ci || !prep || ((uintptr_t)prep & 15)) return DFEPE_ERR_INVALID_ARG;
  for (int l = 0; l < n_hidden; ++l)
    if (Co[l] <= 0 || (Co[l] & 31) || Ci[l] <= 0) return DFEPE_ERR_INVALID_ARG;
  const PrepLayout P = prep_layout(n_hidden, Co, Ci);
  char* pp = static_cast<char*>(prep);
  void* pf[kTabMax]; void* pt[kTabMax];
  for (int l = 0; l < n_hidden; ++l) { pf[l] = pp + P.wf[l]; pt[l] = pp + P.wt[l]; }
  return dfepe_est_wprep(n_hidden, W, Co, Ci, pf, pt, reinterpret_cast<unsigned*>(pp + P.words), pp + P.absws, stream);
}

// logits [cols] = head(stack(x)); saved != null: everything dfepe_est_backward needs is left there (need_gx is accepted for symmetry with
// the size functions and ignored: the first layer's transposed weight planes are a few KB and always kept, so that a backward may ask
// for gx or not).  x [B][C0][N] with element (b, c, n) at b * x_stride_b + c * x_stride_c + n (dense: C0 N, N; the model's channel-major input
// buffers [C0][B][N]: N, B N -- no copy either way), W[l] [Co][Ci], gamma / beta [l] [Co], w_head [Co of the last layer], b_head [1] or null: fp32.
// prep: null, or the planes dfepe_est_prepare made of these very weights.
extern "C" int dfepe_est_forward(const float* x, long x_stride_b, long x_stride_c, long B, int C0, int N, int n_hidden, const float* const* W, const float* const* gamma,
                                 const float* const* beta, const int* Co, const int* Ci, const float* w_head, const float* b_head, float eps,
                                 float slope, void* saved, int need_gx, void* workspace, const void* prep, float* logits, void* stream) {
  PassDims D;
  EST_TRY(pass_dims(D, n_hidden, Co, Ci, B, C0, N));
  if (!x || !W || !gamma || !beta || !w_head || !workspace || !logits || x_stride_b <= 0 || x_stride_c <= 0) return DFEPE_ERR_INVALID_ARG;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)saved & 15) || ((uintptr_t)prep & 15)) return DFEPE_ERR_INVALID_ARG;
  const bool keep = saved != nullptr;
  const SavedLayout S = saved_layout(D, need_gx != 0);
  const FwdLayout F = fwd_layout(D, keep);
  const PrepLayout P = prep_layout(D.n, Co, Ci);
  char* ws = static_cast<char*>(workspace);
  char* sv = static_cast<char*>(saved);
  const char* pp = static_cast<const char*>(prep);
  const long cols = D.cols;
  const unsigned* words = pp ? reinterpret_cast<const unsigned*>(pp + P.words) : reinterpret_cast<unsigned*>(keep ? sv + S.words : ws + F.words);
  // the input's planes
  EST_TRY(dfepe_est_detail::input_split_launch(x, x_stride_b, x_stride_c, B, C0, N, D.K0, ws + F.xh, (size_t)cols * D.K0, keep ? sv + S.act[0] : nullptr,
                                               (size_t)cols * D.K0, stream));
  // every layer's weights: scales, fp16 planes, transposed bf16 planes for the backward -- unless the caller prepared them
  if (!pp) {
    void* pf[kTabMax]; void* pt[kTabMax];
    for (int l = 0; l < D.n; ++l) { pf[l] = ws + F.wf[l]; pt[l] = keep ? sv + S.wt[l] : nullptr; }
    EST_TRY(dfepe_est_wprep(D.n, W, Co, Ci, pf, pt, const_cast<unsigned*>(words), ws + F.absws, stream));
  }
  const char* act = ws + F.xh;
  for (int l = 0; l < D.n; ++l) {
    const int C = D.Co[l], K = D.K[l];
    const void* wf = pp ? static_cast<const void*>(pp + P.wf[l]) : static_cast<const void*>(ws + F.wf[l]);
    char* out = ws + ((l & 1) ? F.pong : F.ping);
    void* out_b = keep ? sv + S.act[l + 1] : nullptr;
    float* rstd = reinterpret_cast<float*>(keep ? sv + S.rstd[l] : ws + F.rstd_scratch);
    const Plan pl = fwd_plan(D, l);
    if (pl.fused) {
      EST_TRY(dfepe_est_layer_fwd(wf, (size_t)C * K, act, (size_t)cols * K, C, (int)cols, K, words + l, gamma[l], beta[l], eps, slope, out,
                                  (size_t)cols * C, out_b, (size_t)cols * C, rstd, stream));
    } else {
      float* Y = reinterpret_cast<float*>(ws + F.Y);
      const size_t ystride = (size_t)cols * C;
      EST_TRY(dfepe_est_gemm_nt_f16_splitk(wf, (size_t)C * K, act, (size_t)cols * K, C, (int)cols, K, words + l, Y, C, pl.S, ystride, stream));
      if (D.resident) {
        EST_TRY(dfepe_est_norm_fwd_r(Y, C, pl.S, ystride, C, B, N, gamma[l], beta[l], eps, slope, out, (size_t)cols * C, out_b, (size_t)cols * C, rstd,
                                     stream));
      } else {
        const int sp = row_splits(B, C, N);
        EST_TRY(dfepe_est_norm_fwd(Y, C, C, B, N, gamma[l], beta[l], eps, slope, out, (size_t)cols * C, out_b, (size_t)cols * C, rstd, sp,
                                   sp > 1 ? reinterpret_cast<float*>(ws + F.npart) : nullptr, stream));
      }
    }
    act = out;
  }
  return dfepe_est_head_fwd(act, (size_t)cols * D.Co[D.n - 1], D.Co[D.n - 1], (int)cols, w_head, b_head, logits, stream);
}

// every gradient of one dfepe_est_forward(saved != null): g_W[l] [Co][Ci], g_bias[l] [Co] (zeros: the bias cancels in the
// normalisation), g_gamma[l], g_beta[l] [Co], g_w_head [C], g_b_head [1] or null, gx or null (needs need_gx at the forward; element
// (b, c, n) at b * gx_stride_b + c * gx_stride_c + n, like x);
// prep: what the forward was given (null: the transposed weight planes are in `saved`)
extern "C" int dfepe_est_backward(const float* g_logits, long B, int C0, int N, int n_hidden, const float* const* W, const float* const* gamma,
                                  const float* const* beta, const int* Co, const int* Ci, const float* w_head, float slope, const void* saved,
                                  void* workspace, const void* prep, float* const* g_W, float* const* g_bias, float* const* g_gamma,
                                  float* const* g_beta, float* g_w_head, float* g_b_head, float* gx, long gx_stride_b, long gx_stride_c, void* stream) {
  PassDims D;
  EST_TRY(pass_dims(D, n_hidden, Co, Ci, B, C0, N));
  if (!g_logits || !W || !gamma || !beta || !w_head || !saved || !workspace || !g_W || !g_bias || !g_gamma || !g_beta || !g_w_head)
    return DFEPE_ERR_INVALID_ARG;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)saved & 15) || ((uintptr_t)prep & 15)) return DFEPE_ERR_INVALID_ARG;
  if (gx && (gx_stride_b <= 0 || gx_stride_c <= 0)) return DFEPE_ERR_INVALID_ARG;
  const bool need_gx = gx != nullptr;
  const SavedLayout S = saved_layout(D, need_gx);
  const BwdLayout L = bwd_layout(D, need_gx);
  const PrepLayout P = prep_layout(D.n, Co, Ci);
  char* ws = static_cast<char*>(workspace);
  const char* sv = static_cast<const char*>(saved);
  const char* pp = static_cast<const char*>(prep);
  const long cols = D.cols;
  const int n = D.n, Clast = D.Co[n - 1];
  const float* src[kSegMax]; float* dst[kSegMax]; int rows[kSegMax], ccols[kSegMax], lds_[kSegMax], ldd_[kSegMax];
  int nseg = 0;
  auto seg = [&](const float* s, int r, int c, float* d, int ld_src = 0, int ld_dst = 0) {
    src[nseg] = s; rows[nseg] = r; ccols[nseg] = c; dst[nseg] = d; lds_[nseg] = ld_src; ldd_[nseg] = ld_dst; ++nseg;
  };
  auto flush = [&]() -> int {
    if (nseg == 0) return DFEPE_OK;
    const int rc = dfepe_est_detail::colsum_launch(nseg, src, rows, ccols, dst, lds_, ldd_, stream);
    nseg = 0;
    return rc;
  };
  // head (the bias gradient's partial sums ride in the same launch)
  const int nblk = 512;
  float* hpart = reinterpret_cast<float*>(ws + L.hpart);
  float* bpart = reinterpret_cast<float*>(ws + L.bpart);
  EST_TRY(dfepe_est_head_dw(sv + S.act[n], (size_t)cols * Clast, Clast, (int)cols, nblk, g_logits, hpart, g_b_head ? bpart : nullptr, stream));
  seg(hpart, nblk, Clast, g_w_head);
  if (g_b_head) seg(bpart, nblk, 1, g_b_head);
  // gamma == 0 fixes (one launch at the end, or layer by layer) and the weight gradients (likewise): see bwd_layout
  const float* f_dA[kTabMax]; const float* f_dl[kTabMax]; const float* f_wh[kTabMax]; const void* f_out[kTabMax]; size_t f_outs[kTabMax];
  const void* f_in[kTabMax]; size_t f_ins[kTabMax]; const float* f_W[kTabMax]; int f_Ci[kTabMax]; const float* f_rstd[kTabMax];
  const float* f_gamma[kTabMax]; int f_C[kTabMax]; float* f_dg[kTabMax]; const void* f_dYn[kTabMax]; size_t f_dyns[kTabMax];
  const float* f_Wn[kTabMax]; int f_Cn[kTabMax];
  int nfix = 0;
  const void* t_dY[kTabMax]; size_t t_dys[kTabMax]; int t_Co[kTabMax]; const void* t_X[kTabMax]; size_t t_xs[kTabMax]; int t_K[kTabMax];
  int t_sl[kTabMax]; float* t_part[kTabMax];
  int ntn = 0;
  float* dA = reinterpret_cast<float*>(ws + L.dA);
  bool pending = false;  // dY / dg / db of the current layer already written by the fused data gradient of the layer above
  Plan up{true, 1};      // how the data gradient above this layer left dA (fused = false: `S` partials in dA)
  for (int l = n - 1; l >= 0; --l) {
    const int C = D.Co[l], K = D.K[l];
    const void* a_out = sv + S.act[l + 1];
    const void* a_in = sv + S.act[l];
    const float* rstd = reinterpret_cast<const float*>(sv + S.rstd[l]);
    char* dY = ws + L.dY[l];
    float* dg = reinterpret_cast<float*>(ws + L.dg[l]);
    float* db = reinterpret_cast<float*>(ws + L.db[l]);
    const bool under_head = (l == n - 1);
    if (!pending) {
      const float* up_dA = under_head ? nullptr : dA;
      const float* up_dl = under_head ? g_logits : nullptr;
      const float* up_wh = under_head ? w_head : nullptr;
      if (under_head && D.fusable) {
        EST_TRY(dfepe_est_in_bwd(nullptr, up_dl, up_wh, a_out, (size_t)cols * C, rstd, gamma[l], beta[l], slope, C, (int)cols, dY, (size_t)cols * C, dg,
                                 db, stream));
      } else if (D.resident) {
        EST_TRY(dfepe_est_in_bwd_r(up_dA, C, up.S, (size_t)cols * C, up_dl, up_wh, a_out, (size_t)cols * C, rstd, gamma[l], beta[l], slope, C, B, N, dY,
                                   (size_t)cols * C, dg, db, stream));
      } else {
        const int sp = row_splits(B, C, N);
        EST_TRY(dfepe_est_in_bwd_n(up_dA, up_dl, up_wh, a_out, (size_t)cols * C, rstd, gamma[l], beta[l], slope, C, B, N, dY, (size_t)cols * C, dg, db,
                                   sp, sp > 1 ? reinterpret_cast<float*>(ws + L.npart) : nullptr, stream));
      }
    }
    if (N <= kFixMaxN) {
      // the upstream gradient of the fix: the head's rank-one form, else recomputed for the channel from dY of the layer above (alive in
      // both layouts until the layer below has been written) -- dA is transient (split-K partials, one buffer for all layers) or never existed
      const int i = nfix;
      f_dA[i] = nullptr; f_dl[i] = under_head ? g_logits : nullptr; f_wh[i] = under_head ? w_head : nullptr;
      f_out[i] = a_out; f_outs[i] = (size_t)cols * C; f_in[i] = a_in; f_ins[i] = (size_t)cols * K; f_W[i] = W[l]; f_Ci[i] = D.Ci[l];
      f_rstd[i] = rstd; f_gamma[i] = gamma[l]; f_C[i] = C; f_dg[i] = dg;
      f_dYn[i] = under_head ? nullptr : ws + L.dY[l + 1]; f_dyns[i] = under_head ? 0 : (size_t)cols * D.Co[l + 1];
      f_Wn[i] = under_head ? nullptr : W[l + 1]; f_Cn[i] = under_head ? 0 : D.Co[l + 1];
      if (L.keep_all) ++nfix;
      else
        EST_TRY(dfepe_est_dgamma_zero(nullptr, f_dl[i], f_wh[i], f_out[i], f_outs[i], f_in[i], f_ins[i], f_W[i], f_Ci[i], f_Ci[i], f_rstd[i],
                                      f_gamma[i], slope, C, N, B, dg, f_dYn[i], f_dyns[i], f_Wn[i], C, f_Cn[i], stream));
    }
    pending = false;
    // dW = dY^T X
    float* partw = reinterpret_cast<float*>(ws + L.partw[l]);
    if (L.keep_all) {
      t_dY[ntn] = dY; t_dys[ntn] = (size_t)cols * C; t_Co[ntn] = C; t_X[ntn] = a_in; t_xs[ntn] = (size_t)cols * K; t_K[ntn] = K; t_sl[ntn] = L.slices[l];
      t_part[ntn] = partw; ++ntn;
    } else {
      EST_TRY(dfepe_est_gemm_tn(dY, (size_t)cols * C, C, a_in, (size_t)cols * K, K, (int)cols, L.slices[l], partw, stream));
    }
    if (nseg + 4 > kSegMax) EST_TRY(flush());  // (never with <= 8 layers: kSegMax >= 2 + 4 kTabMax; a flush before the fixes at the end
                                               // would sum uncorrected d gamma partials)
    seg(dg, (int)B, C, g_gamma[l]);
    seg(db, (int)B, C, g_beta[l]);
    if (K == D.Ci[l]) seg(partw, L.slices[l], C * K, g_W[l]);
    else seg(partw, L.slices[l], C * K, g_W[l], K, D.Ci[l]);  // the first layer: its K - C0 zero-padded input channels dropped
    seg(nullptr, 0, C, g_bias[l]);
    if (l > 0 || need_gx) {
      const void* WT = pp ? static_cast<const void*>(pp + P.wt[l]) : static_cast<const void*>(sv + S.wt[l]);
      if (l == 0) {
        EST_TRY(dfepe_est_gemm_nt_gx(WT, (size_t)K * C, dY, (size_t)cols * C, K, (int)cols, C, gx, C0, N, gx_stride_b, gx_stride_c, stream));
      } else {
        up = dgrad_plan(D, l);
        if (up.fused) {
          EST_TRY(dfepe_est_dgrad_in_bwd(WT, (size_t)K * C, dY, (size_t)cols * C, K, (int)cols, C, a_in, (size_t)cols * K,
                                         reinterpret_cast<const float*>(sv + S.rstd[l - 1]), gamma[l - 1], beta[l - 1], slope, ws + L.dY[l - 1],
                                         (size_t)cols * K, reinterpret_cast<float*>(ws + L.dg[l - 1]), reinterpret_cast<float*>(ws + L.db[l - 1]),
                                         stream));
          pending = true;
        } else {
          EST_TRY(dfepe_est_gemm_nt_splitk(WT, (size_t)K * C, dY, (size_t)cols * C, K, (int)cols, C, dA, K, up.S, (size_t)cols * K, stream));
        }
      }
    }
  }
  if (ntn > 0) EST_TRY(dfepe_est_gemm_tn_multi(ntn, t_dY, t_dys, t_Co, t_X, t_xs, t_K, (int)cols, t_sl, t_part, stream));
  if (nfix > 0)
    EST_TRY(dfepe_est_dgamma_zero_multi(nfix, f_dA, f_dl, f_wh, f_out, f_outs, f_in, f_ins, f_W, f_Ci, f_rstd, f_gamma, f_C, f_dg, f_dYn, f_dyns, f_Wn,
                                        f_Cn, slope, N, B, stream));
  return flush();
}
