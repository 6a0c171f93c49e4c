// sp_process -- the SuperPoint output processing of the reference's end-to-end training path, process_SP_output
// (deepFEPE/train_good_utils.py:727-755), batched over images.  The per-lane arithmetic is in sp_process_math.h (shared with the
// host emulation of the tests); the contract is in include/dfepe.h.  The methods restated belong to the superpoint package, which
// the reference's tree does not hold: published algorithm, unpinned.  Nothing is atomic, every cell has one writer and every sum a
// fixed order, so two calls on the same input are bit-identical.  The launches:
//   flatten        one lane per 8x8 cell: softmax over its 65 channels in fp64 (three passes over the logits, no array), the 64
//                  detection probabilities written as eight rows of two float4.  flatten_bwd: the same lane layout, the adjoint.
//   nms            one 1024-lane workgroup per image runs the greedy loop as a fixpoint (below) until a workgroup-wide test finds
//                  no undecided candidate, removes the border, and compacts the kept points in row-major order (ballot prefix
//                  per wave, wave totals in LDS).  Heat and state live in LDS up to sp::kLdsPixels pixels, else the heat is read
//                  from the heatmap, the state kept in the caller's workspace, and kNmsWideRounds rounds with one lane per pixel
//                  over the whole device come first: the workgroup then only walks the list of what they left undecided.
//   soft_argmax    one lane per listed point, two sweeps over its patch in fp64.
//   soft_argmax_bwd  records: one lane per listed point recomputes its patch, stores what the adjoint needs and its list position
//                  in a dense index map; gather: one lane per pixel sums, in window order, what each point whose patch covers it
//                  sends.
//   sample_desc    one wavefront per listed point, lanes over the D channels: four taps, the squared norm by a DPP wave sum.
#include "dfepe_common.h"
#include "sp_process_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kNmsThreads = 1024;

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- flattenDetection ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) sp_flatten_kernel(const float* __restrict__ semi, int B, int Hc, int Wc,
                                                              float* __restrict__ heatmap) {
  const long cells = (long)Hc * Wc;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (long)B * cells) return;
  const long b = t / cells, rem = t - b * cells;
  const int hc = (int)(rem / Wc), wc = (int)(rem - (long)hc * Wc);
  const float* v = semi + b * sp::kChannels * cells + rem;
  const double m = sp::cell_max(v, cells), s = sp::cell_sum(v, cells, m);
  const long W = (long)Wc * sp::kCell;
  float* out = heatmap + b * cells * 64 + (long)hc * sp::kCell * W + (long)wc * sp::kCell;
  for (int r = 0; r < sp::kCell; ++r) {
    float p[sp::kCell];
#pragma unroll
    for (int c = 0; c < sp::kCell; ++c) p[c] = (float)sp::cell_prob(v[(r * sp::kCell + c) * cells], m, s);
    float4* row = reinterpret_cast<float4*>(out + r * W);  // W and the cell's column are multiples of 8: 32-byte aligned
    row[0] = make_float4(p[0], p[1], p[2], p[3]);
    row[1] = make_float4(p[4], p[5], p[6], p[7]);
  }
}

__global__ void __launch_bounds__(kThreads) sp_flatten_bwd_kernel(const float* __restrict__ semi, const float* __restrict__ g_heatmap,
                                                                  int B, int Hc, int Wc, float* __restrict__ g_semi) {
  const long cells = (long)Hc * Wc;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (long)B * cells) return;
  const long b = t / cells, rem = t - b * cells;
  const int hc = (int)(rem / Wc), wc = (int)(rem - (long)hc * Wc);
  const float* v = semi + b * sp::kChannels * cells + rem;
  float* gs = g_semi + b * sp::kChannels * cells + rem;
  const double m = sp::cell_max(v, cells), s = sp::cell_sum(v, cells, m);
  const long W = (long)Wc * sp::kCell;
  const float* g = g_heatmap + b * cells * 64 + (long)hc * sp::kCell * W + (long)wc * sp::kCell;
  const double dot = sp::cell_dot(v, cells, m, s, g, W);
  for (int c = 0; c < sp::kChannels; ++c) {
    const float vc = v[c * cells];
    const double gc = (c < 64) ? (double)g[(c / sp::kCell) * W + (c % sp::kCell)] : 0.0;
    // a NaN logit was replaced by the constant 0: nothing flows back to it
    gs[c * cells] = (vc != vc) ? 0.0f : (float)(sp::cell_prob(vc, m, s) * (gc - dot));
  }
}

// ---- nms_fast as a fixpoint ----------------------------------------------------------------------------------------------
// Above sp::kLdsPixels the state lives in the workspace, and the first rounds run over the whole device, one lane per pixel
// (round 0 fills the state): one CU alone would wait on its own loads.  A round may read a state that another lane is deciding;
// a decided state is final and is the greedy loop's decision, so either value gives the same fixpoint.  What these rounds leave
// undecided (the long chains), the one-workgroup kernel below finishes, without a round limit.
constexpr int kNmsWideRounds = 4;
__global__ void __launch_bounds__(kThreads) sp_nms_wide_round_kernel(const float* __restrict__ heatmap, int H, int W, float conf_thresh,
                                                                     int d, int round, unsigned char* ws_state) {
  const int n = H * W;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float* heat = heatmap + (size_t)blockIdx.y * n;
  unsigned char* state = ws_state + (size_t)blockIdx.y * n;
  if (round == 0) {
    state[i] = sp::candidate(heat[i], conf_thresh) ? sp::kUndecided : sp::kNone;
    return;
  }
  if (state[i] != sp::kUndecided) return;
  const int y = i / W, x = i - y * W;
  const sp::State s = sp::decide_pixel(heat, state, H, W, d, y, x);
  if (s != sp::kUndecided) state[i] = s;
}

template <bool LDS>
__global__ void __launch_bounds__(kNmsThreads) sp_nms_kernel(const float* __restrict__ heatmap, int H, int W, float conf_thresh, int d,
                                                             int r, unsigned char* ws_state, int* ws_list, int cap,
                                                             float* __restrict__ nms_map, int* __restrict__ pts, float* __restrict__ conf,
                                                             int* __restrict__ count) {
  __shared__ float lheat[LDS ? sp::kLdsPixels : 1];
  __shared__ unsigned char lstate[LDS ? sp::kLdsPixels : 16];
  __shared__ int wsum[kNmsThreads / WAVE];
  __shared__ int any_pending;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = H * W;
  const float* gheat = heatmap + (size_t)b * n;
  const float* heat = LDS ? lheat : gheat;
  unsigned char* state = LDS ? lstate : ws_state + (size_t)b * n;
  int* list = LDS ? nullptr : ws_list + (size_t)b * n;  // the pixels that the device-wide rounds left undecided
  int n_work = n;
  if (LDS) {
    for (int i = tid; i < n; i += kNmsThreads) {
      const float h = gheat[i];
      lheat[i] = h;
      state[i] = sp::candidate(h, conf_thresh) ? sp::kUndecided : sp::kNone;
    }
  } else {
    n_work = 0;
    for (int i0 = 0; i0 < n; i0 += kNmsThreads) {
      const int i = i0 + tid;
      const bool open = i < n && state[i] == sp::kUndecided;
      const int k = compact_slot<kNmsThreads / WAVE>(open, wsum, n_work);
      if (open) list[k] = i;
    }
  }
  for (;;) {  // no round count: it ends when a round leaves nothing undecided, and every round decides at least one candidate
    __syncthreads();  // the states of the last round (or the fill) are visible; every lane has read any_pending
    if (tid == 0) any_pending = 0;
    __syncthreads();
    bool pending = false;
    for (int k = tid; k < n_work; k += kNmsThreads) {
      const int i = LDS ? k : list[k];
      if (state[i] != sp::kUndecided) continue;
      const int y = i / W, x = i - y * W;
      const sp::State s = sp::decide_pixel(heat, state, H, W, d, y, x);
      if (s != sp::kUndecided) state[i] = s;
      else pending = true;
    }
    if (pending) any_pending = 1;
    __syncthreads();
    if (any_pending == 0) break;  // the same value in every lane: the barrier above stands between the writes and this read
  }
  // border removal and the compact list, in row-major order
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += kNmsThreads) {
    const int i = i0 + tid;
    bool keep = false;
    int y = 0, x = 0;
    if (i < n) {
      y = i / W;
      x = i - y * W;
      keep = state[i] == sp::kKept && sp::inside_border(y, x, H, W, r);
      nms_map[(size_t)b * n + i] = keep ? 1.0f : 0.0f;
    }
    const int k = compact_slot<kNmsThreads / WAVE>(keep, wsum, base);
    if (keep && k < cap) {  // k < cap always (two kept points never share a (d+1) x (d+1) block); the test keeps a wrong cap harmless
      const size_t p = (size_t)b * cap + k;
      pts[2 * p] = x;
      pts[2 * p + 1] = y;
      conf[p] = heat[i];
    }
  }
  base = base < cap ? base : cap;
  for (int k = base + tid; k < cap; k += kNmsThreads) {
    const size_t p = (size_t)b * cap + k;
    pts[2 * p] = 0;
    pts[2 * p + 1] = 0;
    conf[p] = 0.0f;
  }
  if (tid == 0) count[b] = base;
}

// ---- pred_soft_argmax ------------------------------------------------------------------------------------------------
__device__ inline bool patch_inside(int x, int y, int H, int W, int p) {
  const int c = p / 2;
  return x >= c && y >= c && x < W - c && y < H - c;
}

__global__ void __launch_bounds__(kThreads) sp_soft_argmax_kernel(const float* __restrict__ heatmap, const int* __restrict__ pts,
                                                                  const int* __restrict__ count, int B, int H, int W, int cap, int p,
                                                                  float* __restrict__ pred, float* __restrict__ patches) {
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (long)B * cap) return;
  const long b = t / cap;
  const int k = (int)(t - b * cap);
  const int n = clampi(count[b], 0, cap);
  float ox = 0.0f, oy = 0.0f;
  const int x = pts[2 * t], y = pts[2 * t + 1];
  const bool live = k < n && patch_inside(x, y, H, W, p);  // a listed point of dfepe_sp_nms with p <= 2r + 1 always is
  const float* h = heatmap + (size_t)b * H * W;
  sp::Patch r = {};
  if (live) {
    r = sp::soft_argmax(h, W, x, y, p);
    if (r.valid) {
      ox = (float)(r.ox - (double)(p / 2));
      oy = (float)(r.oy - (double)(p / 2));
    }
  }
  pred[2 * t] = ox;
  pred[2 * t + 1] = oy;
  if (patches != nullptr) {
    float* q = patches + (size_t)t * p * p;
    const int c = p / 2;
    for (int j = 0; j < p; ++j)
      for (int i = 0; i < p; ++i)
        q[j * p + i] = live ? (float)sp::clamp_q((double)h[(long)(y - c + j) * W + (x - c + i)] / r.denom) : 0.0f;
  }
}

struct Rec {  // what the gather needs of one listed point
  sp::Patch patch;
  double gx, gy, share;
};

__host__ __device__ inline size_t nms_state_bytes(int B, int H, int W) { return ((size_t)B * H * W + 15) / 16 * 16; }
__host__ __device__ inline size_t index_map_bytes(int B, int H, int W) { return (((size_t)B * H * W * sizeof(int)) + 15) / 16 * 16; }

__global__ void __launch_bounds__(kThreads) sp_soft_argmax_rec_kernel(const float* __restrict__ heatmap, const int* __restrict__ pts,
                                                                      const int* __restrict__ count, const float* __restrict__ g_pred,
                                                                      int B, int H, int W, int cap, int p, int* __restrict__ index_map,
                                                                      Rec* __restrict__ recs) {
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (long)B * cap) return;
  const long b = t / cap;
  const int k = (int)(t - b * cap);
  if (k >= clampi(count[b], 0, cap)) return;
  const int x = pts[2 * t], y = pts[2 * t + 1];
  if (!patch_inside(x, y, H, W, p)) return;
  const float* h = heatmap + (size_t)b * H * W;
  Rec rec;
  rec.patch = sp::soft_argmax(h, W, x, y, p);
  rec.gx = (double)g_pred[2 * t];
  rec.gy = (double)g_pred[2 * t + 1];
  rec.share = rec.patch.valid ? sp::grad_norm_share(rec.patch, h, W, x, y, p, rec.gx, rec.gy) : 0.0;
  recs[t] = rec;
  index_map[(size_t)b * H * W + (size_t)y * W + x] = k;  // the listed points of an image are distinct pixels: one writer
}

__global__ void __launch_bounds__(kThreads) sp_soft_argmax_gather_kernel(const float* __restrict__ heatmap, int B, int H, int W, int cap,
                                                                         int p, const int* __restrict__ index_map,
                                                                         const Rec* __restrict__ recs, float* __restrict__ g_heatmap) {
  const long n = (long)H * W;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (long)B * n) return;
  const long b = t / n, i = t - b * n;
  const int y = (int)(i / W), x = (int)(i - (long)y * W);
  const int c = p / 2;
  const double hv = (double)heatmap[t];
  const int* map = index_map + b * n;
  const int y0 = y - c < 0 ? 0 : y - c, y1 = y + c > H - 1 ? H - 1 : y + c;
  const int x0 = x - c < 0 ? 0 : x - c, x1 = x + c > W - 1 ? W - 1 : x + c;
  double acc = 0.0;
  for (int cy = y0; cy <= y1; ++cy)
    for (int cx = x0; cx <= x1; ++cx) {
      const int k = map[(long)cy * W + cx];
      if (k < 0) continue;
      const Rec& rec = recs[b * cap + k];
      if (!rec.patch.valid) continue;
      acc += sp::grad_h(rec.patch, hv, x - cx + c, y - cy + c, rec.gx, rec.gy, rec.share);
    }
  g_heatmap[t] = (float)acc;
}

// ---- sample_desc_from_points -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) sp_sample_desc_kernel(const float* __restrict__ desc, const int* __restrict__ pts,
                                                              const float* __restrict__ pred, const int* __restrict__ count, int D, int Hc,
                                                              int Wc, int cap, int align_corners, float* __restrict__ out) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const size_t b = blockIdx.y;
  const size_t t = b * cap + k;
  float* o = out + t * D;
  if (k >= clampi(count[b], 0, cap)) {  // uniform over the wavefront
    for (int ch = lane; ch < D; ch += WAVE) o[ch] = 0.0f;
    return;
  }
  double x = (double)pts[2 * t], y = (double)pts[2 * t + 1];
  if (pred != nullptr) {
    x += (double)pred[2 * t];
    y += (double)pred[2 * t + 1];
  }
  const sp::Taps taps = sp::bilinear_taps(x, y, Hc, Wc, align_corners);
  const size_t plane = (size_t)Hc * Wc;
  const float* base = desc + b * D * plane;
  double ss = 0.0;
  for (int ch = lane; ch < D; ch += WAVE) {
    const double v = sp::sample(base + ch * plane, Hc, Wc, taps);
    ss += v * v;
  }
  const double norm = sqrt(wave_sum(ss));  // every lane of the wavefront is here
  for (int ch = lane; ch < D; ch += WAVE) {
    const double v = sp::sample(base + ch * plane, Hc, Wc, taps);
    o[ch] = (norm > 0.0) ? (float)(v / norm) : 0.0f;
  }
}

}  // namespace

extern "C" int dfepe_sp_nms_capacity(int H, int W, int nms_dist) {
  if (H <= 0 || W <= 0 || nms_dist < 0 || (long)H * W > sp::kMaxPixels) return 0;
  return (int)sp::nms_capacity(H, W, nms_dist);
}

extern "C" size_t dfepe_sp_nms_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (long)H * W > sp::kMaxPixels) return 0;
  if ((long)H * W <= sp::kLdsPixels) return 0;
  return nms_state_bytes(B, H, W) + (size_t)B * H * W * sizeof(int);  // a state byte per pixel, then the list of undecided pixels
}

extern "C" size_t dfepe_sp_soft_argmax_bwd_workspace_bytes(int B, int H, int W, int cap) {
  if (B <= 0 || H <= 0 || W <= 0 || cap < 0 || (long)H * W > sp::kMaxPixels) return 0;
  return index_map_bytes(B, H, W) + (size_t)B * cap * sizeof(Rec);
}

static int flatten_args(int B, int H, int W) {
  if (B < 0 || H <= 0 || W <= 0 || H % sp::kCell != 0 || W % sp::kCell != 0) return DFEPE_ERR_INVALID_ARG;
  if ((long)H * W > sp::kMaxPixels || (long)B * (H / sp::kCell) * (W / sp::kCell) > 0x7fffffffL) return DFEPE_ERR_UNSUPPORTED;
  return DFEPE_OK;
}

extern "C" int dfepe_sp_flatten(const float* semi, int B, int H, int W, float* heatmap, void* stream) {
  const int rc = flatten_args(B, H, W);
  if (rc != DFEPE_OK) return rc;
  if (B == 0) return DFEPE_OK;
  if (!semi || !heatmap || !aligned16(heatmap)) return DFEPE_ERR_INVALID_ARG;
  const int Hc = H / sp::kCell, Wc = W / sp::kCell;
  const long cells = (long)B * Hc * Wc;
  hipLaunchKernelGGL(sp_flatten_kernel, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), semi, B, Hc, Wc, heatmap);
  return launched();
}

extern "C" int dfepe_sp_flatten_bwd(const float* semi, const float* g_heatmap, int B, int H, int W, float* g_semi, void* stream) {
  const int rc = flatten_args(B, H, W);
  if (rc != DFEPE_OK) return rc;
  if (B == 0) return DFEPE_OK;
  if (!semi || !g_heatmap || !g_semi) return DFEPE_ERR_INVALID_ARG;
  const int Hc = H / sp::kCell, Wc = W / sp::kCell;
  const long cells = (long)B * Hc * Wc;
  hipLaunchKernelGGL(sp_flatten_bwd_kernel, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), semi, g_heatmap, B, Hc, Wc, g_semi);
  return launched();
}

extern "C" int dfepe_sp_nms(const float* heatmap, int B, int H, int W, float conf_thresh, int nms_dist, int border_remove, void* workspace,
                            float* nms_map, int* pts, float* conf, int* count, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || nms_dist < 0 || border_remove < 0) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if ((long)H * W > sp::kMaxPixels || B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  if (!heatmap || !nms_map || !pts || !conf || !count) return DFEPE_ERR_INVALID_ARG;
  const bool lds = (long)H * W <= sp::kLdsPixels;
  if (!lds && !workspace) return DFEPE_ERR_INVALID_ARG;
  const int cap = (int)sp::nms_capacity(H, W, nms_dist);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (lds) {
    hipLaunchKernelGGL(sp_nms_kernel<true>, dim3(B), dim3(kNmsThreads), 0, s, heatmap, H, W, conf_thresh, nms_dist, border_remove,
                       static_cast<unsigned char*>(nullptr), static_cast<int*>(nullptr), cap, nms_map, pts, conf, count);
    return launched();
  }
  unsigned char* state = static_cast<unsigned char*>(workspace);
  int* list = reinterpret_cast<int*>(state + nms_state_bytes(B, H, W));
  const unsigned blocks = (unsigned)(((long)H * W + kThreads - 1) / kThreads);
  for (int round = 0; round <= kNmsWideRounds; ++round)
    hipLaunchKernelGGL(sp_nms_wide_round_kernel, dim3(blocks, B), dim3(kThreads), 0, s, heatmap, H, W, conf_thresh, nms_dist, round, state);
  hipLaunchKernelGGL(sp_nms_kernel<false>, dim3(B), dim3(kNmsThreads), 0, s, heatmap, H, W, conf_thresh, nms_dist, border_remove, state, list,
                     cap, nms_map, pts, conf, count);
  return launched();
}

static int soft_argmax_args(int B, int H, int W, int cap, int p, int r) {
  if (B < 0 || H <= 0 || W <= 0 || cap < 0 || r < 0) return DFEPE_ERR_INVALID_ARG;
  if (p < 1 || p % 2 == 0 || (long)p > 2L * r + 1) return DFEPE_ERR_INVALID_ARG;
  if ((long)H * W > sp::kMaxPixels || p > sp::kMaxPatch || (long)B * cap > 0x7fffffffL) return DFEPE_ERR_UNSUPPORTED;
  return DFEPE_OK;
}

extern "C" int dfepe_sp_soft_argmax(const float* heatmap, const int* pts, const int* count, int B, int H, int W, int cap, int patch_size,
                                    int border_remove, float* pred, float* patches, void* stream) {
  const int rc = soft_argmax_args(B, H, W, cap, patch_size, border_remove);
  if (rc != DFEPE_OK) return rc;
  if (B == 0 || cap == 0) return DFEPE_OK;
  if (!heatmap || !pts || !count || !pred) return DFEPE_ERR_INVALID_ARG;
  const long n = (long)B * cap;
  hipLaunchKernelGGL(sp_soft_argmax_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), heatmap, pts, count, B, H, W, cap, patch_size, pred, patches);
  return launched();
}

extern "C" int dfepe_sp_soft_argmax_bwd(const float* heatmap, const int* pts, const int* count, const float* g_pred, int B, int H, int W,
                                        int cap, int patch_size, int border_remove, void* workspace, float* g_heatmap, void* stream) {
  const int rc = soft_argmax_args(B, H, W, cap, patch_size, border_remove);
  if (rc != DFEPE_OK) return rc;
  if (B == 0) return DFEPE_OK;
  if (!heatmap || !g_heatmap || !workspace || !aligned16(workspace)) return DFEPE_ERR_INVALID_ARG;
  if (cap > 0 && (!pts || !count || !g_pred)) return DFEPE_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* index_map = static_cast<int*>(workspace);
  Rec* recs = reinterpret_cast<Rec*>(static_cast<unsigned char*>(workspace) + index_map_bytes(B, H, W));
  if (hipMemsetAsync(index_map, 0xff, index_map_bytes(B, H, W), s) != hipSuccess) return DFEPE_ERR_HIP;
  const long n = (long)B * cap, px = (long)B * H * W;
  if (n > 0)
    hipLaunchKernelGGL(sp_soft_argmax_rec_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, heatmap, pts, count,
                       g_pred, B, H, W, cap, patch_size, index_map, recs);
  hipLaunchKernelGGL(sp_soft_argmax_gather_kernel, dim3((unsigned)((px + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, heatmap, B, H, W,
                     cap, patch_size, index_map, recs, g_heatmap);
  return launched();
}

extern "C" int dfepe_sp_sample_desc(const float* desc, const int* pts, const float* pred, const int* count, int B, int D, int H, int W,
                                    int cap, int align_corners, float* out, void* stream) {
  if (B < 0 || D <= 0 || H <= 0 || W <= 0 || H % sp::kCell != 0 || W % sp::kCell != 0 || cap < 0) return DFEPE_ERR_INVALID_ARG;
  if (align_corners != 0 && align_corners != 1) return DFEPE_ERR_INVALID_ARG;
  if (B == 0 || cap == 0) return DFEPE_OK;
  if ((long)H * W > sp::kMaxPixels || B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  if (!desc || !pts || !count || !out) return DFEPE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(sp_sample_desc_kernel, dim3(cap, B), dim3(WAVE), 0, static_cast<hipStream_t>(stream), desc, pts, pred, count, D,
                     H / sp::kCell, W / sp::kCell, cap, align_corners, out);
  return launched();
}
