// w8pt16 -- the row-per-pair kernels of the weighted 8-point fit: launchers.
//
// Grid: one 256-thread workgroup = 16 pairs (4 wavefronts x 4 rows).  B = 4096 pairs -> 256 workgroups = one per CU,
// one wavefront per SIMD; larger batches stack more wavefronts per SIMD.  No block-level barrier; each pair owns 36
// doubles of LDS for one exchange.  Bodies: w8pt16_body.h (forward), w8pt16_bwd_body.h (adjoint).
#include "dfepe_common.h"
#include "fit_plan.h"
#include "w8pt16_body.h"
#include "w8pt16_bwd_body.h"
#include "loss_head_body.h"
#include <cstdlib>

#include "cheirality_body.h"

namespace {

constexpr int kPairsPerBlock = 16;
// A/B switches of the environment (measurement only): read once by their callers, handed to the plan functions of fit_plan.h
int env_int(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }

// Kernel arguments (forward and backward alike): what a wavefront needs before it can issue its global loads comes first, as plain scalars / pointers --
// with -amdgpu-kernarg-preload-count=16 (build.py) the command processor hands those 16 dwords over in SGPRs at wave launch,
// so the loads do not wait for a scalar-cache miss on the kernarg segment first; the rest follows as a struct and is fetched
// in the shadow of the global loads.
struct W8FwdRest {
  float* epi_res;
  float* save;
  float* weights_out;
  int logits_mode;
  unsigned variant;
  double* hartley;  // the Hartley record and its mode (w8pt16_body.h): read by the *_shared kernels only, behind everything the others take
  int hartley_mode;
};
// (the Rest structs, their split and their fill live here and not beside W8Args / W8BwdArgs: only these kernels take them, and
// their unnamed-namespace type is part of the kernels' symbol names)
W8FwdRest rest_of(const W8Args& A) { return {A.epi_res, A.save, A.weights_out, A.logits_mode, A.variant, A.hartley, A.hartley_mode}; }
// ... and put together again in the kernel
__device__ __forceinline__ W8Args w8_args(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                                          float clamp_at, float* F_out, float* residual, const W8FwdRest& R) {
  W8Args A;
  A.pts1 = pts1; A.pts2 = pts2; A.wts = wts; A.B = B; A.Bm = Bm; A.N = N; A.hw_sx = hw_sx; A.hw_sy = hw_sy;
  A.clamp_at = clamp_at; A.F_out = F_out; A.residual = residual; A.epi_res = R.epi_res; A.save = R.save;
  A.weights_out = R.weights_out; A.logits_mode = R.logits_mode; A.variant = R.variant; A.row_per_pair = false;
  A.hartley = R.hartley; A.hartley_mode = R.hartley_mode;
  return A;
}

// Start offsets (round 6).  At 4096 pairs a CU holds ONE workgroup whose four wavefronts -- one per SIMD -- start in the same cycle and
// run the same straight-line instruction stream in lockstep, so they reach every shared unit of the CU (instruction fetch, the texture
// addresser with its loads and stores, the LDS exchange of the moments) in the same cycles.  Wavefront w waits w x DFEPE_*_STAGGER
// cycles first.  Measured on one box (scripts/ab_fit.sh, captured step at B = 4096, N = 100, ms): none 0.1058-0.1062; 8 / 16 cycles
// per wavefront 0.1029-0.1034; 32: 0.1041-0.1044; 64: 0.1034-0.1038; 128: 0.1034-0.1037; 192: 0.1041-0.1044; 512: 0.1051-0.1060 -- the
// gain is in not being aligned, more distance only delays the last wavefront.  Also measured and dropped: offsets between the
// workgroups of an XCD (+0.5 ... +1.5 us per step), repeating the offset at the phase boundaries of the body (+1.5 ... +6 us: the loop
// in the middle of the stream costs more than it spreads), the same on the loss tail's F-loss wavefronts (+-0).
#define DFEPE_STAGGER_WAIT(X)                                              \
  do {                                                                     \
    if constexpr ((X) >= 64) __builtin_amdgcn_s_sleep((X) / 64);           \
    else {                                                                 \
      if constexpr ((X) > 16) asm volatile("s_nop 15");                    \
      asm volatile("s_nop %0" ::"n"(((X) - 1) & 15));                      \
    }                                                                      \
  } while (0)
#ifndef DFEPE_PAIR2_STAGGER
#define DFEPE_PAIR2_STAGGER 16  // the N = 1000 fit with two rows per pair (two wavefronts per SIMD at 4096 pairs): wavefront w of a workgroup, and
                                // the workgroups a CU receives second (ids 256 apart), start 16 (w [+ 4]) cycles late: bench.py --config 5
                                // 0.1586-0.1588 -> 0.1561-0.1569 ms (same box, twice).  The same on the lean fit (config 4 as one 32768-pair
                                // batch: workgroups queue for the CUs, only the first wave of them starts together): +-0, not kept
#endif
#ifndef DFEPE_FWD_STAGGER
#define DFEPE_FWD_STAGGER 16  // cycles per wavefront index, forward fit (0: off)
#endif
#ifndef DFEPE_BWD_STAGGER
#define DFEPE_BWD_STAGGER 16  // ... backward fit
#endif
template <int IT, bool RAW, bool PLAIN>
__global__ void __launch_bounds__(256)
w8pt16_fwd_kernel(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                  float clamp_at, float* F_out, float* residual, const W8FwdRest R) {
  __shared__ double xch[kPairsPerBlock * 36];
  const int row = (int)(threadIdx.x >> 4);
  const int pair = (int)blockIdx.x * kPairsPerBlock + row;
  if (pair >= B) return;  // a whole row leaves; rows never wait for each other
#if DFEPE_FWD_STAGGER
  for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) DFEPE_STAGGER_WAIT(DFEPE_FWD_STAGGER);
#endif
  const W8Args A = w8_args(pts1, pts2, wts, B, Bm, N, hw_sx, hw_sy, clamp_at, F_out, residual, R);
  w8pt16_fwd_pair<IT, RAW, PLAIN>(A, pair, xch + row * 36);
}

// The same kernel in <= 256 registers (w8pt16_body.h: LEAN): two wavefronts per SIMD.  Taken from kLeanMinPairs pairs on, where a
// SIMD has wavefronts queueing for it (at 4096 pairs = one wavefront per SIMD the few extra instructions would only cost).
template <int IT, bool RAW, bool PLAIN>
__global__ void __launch_bounds__(256, 2)
w8pt16_fwd_lean_kernel(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                       float clamp_at, float* F_out, float* residual, const W8FwdRest R) {
  __shared__ double xch[kPairsPerBlock * 36];
  const int row = (int)(threadIdx.x >> 4);
  const int pair = (int)blockIdx.x * kPairsPerBlock + row;
  if (pair >= B) return;
  const W8Args A = w8_args(pts1, pts2, wts, B, Bm, N, hw_sx, hw_sy, clamp_at, F_out, residual, R);
  w8pt16_fwd_pair<IT, RAW, PLAIN, 1, true>(A, pair, xch + row * 36);
}

// The two kernels above with the Hartley record (w8pt16_body.h: HM = H16_BY_LAUNCH): layer 1 of a step that fits the same matches at
// every layer writes the transforms, layers 2..L read them.  Kernels of their own, so that a launch without a record runs the very
// code it ran before the record existed; ONE kernel for the writer and its readers, so that the readers find its code in the cache.
template <int IT, bool RAW, bool PLAIN>
__global__ void __launch_bounds__(256)
w8pt16_fwd_shared_kernel(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                         float clamp_at, float* F_out, float* residual, const W8FwdRest R) {
  __shared__ double xch[kPairsPerBlock * 36];
  const int row = (int)(threadIdx.x >> 4);
  const int pair = (int)blockIdx.x * kPairsPerBlock + row;
  if (pair >= B) return;
#if DFEPE_FWD_STAGGER
  for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) DFEPE_STAGGER_WAIT(DFEPE_FWD_STAGGER);
#endif
  const W8Args A = w8_args(pts1, pts2, wts, B, Bm, N, hw_sx, hw_sy, clamp_at, F_out, residual, R);
  w8pt16_fwd_pair<IT, RAW, PLAIN, 1, false, H16_BY_LAUNCH>(A, pair, xch + row * 36);
}
template <int IT, bool RAW, bool PLAIN>
__global__ void __launch_bounds__(256, 2)
w8pt16_fwd_lean_shared_kernel(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                              float clamp_at, float* F_out, float* residual, const W8FwdRest R) {
  __shared__ double xch[kPairsPerBlock * 36];
  const int row = (int)(threadIdx.x >> 4);
  const int pair = (int)blockIdx.x * kPairsPerBlock + row;
  if (pair >= B) return;
  const W8Args A = w8_args(pts1, pts2, wts, B, Bm, N, hw_sx, hw_sy, clamp_at, F_out, residual, R);
  w8pt16_fwd_pair<IT, RAW, PLAIN, 1, true, H16_BY_LAUNCH>(A, pair, xch + row * 36);
}

// N > 128 at a few thousand pairs: TWO rows of a wavefront per pair (w8pt16_body.h: ROWS = 2).  One row per pair is one wavefront per
// SIMD at 4096 pairs -- a lone in-order stream of 21 000 instructions at N = 1000 --; with two rows a pair's correspondences are
// walked by 32 lanes (half the per-correspondence instructions per wavefront), the eigen phases run once per wavefront as before,
// and the 2048 wavefronts are two per SIMD (236 registers) that fill each other's issue bubbles.
constexpr int kPairsPerBlock2 = 8;
template <bool RAW, bool PLAIN>
__global__ void __launch_bounds__(256, 2)  // instantiated for pixel matches only
w8pt16_pair2_fwd_kernel(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                        float clamp_at, float* F_out, float* residual, const W8FwdRest R) {
  __shared__ double xch[kPairsPerBlock2 * 36];
  const int prow = (int)(threadIdx.x >> 5);  // pair within the workgroup
  const int pair = (int)blockIdx.x * kPairsPerBlock2 + prow;
  if (pair >= B) return;  // both rows of a pair leave together
#if DFEPE_PAIR2_STAGGER
  for (int k = 0; k < (int)(threadIdx.x >> 6) + 4 * (int)((blockIdx.x >> 8) & 1u); ++k) DFEPE_STAGGER_WAIT(DFEPE_PAIR2_STAGGER);
#endif
  const W8Args A = w8_args(pts1, pts2, wts, B, Bm, N, hw_sx, hw_sy, clamp_at, F_out, residual, R);
  w8pt16_fwd_pair<0, RAW, PLAIN, 2>(A, pair, xch + prow * 36, nullptr, (int)(threadIdx.x >> 4) & 1);
}

// Cooperative variant: one 256-thread workgroup (16 rows) per pair, for N > 128 (w8pt16_body.h: W8Coop).
template <int IT, bool RAW, bool PLAIN>
__global__ void __launch_bounds__(256, (IT <= 4 ? 2 : 1))  // two workgroups per CU (<= 256 registers) while the correspondences allow it
w8pt16_coop_fwd_kernel(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                       float clamp_at, float* F_out, float* residual, const W8FwdRest R) {
  __shared__ W8Coop co;
  const int pair = (int)blockIdx.x;
  const W8Args A = w8_args(pts1, pts2, wts, B, Bm, N, hw_sx, hw_sy, clamp_at, F_out, residual, R);
  w8pt16_fwd_pair<IT, RAW, PLAIN, 16>(A, pair, nullptr, &co, (int)(threadIdx.x >> 4));
}

// Fit + E-from-F + cheirality-checked pose of one pair in ONE launch (BASELINE config 5 at small batch): the cooperative fit, then
// the same workgroup decomposes pre^T F pre and triangulates its pair's correspondences (cheirality_body.h) -- no second launch,
// no second ramp, F never leaves the CU.
struct W8PoseRest {
  const float* pre;
  const float* K;
  float depth_thres;
  float* Rt_cam;
  int* winner;
  int* counts;
};
template <int IT>
__global__ void __launch_bounds__(256, (IT <= 4 ? 2 : 1))
w8pt16_coop_pose_kernel(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                        float clamp_at, float* F_out, float* residual, const W8FwdRest R, const W8PoseRest P) {
  __shared__ W8Coop co;
  __shared__ CheirLds cl;
  const int pair = (int)blockIdx.x;
  const W8Args A = w8_args(pts1, pts2, wts, B, Bm, N, hw_sx, hw_sy, clamp_at, F_out, residual, R);
  w8pt16_fwd_pair<IT, true, true, 16>(A, pair, nullptr, &co, (int)(threadIdx.x >> 4));
  float Ef[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Ef[k] = co.of[k];  // published by row 0 before the output phase: every thread has passed that barrier
  cheirality_pair(Ef, P.pre, P.K, pts1, (size_t)pair, N, P.depth_thres, P.Rt_cam, P.winner, P.counts, cl);
}

struct W8BwdRest {
  const float* F_out;
  const float* g_F;
  const float* g_res;
  const float* g_epi;
  const float* g_w_extra;
  const float* g_scale;
  float* g_w;
  float* g_p1;
  float* g_p2;
  int logits_mode;
  unsigned variant;
};
W8BwdRest rest_of(const W8BwdArgs& A) {
  return {A.F_out, A.g_F, A.g_res, A.g_epi, A.g_w_extra, A.g_scale, A.g_w, A.g_p1, A.g_p2, A.logits_mode, A.variant};
}
__device__ __forceinline__ W8BwdArgs w8_bwd_args(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx,
                                                 float hw_sy, float clamp_at, const float* save, const W8BwdRest& R) {
  W8BwdArgs A;
  A.pts1 = pts1; A.pts2 = pts2; A.wts = wts; A.B = B; A.Bm = Bm; A.N = N; A.hw_sx = hw_sx; A.hw_sy = hw_sy;
  A.clamp_at = clamp_at; A.save = save; A.F_out = R.F_out; A.g_F = R.g_F; A.g_res = R.g_res; A.g_epi = R.g_epi;
  A.g_w_extra = R.g_w_extra; A.g_scale = R.g_scale; A.g_w = R.g_w; A.g_p1 = R.g_p1; A.g_p2 = R.g_p2;
  A.logits_mode = R.logits_mode; A.variant = R.variant; A.pending_head = nullptr; A.row_per_pair = false;
  return A;
}

template <int IT, bool RAW, bool PGRAD, bool PLAIN, bool UP = true>
__global__ void __launch_bounds__(256)
w8pt16_bwd_kernel(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                  float clamp_at, const float* save, const W8BwdRest R) {
  const int row = (int)(threadIdx.x >> 4);
  const int pair = (int)blockIdx.x * kPairsPerBlock + row;
  if (pair >= B) return;
#if DFEPE_BWD_STAGGER
  for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) DFEPE_STAGGER_WAIT(DFEPE_BWD_STAGGER);
#endif
  const W8BwdArgs A = w8_bwd_args(pts1, pts2, wts, B, Bm, N, hw_sx, hw_sy, clamp_at, save, R);
  w8pt16_bwd_pair_impl<IT, RAW, PGRAD, PLAIN, 1, UP>(A, pair, nullptr);
}

template <int IT, bool RAW>
__global__ void __launch_bounds__(256, (IT <= 4 ? 2 : 1))
w8pt16_coop_bwd_kernel(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                       float clamp_at, const float* save, const W8BwdRest R) {
  __shared__ W8BwdCoop co;
  const int pair = (int)blockIdx.x;
  const W8BwdArgs A = w8_bwd_args(pts1, pts2, wts, B, Bm, N, hw_sx, hw_sy, clamp_at, save, R);
  w8pt16_bwd_pair_impl<IT, RAW, false, true, 16>(A, pair, nullptr, &co, (int)(threadIdx.x >> 4));
}

// The same backward fit with three more wavefronts per workgroup; in workgroup 0 they run the loss head that dfepe_loss_tail
// deferred (loss_head_body.h: one wavefront per kind of partial), elsewhere they leave at once.  The head is off the step's
// critical path this way: nothing in the backward needs its scalars; the 448-thread workgroup (two wavefronts on three of the
// SIMDs) limits this ONE launch of the step to 256 registers.
template <int IT, bool RAW, bool UP = true>
__global__ void __launch_bounds__(448)
w8pt16_bwd_head_kernel(const float* pts1, const float* pts2, const float* wts, int B, int Bm, int N, float hw_sx, float hw_sy,
                       float clamp_at, const float* save, const W8BwdRest R, const TailHead* __restrict__ head) {
  __shared__ TailHeadLds lds;
  if (blockIdx.x == 0) {  // uniform over the workgroup: all seven wavefronts are still alive here
    if (threadIdx.x == 0) lds.arrived = 0u;
    __syncthreads();
  }
  if (threadIdx.x >= 256u) {
    if (blockIdx.x == 0) {
      const TailHead H = *head;
      loss_head_run(H, (int)(threadIdx.x & 63u), (int)(threadIdx.x >> 6) - 4, &lds);
    }
    return;
  }
  const int row = (int)(threadIdx.x >> 4);
  const int pair = (int)blockIdx.x * kPairsPerBlock + row;
  if (pair >= B) return;
#if DFEPE_BWD_STAGGER
  for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) DFEPE_STAGGER_WAIT(DFEPE_BWD_STAGGER);
#endif
  const W8BwdArgs A = w8_bwd_args(pts1, pts2, wts, B, Bm, N, hw_sx, hw_sy, clamp_at, save, R);
  w8pt16_bwd_pair_impl<IT, RAW, false, true, 1, UP>(A, pair, nullptr);
}

// Every fit kernel starts with the same nine arguments (the ones that arrive in SGPRs); `tail` is what follows them.
template <class Kernel, class Args, class... Tail>
void launch_fit(Kernel kernel, unsigned blocks, unsigned threads, hipStream_t st, const Args& A, const Tail&... tail) {
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, st, A.pts1, A.pts2, A.wts, A.B, A.Bm, A.N, A.hw_sx, A.hw_sy, A.clamp_at, tail...);
}
unsigned blocks_of(int pairs, int pairs_per_block) { return (unsigned)((pairs + pairs_per_block - 1) / pairs_per_block); }

FitPlan fwd_plan(const W8Args& A, bool raw) {
  static const int force_lean = env_int("DFEPE_FIT_LEAN", -1), force_pair2 = env_int("DFEPE_FIT_PAIR2", -1);
  return fit_fwd_plan(A.N, A.B, raw, A.row_per_pair, force_lean, force_pair2);
}

// The launchers return whether the plan named a kernel that was built (it always does: the lists below are what fit_plan.h returns).
template <bool RAW, bool PLAIN>
bool launch_fwd(const W8Args& A, hipStream_t st) {
  const FitPlan p = fwd_plan(A, RAW);
  const unsigned rows = blocks_of(A.B, kPairsPerBlock);
  auto go = [&](auto kernel, unsigned blocks) { launch_fit(kernel, blocks, 256, st, A, A.F_out, A.residual, rest_of(A)); };
  auto row = [&](auto it) { go(w8pt16_fwd_kernel<it.value, RAW, PLAIN>, rows); };
  if (p.kind == FitKind::Coop) return with_coop_it(p.it, [&](auto it) { go(w8pt16_coop_fwd_kernel<it.value, RAW, PLAIN>, A.B); });
  if (p.kind == FitKind::Pair2) {
    if constexpr (RAW) go(w8pt16_pair2_fwd_kernel<true, PLAIN>, blocks_of(A.B, kPairsPerBlock2));
    return RAW;
  }
  // with the Hartley record (A.hartley_mode is set only where fit_shares_hartley holds: a row kernel with p.it > 0)
  if (A.hartley_mode != DFEPE_HARTLEY_NONE) {
    if (p.kind == FitKind::RowLean) return with_it_in<7, 8>(p.it, [&](auto it) { go(w8pt16_fwd_lean_shared_kernel<it.value, RAW, PLAIN>, rows); });
    return with_it_in<1, 2, 4, 7, 8>(p.it, [&](auto it) { go(w8pt16_fwd_shared_kernel<it.value, RAW, PLAIN>, rows); });
  }
  if (p.it < 7) return with_it_in<0, 1, 2, 4>(p.it, row);
  // 7 or 8 correspondences per lane: the two rungs that have a lean build
  if (p.kind == FitKind::RowLean) return with_it_in<7, 8>(p.it, [&](auto it) { go(w8pt16_fwd_lean_kernel<it.value, RAW, PLAIN>, rows); });
  return with_it_in<7, 8>(p.it, row);
}

template <bool RAW, bool PGRAD, bool PLAIN>
bool launch_bwd(const W8BwdArgs& A, const FitPlan& p, hipStream_t st) {
  const unsigned rows = blocks_of(A.B, kPairsPerBlock);
  auto go = [&](auto kernel, unsigned blocks) { launch_fit(kernel, blocks, 256, st, A, A.save, rest_of(A)); };
  if constexpr (!PGRAD && PLAIN) {
    if (p.kind == FitKind::Coop) return with_coop_it(p.it, [&](auto it) { go(w8pt16_coop_bwd_kernel<it.value, RAW>, A.B); });
    if (!p.up) return with_it(p.it, [&](auto it) { go(w8pt16_bwd_kernel<it.value, RAW, false, true, false>, rows); });
  }
  return p.kind == FitKind::Row && with_it(p.it, [&](auto it) { go(w8pt16_bwd_kernel<it.value, RAW, PGRAD, PLAIN>, rows); });
}

// with the deferred loss head riding along.  Built for the ONE shape that uses it: pixel matches and g_F only (the captured
// solver-only step of pipeline.hot_path_fused; 250 registers at N = 100).  The 448-thread workgroup caps the launch at 256
// registers, and the instantiations with pass A (g_residual / g_epi, the recurrent model's backward) or homogeneous points need
// more (they spilled 24..208 bytes of scratch in round 3): those shapes take the plain launch plus a head launch of its own.
bool launch_bwd_head(const W8BwdArgs& A, const FitPlan& p, hipStream_t st) {
  return with_it(p.it, [&](auto it) {
    launch_fit(w8pt16_bwd_head_kernel<it.value, true, false>, blocks_of(A.B, kPairsPerBlock), 448, st, A, A.save, rest_of(A),
               static_cast<const TailHead*>(A.pending_head));
  });
}

}  // namespace

// Called by dfepe_w8pt_fwd / dfepe_w8pt_bwd (w8pt_fwd.hip / w8pt_bwd.hip) after argument validation.
int dfepe_w8pt16_fwd_launch(const W8Args& A, bool raw, hipStream_t st) {
  const bool plain = A.variant == 0;
  const bool launched = raw ? (plain ? launch_fwd<true, true>(A, st) : launch_fwd<true, false>(A, st))
                            : (plain ? launch_fwd<false, true>(A, st) : launch_fwd<false, false>(A, st));
  return (launched && hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

int dfepe_loss_head_from_workspace(const void* workspace_desc, hipStream_t st);  // loss_tail.hip

int dfepe_w8pt16_bwd_launch(const W8BwdArgs& A, bool raw, hipStream_t st) {
  const bool pgrad = A.g_p1 != nullptr, plain = A.variant == 0u;
  if (!plain && pgrad) return DFEPE_ERR_UNSUPPORTED;  // un-normalised rows: weight gradients only
  const FitPlan p = fit_bwd_plan(A.N, A.B, A.row_per_pair, pgrad, plain, !A.g_res && !A.g_epi && !A.g_w_extra);
  const bool rides = A.pending_head != nullptr && fit_bwd_head_rides(p, raw);
  bool launched;
  if (rides) launched = launch_bwd_head(A, p, st);
  else if (!plain) launched = raw ? launch_bwd<true, false, false>(A, p, st) : launch_bwd<false, false, false>(A, p, st);
  else if (raw) launched = pgrad ? launch_bwd<true, true, true>(A, p, st) : launch_bwd<true, false, true>(A, p, st);
  else launched = pgrad ? launch_bwd<false, true, true>(A, p, st) : launch_bwd<false, false, true>(A, p, st);
  if (!launched || hipGetLastError() != hipSuccess) return DFEPE_ERR_HIP;
  return (A.pending_head != nullptr && !rides) ? dfepe_loss_head_from_workspace(A.pending_head, st) : DFEPE_OK;
}

// ---- fit + E-from-F + cheirality-checked pose --------------------------------------------------------------------------------
extern "C" int dfepe_w8pt_fwd(const float* pts1, const float* pts2, const float* weights, int B, int N, int n_weight_sets, unsigned flags,
                              float image_w, float image_h, float clamp_at, float* F_out, float* residual, float* epi_res, float* save,
                              float* weights_out, void* stream);

extern "C" int dfepe_w8pt_pose_fwd(const float* matches, const float* weights, int B, int N, unsigned flags, float image_w, float image_h,
                                   float clamp_at, const float* K, const float* pre, float depth_thres, float* F_out, float* residual,
                                   float* epi_res, float* weights_out, float* Rt_cam, int* winner, int* counts, void* workspace,
                                   void* stream) {
  if (!(flags & DFEPE_W8PT_RAW_MATCHES) || (flags & ~(DFEPE_W8PT_RAW_MATCHES | DFEPE_W8PT_LOGITS | DFEPE_W8PT_ROW_PER_PAIR))) return DFEPE_ERR_INVALID_ARG;
  if (B < 0 || N <= 0) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!matches || !weights || !K || !F_out || !residual || !Rt_cam || !(image_w > 0.f && image_h > 0.f)) return DFEPE_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(matches) & 15u) return DFEPE_ERR_INVALID_ARG;
  // A/B switch (measurement only, read once): DFEPE_POSE_LAUNCHES=2 forces the two launches, =1 the fused one where it exists
  static const int forced_launches = env_int("DFEPE_POSE_LAUNCHES", 0);
  if (!fit_pose_fused(N, B, (flags & DFEPE_W8PT_ROW_PER_PAIR) != 0, forced_launches)) {  // any other shape: the two launches this one replaces
    const int rc = dfepe_w8pt_fwd(matches, nullptr, weights, B, N, 1, flags, image_w, image_h, clamp_at, F_out, residual, epi_res, nullptr,
                                  weights_out, stream);
    if (rc != DFEPE_OK) return rc;
    return dfepe_cheirality_ex(F_out, pre, K, matches, B, N, depth_thres, 0u, workspace, Rt_cam, winner, counts, stream);
  }
  const W8Args A = w8_args_of(matches, nullptr, weights, B, N, 1, flags, image_w, image_h, clamp_at, F_out, residual, epi_res, nullptr, weights_out);
  const W8PoseRest P = {pre, K, depth_thres, Rt_cam, winner, counts};
  const bool launched = with_coop_it(coop_it(N), [&](auto it) {
    launch_fit(w8pt16_coop_pose_kernel<it.value>, B, 256, static_cast<hipStream_t>(stream), A, A.F_out, A.residual, rest_of(A), P);
  });
  return (launched && hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
