// fit_plan -- which kernel of the weighted 8-point fit serves a shape, and with how many correspondences per lane: the ONE
// statement of that rule.  Plain C++17, no HIP: w8pt16.hip and loss_tail.hip launch by it, tests/emu/ runs the kernel bodies
// on the host by it and hands its answers to the plan-table test (tests/test_emu_cpu.py).  Nothing here reads the environment:
// the A/B switches (DFEPE_FIT_LEAN, DFEPE_FIT_PAIR2, DFEPE_POSE_LAUNCHES) are read once in w8pt16.hip and passed in.
#pragma once
#include <type_traits>

// ---- correspondences per lane --------------------------------------------------------------------------------------------
// One 16-lane row per pair: the lane keeps IT correspondences in registers for the whole kernel (1 / 2 / 4 / 7 / 8 for
// N <= 16 / 32 / 64 / 112 / 128); 0 = any N, correspondences re-read per phase.
constexpr int fit_it(int N) { return N <= 16 ? 1 : N <= 32 ? 2 : N <= 64 ? 4 : N <= 112 ? 7 : N <= 128 ? 8 : 0; }
// The 16 rows of a workgroup per pair (256 lanes): N <= 512 / 1024 / 2048.
constexpr int coop_it(int N) { return N <= 512 ? 2 : N <= 1024 ? 4 : 8; }

// The run-time value as a template argument: calls f(std::integral_constant<int, IT>{}) for the member of the list that equals
// `it`, and says whether there was one.  The list is what gets instantiated, so a kernel built for a part of the ladder names it.
template <int IT, int... Rest, class F>
bool with_it_in(int it, F&& f) {
  if (it == IT) return f(std::integral_constant<int, IT>{}), true;
  if constexpr (sizeof...(Rest) > 0) return with_it_in<Rest...>(it, f);
  return false;
}
template <class F>
bool with_it(int it, F&& f) { return with_it_in<0, 1, 2, 4, 7, 8>(it, f); }  // everything fit_it returns
template <class F>
bool with_coop_it(int it, F&& f) { return with_it_in<2, 4, 8>(it, f); }  // everything coop_it returns

// ---- thresholds ----------------------------------------------------------------------------------------------------------
constexpr int kCoopMaxN = 2048;  // cooperative workgroup per pair: N / 256 correspondences per lane in registers (IT <= 8)
// ... while the batch is small: the solver phase needs ~256 registers, so two workgroups (two pairs) fit a CU and a launch
// takes ceil(pairs / 512) rounds of ~13 us (N = 1000); from 4096 pairs on one row per pair (IT = 0, 78 us) is faster
constexpr int kCoopMaxPairs = 3072;
// the FORWARD fit leaves the cooperative workgroup earlier since round 5: two rows of a wavefront per pair (w8pt16_pair2_fwd_kernel) beat it
// from ~1300 pairs on (N = 1000, scripts/fit_n1000_sizes.py: 1024 pairs 29.7 vs 34.1 us, 2048 54.7 vs 37.7, 3072 78.3 vs 57.0); the `save`
// record is the same whichever kernel wrote it, so the backward keeps its own threshold
constexpr int kCoopFwdMaxPairs = 1280;
// N > 128, one row per pair: below this many pairs a SIMD holds a single wavefront, and two rows per pair (twice the wavefronts, each
// with half the per-correspondence work) are faster.  DFEPE_FIT_PAIR2 = 0 / 1 forces it off / on (A/B timing).
constexpr int kPair2MaxPairs = 8192;
// the lean forward fit (<= 256 registers) from this many pairs on.  Measured against the resident build (scripts/ab_fit_sizes.py, us per
// 4096 pairs, N = 100): 4096 pairs 14.5 vs 12.5 (one wavefront per SIMD: the extra instructions only cost), 8192 11.4 vs 11.2, 16384
// 9.9 vs 10.9, 32768 9.1 vs 10.4 (issue floor of its 4 140 instructions at the sustained clock: ~8.1).  DFEPE_FIT_LEAN = 0 / 1 in the
// environment forces it off / on (A/B timing; the outputs are bit-identical either way)
constexpr int kLeanMinPairs = 12288;

// ---- the plan ------------------------------------------------------------------------------------------------------------
enum class FitKind {
  Row,      // one 16-lane row per pair (w8pt16_fwd_kernel / w8pt16_bwd_kernel), it = fit_it(N)
  RowLean,  // the same in <= 256 registers (w8pt16_fwd_lean_kernel): forward, 64 < N <= 128
  Pair2,    // two rows of a wavefront per pair (w8pt16_pair2_fwd_kernel): forward, pixel matches, it = 0
  Coop      // the 16 rows of a workgroup per pair (w8pt16_coop_*_kernel), it = coop_it(N)
};
struct FitPlan {
  FitKind kind;
  int it;
  bool up = true;  // backward rows only: false = the instantiation without pass A and its loads (g_F is the only gradient given)
};

constexpr bool fit_switch(int forced, bool by_default) { return forced < 0 ? by_default : forced != 0; }  // forced: < 0 = not forced

// what the backward asks; the forward adds its own pair limit
constexpr bool fit_coop_serves(int N, int pairs, bool row_per_pair) {
  return N > 128 && N <= kCoopMaxN && pairs <= kCoopMaxPairs && !row_per_pair;
}

// raw: pixel matches (DFEPE_W8PT_RAW_MATCHES); force_lean / force_pair2: DFEPE_FIT_LEAN / DFEPE_FIT_PAIR2, -1 when unset
constexpr FitPlan fit_fwd_plan(int N, int pairs, bool raw, bool row_per_pair, int force_lean = -1, int force_pair2 = -1) {
  if (fit_coop_serves(N, pairs, row_per_pair) && (pairs <= kCoopFwdMaxPairs || !raw)) return {FitKind::Coop, coop_it(N)};
  // the homogeneous-point instantiations of two rows per pair need 300 registers and keep the row kernel
  if (N > 128) return {raw && fit_switch(force_pair2, pairs < kPair2MaxPairs) ? FitKind::Pair2 : FitKind::Row, 0};
  // 65 .. 128 correspondences at >= kLeanMinPairs pairs: two wavefronts per SIMD
  return {N > 64 && fit_switch(force_lean, pairs >= kLeanMinPairs) ? FitKind::RowLean : FitKind::Row, fit_it(N)};
}

// Does a forward launch of this shape write / read the Hartley record (dfepe_w8pt_fwd_shared)?  The registers-resident row kernels
// do -- every rung of fit_it, resident and lean -- unless the fit has no Hartley normalisation to hand on.  For N > 128 (cooperative,
// two-row and looped kernels) the record would remove one or two of four passes over the correspondences: not built.  The answer
// depends on N and the flags alone, never on the pair count or the environment, so a writer and its readers always agree.
// no_hartley: DFEPE_W8PT_NO_HARTLEY is set
constexpr bool fit_shares_hartley(int N, bool no_hartley) { return fit_it(N) > 0 && !no_hartley; }

// pgrad: point gradients wanted; plain: no variant flag; gF_only: neither g_residual nor g_epi nor g_weights_extra given
constexpr FitPlan fit_bwd_plan(int N, int pairs, bool row_per_pair, bool pgrad, bool plain, bool gF_only) {
  if (!pgrad && plain && fit_coop_serves(N, pairs, row_per_pair)) return {FitKind::Coop, coop_it(N)};
  return {FitKind::Row, fit_it(N), !(!pgrad && plain && gF_only)};
}

// A deferred loss head rides in spare wavefronts of the backward fit (w8pt16_bwd_head_kernel) for the ONE shape that kernel is
// built for: pixel matches through the g_F-only row kernel.  Anything else launches the head on its own.
constexpr bool fit_bwd_head_rides(const FitPlan& bwd, bool raw) { return raw && bwd.kind == FitKind::Row && !bwd.up; }

// dfepe_w8pt_pose_fwd is ONE launch where the cooperative workgroup serves the forward fit of pixel matches
// (forced_launches: DFEPE_POSE_LAUNCHES, 2 = always the two launches, 0 when unset)
constexpr bool fit_pose_fused(int N, int pairs, bool row_per_pair, int forced_launches = 0) {
  return forced_launches != 2 && fit_fwd_plan(N, pairs, true, row_per_pair).kind == FitKind::Coop;
}
