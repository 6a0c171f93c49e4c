// dfepe_w8pt_fwd -- C-ABI entry point of the weighted normalised 8-point fit (argument validation, then w8pt16.hip).
//
// Arithmetic contract: Fit.normalize / Fit.weighted_svd / NormalizeAndExpand_HW / compute_epi_residual
// (deepFEPE/models/DeepFNet.py:93-120,148-257, deepFEPE/dsac_tools/utils_F.py:400-413); bodies in w8pt16_body.h.
// One kernel family serves every shape: one 16-lane row per pair (N <= 128, or large batches of any N) or the 16 rows of a
// workgroup per pair (N > 128 at small batch).  The round-1 family (one wavefront per pair, fp32 Jacobi in LDS, its own `save`
// format) was retired in round 3: the cooperative rows are faster at every size it still served (N = 1000, 512 pairs: 20 vs 32 us).
#include "dfepe_common.h"
#include "fit_plan.h"
#include "w8pt16_body.h"
#include <cstdlib>

int dfepe_w8pt16_fwd_launch(const W8Args& A, bool raw, hipStream_t st);  // w8pt16.hip

namespace {
// hartley / hartley_mode: the Hartley record of dfepe_w8pt_fwd_shared (null / DFEPE_HARTLEY_NONE from dfepe_w8pt_fwd)
int w8pt_fwd(const float* pts1, const float* pts2, const float* weights, int B, int N, int n_weight_sets, unsigned flags, float image_w,
             float image_h, float clamp_at, float* F_out, float* residual, float* epi_res, float* save, float* weights_out, double* hartley,
             int hartley_mode, void* stream) {
  const bool raw = (flags & DFEPE_W8PT_RAW_MATCHES) != 0;
  const unsigned variant = flags & (DFEPE_W8PT_SQRT2 | DFEPE_W8PT_NO_ROWNORM | DFEPE_W8PT_FORCE_110 | DFEPE_W8PT_NO_HARTLEY);
  if (B < 0 || N <= 0 || n_weight_sets < 1) return DFEPE_ERR_INVALID_ARG;
  // the textbook variants are forward-only; un-normalised rows alone (Fit(normalize_SVD=False)) have a backward
  if (variant && save && variant != DFEPE_W8PT_NO_ROWNORM) return DFEPE_ERR_UNSUPPORTED;
  if (B == 0) return DFEPE_OK;
  if (!pts1 || (!raw && !pts2) || !weights || !F_out || !residual) return DFEPE_ERR_INVALID_ARG;
  if (raw && !(image_w > 0.f && image_h > 0.f)) return DFEPE_ERR_INVALID_ARG;
  if (raw && (reinterpret_cast<uintptr_t>(pts1) & 15u)) return DFEPE_ERR_INVALID_ARG;  // float4 loads
  if (reinterpret_cast<uintptr_t>(save) & 15u) return DFEPE_ERR_INVALID_ARG;          // wide stores of the record

  if (flags & ~DFEPE_W8PT_ALL_FLAGS) return DFEPE_ERR_INVALID_ARG;  // unknown flag bits are rejected, not ignored
  W8Args A = w8_args_of(pts1, pts2, weights, B, N, n_weight_sets, flags, image_w, image_h, clamp_at, F_out, residual, epi_res, save,
                        weights_out);
  // the record is written / read where the ONE rule of fit_plan.h says so (it knows N and the flags only, so that a writer and its
  // readers agree); anywhere else the launch is that of dfepe_w8pt_fwd
  if (hartley_mode != DFEPE_HARTLEY_NONE && fit_shares_hartley(N, (flags & DFEPE_W8PT_NO_HARTLEY) != 0)) {
    A.hartley = hartley;
    A.hartley_mode = hartley_mode;
  }
  return dfepe_w8pt16_fwd_launch(A, raw, static_cast<hipStream_t>(stream));
}
}  // namespace

extern "C" int dfepe_w8pt_fwd(const float* pts1, const float* pts2, const float* weights, int B, int N,
                              int n_weight_sets, unsigned flags, float image_w, float image_h, float clamp_at, float* F_out,
                              float* residual, float* epi_res, float* save, float* weights_out, void* stream) {
  return w8pt_fwd(pts1, pts2, weights, B, N, n_weight_sets, flags, image_w, image_h, clamp_at, F_out, residual, epi_res, save, weights_out,
                  nullptr, DFEPE_HARTLEY_NONE, stream);
}

extern "C" int dfepe_w8pt_fwd_shared(const float* pts1, const float* pts2, const float* weights, int B, int N, int n_weight_sets,
                                     unsigned flags, float image_w, float image_h, float clamp_at, float* F_out, float* residual,
                                     float* epi_res, float* save, float* weights_out, double* hartley, int hartley_mode, void* stream) {
  // the record's own arguments are checked whatever the shape and the switch below: a mode that does not exist, a record that
  // a launch of another shape could not take
  if (hartley_mode < DFEPE_HARTLEY_NONE || hartley_mode > DFEPE_HARTLEY_READ) return DFEPE_ERR_INVALID_ARG;
  if (hartley_mode != DFEPE_HARTLEY_NONE && (!hartley || (reinterpret_cast<uintptr_t>(hartley) & 63u))) return DFEPE_ERR_INVALID_ARG;
  // A/B switch (measurement only, read once): DFEPE_HARTLEY_SHARE=0 ignores the record in both modes
  static const bool share = [] { const char* e = getenv("DFEPE_HARTLEY_SHARE"); return !(e && atoi(e) == 0); }();
  return w8pt_fwd(pts1, pts2, weights, B, N, n_weight_sets, flags, image_w, image_h, clamp_at, F_out, residual, epi_res, save, weights_out,
                  hartley, share ? hartley_mode : DFEPE_HARTLEY_NONE, stream);
}

extern "C" int dfepe_w8pt_shares_hartley(int N, unsigned flags) {
  return (N > 0 && fit_shares_hartley(N, (flags & DFEPE_W8PT_NO_HARTLEY) != 0)) ? 1 : 0;
}
