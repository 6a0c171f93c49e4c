// Host build of the forward fit with the Hartley record (w8pt16_body.h: HM) -- TEST INFRASTRUCTURE ONLY (see tests/emu/rowgroup.h).
//   g++ -O1 -std=c++17 -shared -fPIC -Itests/emu -Ipytorch-deepfepe_amd/csrc -Iinclude tests/emu/emu_w8pt16_hartley.cpp -o tests/emu/_build/libemu_w8pt16_hartley.so
// The row scheduler, the dispatch over the correspondences per lane and the plain bodies are those of emu_w8pt16.cpp, which this
// source includes as it is; it adds emu_w8pt16_fwd_shared with the argument list of dfepe_w8pt_fwd_shared (host pointers, no
// stream; `lean`: the <= 256-register body where the library has one) and the rule of csrc/fit_plan.h for the record.
#include "emu_w8pt16.cpp"

namespace {
bool g_lean_shared = false;

// the instantiation the library's *_shared kernels run: the mode is the launch's (A.hartley_mode)
template <int IT, bool RAW>
struct FwdSharedBody {
  static void run(const W8Args& A, int pair, double* xch) {
    if constexpr (IT > 0) {
      if constexpr (IT == 7 || IT == 8) {
        if (g_lean_shared) {
          if (A.variant == 0) w8pt16_fwd_pair<IT, RAW, true, 1, true, H16_BY_LAUNCH>(A, pair, xch);
          else w8pt16_fwd_pair<IT, RAW, false, 1, true, H16_BY_LAUNCH>(A, pair, xch);
          return;
        }
      }
      if (A.variant == 0) w8pt16_fwd_pair<IT, RAW, true, 1, false, H16_BY_LAUNCH>(A, pair, xch);
      else w8pt16_fwd_pair<IT, RAW, false, 1, false, H16_BY_LAUNCH>(A, pair, xch);
    }
  }
};
}  // namespace

extern "C" int emu_fit_shares_hartley(int N, unsigned flags) { return fit_shares_hartley(N, (flags & DFEPE_W8PT_NO_HARTLEY) != 0) ? 1 : 0; }

extern "C" int emu_w8pt16_fwd_shared(const float* pts1, const float* pts2, const float* weights, int B, int N, int n_weight_sets,
                                     unsigned flags, float image_w, float image_h, float clamp_at, float* F_out, float* residual,
                                     float* epi_res, float* save, float* weights_out, double* hartley, int hartley_mode, int lean) {
  if (N < 1) return -3;
  if (hartley_mode < DFEPE_HARTLEY_NONE || hartley_mode > DFEPE_HARTLEY_READ) return -1;
  if (hartley_mode != DFEPE_HARTLEY_NONE && hartley == nullptr) return -1;
  W8Args A = w8_args_of(pts1, pts2, weights, B, N, n_weight_sets, flags, image_w, image_h, clamp_at, F_out, residual, epi_res, save,
                        weights_out);
  const bool raw = (flags & DFEPE_W8PT_RAW_MATCHES) != 0;
  // as dfepe_w8pt_fwd_shared does: the record is taken where the rule of fit_plan.h says so, the plain launch anywhere else
  if (hartley_mode == DFEPE_HARTLEY_NONE || !fit_shares_hartley(N, (flags & DFEPE_W8PT_NO_HARTLEY) != 0)) {
    g_lean = lean != 0;
    const int rc = dispatch<FwdBody>(A, raw);
    g_lean = false;
    return rc;
  }
  A.hartley = hartley;
  A.hartley_mode = hartley_mode;
  g_lean_shared = lean != 0;
  const int rc = dispatch<FwdSharedBody>(A, raw);
  g_lean_shared = false;
  return rc;
}
