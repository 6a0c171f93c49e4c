// Host build of csrc/epi_adjoint_math.h: the launches of csrc/epi_adjoint.hip as plain loops with the arguments of the C ABI
// (include/dfepe.h) minus the stream and the workspace, for valid arguments only (the refusals are the library's and are tested
// against it), plus two entries that hand out the per-point fp64 values before they are rounded (what
// tests/test_epi_adjoint_ref_cpu.py measures the constant of the bound from).  The sums follow the kernel's tree at the level the
// contract states: a chunk of ea::kChunk points is added up on its own, then the chunks in ascending order.
#include <cstddef>

#include "epi_adjoint_math.h"

namespace {

constexpr int kHomo = 8;

inline void point_of(const float* P, size_t at, bool homo, double* x) {
  const int sd = homo ? 3 : 2;
  x[0] = (double)P[at * sd];
  x[1] = (double)P[at * sd + 1];
  x[2] = homo ? (double)P[at * sd + 2] : 1.0;
}

inline void store_of(float* P, size_t at, bool homo, const double* g) {
  const int sd = homo ? 3 : 2;
  for (int k = 0; k < sd; ++k) P[at * sd + k] = (float)g[k];
}

inline int chunks_of(int N) { return (int)(((long long)N + ea::kChunk - 1) / ea::kChunk); }

// mode 0: upstream g_out per point; 1: g_sum[pair] * w; 2: the loss sum
int run(int mode, int kind, const float* F, const float* X, const float* Y, const float* w, int B, int N, float clamp_at, float eps,
        const float* g_out, const float* g_sum, float* g_F, float* g_X, float* g_Y, float* g_w, float* sum_out) {
  const bool homo = (kind & kHomo) != 0;
  kind &= 7;
  const size_t plane = (size_t)B * N;
  for (size_t pair = 0; pair < (size_t)B; ++pair) {
    double f[9], tot[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 9; ++c) f[c] = (double)F[pair * 9 + c];
    for (int ch = 0; ch < chunks_of(N); ++ch) {
      double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int i = ch * ea::kChunk; i < N && i < (ch + 1) * ea::kChunk; ++i) {
        const size_t at = pair * (size_t)N + i;
        double x[3], y[3];
        point_of(X, at, homo, x);
        point_of(Y, at, homo, y);
        const ea::Terms t = ea::terms(f, x, y);
        const double wgt = (mode != 0 && w != nullptr) ? (double)w[at] : 1.0;
        if (mode == 2) {
          acc[0] += wgt * ea::value(kind, t, (double)clamp_at, (double)eps);
          continue;
        }
        double g0 = 0.0, g1 = 0.0, g2 = 0.0;
        if (mode == 0) {
          g0 = (double)g_out[at];
          if (kind == 2) {
            g1 = (double)g_out[plane + at];
            g2 = (double)g_out[2 * plane + at];
          }
        } else {
          const double gs = (double)g_sum[pair];
          g0 = gs * wgt;
          if (g_w != nullptr) g_w[at] = (float)(gs * ea::value(kind, t, (double)clamp_at, (double)eps));
        }
        double cs, cA, cQ, gF[9], gx[3], gy[3];
        ea::coeffs(kind, t, (double)clamp_at, (double)eps, g0, g1, g2, &cs, &cA, &cQ);
        ea::point_adjoint(f, x, y, t, cs, cA, cQ, gF, gx, gy);
        if (g_X != nullptr) store_of(g_X, at, homo, gx);
        if (g_Y != nullptr) store_of(g_Y, at, homo, gy);
        for (int c = 0; c < 9; ++c) acc[c] += gF[c];
      }
      for (int c = 0; c < 9; ++c) tot[c] += acc[c];
    }
    if (mode == 2) sum_out[pair] = (float)tot[0];
    else if (g_F != nullptr) {
      for (int c = 0; c < 9; ++c) g_F[pair * 9 + c] = (float)tot[c];
    }
  }
  return 0;
}

}  // namespace

extern "C" int emu_epi_adjoint_chunk(void) { return ea::kChunk; }

extern "C" int emu_epi_metrics_bwd(int kind, const float* F, const float* X, const float* Y, int B, int N, float clamp_at, float eps,
                                   const float* g_out, float* g_F, float* g_X, float* g_Y) {
  return run(0, kind, F, X, Y, nullptr, B, N, clamp_at, eps, g_out, nullptr, g_F, g_X, g_Y, nullptr, nullptr);
}

extern "C" int emu_epi_loss_fwd(int kind, const float* F, const float* X, const float* Y, const float* w, int B, int N, float clamp_at,
                                float eps, float* sum_out) {
  return run(2, kind, F, X, Y, w, B, N, clamp_at, eps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sum_out);
}

extern "C" int emu_epi_loss_bwd(int kind, const float* F, const float* X, const float* Y, const float* w, int B, int N, float clamp_at,
                                float eps, const float* g_sum, float* g_F, float* g_X, float* g_Y, float* g_w) {
  return run(1, kind, F, X, Y, w, B, N, clamp_at, eps, nullptr, g_sum, g_F, g_X, g_Y, g_w, nullptr);
}

extern "C" int emu_epi_residual_bwd_pts(const float* pts1, const float* pts2, const float* F, int B, int N, float clamp_at,
                                        const float* g_out, float* g_pts1, float* g_pts2) {
  for (size_t pair = 0; pair < (size_t)B; ++pair) {
    double f[9];
    for (int c = 0; c < 9; ++c) f[c] = (double)F[pair * 9 + c];
    for (int i = 0; i < N; ++i) {
      const size_t at = pair * (size_t)N + i;
      double x1[3], x2[3], g1[3], g2[3];
      point_of(pts1, at, true, x1);
      point_of(pts2, at, true, x2);
      ea::residual_point_adjoint(f, x1, x2, (double)clamp_at, (double)g_out[at], g1, g2);
      if (g_pts1 != nullptr) store_of(g_pts1, at, true, g1);
      if (g_pts2 != nullptr) store_of(g_pts2, at, true, g2);
    }
  }
  return 0;
}

// The per-point values in fp64, before any rounding to fp32: value [planes,B,N] (1 plane, 3 for kind 2), gF_pt [B,N,9], gX, gY [B,N,3].
extern "C" int emu_epi_point_terms(int kind, const float* F, const float* X, const float* Y, int B, int N, float clamp_at, float eps,
                                   const float* g_out, double* value, double* gF_pt, double* gX, double* gY) {
  const bool homo = (kind & kHomo) != 0;
  kind &= 7;
  const size_t plane = (size_t)B * N;
  for (size_t pair = 0; pair < (size_t)B; ++pair) {
    double f[9];
    for (int c = 0; c < 9; ++c) f[c] = (double)F[pair * 9 + c];
    for (int i = 0; i < N; ++i) {
      const size_t at = pair * (size_t)N + i;
      double x[3], y[3], cs, cA, cQ;
      point_of(X, at, homo, x);
      point_of(Y, at, homo, y);
      const ea::Terms t = ea::terms(f, x, y);
      if (kind == 2) {
        const double as = fabs(t.s);
        value[at] = ea::value(2, t, -1.0, 0.0);
        value[plane + at] = as / sqrt(t.A);
        value[2 * plane + at] = as / sqrt(t.Q);
      } else {
        value[at] = ea::value(kind, t, (double)clamp_at, (double)eps);
      }
      const double g1 = (kind == 2) ? (double)g_out[plane + at] : 0.0, g2 = (kind == 2) ? (double)g_out[2 * plane + at] : 0.0;
      ea::coeffs(kind, t, (double)clamp_at, (double)eps, (double)g_out[at], g1, g2, &cs, &cA, &cQ);
      ea::point_adjoint(f, x, y, t, cs, cA, cQ, gF_pt + at * 9, gX + at * 3, gY + at * 3);
    }
  }
  return 0;
}

extern "C" int emu_epi_residual_point_terms(const float* pts1, const float* pts2, const float* F, int B, int N, float clamp_at,
                                            const float* g_out, double* g1, double* g2) {
  for (size_t pair = 0; pair < (size_t)B; ++pair) {
    double f[9];
    for (int c = 0; c < 9; ++c) f[c] = (double)F[pair * 9 + c];
    for (int i = 0; i < N; ++i) {
      const size_t at = pair * (size_t)N + i;
      double x1[3], x2[3];
      point_of(pts1, at, true, x1);
      point_of(pts2, at, true, x2);
      ea::residual_point_adjoint(f, x1, x2, (double)clamp_at, (double)g_out[at], g1 + at * 3, g2 + at * 3);
    }
  }
  return 0;
}
