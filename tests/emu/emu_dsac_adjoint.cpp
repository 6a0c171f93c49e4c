// Host build of csrc/dsac_adjoint_math.h: the five kernels of csrc/dsac_adjoint.hip as plain loops over the same per-lane functions,
// with the buffers laid out as dfepe_dsac_bwd lays them out (include/dfepe.h), for valid arguments only (the refusals are the
// library's and are tested against it).  The two fit adjoints between them are tests/emu/emu_eight_point_adjoint.cpp;
// tests/test_dsac_adjoint_ref_cpu.py chains the steps as dfepe_dsac_bwd chains its launches.  The sums follow the kernel's order:
// lane l adds n = l, l + 64, ..., the 64 partial sums are added by the balanced tree of ds::tree_sum64; the points step adds the four
// quarters of the hypotheses in order.
#include <cstddef>

#include "dsac_adjoint_math.h"

namespace {

inline void load9(const float* p, double* m) {
  for (int c = 0; c < 9; ++c) m[c] = (double)p[c];
}
inline void pair_Ki(const float* K, size_t b, double* Ki) {
  double Km[9];
  load9(K + b * 9, Km);
  ds::inv3(Km, Ki);
}

}  // namespace

extern "C" int emu_dsac_bwd_point_lanes(void) { return da::kPointLanes; }
extern "C" int emu_dsac_bwd_point_waves(void) { return da::kPointWaves; }

// launch 1: pn1, pn2 [B,N,2]; g1, g2 [B H,S,2]; wts [H,B,N]; E_hb [H,B,9]; Fd, Md [B,H,9] fp64
extern "C" void emu_dsac_bwd_prep(const float* X, const float* Y, const float* K, const int* idx, const float* soft,
                                  const float* E_sample, const float* E_refit, int B, int N, int H, int S, int loss_kind, float* pn1,
                                  float* pn2, float* g1, float* g2, float* wts, float* E_hb, double* Fd, double* Md) {
  for (size_t b = 0; b < (size_t)B; ++b) {
    double Ki[9];
    pair_Ki(K, b, Ki);
    for (size_t n = 0; n < (size_t)N; ++n) {
      const size_t t = b * N + n;
      ds::normalized_point(Ki, (double)X[2 * t], (double)X[2 * t + 1], pn1 + 2 * t);
      ds::normalized_point(Ki, (double)Y[2 * t], (double)Y[2 * t + 1], pn2 + 2 * t);
    }
    for (size_t q = b * H * S; q < (b + 1) * H * S; ++q) {
      int n = idx[q];
      n = n < 0 ? 0 : (n >= N ? N - 1 : n);
      const size_t t = b * N + n;
      ds::normalized_point(Ki, (double)X[2 * t], (double)X[2 * t + 1], g1 + 2 * q);
      ds::normalized_point(Ki, (double)Y[2 * t], (double)Y[2 * t + 1], g2 + 2 * q);
    }
    for (size_t h = 0; h < (size_t)H; ++h) {
      const size_t bh = b * H + h, hb = h * B + b;
      for (size_t n = 0; n < (size_t)N; ++n) wts[hb * N + n] = ds::refit_weight(soft[bh * N + n]);
      double E[9], M[9];
      load9(E_sample + bh * 9, E);
      ds::e_to_f(Ki, E, M);
      for (int c = 0; c < 9; ++c) Fd[bh * 9 + c] = M[c];
      load9(E_refit + bh * 9, E);
      for (int c = 0; c < 9; ++c) E_hb[hb * 9 + c] = (float)E[c];
      if (loss_kind == 2) ds::e_to_f(Ki, E, M);
      for (int c = 0; c < 9; ++c) Md[bh * 9 + c] = (loss_kind == 2) ? M[c] : E[c];
    }
  }
}

// launch 2
extern "C" void emu_dsac_bwd_head(const int* idx, const float* score, const float* loss, const float* counts, const float* g_score,
                                  const float* g_loss, const float* g_quality, const float* g_exp_loss, float alpha_f, int B, int N, int H,
                                  int S, float* t_score, float* t_loss) {
  const double alpha = (double)alpha_f;
  for (size_t b = 0; b < (size_t)B; ++b) {
    const float* sc = score + b * H;
    const float* ls = loss + b * H;
    double m = 0.0, Z = 1.0, Lbar = 0.0, ge = 0.0;
    if (g_exp_loss) {
      ge = (double)g_exp_loss[b];
      m = -INFINITY;
      for (int h = 0; h < H; ++h) m = fmax(m, alpha * (double)sc[h]);
      double Zl[ds::kLanes], nl[ds::kLanes];
      for (int l = 0; l < ds::kLanes; ++l) {
        Zl[l] = nl[l] = 0.0;
        for (int h = l; h < H; h += ds::kLanes) {
          const double e = exp(alpha * (double)sc[h] - m);
          Zl[l] += e;
          nl[l] += e * (double)ls[h];
        }
      }
      Z = ds::tree_sum64(Zl);
      Lbar = ds::tree_sum64(nl) / Z;
    }
    for (int h = 0; h < H; ++h) {
      const size_t bh = b * H + h;
      double tl = g_loss ? (double)g_loss[bh] : 0.0;
      double ts = g_score ? (double)g_score[bh] : 0.0;
      if (g_exp_loss) {
        const double ph = exp(alpha * (double)sc[h] - m) / Z;
        tl = da::head_loss(tl, ge, ph);
        ts = ts + da::head_score_exp(ge, alpha, ph, (double)ls[h], Lbar);
      }
      if (g_quality) {
        for (int j = 0; j < S; ++j) {
          const int n = idx[bh * S + j];
          if (n >= 0 && n < N) ts = ts + da::head_vote((double)g_quality[b * N + n], (double)counts[b * N + n]);
        }
      }
      t_loss[bh] = (float)tl;
      t_score[bh] = (float)ts;
    }
  }
}

// launches 3 (is_loss = 1: Md = M_h, t_head = t_loss -> t_E [B,H,9] and t_E_hb [H,B,9]) and 6 (is_loss = 0: Md = F_h, t_head = t_score)
extern "C" void emu_dsac_bwd_hyp(int is_loss, const float* X, const float* Y, const float* K, const float* g_E, const double* Md,
                                 const float* t_head, const float* soft, const float* wts, const float* t_w, float beta_f, int loss_kind,
                                 int B, int N, int H, float* t_E, float* t_E_hb) {
  const double beta = (double)beta_f;
  for (size_t b = 0; b < (size_t)B; ++b) {
    for (size_t h = 0; h < (size_t)H; ++h) {
      const size_t bh = b * H + h, hb = h * B + b;
      double tE[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      if (!is_loss || loss_kind != 0) {
        const double* M = Md + bh * 9;
        const double th = (double)t_head[bh];
        double lanes[9][ds::kLanes];
        for (int l = 0; l < ds::kLanes; ++l) {
          double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, gM[9], gx[2], gy[2];
          for (size_t n = l; n < (size_t)N; n += ds::kLanes) {
            const float* x = X + (b * N + n) * 2;
            const float* y = Y + (b * N + n) * 2;
            double g0 = 1.0;
            if (!is_loss) g0 = da::score_coeff(beta, (double)soft[bh * N + n], (double)wts[hb * N + n], th, (double)t_w[hb * N + n]);
            da::sampson_adjoint(M, (double)x[0], (double)x[1], (double)y[0], (double)y[1], g0, gM, gx, gy);
            for (int c = 0; c < 9; ++c) acc[c] += gM[c];
          }
          for (int c = 0; c < 9; ++c) lanes[c][l] = acc[c];
        }
        double tM[9];
        for (int c = 0; c < 9; ++c) tM[c] = ds::tree_sum64(lanes[c]);
        if (is_loss) {
          const double k = th / (double)N;
          for (int c = 0; c < 9; ++c) tM[c] = k * tM[c];
        }
        if (!is_loss || loss_kind == 2) {
          double Ki[9];
          pair_Ki(K, b, Ki);
          da::f_to_e_adjoint(Ki, tM, tE);
        } else {
          for (int c = 0; c < 9; ++c) tE[c] = tM[c];
        }
      }
      for (int c = 0; c < 9; ++c) {
        const double up = g_E ? (double)g_E[bh * 9 + c] : 0.0;
        const float v = (float)(up + tE[c]);
        t_E[bh * 9 + c] = v;
        if (is_loss) t_E_hb[hb * 9 + c] = v;
      }
    }
  }
}

// launch 8
extern "C" void emu_dsac_bwd_points(const float* X, const float* Y, const float* K, const int* idx, const float* soft, const float* wts,
                                    const float* t_w, const float* t_score, const float* t_loss, const double* Fd, const double* Md,
                                    const float* gpn1, const float* gpn2, const float* gg1, const float* gg2, float beta_f, int loss_kind,
                                    int B, int N, int H, int S, float* g_X, float* g_Y) {
  const double beta = (double)beta_f, inv_n = 1.0 / (double)N;
  const int Hq = (H + da::kPointWaves - 1) / da::kPointWaves;
  for (size_t b = 0; b < (size_t)B; ++b) {
    double Ki[9];
    pair_Ki(K, b, Ki);
    for (size_t n = 0; n < (size_t)N; ++n) {
      const float* x = X + (b * N + n) * 2;
      const float* y = Y + (b * N + n) * 2;
      double Pw[da::kPointWaves][4], Dw[da::kPointWaves][4];
      for (int v = 0; v < da::kPointWaves; ++v) {
        double* P = Pw[v];
        double* D = Dw[v];
        for (int k = 0; k < 4; ++k) P[k] = D[k] = 0.0;
        const int h_end = (v + 1) * Hq < H ? (v + 1) * Hq : H;
        for (int h = v * Hq; h < h_end; ++h) {
          const size_t bh = b * H + h, hb = (size_t)h * B + b;
          for (int j = 0; j < S; ++j) {
            if (idx[bh * S + j] == (int)n) {
              const float* a1 = gg1 + (bh * S + j) * 2;
              const float* a2 = gg2 + (bh * S + j) * 2;
              P[0] += (double)a1[0]; P[1] += (double)a1[1]; P[2] += (double)a2[0]; P[3] += (double)a2[1];
            }
          }
          double gM[9], gx[2], gy[2];
          const double c = da::score_coeff(beta, (double)soft[bh * N + n], (double)wts[hb * N + n], (double)t_score[bh], (double)t_w[hb * N + n]);
          da::sampson_adjoint(Fd + bh * 9, (double)x[0], (double)x[1], (double)y[0], (double)y[1], c, gM, gx, gy);
          D[0] += gx[0]; D[1] += gx[1]; D[2] += gy[0]; D[3] += gy[1];
          if (loss_kind != 0) {
            da::sampson_adjoint(Md + bh * 9, (double)x[0], (double)x[1], (double)y[0], (double)y[1], (double)t_loss[bh] * inv_n, gM, gx, gy);
            D[0] += gx[0]; D[1] += gx[1]; D[2] += gy[0]; D[3] += gy[1];
          }
        }
      }
      const float* r1 = gpn1 + (b * N + n) * 2;
      const float* r2 = gpn2 + (b * N + n) * 2;
      double G[4] = {(double)r1[0] + Pw[0][0], (double)r1[1] + Pw[0][1], (double)r2[0] + Pw[0][2], (double)r2[1] + Pw[0][3]};
      double D[4] = {Dw[0][0], Dw[0][1], Dw[0][2], Dw[0][3]};
      for (int v = 1; v < da::kPointWaves; ++v)
        for (int k = 0; k < 4; ++k) {
          G[k] += Pw[v][k];
          D[k] += Dw[v][k];
        }
      double pix[2];
      if (g_X) {
        da::pixel_from_normalized(Ki, (double)x[0], (double)x[1], G, pix);
        g_X[(b * N + n) * 2] = (float)(pix[0] + D[0]);
        g_X[(b * N + n) * 2 + 1] = (float)(pix[1] + D[1]);
      }
      if (g_Y) {
        da::pixel_from_normalized(Ki, (double)y[0], (double)y[1], G + 2, pix);
        g_Y[(b * N + n) * 2] = (float)(pix[0] + D[2]);
        g_Y[(b * N + n) * 2 + 1] = (float)(pix[1] + D[3]);
      }
    }
  }
}
