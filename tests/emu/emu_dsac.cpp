// Host build of csrc/dsac_math.h: the four kernels of csrc/dsac.hip as plain loops over the same per-lane functions, with the
// buffers laid out as dfepe_dsac's workspace lays them out (include/dfepe.h), for valid arguments only (the refusals are the
// library's and are tested against it).  The two fits between them are the library's fit kernels, whose host build is
// tests/emu/emu_w8pt16.cpp; tests/test_dsac_ref_cpu.py chains the six steps as dfepe_dsac does.  The sums follow the kernel's
// order: lane l adds n = l, l + 64, ..., the 64 partial sums are added by the balanced tree of ds::tree_sum64.
#include <cstddef>

#include "dsac_math.h"

namespace {

inline void load9(const float* p, double* m) {
  for (int c = 0; c < 9; ++c) m[c] = (double)p[c];
}

inline void write_point(float* dst, const double* Ki, const float* src) {
  ds::normalized_point(Ki, (double)src[0], (double)src[1], dst);
  dst[2] = 1.0f;
}

}  // namespace

extern "C" int emu_dsac_hyps_per_block(void) { return ds::kHypsPerBlock; }
extern "C" int emu_dsac_vote_chunk(void) { return ds::kVoteChunk; }
extern "C" int emu_dsac_vote_tile(void) { return ds::kVoteTile; }

// launch 1: pn1, pn2 [B,N,3]; g1, g2 [B H,S,3]; ones [B H,S]
extern "C" void emu_dsac_prep(const float* X, const float* Y, const float* K, const int* idx, int B, int N, int H, int S, float* pn1,
                              float* pn2, float* g1, float* g2, float* ones) {
  for (size_t b = 0; b < (size_t)B; ++b) {
    double Km[9], Ki[9];
    load9(K + b * 9, Km);
    ds::inv3(Km, Ki);
    for (size_t n = 0; n < (size_t)N; ++n) {
      const size_t t = b * N + n;
      write_point(pn1 + t * 3, Ki, X + t * 2);
      write_point(pn2 + t * 3, Ki, Y + t * 2);
    }
    for (size_t q = b * H * S; q < (b + 1) * H * S; ++q) {
      int n = idx[q];
      n = n < 0 ? 0 : (n >= N ? N - 1 : n);
      write_point(g1 + q * 3, Ki, X + (b * N + n) * 2);
      write_point(g2 + q * 3, Ki, Y + (b * N + n) * 2);
      ones[q] = 1.0f;
    }
  }
}

// launches 3 (is_loss = 0: E [B,H,9] -> soft, sampson [B,H,N] or null, score [B,H], wts [H,B,N]) and 5 (is_loss = 1: E [H,B,9] ->
// E_out [B,H,9], loss [B,H])
extern "C" void emu_dsac_hyp(int is_loss, const float* X, const float* Y, const float* K, const float* E, int B, int N, int H,
                             float thresh, float beta, int loss_kind, float* soft, float* sampson, float* score, float* wts, float* E_out,
                             float* loss) {
  for (size_t b = 0; b < (size_t)B; ++b) {
    for (size_t h = 0; h < (size_t)H; ++h) {
      const size_t bh = b * H + h, hb = h * B + b;
      double Km[9], Ki[9], Em[9], M[9];
      load9(E + (is_loss ? hb : bh) * 9, Em);
      if (!is_loss || loss_kind == 2) {
        load9(K + b * 9, Km);
        ds::inv3(Km, Ki);
        ds::e_to_f(Ki, Em, M);
      } else {
        for (int c = 0; c < 9; ++c) M[c] = Em[c];
      }
      if (is_loss) {
        for (int c = 0; c < 9; ++c) E_out[bh * 9 + c] = (float)Em[c];
        if (loss_kind == 0) {
          loss[bh] = 0.0f;
          continue;
        }
      }
      double lanes[ds::kLanes];
      for (int l = 0; l < ds::kLanes; ++l) {
        double acc = 0.0;
        for (size_t n = l; n < (size_t)N; n += ds::kLanes) {
          const float* x = X + (b * N + n) * 2;
          const float* y = Y + (b * N + n) * 2;
          const double d = ds::sampson(M, (double)x[0], (double)x[1], (double)y[0], (double)y[1]);
          if (is_loss) {
            acc += d;
          } else {
            const double s = ds::soft_inlier(d, (double)thresh, (double)beta);
            const float sf = (float)s;
            if (soft) soft[bh * N + n] = sf;
            if (sampson) sampson[bh * N + n] = (float)d;
            wts[hb * N + n] = ds::refit_weight(sf);
            acc += s;
          }
        }
        lanes[l] = acc;
      }
      const double tot = ds::tree_sum64(lanes);
      if (is_loss) loss[bh] = (float)(tot / (double)N);
      else score[bh] = (float)tot;
    }
  }
}

// launch 6
extern "C" void emu_dsac_vote(const int* idx, const float* score, const float* loss, float alpha, int B, int N, int H, int S,
                              float* quality, float* counts, int* best, float* exp_loss, float* top_loss) {
  for (size_t b = 0; b < (size_t)B; ++b) {
    const float* sc = score + b * H;
    const int* ix = idx + b * H * S;
    for (int n = 0; n < N; ++n) {
      float ns = 0.f, nc = 0.f;
      for (int h = 0; h < H; ++h) {
        bool hit = false;
        for (int s = 0; s < S; ++s) hit = hit || ix[(size_t)h * S + s] == n;
        if (hit) {
          ns = ns + sc[h];
          nc = nc + 1.0f;
        }
      }
      quality[b * N + n] = ds::quality(ns, nc);
      counts[b * N + n] = nc;
    }
    float bv = 0.f;
    int bi = -1;
    for (int h = 0; h < H; ++h)
      if (sc[h] > bv) { bv = sc[h]; bi = h; }
    best[b] = bi;
    if (top_loss) top_loss[b] = bi >= 0 ? loss[b * H + bi] : 0.0f;
    if (!exp_loss) continue;
    double m = -INFINITY;
    for (int h = 0; h < H; ++h) m = fmax(m, (double)alpha * (double)sc[h]);
    double Zl[ds::kLanes], nl[ds::kLanes];
    for (int l = 0; l < ds::kLanes; ++l) {
      Zl[l] = nl[l] = 0.0;
      for (int h = l; h < H; h += ds::kLanes) {
        const double e = exp((double)alpha * (double)sc[h] - m);
        Zl[l] += e;
        nl[l] += e * (double)loss[b * H + h];
      }
    }
    const double Z = ds::tree_sum64(Zl), num = ds::tree_sum64(nl);
    exp_loss[b] = (float)(num / Z);
  }
}
