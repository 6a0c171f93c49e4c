// Host build of csrc/sample_loss_math.h: the launches of csrc/sample_loss.hip as plain loops over the same per-lane functions, for
// valid arguments only (the refusals are the library's and are tested against it).  Integer sums have a free order, so the scan is
// one sequential loop; the fp64 sums run in ascending order here and in a tree on the device, which the tests allow for in their
// bounds.  With -DEMU_SAMPLE_LOSS_MAIN the file is a stand-alone program that runs every stage at the shapes of the GPU tests and
// checks what can be checked without a reference: what a host sanitizer run is made of.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "sample_loss_math.h"

static void scan_pair(const float* w, int n, int N, uint64_t* P) {
  uint32_t m = 0u;
  for (int i = 0; i < n; ++i) {
    uint32_t bits;
    memcpy(&bits, w + i, 4);
    if (sm::drawable(bits) && bits > m) m = bits;
  }
  const int e = m ? sm::frexp_exponent(m) : 0;
  uint64_t run = 0, positive = 0;
  for (int i = 0; i < n; ++i) {
    uint32_t bits;
    memcpy(&bits, w + i, 4);
    const uint32_t q = sm::quantise(bits, e);
    P[i] = run;
    run += q;
    positive += q != 0u;
  }
  P[n] = run;
  P[(size_t)N + 1] = positive;
}

extern "C" void emu_sample_multisets(int B, int N, int H, int K, uint64_t seed, uint32_t offset, const uint32_t* counter,
                                     const float* weights, const int* n_valid, int* idx, int* fallback) {
  const uint32_t off = offset + (counter ? *counter : 0u);
  std::vector<uint64_t> P((size_t)N + 2);
  for (size_t b = 0; b < (size_t)B; ++b) {
    const int n = n_valid ? sm::clamp_valid(n_valid[b], K, N) : N;
    bool fall = false;
    if (weights) {
      scan_pair(weights + b * N, n, N, P.data());
      fall = P[(size_t)N + 1] == 0;
    }
    if (fallback) fallback[b] = fall ? 1 : 0;
    const uint64_t* Pd = (weights && !fall) ? P.data() : nullptr;
    for (size_t h = 0; h < (size_t)H; ++h) {
      sm::Stream s = sm::make_stream(seed, off, (uint32_t)b, (uint32_t)h);
      for (int j = 0; j < K; ++j) idx[(b * H + h) * K + j] = sl::draw_one(s, j, Pd, n);
    }
  }
}

extern "C" void emu_topk_select(const float* x, const int* n_valid, int B, int N, int K, int* idx) {
  for (size_t b = 0; b < (size_t)B; ++b) {
    const int n = n_valid ? sm::clamp_valid(n_valid[b], K, N) : N;
    const uint32_t* bits = reinterpret_cast<const uint32_t*>(x + b * N);
    uint64_t below = ~(uint64_t)0;
    for (int k = 0; k < K; ++k) {
      below = sl::best_below(bits, n, 0, 1, below);
      idx[b * K + k] = sl::position_index(below);
    }
  }
}

extern "C" void emu_sample_gather(const float* pts1, const float* pts2, const float* weights, const int* idx, int B, int N, int H, int K,
                                  float* pts1_sel, float* pts2_sel, float* w_sel, float* accu) {
  for (size_t b = 0; b < (size_t)B; ++b) {
    const size_t cell0 = b * H * K;
    const float* w = weights + b * N;
    for (size_t c = 0; c < (size_t)H * K; ++c) {
      const size_t i = (size_t)sl::safe_index(idx[cell0 + c], N);
      for (int d = 0; d < 3; ++d) {
        pts1_sel[(cell0 + c) * 3 + d] = pts1[(b * N + i) * 3 + d];
        pts2_sel[(cell0 + c) * 3 + d] = pts2[(b * N + i) * 3 + d];
      }
      w_sel[cell0 + c] = w[i];
    }
    if (!accu) continue;
    double total = 0.0;
    for (int h = 0; h < H; ++h) total = total + sl::set_product(w, idx + cell0 + (size_t)h * K, K, N);
    total = total + 1e-10;
    for (int h = 0; h < H; ++h) accu[b * H + h] = (float)(sl::set_product(w, idx + cell0 + (size_t)h * K, K, N) / total);
  }
}

// g_loss_sum null: forward (loss_sum written); else backward (g_F written)
extern "C" void emu_sample_floss(const float* F_sel, int B, int H, const float* T1, const float* T2, int t_stride, const float* virt1,
                                 const float* virt2, int M, float clamp_at, float* loss_sum, const float* g_loss_sum, float* g_F) {
  std::vector<float> pts((size_t)M * 6);
  for (size_t b = 0; b < (size_t)B; ++b) {
    for (int i = 0; i < M; ++i) {
      sl::eval_point(T1 + b * t_stride, virt1 + (b * M + i) * 3, &pts[6 * (size_t)i]);
      sl::eval_point(T2 + b * t_stride, virt2 + (b * M + i) * 3, &pts[6 * (size_t)i + 3]);
    }
    for (int h = 0; h < H; ++h) {
      const size_t bh = b * H + h;
      double F[9];
      for (int c = 0; c < 9; ++c) F[c] = (double)F_sel[bh * 9 + c];
      if (!g_loss_sum) {
        double acc = 0.0;
        for (int i = 0; i < M; ++i) acc = acc + sl::residual(F, &pts[6 * (size_t)i], &pts[6 * (size_t)i + 3], (double)clamp_at);
        loss_sum[bh] = (float)acc;
      } else {
        double g[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < M; ++i) sl::residual_adjoint_F(F, &pts[6 * (size_t)i], &pts[6 * (size_t)i + 3], (double)clamp_at, g);
        for (int c = 0; c < 9; ++c) g_F[bh * 9 + c] = (float)((double)g_loss_sum[bh] * g[c]);
      }
    }
  }
}

extern "C" void emu_sample_scatter_bwd(const float* g_w_sel, const float* g_accu, const float* weights, const float* accu, const int* idx,
                                       int B, int N, int H, int K, float* g_w) {
  for (size_t b = 0; b < (size_t)B; ++b) {
    double G = 0.0;
    if (g_accu)
      for (int h = 0; h < H; ++h) G = G + (double)g_accu[b * H + h] * (double)accu[b * H + h];
    for (int n = 0; n < N; ++n) {
      double direct = 0.0, through = 0.0;
      for (size_t c = 0; c < (size_t)H * K; ++c) {
        if (idx[b * H * K + c] != n) continue;
        const size_t bh = b * H + c / K;
        direct = direct + (g_w_sel ? (double)g_w_sel[b * H * K + c] : 0.0);
        through = through + (g_accu ? sl::cell_accu((double)accu[bh], (double)g_accu[bh], G) : 0.0);
      }
      g_w[b * N + n] = sl::scatter_finish(direct, through, g_accu ? weights[b * N + n] : 1.0f);
    }
  }
}

#ifdef EMU_SAMPLE_LOSS_MAIN
#include <cmath>
#include <cstdio>
#include <limits>

static int run(int B, int N, int H, int K, int M, bool special, const int* n_valid) {
  std::vector<float> w((size_t)B * N), p1((size_t)B * N * 3), p2((size_t)B * N * 3);
  for (size_t i = 0; i < w.size(); ++i) {
    float v = std::ldexp(1.0f + (float)((i * 7919u) % 97u), -(int)(i % 30));
    if (special && i % 11 == 3) v = std::numeric_limits<float>::quiet_NaN();
    if (special && i % 13 == 5) v = -1.0f;
    if (special && i % 17 == 7) v = std::numeric_limits<float>::infinity();
    if (special && i % 19 == 9) v = 1e-42f;
    if (special && i % 23 == 1) v = 0.0f;
    w[i] = v;
  }
  for (size_t i = 0; i < p1.size(); ++i) {
    p1[i] = (i % 3 == 2) ? 1.0f : std::sin(0.37f * (float)i);
    p2[i] = (i % 3 == 2) ? 1.0f : std::cos(0.23f * (float)i);
  }
  std::vector<int> idx((size_t)B * H * K, -1), fb(B, -1), top((size_t)B * K, -1);
  uint32_t counter = 0xfffffffeu;
  emu_sample_multisets(B, N, H, K, 0xfedcba9876543210ull, 5, &counter, w.data(), n_valid, idx.data(), fb.data());
  emu_topk_select(w.data(), n_valid, B, N, K, top.data());
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    const int n = n_valid ? sm::clamp_valid(n_valid[b], K, N) : N;
    for (int c = 0; c < H * K; ++c) {
      const int i = idx[(size_t)b * H * K + c];
      bad += i < 0 || i >= n;
      if (!fb[b] && i >= 0 && i < n) bad += !(w[(size_t)b * N + i] > 0.0f) || std::isinf(w[(size_t)b * N + i]);
    }
    for (int k = 0; k < K; ++k) {
      const int i = top[(size_t)b * K + k];
      bad += i < 0 || i >= n;
      for (int j = 0; j < k; ++j) bad += top[(size_t)b * K + j] == i;
    }
  }
  std::vector<float> s1((size_t)B * H * K * 3), s2(s1.size()), sw((size_t)B * H * K), accu((size_t)B * H), F((size_t)B * H * 9),
      loss((size_t)B * H), gl((size_t)B * H, 0.5f), gF(F.size()), gws(sw.size(), 0.25f), gw((size_t)B * N), v1((size_t)B * M * 3), v2(v1.size());
  emu_sample_gather(p1.data(), p2.data(), w.data(), idx.data(), B, N, H, K, s1.data(), s2.data(), sw.data(), accu.data());
  for (size_t i = 0; i < F.size(); ++i) F[i] = std::sin(1.3f * (float)i);
  for (size_t i = 0; i < v1.size(); ++i) {
    v1[i] = (i % 3 == 2) ? 1.0f : 600.0f + 500.0f * std::sin(0.11f * (float)i);
    v2[i] = (i % 3 == 2) ? 1.0f : 600.0f + 500.0f * std::cos(0.07f * (float)i);
  }
  const float T[9] = {2.0f / 1241, 0, -1, 0, 2.0f / 376, -1, 0, 0, 1};
  emu_sample_floss(F.data(), B, H, T, T, 0, v1.data(), v2.data(), M, 0.02f, loss.data(), nullptr, nullptr);
  emu_sample_floss(F.data(), B, H, T, T, 0, v1.data(), v2.data(), M, 0.02f, nullptr, gl.data(), gF.data());
  for (float v : loss) bad += !(v >= 0.0f && v <= 0.02f * (float)M * 1.000001f);
  emu_sample_scatter_bwd(gws.data(), special ? nullptr : gl.data(), w.data(), accu.data(), idx.data(), B, N, H, K, gw.data());
  double total = 0.0;
  for (float v : gw) total += v;
  if (special) bad += std::fabs(total - 0.25 * (double)B * H * K) > 1e-3 * (double)B * H * K;  // the direct term: every cell lands once
  std::printf("B=%d N=%d H=%d K=%d M=%d special=%d fallback[0]=%d: %d bad\n", B, N, H, K, M, (int)special, fb[0], bad);
  return bad;
}

int main() {
  int bad = 0;
  const int nv[3] = {5, 40, 2000};
  for (int K : {8, 20, 32})
    for (int N : {K, K + 1, 63, 64, 65, 1025}) {
      if (N < K) continue;
      bad += run(1, N, 1, K, 1, false, nullptr);
      bad += run(3, N, 65, K, 65, true, nv);
    }
  bad += run(3, 100, 100, 20, 100, false, nullptr);
  bad += run(2, 257, 100, 20, 129, true, nullptr);
  std::printf(bad ? "FAILED\n" : "every index in range and drawable, every loss within its clamp\n");
  return bad != 0;
}
#endif
