// Host build of csrc/sampler_math.h: the two launches of csrc/sampler.hip as plain loops over the same per-lane functions, with the
// workspace laid out as dfepe_sample_sets lays it out (include/dfepe.h: per pair P[0 .. N] and the number of q > 0), for valid
// arguments only (the refusals are the library's and are tested against it).  The prefix sums are integer sums: their order is free,
// so the scan is one sequential loop here.  With -DEMU_SAMPLER_MAIN the file is a stand-alone program that draws a few shapes and
// checks each set (distinct, inside [0, n), q > 0): what a host sanitizer run is made of.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "sampler_math.h"

extern "C" int emu_sampler_scan_chunk(void) { return sm::kScanChunk; }

extern "C" void emu_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  for (int i = 0; i < 4; ++i) out[i] = counter[i];
  sm::philox4x32_10(out, key[0], key[1]);
}

// launch 1: ws [B, N + 2] uint64
extern "C" void emu_sampler_scan(const float* weights, const int* n_valid, int B, int N, int S, uint64_t* ws) {
  for (size_t b = 0; b < (size_t)B; ++b) {
    const int n = n_valid ? sm::clamp_valid(n_valid[b], S, N) : N;
    const float* w = weights + b * N;
    uint64_t* P = ws + b * ((size_t)N + 2);
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
}

// launch 2: ws null = uniform mode
extern "C" void emu_sampler_draw(int B, int N, int H, int S, uint64_t seed, uint32_t offset, const uint32_t* counter, const uint64_t* ws,
                                 const int* n_valid, int* idx, int* fallback) {
  const uint32_t off = offset + (counter ? *counter : 0u);
  for (size_t b = 0; b < (size_t)B; ++b) {
    const int n = n_valid ? sm::clamp_valid(n_valid[b], S, N) : N;
    const uint64_t* P = ws ? ws + b * ((size_t)N + 2) : nullptr;
    const bool fall = P && P[(size_t)N + 1] < (uint64_t)S;
    if (fallback) fallback[b] = fall ? 1 : 0;
    for (size_t h = 0; h < (size_t)H; ++h) {
      int out[sm::kMaxSample];
      sm::Stream s = sm::make_stream(seed, off, (uint32_t)b, (uint32_t)h);
      if (P && !fall) sm::weighted_set(s, P, n, S, out);
      else sm::uniform_set(s, n, S, out);
      for (int i = 0; i < S; ++i) idx[(b * H + h) * S + i] = out[i];
    }
  }
}

#ifdef EMU_SAMPLER_MAIN
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int run(int B, int N, int H, int S, uint64_t seed, uint32_t offset, bool weighted, int positive, const int* n_valid) {
  std::vector<int> idx((size_t)B * H * S, -1), fb(B, -1);
  std::vector<float> w;
  std::vector<uint64_t> ws;
  if (weighted) {
    w.assign((size_t)B * N, 0.0f);
    ws.assign((size_t)B * ((size_t)N + 2), ~(uint64_t)0);
    for (size_t b = 0; b < (size_t)B; ++b)
      for (int i = 0; i < N; ++i) {
        float v = i < positive ? std::ldexp(1.0f + (float)(((unsigned)i * 7919u + (unsigned)b) % 97u), -(i % 40)) : 0.0f;
        if (i % 11 == 3) v = std::numeric_limits<float>::quiet_NaN();
        if (i % 13 == 5) v = -1.0f;
        if (i % 17 == 7) v = std::numeric_limits<float>::infinity();
        if (i % 19 == 9) v = 1e-42f;
        w[b * N + i] = v;
      }
    emu_sampler_scan(w.data(), n_valid, B, N, S, ws.data());
  }
  uint32_t counter = 2;
  emu_sampler_draw(B, N, H, S, seed, offset, &counter, weighted ? ws.data() : nullptr, n_valid, idx.data(), fb.data());
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    const int n = n_valid ? sm::clamp_valid(n_valid[b], S, N) : N;
    for (int h = 0; h < H; ++h) {
      const int* s = &idx[((size_t)b * H + h) * S];
      for (int i = 0; i < S; ++i) {
        bad += s[i] < 0 || s[i] >= n;
        for (int k = 0; k < i; ++k) bad += s[k] == s[i];
        if (weighted && !fb[b] && s[i] >= 0 && s[i] < n) {
          const uint64_t* P = &ws[(size_t)b * ((size_t)N + 2)];
          bad += P[s[i] + 1] == P[s[i]];
        }
      }
    }
  }
  std::printf("B=%d N=%d H=%d S=%d weighted=%d positive=%d fallback[0]=%d: %d bad\n", B, N, H, S, (int)weighted, positive, fb[0], bad);
  return bad;
}

int main() {
  int bad = 0;
  const int nv[5] = {10, 7, 40, 45, 23};
  bad += run(1, 8, 1, 8, 0, 0, false, 0, nullptr);
  bad += run(1, 9, 1, 8, 1, 0xffffffffu, false, 0, nullptr);
  bad += run(3, 257, 100, 16, 0xfedcba9876543210ull, 0, false, 0, nullptr);
  bad += run(1, 2147483647, 64, 16, 1, 0, false, 0, nullptr);
  bad += run(5, 40, 33, 10, 7, 3, false, 0, nv);
  bad += run(2, 10, 65, 10, 3, 0, true, 10, nullptr);
  bad += run(2, 40, 65, 10, 3, 0, true, 9, nullptr);
  bad += run(5, 40, 33, 10, 7, 3, true, 40, nv);
  for (int N : {sm::kScanChunk - 1, sm::kScanChunk, sm::kScanChunk + 1, 2 * sm::kScanChunk + 1}) bad += run(2, N, 65, 16, 11, 5, true, N, nullptr);
  bad += run(1, 1 << 20, 64, 16, 5, 0, true, 1 << 20, nullptr);
  std::printf(bad ? "FAILED\n" : "all sets distinct, in range and drawable\n");
  return bad != 0;
}
#endif
