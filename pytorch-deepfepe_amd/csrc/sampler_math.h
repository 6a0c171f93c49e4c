// sampler_math.h -- per-lane arithmetic of the device-side DSAC sampler (csrc/sampler.hip), written once for the device and for the
// host (tests/emu/emu_sampler.cpp compiles it with g++).  The contract is in include/dfepe.h (dfepe_sample_sets), the algorithm in
// DESIGN.md 3.21, the restatement in Python integers in tests/sampler_ref.py.  Everything here is integer arithmetic on 32- and
// 64-bit words, a float is only ever looked at through its bits: the kernel, the host build and the restatement agree bit for bit,
// whatever the denormal mode or the contraction setting of the translation unit is.
//
//   generator   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers
//               0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds.
//   streams     key = (seed & 0xffffffff, seed >> 32); counter = (k, h, b, off): block k of hypothesis h of pair b.  Block k yields
//               the words 4k .. 4k+3, draw j of a hypothesis uses r64 = word[2j+1] << 32 | word[2j].  A hypothesis uses exactly 2 S <= 32
//               words: no rejection loop, no divergence.  A set depends on (seed, off, b, h, n, S) and its pair's weights only.
//   bounded     t = mulhi64(r64, range) in [0, range).  A value is hit by floor or ceil of 2^64 / range of the 2^64 words, so its
//               probability is off by less than 2^-64 and the bias of a draw, summed over its values, is at most range / 2^64:
//               < 2^-33 in uniform mode (range < 2^31); in weighted mode range = the mass left < N 2^30, i.e. < 2^-24 at N = 1000
//               and < 2^-14 at the largest N, 2^20.  It is stated, not removed: a rejection loop would make lanes diverge and the
//               number of words a hypothesis uses vary.
//   uniform     Floyd's subset algorithm over 0..n-1: for i = 0 .. S-1, j = n - S + i, t = mulhi64(r64_i, j + 1), take j if t is
//               already in the set, else t.  Every S-subset has the same probability (random.sample's law for the SET).  The ORDER
//               within a set is not uniform (n - 1 can only come last) and need not be: the fit and the vote are symmetric in the
//               sample.  No memory: n may be anything up to 2^31 - 1.
//   weighted    successive sampling without replacement in proportion to quantised weights q (quantise below), over the exclusive
//               prefix sums P[0..n] of q: weighted_set.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SM_HD __host__ __device__ inline
#else
#define SM_HD inline
#endif

namespace sm {

constexpr int kMinSample = 8, kMaxSample = 16;
constexpr int kScanThreads = 256;                         // lanes of the one workgroup that scans a pair's weights
constexpr int kScanPerLane = 4;                           // consecutive weights per lane and chunk
constexpr int kScanChunk = kScanThreads * kScanPerLane;   // weights per chunk; the carry goes from chunk to chunk (dfepe_sampler_scan_chunk)
constexpr int kQuantBits = 30;                            // the largest weight of a pair quantises into [2^29, 2^30)
constexpr int kMaxWeightedN = 1 << 20;                    // so that P[n] <= 2^20 * 2^30 = 2^50 <= 2^61
constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;

SM_HD uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

SM_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// Philox4x32-10: c[4] counter in, the four output words out (in place).
SM_HD void philox4x32_10(uint32_t* c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(kM0, c[0]), lo0 = kM0 * c[0];
    const uint32_t hi1 = mulhi32(kM1, c[2]), lo1 = kM1 * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += kW0; k1 += kW1;
  }
}

// The word stream of one hypothesis.  next64 gives r64 of draw j; the draws are asked for in ascending j (a block serves two).
struct Stream {
  uint32_t k0, k1, h, b, off;
  uint32_t w[4];
};
SM_HD Stream make_stream(uint64_t seed, uint32_t off, uint32_t b, uint32_t h) {
  Stream s;
  s.k0 = (uint32_t)(seed & 0xffffffffu); s.k1 = (uint32_t)(seed >> 32);
  s.h = h; s.b = b; s.off = off;
  s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0u;
  return s;
}
SM_HD uint64_t next64(Stream& s, int j) {
  if ((j & 1) == 0) {
    s.w[0] = (uint32_t)(j >> 1); s.w[1] = s.h; s.w[2] = s.b; s.w[3] = s.off;
    philox4x32_10(s.w, s.k0, s.k1);
    return ((uint64_t)s.w[1] << 32) | (uint64_t)s.w[0];
  }
  return ((uint64_t)s.w[3] << 32) | (uint64_t)s.w[2];
}

// n = clamp(n_valid, S, N): the correspondences of a pair that can be drawn.
SM_HD int clamp_valid(int n_valid, int S, int N) { return n_valid < S ? S : (n_valid > N ? N : n_valid); }

// Uniform mode.  out[0 .. S-1], in the order generated; out has kMaxSample slots.
SM_HD void uniform_set(Stream& s, int n, int S, int* out) {
#pragma unroll
  for (int i = 0; i < kMaxSample; ++i) {
    if (i < S) {
      const int j = n - S + i;
      const int t = (int)mulhi64(next64(s, i), (uint64_t)j + 1u);
      bool hit = false;
#pragma unroll
      for (int k = 0; k < i; ++k) hit = hit || out[k] == t;
      out[i] = hit ? j : t;
    }
  }
}

// ---- weighted mode -----------------------------------------------------------------------------------------------------------------
// A weight can be drawn when it is positive and finite (not NaN, not +-inf, not <= 0): as bits, 0 < bits < 0x7f800000.  Among such
// floats the order of the values is the order of the bits, so the largest weight of a pair is the largest word.
SM_HD bool drawable(uint32_t bits) { return bits - 1u < 0x7f7fffffu; }

// e of frexp: bits = f 2^e with f in [0.5, 1), for a drawable float (denormals included).
SM_HD int frexp_exponent(uint32_t bits) {
  const int E = (int)(bits >> 23);
  if (E != 0) return E - 126;
  return (32 - __builtin_clz(bits)) - 149;
}

// q = floor(w 2^(30 - e)), e = frexp_exponent(largest drawable weight of the pair): the scaling is a shift of the significand, exact,
// no division.  The largest weight gives [2^29, 2^30); a weight below 2^-30 of it gives 0 and is never drawn; so does a weight that is
// not drawable.  w <= the largest is the caller's business (it is the maximum): the left shift then stays below 2^30.
SM_HD uint32_t quantise(uint32_t bits, int e) {
  if (!drawable(bits)) return 0u;
  const int E = (int)(bits >> 23);
  const uint32_t M = E != 0 ? ((bits & 0x7fffffu) | 0x800000u) : bits;  // w = M 2^x
  const int x = (E != 0 ? E : 1) - 150;
  const int sh = x + kQuantBits - e;
  if (sh >= 0) return M << sh;
  return sh <= -24 ? 0u : (M >> (-sh));
}

// P[0 .. n]: exclusive prefix sums of q (P[0] = 0, P[n] = the total), q[i] = P[i+1] - P[i].  Draw k: total = P[n] - sum of the chosen
// q, t = mulhi64(r64_k, total): the t-th unit of what is left.  Its place among ALL units is u = t + rem, rem = the mass of the chosen
// indices that lie before it: walk the chosen ones by ascending index, `while u >= P[c]: u += q[c]`, stop at the first c that fails
// (the later ones start even further right).  The index drawn is the largest i < n with P[i] <= u, by binary search: P[i+1] > u, so
// q[i] > 0, and u lies in no chosen interval, so i is new.  The chosen ones are kept sorted by an insertion with fixed slots (no
// dynamic register index).  Needs at least S indices with q > 0 (the caller falls back to uniform_set otherwise).
SM_HD void weighted_set(Stream& s, const uint64_t* P, int n, int S, int* out) {
  uint64_t cp[kMaxSample];  // P[c] of the chosen, ascending
  uint32_t cq[kMaxSample];  // their q
  uint64_t total = P[n];
#pragma unroll
  for (int k = 0; k < kMaxSample; ++k) {
    if (k < S) {
      uint64_t u = mulhi64(next64(s, k), total);
#pragma unroll
      for (int c = 0; c < k; ++c)
        if (u >= cp[c]) u += (uint64_t)cq[c];
      int lo = 0, hi = n;
      while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (P[mid] <= u) lo = mid; else hi = mid;
      }
      out[k] = lo;
      uint64_t ip = P[lo];
      uint32_t iq = (uint32_t)(P[lo + 1] - ip);
      total -= (uint64_t)iq;
#pragma unroll
      for (int c = 0; c < k; ++c) {
        if (cp[c] > ip) {
          const uint64_t tp = cp[c]; cp[c] = ip; ip = tp;
          const uint32_t tq = cq[c]; cq[c] = iq; iq = tq;
        }
      }
      cp[k] = ip; cq[k] = iq;
    }
  }
}

}  // namespace sm
