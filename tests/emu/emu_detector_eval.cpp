// Host build of csrc/detector_eval_math.h: a stand-alone program that runs the launches of csrc/detector_eval.hip one after the
// other over records read from a file, with the sums in index order.  tests/test_detector_eval_ref_cpu.py feeds it and checks
// the output through the same check() as the GPU; it is also built with -fsanitize=address,undefined and run on its own.
//   usage: emu_detector_eval <in> <out>
//   record 1 (repeatability of a pair): int32 1, n1, n2, C, height, width, keep_k, T; double H[9], thresh[T], kp1[n1*C], kp2[n2*C]
//     -> int32 kept1, kept2, n_unwarped, count1[T], count2[T]; double repeatability[T], loc_err[T]
//   record 2 (average precision): int32 2, m; uint8 labels[m]; double scores[m] -> double ap; int32 n_pos, tp_at[m], cnt_at[m]
//   record 3 (matching score): int32 3, n_inliers, n_kp1, n_unwarped -> double mscore
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "detector_eval_math.h"

namespace {

struct Reader {
  std::vector<unsigned char> buf;
  size_t off = 0;
  template <class T>
  bool take(T* out, size_t count) {
    if (count == 0) return true;
    if (off + count * sizeof(T) > buf.size()) return false;
    std::memcpy(out, buf.data() + off, count * sizeof(T));
    off += count * sizeof(T);
    return true;
  }
};

template <class T>
void put(std::vector<unsigned char>& out, const T* v, size_t count) {
  if (count == 0) return;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(v);
  out.insert(out.end(), p, p + count * sizeof(T));
}

struct Set {  // what the select launch leaves of one image
  std::vector<double> x, y;
  std::vector<uint64_t> key;
  std::vector<unsigned char> sel;
  int kept = 0, unwarped = 0;
};

Set select(const std::vector<double>& kp, int n, int C, const double* M, bool image2, int height, int width, int keep_k) {
  Set s;
  s.x.resize(n); s.y.resize(n); s.key.assign(n, 0); s.sel.assign(n, 0);
  int nk = 0;
  for (int i = 0; i < n; ++i) {
    const double x = kp[(size_t)i * C], y = kp[(size_t)i * C + 1];
    double wx, wy;
    de::warp(M, x, y, &wx, &wy);
    s.x[i] = image2 ? x : wx;
    s.y[i] = image2 ? y : wy;
    if (de::inside_half_open(wx, wy, height, width)) {
      s.key[i] = (C == 3) ? de::prob_key(kp[(size_t)i * C + 2]) : 1ull;
      ++nk;
    }
    if (de::inside_closed(wx, wy, height, width)) ++s.unwarped;
  }
  const bool all = (C == 2) || keep_k == 0 || keep_k >= nk;
  s.kept = all ? nk : keep_k;
  for (int i = 0; i < n; ++i) {
    bool keep = s.key[i] != 0;
    if (keep && !all) {
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += (s.key[j] != 0 && de::stands_after(s.key[j], j, s.key[i], i)) ? 1 : 0;
      keep = de::selected(rank, keep_k, nk);
    }
    s.sel[i] = keep ? 1 : 0;
  }
  return s;
}

std::vector<double> nearest(const Set& own, const Set& other) {
  std::vector<double> mind(own.x.size(), INFINITY);
  for (size_t i = 0; i < own.x.size(); ++i) {
    if (!own.sel[i]) continue;
    double best = INFINITY;
    for (size_t j = 0; j < other.x.size(); ++j) {
      if (!other.sel[j]) continue;
      const double d2 = de::dist2(own.x[i], own.y[i], other.x[j], other.y[j]);
      if (d2 < best) best = d2;
    }
    mind[i] = sqrt(best);
  }
  return mind;
}

bool repeatability(Reader& in, std::vector<unsigned char>& out) {
  int h[7];
  if (!in.take(h, 7)) return false;
  const int n1 = h[0], n2 = h[1], C = h[2], height = h[3], width = h[4], keep_k = h[5], T = h[6];
  if (n1 < 0 || n2 < 0 || n1 > de::kMaxN || n2 > de::kMaxN || (C != 2 && C != 3) || T < 0 || T > 64 || keep_k < 0) return false;
  double H[9], A[9];
  std::vector<double> thresh(T), kp1((size_t)n1 * C), kp2((size_t)n2 * C);
  if (!in.take(H, 9) || !in.take(thresh.data(), T) || !in.take(kp1.data(), kp1.size()) || !in.take(kp2.data(), kp2.size())) return false;
  de::adjugate(H, A);
  const Set s1 = select(kp1, n1, C, H, false, height, width, keep_k);
  const Set s2 = select(kp2, n2, C, A, true, height, width, keep_k);
  const std::vector<double> min1 = nearest(s1, s2), min2 = nearest(s2, s1);
  const int head[3] = {s1.kept, s2.kept, s2.unwarped};
  put(out, head, 3);
  std::vector<int> c1(T, 0), c2(T, 0);
  std::vector<double> rep(T), loc(T);
  for (int t = 0; t < T; ++t) {
    double sum1 = 0.0, sum2 = 0.0;
    if (s2.kept > 0)
      for (int i = 0; i < n1; ++i)
        if (s1.sel[i] && min1[i] <= thresh[t]) { ++c1[t]; sum1 += min1[i]; }
    if (s1.kept > 0)
      for (int i = 0; i < n2; ++i)
        if (s2.sel[i] && min2[i] <= thresh[t]) { ++c2[t]; sum2 += min2[i]; }
    rep[t] = de::repeatability_of(c1[t], c2[t], s1.kept, s2.kept);
    loc[t] = de::loc_err_of(c1[t], c2[t], sum1, sum2);
  }
  put(out, c1.data(), T); put(out, c2.data(), T); put(out, rep.data(), T); put(out, loc.data(), T);
  return true;
}

bool average_precision(Reader& in, std::vector<unsigned char>& out) {
  int m;
  if (!in.take(&m, 1) || m < 0 || m > de::kMaxN) return false;
  std::vector<unsigned char> lab(m);
  std::vector<double> sc(m);
  if (!in.take(lab.data(), m) || !in.take(sc.data(), m)) return false;
  std::vector<int> tp(m, 0), cnt(m, 0);
  int P = 0;
  double acc = 0.0;
  for (int i = 0; i < m; ++i) P += lab[i] ? 1 : 0;
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j < m; ++j) {
      const int ge = (sc[j] >= sc[i]) ? 1 : 0;
      cnt[i] += ge;
      tp[i] += ge & (lab[j] ? 1 : 0);
    }
    if (lab[i]) acc += de::ap_term(tp[i], cnt[i]);
  }
  const double ap = (P > 0) ? acc / (double)P : 0.0;
  put(out, &ap, 1); put(out, &P, 1); put(out, tp.data(), m); put(out, cnt.data(), m);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  Reader in;
  if (FILE* f = std::fopen(argv[1], "rb")) {
    unsigned char chunk[65536];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) in.buf.insert(in.buf.end(), chunk, chunk + got);
    std::fclose(f);
  } else { std::perror(argv[1]); return 2; }
  std::vector<unsigned char> out;
  while (in.off < in.buf.size()) {
    int type;
    bool ok = in.take(&type, 1);
    if (ok && type == 1) ok = repeatability(in, out);
    else if (ok && type == 2) ok = average_precision(in, out);
    else if (ok && type == 3) {
      int v[3];
      ok = in.take(v, 3);
      if (ok) { const double s = de::matching_score(v[0], v[1], v[2]); put(out, &s, 1); }
    } else ok = false;
    if (!ok) { std::fprintf(stderr, "bad record at byte %zu\n", in.off); return 1; }
  }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  if (!out.empty()) std::fwrite(out.data(), 1, out.size(), f);
  std::fclose(f);
  return 0;
}
