// Host build of csrc/homography_math.h (the per-lane arithmetic of the RANSAC homography estimator) for
// tests/test_homography_ref_cpu.py.  A stand-alone program: emu_homography IN OUT reads binary records from IN and writes the
// answers to OUT, so that it can also be built with -fsanitize=address,undefined and run on its own.
// Test infrastructure only: the product never loads it.
//
// Records (little endian, packed in order):
//   1 sample   u64 seed, i32 k, i32 n, f32 pts[n][4]                   -> i32 ok, i32 idx[4]
//   2 solve4   f32 pts[4][4]                                           -> i32 ok, f64 H[9]
//   3 select   i32 n, f64 confidence, i32 max_iters, i32 table[]       -> i32 best, i32 best_k, i32 iters
//   4 iters    f64 p, f64 ep, i32 niters                               -> i32
//   5 pair     i32 n, f64 threshold, f64 confidence, i32 max_iters, u64 seed, u32 flags, f32 pts[n][4]
//              -> i32 table[max_iters], i32 best, best_k, iters, f64 H_model[9], u8 mask[n], i32 refit_ok, f64 H_refit[9],
//                 f64 H_out[9], i32 lm_iters, f64 R[10], f64 S0, f64 S1
//              the whole estimate of one pair, launch by launch as csrc/homography.hip does it, with sequential sums
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "homography_math.h"

namespace {

struct P4 {
  float x, y, z, w;
};

struct HostCtx {
  const P4* m;
  const unsigned char* mask;
  int n;
  bool leader() const { return true; }
  void sync() const {}
  template <int KIND>
  void run(const double* par, double* out, int first, int last) const {
    double acc[hg::kRed];
    for (int i = 0; i < hg::kRed; ++i) acc[i] = 0.0;
    for (int i = 0; i < n; ++i)
      if (mask[i]) hg::point_add<KIND>(par, m[i].x, m[i].y, m[i].z, m[i].w, acc);
    for (int i = first; i < last; ++i) out[i] = acc[i];
  }
  void reduce(int kind, const double* par, double* out) const {
    switch (kind) {
      case hg::kSum: run<hg::kSum>(par, out, 0, 4); break;
      case hg::kAbs: run<hg::kAbs>(par, out, 0, 4); break;
      case hg::kLtL: run<hg::kLtL>(par, out, 0, 45); break;
      case hg::kLmFull: run<hg::kLmFull>(par, out, 0, 46); break;
      default: run<hg::kLmRes>(par, out, 44, 46); break;
    }
  }
};

struct Reader {
  FILE* f;
  template <class T>
  bool get(T* v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }
};
struct Writer {
  FILE* f;
  template <class T>
  void put(const T* v, size_t n = 1) { fwrite(v, sizeof(T), n, f); }
};

void do_pair(Reader& in, Writer& out) {
  int n, max_iters;
  double threshold, confidence;
  unsigned long long seed;
  unsigned flags;
  in.get(&n); in.get(&threshold); in.get(&confidence); in.get(&max_iters); in.get(&seed); in.get(&flags);
  std::vector<P4> pts((size_t)(n > 0 ? n : 1));
  if (n > 0) in.get(pts.data(), (size_t)n);
  const P4* p = pts.data();
  if (!(threshold > 0.0)) threshold = 3.0;
  const double t2 = threshold * threshold;
  const bool all = flags & 1u, norefine = flags & 2u;
  const bool sampled = n > 4 && !all;
  std::vector<int> table((size_t)max_iters, rs::kNoSample);
  auto at = [&](int i) { return p[i]; };
  if (sampled) {
    for (int k = 0; k < max_iters; ++k) {
      double H[9];
      const int st = hg::solve_iteration(seed, k, n, at, H);
      if (st == rs::kNoSample) continue;
      if (st == 0) { table[k] = rs::kNoRoot; continue; }
      int c = 0;
      for (int i = 0; i < n; ++i) c += hg::is_inlier(H, p[i].x, p[i].y, p[i].z, p[i].w, t2) ? 1 : 0;
      table[k] = c;
    }
  }
  int best = 0, bk = -1, iters = 0;
  double Hm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (sampled) best = hg::select_best(table.data(), n, confidence, max_iters, &bk, &iters);
  if (n == 4 || (sampled && bk >= 0)) {
    const int all4[4] = {0, 1, 2, 3};
    double H[9];
    const bool ok = sampled ? hg::solve_iteration(seed, bk, n, at, H) == 1 : hg::solve_sample(at, all4, H);
    if (ok) memcpy(Hm, H, sizeof(H));
    if (!sampled) best = ok ? 4 : 0;
  } else if (n > 4 && all) {
    best = n;
  }
  std::vector<unsigned char> mask((size_t)(n > 0 ? n : 1), 0);
  for (int i = 0; i < n; ++i)
    mask[i] = (best > 0) && ((n == 4 || all) ? true : hg::is_inlier(Hm, p[i].x, p[i].y, p[i].z, p[i].w, t2));
  int refit_ok = 0, lm_iters = 0;
  double Hr[9], Ho[9], R[hg::kLmIters], S0 = 0.0, S1 = 0.0;
  for (int i = 0; i < hg::kLmIters; ++i) R[i] = NAN;
  memcpy(Hr, Hm, sizeof(Hm));
  memcpy(Ho, Hm, sizeof(Hm));
  if (best > 0 && n > 4) {
    static hg::Work W;
    HostCtx ctx{p, mask.data(), n};
    memcpy(W.H, Hm, sizeof(Hm));
    refit_ok = hg::refit(ctx, W, best) ? 1 : 0;
    if (all && !refit_ok) {
      best = 0;
      for (int i = 0; i < n; ++i) mask[i] = 0;
      memset(Hm, 0, sizeof(Hm)); memset(Hr, 0, sizeof(Hr)); memset(Ho, 0, sizeof(Ho));
    } else {
      if (all) memcpy(Hm, W.H, sizeof(Hm));
      memcpy(Hr, W.H, sizeof(Hr));
      if (!norefine) {
        for (int i = 0; i < 8; ++i) W.h[i] = W.H[i];
        lm_iters = hg::lm_refine(ctx, W, R, &S0, &S1);
        for (int i = 0; i < 8; ++i) W.H[i] = W.h[i];
      }
      memcpy(Ho, W.H, sizeof(Ho));
    }
  }
  out.put(table.data(), (size_t)max_iters);
  out.put(&best); out.put(&bk); out.put(&iters);
  out.put(Hm, 9);
  if (n > 0) out.put(mask.data(), (size_t)n);
  out.put(&refit_ok); out.put(Hr, 9); out.put(Ho, 9); out.put(&lm_iters); out.put(R, hg::kLmIters); out.put(&S0); out.put(&S1);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  Reader in{fi};
  Writer out{fo};
  int op;
  while (in.get(&op)) {
    if (op == 1) {
      unsigned long long seed;
      int k, n;
      in.get(&seed); in.get(&k); in.get(&n);
      std::vector<P4> pts((size_t)n);
      in.get(pts.data(), (size_t)n);
      const P4* p = pts.data();
      auto at = [&](int i) { return p[i]; };
      int idx[4] = {-1, -1, -1, -1};
      const int ok = hg::draw_sample4(seed, k, n, at, idx) ? 1 : 0;
      out.put(&ok); out.put(idx, 4);
    } else if (op == 2) {
      P4 p[4];
      in.get(p, 4);
      const int idx[4] = {0, 1, 2, 3};
      auto at = [&](int i) { return p[i]; };
      double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      const int ok = hg::solve_sample(at, idx, H) ? 1 : 0;
      out.put(&ok); out.put(H, 9);
    } else if (op == 3) {
      int n, max_iters;
      double confidence;
      in.get(&n); in.get(&confidence); in.get(&max_iters);
      std::vector<int> table((size_t)max_iters);
      in.get(table.data(), (size_t)max_iters);
      int r[3];
      r[0] = hg::select_best(table.data(), n, confidence, max_iters, &r[1], &r[2]);
      out.put(r, 3);
    } else if (op == 4) {
      double p, ep;
      int niters;
      in.get(&p); in.get(&ep); in.get(&niters);
      const int r = hg::update_num_iters4(p, ep, niters);
      out.put(&r);
    } else if (op == 5) {
      do_pair(in, out);
    } else {
      fprintf(stderr, "unknown record %d\n", op);
      return 3;
    }
  }
  fclose(fi);
  fclose(fo);
  return 0;
}
