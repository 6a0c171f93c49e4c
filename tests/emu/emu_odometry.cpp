// Host build of csrc/odometry_math.h (the arithmetic of dfepe_pose_chain and dfepe_snippet_errors) for
// tests/test_odometry_ref_cpu.py.  emu_pose_chain walks the association order of pose_chain_kernel (csrc/odometry.hip) for a
// given launch plan: `threads` lanes in wavefronts of 64, `chunk` consecutive poses per lane, tiles of threads * chunk poses.
// Test infrastructure only: the product never loads it.
#include <vector>

#include "odometry_math.h"

namespace {

constexpr int kWave = 64;

odo::Aff pose(const double* rel, const double* c2b, long c2b_stride, int j) {
  const odo::Aff M = odo::load(rel + 12L * j);
  if (c2b == nullptr) return M;
  return odo::conjugate(M, odo::load(c2b + c2b_stride * j));
}

}  // namespace

extern "C" {

// one sequence: rel [n,12], c2b NULL / [n,12] (stride 12) / [12] (stride 0); out [n+1,12].  Returns 0, or -1 for a bad plan.
int emu_pose_chain(const double* rel, int n, const double* c2b, long c2b_stride, int threads, int chunk, double* out) {
  if (threads < kWave || threads % kWave != 0 || chunk < 1) return -1;
  const int waves = threads / kWave, tile = threads * chunk;
  odo::store(out, odo::identity());
  odo::Aff carry = odo::identity();
  std::vector<odo::Aff> incl(threads), next(threads);
  for (int base = 0; base < n; base += tile) {
    auto j0 = [&](int t) { return base + t * chunk < n ? base + t * chunk : n; };
    auto j1 = [&](int t) { return j0(t) + chunk < n ? j0(t) + chunk : n; };
    for (int t = 0; t < threads; ++t) {
      incl[t] = odo::identity();
      for (int j = j0(t); j < j1(t); ++j) incl[t] = odo::affine_mul(pose(rel, c2b, c2b_stride, j), incl[t]);
    }
    for (int d = 1; d < kWave; d <<= 1) {  // every lane reads its neighbour's value of the step before
      for (int t = 0; t < threads; ++t) next[t] = (t % kWave >= d) ? odo::affine_mul(incl[t], incl[t - d]) : incl[t];
      incl.swap(next);
    }
    for (int t = 0; t < threads; ++t) {
      odo::Aff prefix = carry;
      for (int w = 0; w < t / kWave; ++w) prefix = odo::affine_mul(incl[w * kWave + kWave - 1], prefix);
      if (t % kWave > 0) prefix = odo::affine_mul(incl[t - 1], prefix);
      odo::Aff cur = prefix;
      for (int j = j0(t); j < j1(t); ++j) {
        cur = odo::affine_mul(pose(rel, c2b, c2b_stride, j), cur);
        odo::store(out + 12L * (j + 1), odo::affine_inv(cur));
      }
    }
    for (int w = 0; w < waves; ++w) carry = odo::affine_mul(incl[w * kWave + kWave - 1], carry);
  }
  return 0;
}

// the plain loop of get_abs_poses with the header's operations
void emu_pose_chain_sequential(const double* rel, int n, const double* c2b, long c2b_stride, double* out) {
  odo::store(out, odo::identity());
  odo::Aff last = odo::identity();
  for (int j = 0; j < n; ++j) {
    last = odo::affine_mul(pose(rel, c2b, c2b_stride, j), last);
    odo::store(out + 12L * (j + 1), odo::affine_inv(last));
  }
}

void emu_affine_inv(const double* a, double* out) { odo::store(out, odo::affine_inv(odo::load(a))); }
void emu_affine_mul(const double* a, const double* b, double* out) { odo::store(out, odo::affine_mul(odo::load(a), odo::load(b))); }
void emu_conjugate(const double* m, const double* c, double* out) { odo::store(out, odo::conjugate(odo::load(m), odo::load(c))); }

// nw windows of est, gt [m,12]: errors [nw,2] fp64 (before the kernel's rounding to float), scale [nw], aligned [nw,12],
// compensated [nw,L,12] or NULL
void emu_snippet_errors(const double* est, const double* gt, int nw, int L, int compensate, double* errors, double* scale,
                        double* aligned, double* compensated) {
  for (int w = 0; w < nw; ++w) {
    const odo::Snippet r = odo::snippet(est + 12L * w, gt + 12L * w, L, compensate != 0,
                                        compensated != nullptr ? compensated + 12L * L * w : nullptr);
    errors[2 * w] = r.ate;
    errors[2 * w + 1] = r.re;
    scale[w] = r.scale;
    odo::store(aligned + 12L * w, odo::aligned_pose(est + 12L * w, r.scale));
  }
}
}
