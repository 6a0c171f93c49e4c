// Host build of csrc/eight_point_adjoint_math.h: the launches of csrc/eight_point_adjoint.hip as plain loops with the arguments of
// the C ABI (include/dfepe.h) minus the stream and the workspace, for valid arguments only (the refusals are the library's and are
// tested against it).  The sums over the correspondences follow the kernel: lane l adds n = l, l + 64, ... in order, the 64 partial
// sums go through the balanced tree; the weight sets are added in ascending order in fp64 and rounded once.
#include <cstddef>
#include <vector>

#include "eight_point_adjoint_math.h"

namespace {

constexpr unsigned kForce110 = 16u, kNoHartley = 32u;  // DFEPE_W8PT_FORCE_110, DFEPE_W8PT_NO_HARTLEY

inline double tree_sum64(double* v) {
  for (int step = 1; step < e8::kLanes; step *= 2)
    for (int i = 0; i < e8::kLanes; i += 2 * step) v[i] = v[i] + v[i + step];
  return v[0];
}

}  // namespace

// The 3x3 SVD of the dense step on its own: F [9] -> U [9], s [3], V [9], all row-major.
extern "C" void emu_eight_point_svd3(const double* F, double* U, double* s, double* V) { e8::svd3(F, U, s, V); }

extern "C" int emu_eight_point_bwd(const float* X, const float* Y, const float* w, int B, int N, int S, unsigned flags,
                                   const float* F_out, const float* g_F, float* g_X, float* g_Y, float* g_w) {
  const bool hartley = (flags & kNoHartley) == 0, force110 = (flags & kForce110) != 0;
  std::vector<double> partial((size_t)S * B * N * 4);
  for (int set = 0; set < S; ++set) {
    for (int pair = 0; pair < B; ++pair) {
      const size_t problem = (size_t)set * B + pair;
      const float* x = X + (size_t)pair * N * 2;
      const float* y = Y + (size_t)pair * N * 2;
      const float* wt = w ? w + problem * N : nullptr;
      e8::Norm t1 = {0.0, 0.0, 1.0}, t2 = {0.0, 0.0, 1.0};
      double lanes[4][e8::kLanes];
      if (hartley) {
        for (int k = 0; k < 4; ++k)
          for (int l = 0; l < e8::kLanes; ++l) lanes[k][l] = 0.0;
        for (int n = 0; n < N; ++n) {
          const int l = n % e8::kLanes;
          lanes[0][l] += (double)x[2 * n]; lanes[1][l] += (double)x[2 * n + 1];
          lanes[2][l] += (double)y[2 * n]; lanes[3][l] += (double)y[2 * n + 1];
        }
        t1.cx = tree_sum64(lanes[0]) / (double)N; t1.cy = tree_sum64(lanes[1]) / (double)N;
        t2.cx = tree_sum64(lanes[2]) / (double)N; t2.cy = tree_sum64(lanes[3]) / (double)N;
        for (int k = 0; k < 2; ++k)
          for (int l = 0; l < e8::kLanes; ++l) lanes[k][l] = 0.0;
        for (int n = 0; n < N; ++n) {
          const int l = n % e8::kLanes;
          const double ax = (double)x[2 * n] - t1.cx, ay = (double)x[2 * n + 1] - t1.cy;
          const double bx = (double)y[2 * n] - t2.cx, by = (double)y[2 * n + 1] - t2.cy;
          lanes[0][l] += sqrt(ax * ax + ay * ay);
          lanes[1][l] += sqrt(bx * bx + by * by);
        }
        t1.s = sqrt(2.0) / (tree_sum64(lanes[0]) / (double)N);
        t2.s = sqrt(2.0) / (tree_sum64(lanes[1]) / (double)N);
      }
      std::vector<double> m((size_t)e8::kLanes * 45, 0.0);
      for (int n = 0; n < N; ++n) {
        double p1[2], p2[2], r[9];
        e8::normalized(t1, hartley, (double)x[2 * n], (double)x[2 * n + 1], p1);
        e8::normalized(t2, hartley, (double)y[2 * n], (double)y[2 * n + 1], p2);
        e8::row(p1, p2, r);
        e8::accumulate(r, wt ? (double)wt[n] : 1.0, &m[(size_t)(n % e8::kLanes) * 45]);
      }
      double m45[45];
      for (int k = 0; k < 45; ++k) {
        double v[e8::kLanes];
        for (int l = 0; l < e8::kLanes; ++l) v[l] = m[(size_t)l * 45 + k];
        m45[k] = tree_sum64(v);
      }
      double Fo[9], gF[9], work[e8::kDenseDoubles], f[9], u[9];
      for (int c = 0; c < 9; ++c) {
        Fo[c] = (double)F_out[problem * 9 + c];
        gF[c] = (double)g_F[problem * 9 + c];
      }
      e8::dense_step(m45, t1, t2, hartley, force110, Fo, gF, work, f, u);
      const double sc1 = hartley ? t1.s / e8::kDeHomo : 1.0, sc2 = hartley ? t2.s / e8::kDeHomo : 1.0;
      for (int n = 0; n < N; ++n) {
        double p1[2], p2[2], gw;
        e8::normalized(t1, hartley, (double)x[2 * n], (double)x[2 * n + 1], p1);
        e8::normalized(t2, hartley, (double)y[2 * n], (double)y[2 * n + 1], p2);
        e8::point_adjoint(p1, p2, wt ? (double)wt[n] : 1.0, f, u, sc1, sc2, N == 8, &partial[(problem * N + n) * 4], &gw);
        if (g_w) g_w[problem * N + n] = (float)gw;
      }
    }
  }
  const size_t points = (size_t)B * N;
  for (size_t i = 0; i < points; ++i) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (S == 1) {
      for (int k = 0; k < 4; ++k) acc[k] = partial[i * 4 + k];
    } else {
      for (int set = 0; set < S; ++set)
        for (int k = 0; k < 4; ++k) acc[k] += partial[((size_t)set * points + i) * 4 + k];
    }
    if (g_X) { g_X[2 * i] = (float)acc[0]; g_X[2 * i + 1] = (float)acc[1]; }
    if (g_Y) { g_Y[2 * i] = (float)acc[2]; g_Y[2 * i + 1] = (float)acc[3]; }
  }
  return 0;
}
