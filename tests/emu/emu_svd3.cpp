// Host build of csrc/dfepe_math.h's closed-form 3x3 SVD (svd3_closed) for tests/test_pose_helper_ref_cpu.py -- TEST INFRASTRUCTURE
// ONLY, the product never loads it.  The hardware seeds come from tests/emu/rowgroup.h (24-bit reciprocal / reciprocal square root),
// so the Newton steps of the header run as they do on the device.
//   g++ -O1 -std=c++17 -shared -fPIC -Itests/emu -Ipytorch-deepfepe_amd/csrc tests/emu/emu_svd3.cpp -o tests/emu/_build/libemu_svd3.so
#include "rowgroup.h"  // the emulation (this directory comes first on the include path)
#include "dfepe_math.h"

thread_local emu::Row* emu::g_row = nullptr;

constexpr int kGeoNewton = 64;  // as csrc/geom.hip instantiates it for kinds 3 and 4

extern "C" {

// F [n,9] -> U, V [n,9], S [n,3]: F = U diag(S) V^T
void emu_svd3_closed(const double* F, int n, double* U, double* S, double* V) {
  for (int i = 0; i < n; ++i) svd3_closed<kGeoNewton>(F + 9 * i, U + 9 * i, S + 3 * i, V + 9 * i);
}

// kind 3 of geo_misc_kernel (csrc/geom.hip) up to its last line: float32 E [n,9] widened, U diag(1, 1, 0) V^T in float64 (out64) and
// rounded once to float32 (out32)
void emu_project_essential(const float* E32, int n, double* out64, float* out32) {
  for (int i = 0; i < n; ++i) {
    double E[9], U[9], S[3], V[9];
    for (int k = 0; k < 9; ++k) E[k] = (double)E32[9 * i + k];
    svd3_closed<kGeoNewton>(E, U, S, V);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const double e = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1];
        out64[9 * i + 3 * r + c] = e;
        out32[9 * i + 3 * r + c] = (float)e;
      }
  }
}
}
