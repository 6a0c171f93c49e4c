// trajectory -- the KITTI odometry table on the device: first-frame re-basing, trajectory alignment, the devkit's segment errors,
// the whole-trajectory ATE and the RPE.  The per-item arithmetic is in trajectory_math.h (shared with the host emulation of the
// tests); the contract is in include/dfepe.h.  All of it is fp64, there are no atomics, and no result depends on the order in which
// workgroups or wavefronts arrive: two runs give the same bits.  One workgroup of 256 lanes per sequence, as in odometry.hip; a
// lane owns the frames tid, tid + 256, ... in every pass, so what it stored in one pass it may read back in the next.
//
// trajectory_align_kernel: pass 1 re-bases both trajectories, stores them and sums the translations; pass 2 (the Umeyama modes)
// sums the centred squares and products about the means of pass 1, as numpy's two-pass formulas do; every lane then runs the
// closed form (3x3 Jacobi SVD) on the same sums; pass 3 applies the result to the lane's own frames.
// kitti_errors_kernel: an inclusive scan of the ground truth's step lengths (shuffles across the wavefront, LDS across
// wavefronts, a carry from tile to tile), one lane per (first frame, length) pair bisecting the scanned distances for the end
// frame, then the ATE and RPE terms over the lanes' frames and one reduction for the five numbers.
// Every reduction is a fixed tree: the lane's own terms in ascending order, a butterfly across the wavefront (both partners
// add the same two numbers, so all lanes hold the same bits), the four wavefront totals left to right.
#include "dfepe_common.h"
#include "trajectory_math.h"

namespace {

constexpr int kTrajThreads = 256;
constexpr int kTrajWaves = kTrajThreads / WAVE;
constexpr int kDistLds = 4096;  // _lib.KITTI_DIST_LDS: the path length stays in LDS up to this many frames (32 KiB)
constexpr int kLens = 8;        // 100 m .. 800 m

template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*red)[K]) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) v[k] = v[k] + __shfl_xor(v[k], d, WAVE);
  }
  __syncthreads();  // red may still be read from the reduction before
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double t = red[0][k];
#pragma unroll
    for (int w = 1; w < kTrajWaves; ++w) t = t + red[w][k];
    v[k] = t;
  }
}

__device__ __forceinline__ void seq_lengths(const int* est_len, const int* gt_len, int s, int n_max, int* m, int* n) {
  int g = (gt_len != nullptr) ? gt_len[s] : n_max;
  int e = (est_len != nullptr) ? est_len[s] : n_max;
  g = min(max(g, 0), n_max);
  *n = g;
  *m = min(max(e, 0), g);  // m <= n: frame i of one is frame i of the other
}

__global__ void __launch_bounds__(kTrajThreads) trajectory_align_kernel(const double* __restrict__ est, const double* __restrict__ gt,
                                                                       const int* __restrict__ est_len, const int* __restrict__ gt_len,
                                                                       int n_max, int mode, double* est_out, double* gt_out,
                                                                       double* __restrict__ rtc) {
  __shared__ double red[kTrajWaves][10];
  const int s = blockIdx.x, tid = threadIdx.x;
  int m, n;
  seq_lengths(est_len, gt_len, s, n_max, &m, &n);
  const double* E = est + (long)s * n_max * 12;
  const double* G = gt + (long)s * n_max * 12;
  double* EO = est_out + (long)s * n_max * 12;
  double* GO = gt_out + (long)s * n_max * 12;
  const odo::Aff G0i = (n > 0) ? odo::affine_inv(odo::load(G)) : odo::identity();
  const odo::Aff E0i = (m > 0) ? odo::affine_inv(odo::load(E)) : odo::identity();
  double a[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) a[k] = 0.0;
  for (int i = tid; i < n; i += kTrajThreads) {  // a: sum x [0..2], sum y [3..5], sum x.y [6], sum x.x [7]
    const odo::Aff g = odo::affine_mul(G0i, odo::load(G + 12L * i));
    odo::store(GO + 12L * i, g);
    if (i < m) {
      const odo::Aff e = odo::affine_mul(E0i, odo::load(E + 12L * i));
      odo::store(EO + 12L * i, e);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double x = e.m[4 * c + 3], y = g.m[4 * c + 3];
        a[c] = a[c] + x;
        a[3 + c] = a[3 + c] + y;
        a[6] = a[6] + x * y;
        a[7] = a[7] + x * x;
      }
    }
  }
  traj::Sim sim = traj::identity_sim();
  if (m > 0 && mode != traj::kNone) {  // uniform over the workgroup
    block_sum<10>(a, red);
    if (mode == traj::kScale) {
      sim.c = a[6] / a[7];
    } else {
      const double mx[3] = {a[0] / (double)m, a[1] / (double)m, a[2] / (double)m};
      const double my[3] = {a[3] / (double)m, a[4] / (double)m, a[5] / (double)m};
      double q[10];  // sum |x - mx|^2 in [0], sum (y - my)(x - mx)^T in [1..9]
#pragma unroll
      for (int k = 0; k < 10; ++k) q[k] = 0.0;
      for (int i = tid; i < m; i += kTrajThreads) {
        double dx[3], dy[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          dx[c] = EO[12L * i + 4 * c + 3] - mx[c];  // this lane's own stores
          dy[c] = GO[12L * i + 4 * c + 3] - my[c];
          q[0] = q[0] + dx[c] * dx[c];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) q[1 + 3 * r + c] = q[1 + 3 * r + c] + dy[r] * dx[c];
        }
      }
      block_sum<10>(q, red);
      const double sx = q[0] / (double)m;
      double C[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) C[k] = q[1 + k] / (double)m;
      sim = traj::umeyama(mx, my, sx, C, mode != traj::k6dof);
    }
    const bool rigid = (mode == traj::k7dof || mode == traj::k6dof);
    for (int i = tid; i < m; i += kTrajThreads)
      odo::store(EO + 12L * i, traj::apply_sim(odo::load(EO + 12L * i), sim, rigid));
  }
  if (tid == 0) {
    double* o = rtc + 13L * s;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = sim.r[k];
    o[9] = sim.t[0];
    o[10] = sim.t[1];
    o[11] = sim.t[2];
    o[12] = sim.c;
  }
}

__global__ void __launch_bounds__(kTrajThreads) kitti_errors_kernel(const double* __restrict__ est, const double* __restrict__ gt,
                                                                   const int* __restrict__ est_len, const int* __restrict__ gt_len,
                                                                   int n_max, int step, int F, double* dist_g, double* __restrict__ rows,
                                                                   unsigned char* __restrict__ valid, int* __restrict__ count,
                                                                   double* __restrict__ summary) {
  __shared__ double dist_s[kDistLds];
  __shared__ double wtot[kTrajWaves];
  __shared__ double red[kTrajWaves][6];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  int m, n;
  seq_lengths(est_len, gt_len, s, n_max, &m, &n);
  const double* E = est + (long)s * n_max * 12;
  const double* G = gt + (long)s * n_max * 12;
  double* D = dist_g + (long)s * n_max;
  const bool in_lds = n <= kDistLds;

  // dist[i] = dist[i - 1] + |gt_xyz,i - gt_xyz,i-1|, dist[0] = 0
  double carry = 0.0;
  for (int base = 0; base < n; base += kTrajThreads) {
    const int i = base + tid;
    double v = (i > 0 && i < n) ? traj::step_len(G + 12L * (i - 1), G + 12L * i) : 0.0;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const double o = __shfl_up(v, (unsigned)d, WAVE);
      if (lane >= d) v = v + o;
    }
    if (lane == WAVE - 1) wtot[wave] = v;
    __syncthreads();
    double prefix = carry;
#pragma unroll
    for (int w = 0; w < kTrajWaves; ++w) {
      const double t = wtot[w];
      if (w < wave) prefix = prefix + t;
      carry = carry + t;
    }
    v = prefix + v;
    if (i < n) {
      D[i] = v;
      if (in_lds) dist_s[i] = v;
    }
    __syncthreads();  // wtot is rewritten by the next tile; after the last one dist is complete for every lane
  }

  // one lane per (first, len) pair; rows past the sequence's own first frames are not written
  const int nf = (n > 0) ? min((n - 1) / step + 1, F) : 0;
  double acc[6];  // sum t / len, sum r / len, segments, sum |gt - est|^2, sum RPE t, sum RPE angle
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = 0.0;
  for (int p = tid; p < nf * kLens; p += kTrajThreads) {
    const int first = (p / kLens) * step;
    const double len = 100.0 * (double)(p % kLens + 1);
    const double target = (in_lds ? dist_s[first] : D[first]) + len;
    // The first i in [first, n) with dist[i] > target, n without one.  The scan adds neighbouring prefixes in different
    // associations, so with a zero or tiny step dist[i + 1] can round below dist[i] by a few last places; the bisection then
    // still ends at a crossing, which can differ from the devkit's linear search only where dist is within that rounding of
    // the target (the band the tests call undecided).
    int lo = first, hi = n;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      const double d = in_lds ? dist_s[mid] : D[mid];
      if (d > target) hi = mid; else lo = mid + 1;
    }
    const int last = lo;
    const bool ok = last < n && last < m && first < m;
    double row[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (ok) {
      traj::segment_row(odo::load(E + 12L * first), odo::load(E + 12L * last), odo::load(G + 12L * first), odo::load(G + 12L * last),
                        first, last, len, row);
      acc[0] = acc[0] + row[2];
      acc[1] = acc[1] + row[1];
      acc[2] = acc[2] + 1.0;
    }
    const long o = (long)s * F * kLens + p;
#pragma unroll
    for (int k = 0; k < 5; ++k) rows[5 * o + k] = row[k];
    valid[o] = ok ? 1 : 0;
  }
  for (int i = tid; i < m; i += kTrajThreads) {
    acc[3] = acc[3] + traj::ate_term(E + 12L * i, G + 12L * i);
    if (i + 1 < m) {
      const traj::RelErr r = traj::rpe_term(odo::load(E + 12L * i), odo::load(E + 12L * (i + 1)), odo::load(G + 12L * i),
                                            odo::load(G + 12L * (i + 1)));
      acc[4] = acc[4] + r.trans;
      acc[5] = acc[5] + r.angle;
    }
  }
  block_sum<6>(acc, red);
  if (tid == 0) {
    const double cnt = acc[2], pairs = (double)max(m - 1, 0);
    count[s] = (int)cnt;
    double* o = summary + 5L * s;
    o[0] = cnt > 0.0 ? 100.0 * (acc[0] / cnt) : 0.0;                                 // as the devkit: 0 without segments
    o[1] = cnt > 0.0 ? (acc[1] / cnt) * 180.0 / 3.141592653589793 * 100.0 : 0.0;
    o[2] = sqrt(acc[3] / (double)m);                                                  // m == 0: 0 / 0 = NaN, numpy's mean of nothing
    o[3] = acc[4] / pairs;                                                            // m <= 1: 0 / 0
    o[4] = (acc[5] / pairs) * 180.0 / 3.141592653589793;
  }
}

}  // namespace

extern "C" int dfepe_trajectory_align(void* stream, const double* est, const double* gt, const int* est_len, const int* gt_len, int S,
                                      int n_max, int mode, double* est_out, double* gt_out, double* rtc) {
  if (S < 0 || n_max < 0 || mode < traj::kNone || mode > traj::k6dof) return DFEPE_ERR_INVALID_ARG;
  if (S == 0) return DFEPE_OK;  // nothing to read or write: empty tensors have no address
  if (!rtc || (n_max > 0 && (!est || !gt || !est_out || !gt_out))) return DFEPE_ERR_INVALID_ARG;
  if (n_max > 0x7fffffff / 12 - 1) return DFEPE_ERR_UNSUPPORTED;  // 12 i is formed in int
  hipLaunchKernelGGL(trajectory_align_kernel, dim3((unsigned)S), dim3(kTrajThreads), 0, static_cast<hipStream_t>(stream), est, gt,
                     est_len, gt_len, n_max, mode, est_out, gt_out, rtc);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}

extern "C" int dfepe_kitti_odometry_errors(void* stream, const double* est, const double* gt, const int* est_len, const int* gt_len,
                                           int S, int n_max, int step, int F, double* dist, double* rows, unsigned char* valid,
                                           int* count, double* summary) {
  if (S < 0 || n_max < 0 || step < 1 || F < 0) return DFEPE_ERR_INVALID_ARG;
  if (S == 0) return DFEPE_OK;
  if (!count || !summary || (n_max > 0 && (!est || !gt || !dist)) || (F > 0 && (!rows || !valid))) return DFEPE_ERR_INVALID_ARG;
  if (n_max > 0x7fffffff / 12 - 1 || F > 0x7fffffff / (5 * kLens)) return DFEPE_ERR_UNSUPPORTED;
  if ((long)F * step < n_max) return DFEPE_ERR_INVALID_ARG;  // rows must hold every first frame
  hipLaunchKernelGGL(kitti_errors_kernel, dim3((unsigned)S), dim3(kTrajThreads), 0, static_cast<hipStream_t>(stream), est, gt, est_len,
                     gt_len, n_max, step, F, dist, rows, valid, count, summary);
  return (hipGetLastError() == hipSuccess) ? DFEPE_OK : DFEPE_ERR_HIP;
}
