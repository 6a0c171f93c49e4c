// detector_eval -- the front-end detector evaluation of the reference, batched over image pairs: compute_repeatability
// (evaluations/detector_evaluation.py:150-279), the matching score (deepFEPE/evaluate_frontend.py:176-183) and the nn mean AP
// (evaluate_frontend.py:185-275).  The per-lane arithmetic is in detector_eval_math.h (shared with the host emulation of the
// tests); the contract is in include/dfepe.h.  Everything is fp64, nothing is atomic, every cell has one writer and every sum a
// fixed order, so two calls on the same input are bit-identical.  The launches of dfepe_keypoint_repeatability:
//   select   one 256-thread workgroup per (pair, image): one lane per point warps it (image 1 by H, image 2 by adj(H)), applies
//            the inside tests and writes the point, its probability key (0: dropped) and, after a rank count over the keys
//            staged in LDS in tiles of kTile, whether select_k_best keeps it; the kept sizes and n_unwarped leave here.
//   nearest  one lane per kept point of one image, the other image's points staged in LDS in tiles of kTile (NaN for a point that
//            is not kept): the distance to the nearest kept point.  blockIdx.z swaps the roles, so the row and the column minima
//            come from one device function.
//   reduce   one workgroup per pair: per threshold the two counts and the two sums of the counted minima (each lane adds its
//            points in index order, then a binary tree over the 256 lanes), and the two results.
// dfepe_average_precision is one workgroup per pair with the pair's scores and labels staged in LDS (36 KiB at the cap): one
// lane per entry counts the entries scored at least as high; dfepe_matching_score is one lane per pair.
#include "dfepe_common.h"
#include "detector_eval_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;  // points (16 B) or keys (8 B) staged in LDS at a time

__device__ inline int pair_count(const int* __restrict__ n_valid, size_t pair, int N) {
  if (n_valid == nullptr) return N;
  const int n = n_valid[pair];
  return n < 0 ? 0 : (n > N ? N : n);
}

// Sum over the workgroup in a fixed order (a binary tree over the lanes), the same total in every lane.  buf: kThreads cells.
template <class T>
__device__ inline T block_sum(T v, T* buf) {
  const int tid = threadIdx.x;
  __syncthreads();  // buf may still be read from the previous sum
  buf[tid] = v;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) buf[tid] = buf[tid] + buf[tid + o];
    __syncthreads();
  }
  return buf[0];
}

struct Work {  // the workspace of one call, [B][N1 + N2] each, image 1's N1 cells first
  double2* pts;
  unsigned long long* key;
  double* mind;
  unsigned char* sel;
};

__host__ __device__ inline Work carve(void* workspace, int B, int NT) {
  const size_t cells = (size_t)B * NT;
  Work w;
  w.pts = static_cast<double2*>(workspace);
  w.key = reinterpret_cast<unsigned long long*>(w.pts + cells);
  w.mind = reinterpret_cast<double*>(w.key + cells);
  w.sel = reinterpret_cast<unsigned char*>(w.mind + cells);
  return w;
}

__global__ void __launch_bounds__(kThreads) detector_select_kernel(const double* __restrict__ kp1, const double* __restrict__ kp2,
                                                                   const int* __restrict__ n1, const int* __restrict__ n2,
                                                                   const double* __restrict__ H, int B, int N1, int N2, int C, int height,
                                                                   int width, int keep_k, void* workspace, int* __restrict__ kept1,
                                                                   int* __restrict__ kept2, int* __restrict__ n_unwarped) {
  __shared__ unsigned long long tkey[kTile];
  __shared__ int ibuf[kThreads];
  const size_t pair = blockIdx.x;
  const int set = blockIdx.y, tid = threadIdx.x;
  const int N = set ? N2 : N1, NT = N1 + N2;
  const int n = pair_count(set ? n2 : n1, pair, N);
  const double* kp = (set ? kp2 : kp1) + pair * (size_t)N * C;
  const Work w = carve(workspace, B, NT);
  const size_t off = pair * (size_t)NT + (set ? N1 : 0);
  double M[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) M[j] = H[pair * 9 + j];
  if (set) {
    double A[9];
    de::adjugate(M, A);
#pragma unroll
    for (int j = 0; j < 9; ++j) M[j] = A[j];
  }
  int nk = 0, nu = 0;
  for (int i = tid; i < N; i += kThreads) {
    unsigned long long key = 0;
    double2 pt = make_double2(0.0, 0.0);
    if (i < n) {
      const double x = kp[(size_t)i * C], y = kp[(size_t)i * C + 1];
      double wx, wy;
      de::warp(M, x, y, &wx, &wy);
      pt = set ? make_double2(x, y) : make_double2(wx, wy);  // image 2's points stay where they are; only the test is on the warp
      if (de::inside_half_open(wx, wy, height, width)) {
        key = (C == 3) ? de::prob_key(kp[(size_t)i * C + 2]) : 1ull;
        ++nk;
      }
      if (de::inside_closed(wx, wy, height, width)) ++nu;
    }
    w.pts[off + i] = pt;
    w.key[off + i] = key;
  }
  nk = block_sum(nk, ibuf);
  if (set) {
    nu = block_sum(nu, ibuf);
    if (tid == 0) n_unwarped[pair] = nu;
  }
  const bool all = (C == 2) || keep_k == 0 || keep_k >= nk;  // nothing to rank: select_k_best keeps every point that passed
  if (tid == 0) (set ? kept2 : kept1)[pair] = all ? nk : keep_k;
  // the keys this workgroup wrote are read back below: block_sum's barriers stand between
  for (int base = 0; base < N; base += kThreads) {  // the same trip count in every lane: the tiles below are staged by all
    const int i = base + tid;
    const unsigned long long mine = (i < N) ? w.key[off + i] : 0ull;
    bool keep = mine != 0;
    if (!all) {
      int rank = 0;
      for (int t0 = 0; t0 < n; t0 += kTile) {
        const int cnt = (n - t0 < kTile) ? n - t0 : kTile;
        __syncthreads();
        for (int j = tid; j < cnt; j += kThreads) tkey[j] = w.key[off + t0 + j];
        __syncthreads();
        if (mine != 0) {
#pragma unroll 8
          for (int j = 0; j < cnt; ++j) {
            const unsigned long long kj = tkey[j];
            rank += (kj != 0 && de::stands_after(kj, t0 + j, mine, i)) ? 1 : 0;
          }
        }
      }
      keep = keep && de::selected(rank, keep_k, nk);
    }
    if (i < N) w.sel[off + i] = keep ? 1 : 0;
  }
}

// The distance from each kept point of `own` to the nearest kept point of `other` (+inf where there is none, and for a point
// that is not kept).  One lane per own point, the others staged in tiles; a point that is not kept is staged as NaN, which no
// comparison takes for a minimum, so the sweep has no branch and its LDS reads can be issued ahead.
__device__ inline void nearest(const double2* __restrict__ own, const unsigned char* __restrict__ own_sel, int n_own,
                               const double2* __restrict__ other, const unsigned char* __restrict__ other_sel, int n_other,
                               double* __restrict__ mind, double2* tpt) {
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kThreads + tid;
  const bool mine = i < n_own && own_sel[i] != 0;
  const double2 p = mine ? own[i] : make_double2(0.0, 0.0);
  double best = INFINITY;
  for (int t0 = 0; t0 < n_other; t0 += kTile) {
    const int cnt = (n_other - t0 < kTile) ? n_other - t0 : kTile;
    __syncthreads();
    for (int j = tid; j < cnt; j += kThreads) tpt[j] = other_sel[t0 + j] ? other[t0 + j] : make_double2(NAN, NAN);
    __syncthreads();
    if (mine) {
#pragma unroll 8
      for (int j = 0; j < cnt; ++j) {
        const double2 q = tpt[j];  // every lane reads the same cell: a broadcast
        const double d2 = de::dist2(p.x, p.y, q.x, q.y);
        if (d2 < best) best = d2;
      }
    }
  }
  if (i < n_own) mind[i] = mine ? sqrt(best) : INFINITY;
}

__global__ void __launch_bounds__(kThreads) detector_nearest_kernel(const int* __restrict__ n1, const int* __restrict__ n2, int B, int N1,
                                                                    int N2, void* workspace) {
  __shared__ double2 tpt[kTile];
  const size_t pair = blockIdx.y;
  const int c1 = pair_count(n1, pair, N1), c2 = pair_count(n2, pair, N2);
  const bool swap = blockIdx.z != 0;
  if ((int)(blockIdx.x * kThreads) >= (swap ? c2 : c1)) return;  // uniform over the workgroup, before any barrier
  const Work w = carve(workspace, B, N1 + N2);
  const size_t o1 = pair * (size_t)(N1 + N2), o2 = o1 + N1;
  if (!swap) nearest(w.pts + o1, w.sel + o1, c1, w.pts + o2, w.sel + o2, c2, w.mind + o1, tpt);
  else nearest(w.pts + o2, w.sel + o2, c2, w.pts + o1, w.sel + o1, c1, w.mind + o2, tpt);
}

__global__ void __launch_bounds__(kThreads) detector_reduce_kernel(const int* __restrict__ n1, const int* __restrict__ n2, int B, int N1,
                                                                   int N2, const void* workspace, const int* __restrict__ kept1,
                                                                   const int* __restrict__ kept2, const double* __restrict__ thresh, int T,
                                                                   double* __restrict__ repeatability, double* __restrict__ loc_err,
                                                                   int* __restrict__ count1, int* __restrict__ count2) {
  __shared__ double dbuf[kThreads];
  __shared__ int ibuf[kThreads];
  const size_t pair = blockIdx.x;
  const int tid = threadIdx.x;
  const Work w = carve(const_cast<void*>(workspace), B, N1 + N2);
  const size_t o1 = pair * (size_t)(N1 + N2), o2 = o1 + N1;
  const int k1 = kept1[pair], k2 = kept2[pair];
  // without a point in the other image there is no minimum and nothing is counted (lines 253 and 259)
  const int c1n = (k2 > 0) ? pair_count(n1, pair, N1) : 0, c2n = (k1 > 0) ? pair_count(n2, pair, N2) : 0;
  for (int t = 0; t < T; ++t) {
    const double th = thresh[t];
    int c1 = 0, c2 = 0;
    double s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < c1n; i += kThreads) {
      const double m = w.mind[o1 + i];
      if (w.sel[o1 + i] && m <= th) { ++c1; s1 += m; }
    }
    for (int i = tid; i < c2n; i += kThreads) {
      const double m = w.mind[o2 + i];
      if (w.sel[o2 + i] && m <= th) { ++c2; s2 += m; }
    }
    c1 = block_sum(c1, ibuf);
    c2 = block_sum(c2, ibuf);
    s1 = block_sum(s1, dbuf);
    s2 = block_sum(s2, dbuf);
    if (tid == 0) {
      const size_t o = pair * (size_t)T + t;
      count1[o] = c1;
      count2[o] = c2;
      repeatability[o] = de::repeatability_of(c1, c2, k1, k2);
      loc_err[o] = de::loc_err_of(c1, c2, s1, s2);
    }
  }
}

__global__ void __launch_bounds__(kThreads) average_precision_kernel(const unsigned char* __restrict__ labels, const double* __restrict__ scores,
                                                                     const int* __restrict__ n_valid, int M, double* __restrict__ ap,
                                                                     int* __restrict__ n_pos, int* __restrict__ tp_at,
                                                                     int* __restrict__ cnt_at) {
  __shared__ double sc[de::kMaxN];
  __shared__ unsigned char lb[de::kMaxN];
  __shared__ double dbuf[kThreads];
  __shared__ int ibuf[kThreads];
  const size_t pair = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = pair_count(n_valid, pair, M);
  int pos = 0;
  for (int i = tid; i < n; i += kThreads) {
    sc[i] = scores[pair * M + i];
    const unsigned char l = labels[pair * M + i] ? 1 : 0;
    lb[i] = l;
    pos += l;
  }
  const int P = block_sum(pos, ibuf);  // its barriers also publish sc and lb
  double acc = 0.0;
  for (int base = 0; base < M; base += kThreads) {
    const int i = base + tid;
    int tp = 0, cnt = 0;
    if (i < n) {
      const double s = sc[i];
#pragma unroll 8
      for (int j = 0; j < n; ++j) {
        const int ge = (sc[j] >= s) ? 1 : 0;
        cnt += ge;
        tp += ge & (int)lb[j];
      }
      if (lb[i]) acc += de::ap_term(tp, cnt);
    }
    if (i < M) {
      if (tp_at != nullptr) tp_at[pair * M + i] = tp;
      if (cnt_at != nullptr) cnt_at[pair * M + i] = cnt;
    }
  }
  const double total = block_sum(acc, dbuf);
  if (tid == 0) {
    ap[pair] = (P > 0) ? total / (double)P : 0.0;
    if (n_pos != nullptr) n_pos[pair] = P;
  }
}

__global__ void __launch_bounds__(kThreads) matching_score_kernel(const int* __restrict__ n_inliers, const int* __restrict__ n_kp1,
                                                                  const int* __restrict__ n_unwarped, int B, double* __restrict__ mscore) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) mscore[b] = de::matching_score(n_inliers[b], n_kp1[b], n_unwarped[b]);
}

}  // namespace

extern "C" size_t dfepe_keypoint_repeatability_workspace_bytes(int B, int N1, int N2) {
  if (B <= 0 || N1 < 0 || N2 < 0 || N1 > de::kMaxN || N2 > de::kMaxN) return 0;
  const size_t cells = (size_t)B * ((size_t)N1 + (size_t)N2);
  return cells * (sizeof(double2) + sizeof(unsigned long long) + sizeof(double)) + ((cells + 15) / 16) * 16;
}

extern "C" int dfepe_keypoint_repeatability(const double* kp1, const double* kp2, const int* n1, const int* n2, const double* H, int B,
                                            int N1, int N2, int C, int height, int width, int keep_k, const double* thresh, int T,
                                            void* workspace, double* repeatability, double* loc_err, int* count1, int* count2,
                                            int* kept1, int* kept2, int* n_unwarped, void* stream) {
  if (B < 0 || N1 < 0 || N2 < 0 || (C != 2 && C != 3) || T < 0 || height < 1 || width < 1 || keep_k < 0) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (N1 > de::kMaxN || N2 > de::kMaxN || B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  if ((N1 > 0 && !kp1) || (N2 > 0 && !kp2) || !H || !kept1 || !kept2 || !n_unwarped) return DFEPE_ERR_INVALID_ARG;
  if (T > 0 && (!thresh || !repeatability || !loc_err || !count1 || !count2)) return DFEPE_ERR_INVALID_ARG;
  if (N1 + N2 > 0 && (!workspace || !aligned16(workspace))) return DFEPE_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(detector_select_kernel, dim3(B, 2), dim3(kThreads), 0, s, kp1, kp2, n1, n2, H, B, N1, N2, C, height, width, keep_k,
                     workspace, kept1, kept2, n_unwarped);
  const int nmax = N1 > N2 ? N1 : N2;
  if (nmax > 0) hipLaunchKernelGGL(detector_nearest_kernel, dim3((nmax + kThreads - 1) / kThreads, B, 2), dim3(kThreads), 0, s, n1, n2, B, N1, N2,
                                   workspace);
  if (T > 0) hipLaunchKernelGGL(detector_reduce_kernel, dim3(B), dim3(kThreads), 0, s, n1, n2, B, N1, N2, workspace, kept1, kept2, thresh, T,
                                repeatability, loc_err, count1, count2);
  return launched();
}

extern "C" int dfepe_average_precision(const unsigned char* labels, const double* scores, const int* n_valid, int B, int M, double* ap,
                                       int* n_pos, int* tp_at, int* cnt_at, void* stream) {
  if (B < 0 || M < 0) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (M > de::kMaxN || B > kMaxGridY) return DFEPE_ERR_UNSUPPORTED;
  if (!ap || (M > 0 && (!labels || !scores))) return DFEPE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(average_precision_kernel, dim3(B), dim3(kThreads), 0, static_cast<hipStream_t>(stream), labels, scores, n_valid, M, ap,
                     n_pos, tp_at, cnt_at);
  return launched();
}

extern "C" int dfepe_matching_score(const int* n_inliers, const int* n_kp1, const int* n_unwarped, int B, double* mscore, void* stream) {
  if (B < 0) return DFEPE_ERR_INVALID_ARG;
  if (B == 0) return DFEPE_OK;
  if (!n_inliers || !n_kp1 || !n_unwarped || !mscore) return DFEPE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(matching_score_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     n_inliers, n_kp1, n_unwarped, B, mscore);
  return launched();
}
