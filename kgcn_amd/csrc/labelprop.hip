// Active learning on the device: the numerical core of the reference's active_learning/models.py (scikit-learn's LabelPropagation /
// LabelSpreading once per task, then uncertainty scores over the pool), with the work every task and every query repeats done once.
// The driver is kgcn_amd/active_learning.py; include/kgcn_hip.h states the contract and every summation order,
// tests/active_learning_oracle.py restates them in numpy.  fp64 and integers, no float atomics: a pure function of the input.
//
//   affinity  W = exp(-gamma max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j)), the Gram tiles on v_mfma_f64_16x16x4_f64: one workgroup an upper-
//             triangle 64 x 64 tile (four waves, each 2 x 2 MFMA blocks), every entry stored at (i, j) and (j, i) from ONE value.
//   degrees   one wave a row.
//   step      F' = scale (W F) and the clamp for ALL tasks in one sweep over W: a workgroup owns 32 rows (four waves, 8 rows each), a
//             lane the columns j = lane (mod 64) of W, so a row of F is fetched once for 8 rows of W.  The raw sums go through LDS to
//             an epilogue that owns one (row, task) a thread: scaling, clamp, |F' - F|.  The per-task sums of a workgroup are its
//             partial; a one-workgroup `decide` launch adds the partials in workgroup order and freezes tasks.
//   matrix-free   rbf_apply, rbf_degrees and the step without W: a workgroup rebuilds each 64 x 64 tile of w in LDS where it is
//             consumed, with the arithmetic of `affinity` and the summation order of `degrees` / `step`, so the results are theirs
//             bit for bit in O(n (d + K)) memory.
//   finish / scores / select   one thread a (row, task) / a candidate; one workgroup picks the k best in a total order.
// Nothing is fused: the Makefile builds this file with -ffp-contract=off (see hashkern.hip for why a pragma is not enough).
#include <math.h>

#include "gram_tile.h"
#include "workspace.h"

namespace kgcn {
namespace {

constexpr int kRowsWave = 8;               // rows of W a wave carries through the step
constexpr int kRowsWg = KGCN_LP_BLOCK_ROWS;   // 4 waves x 8 rows: the unit of the convergence partials
constexpr int kMaxTasks = KGCN_LP_MAX_TASKS;
constexpr int kMaxCols = KGCN_LP_MAX_COLS;
static_assert(kRowsWg == 4 * kRowsWave, "a step workgroup is four waves");

// the sum of a value over the 64 lanes in the stated tree: v = v + (v of lane ^ off) for off = 32, 16, 8, 4, 2, 1; every lane ends
// with the same bits (an addition commutes)
__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// ---- affinity -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lp_norms_kernel(const double* __restrict__ x, long n, int d, double* __restrict__ norms) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  for (int k = 0; k < d; ++k) acc = acc + x[i * d + k] * x[i * d + k];
  norms[i] = acc;
}

// THE Gram tile of this file (gram_tile.h): acc = x_a . x_b for the 64 rows of xa [na, d] from ia0 against the 64 rows of xb [nb, d]
// from ib0.  Rows past the set and attributes past d are staged as 0.  The panels are free again on return.
__device__ __forceinline__ void gram_tile(const double* __restrict__ xa, long ia0, long na, const double* __restrict__ xb, long ib0,
                                          long nb, int d, double* as, double* bs, f64x4 (&acc)[2][2]) {
  for (auto& row : acc)
    for (auto& blk : row) blk = f64x4{0.0, 0.0, 0.0, 0.0};
  gram_tile_64(
      as, bs, d, [&](int r, int k0, int kk) { const long ia = ia0 + r; return (k0 + kk < d && ia < na) ? xa[ia * d + k0 + kk] : 0.0; },
      [&](int r, int k0, int kk) { const long ib = ib0 + r; return (k0 + kk < d && ib < nb) ? xb[ib * d + k0 + kk] : 0.0; }, acc);
}

// w = exp(-gamma max(0, (|a|^2 + |b|^2) - 2 a.b)), NaN kept; same_point: the two are the same row of the same set, dist = 0
__device__ __forceinline__ double rbf_weight(double na, double nb, double dot, double gamma, bool same_point) {
  double dist = (na + nb) - 2.0 * dot;
  if (!(dist > 0.0)) dist = dist != dist ? dist : 0.0;          // max(0, .), NaN kept
  if (same_point) dist = 0.0;
  return exp(-gamma * dist);
}

__global__ __launch_bounds__(256) void lp_affinity_kernel(const double* __restrict__ x, const double* __restrict__ norms, long n, int d,
                                                          double gamma, double* __restrict__ W) {
  __shared__ double as[kTile * kLd], bs[kTile * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, hi = lane >> 4, wr = wv >> 1, wc = wv & 1;
  int ti, tj;
  tile_of((long)blockIdx.x, ti, tj);
  f64x4 acc[2][2];
  gram_tile(x, (long)ti * kTile, n, x, (long)tj * kTile, n, d, as, bs, acc);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long i = (long)ti * kTile + wr * 32 + p * 16 + hi + 4 * r, j = (long)tj * kTile + wc * 32 + q * 16 + li;
        if (i >= n || j >= n || i > j) continue;             // a diagonal tile stores its upper half and mirrors it, like the others
        const double w = rbf_weight(norms[i], norms[j], acc[p][q][r], gamma, i == j);
        W[i * n + j] = w;
        W[j * n + i] = w;
      }
}

// ---- the affinity without its matrix ---------------------------------------------------------------------------------------------
// A tile of w is rebuilt where it is consumed.  Every w_ij carries the bits lp_affinity_kernel stores: the same gram_tile, the same
// norms, the same rbf_weight (a.b and b.a are the same products in the same k order).  The consumers keep the stored kernels'
// summation order: lane l owns the columns j = l (mod 64), so column tiles start at multiples of 64 and are walked upwards.
struct RbfSets {
  const double *xq, *nq;       // queries [m, d] and their norms
  long m;
  const double *xr, *nr;       // references [n, d] and their norms
  long n;
  int d, same;                 // same: xq IS xr (row i of one is row i of the other)
  double gamma;
};

constexpr int kWt = kTile + 1;                                  // the tile's row pitch in LDS
constexpr int kTileDoubles = kTile * kWt;                       // ... which lies over the two staging panels
constexpr int kRowsTileWave = kTile / 4;                        // rows of a tile a wave consumes
static_assert(2 * kTile * kLd <= kTileDoubles, "the tile covers the panels it is built from");

// tile (rows i0 .., columns j0 ..) of w -> wt [kTile][kWt] at smem; entries outside the sets are 0 and unused
__device__ __forceinline__ void rbf_tile(const RbfSets& s, long i0, long j0, double* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, hi = lane >> 4, wr = wv >> 1, wc = wv & 1;
  f64x4 acc[2][2];
  gram_tile(s.xq, i0, s.m, s.xr, j0, s.n, s.d, smem, smem + kTile * kLd, acc);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tr = wr * 32 + p * 16 + hi + 4 * r, tc = wc * 32 + q * 16 + li;
        const long i = i0 + tr, j = j0 + tc;
        smem[tr * kWt + tc] = (i < s.m && j < s.n) ? rbf_weight(s.nq[i], s.nr[j], acc[p][q][r], s.gamma, s.same && i == j) : 0.0;
      }
  __syncthreads();
}

// use(j0) once per column tile, in ascending order, with the tile in smem
template <typename Fn>
__device__ __forceinline__ void rbf_for_tiles(const RbfSets& s, long i0, double* smem, Fn&& use) {
  for (long j0 = 0; j0 < s.n; j0 += kTile) {
    rbf_tile(s, i0, j0, smem);
    use(j0);
    __syncthreads();
  }
}

// The terms of one tile: acc[r][c] = acc[r][c] + w_ij G_jc for the wave's rows i = irow0 + r and the lane's column j, each
// product rounded before it is added; a column past the set adds nothing; zero_diag: w_ii counts as +0.0.
template <int KC>
__device__ __forceinline__ void rbf_terms(const double* wt, long irow0, long j, long n, bool zero_diag, const double* __restrict__ G,
                                          int K, int c0, double (&acc)[kRowsTileWave][KC]) {
  if (j >= n) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double g[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) g[c] = c0 + c < K ? G[j * K + c0 + c] : 0.0;
#pragma unroll
  for (int r = 0; r < kRowsTileWave; ++r) {
    double w = wt[(wv * kRowsTileWave + r) * kWt + lane];
    if (zero_diag && j == irow0 + r) w = 0.0;
#pragma unroll
    for (int c = 0; c < KC; ++c) acc[r][c] = acc[r][c] + w * g[c];
  }
}

// out[i, c] = sum_j w(q_i, r_j) G_jc: a workgroup owns 64 queries, a wave 16 of them, KC columns of G at a time
template <int KC>
__global__ __launch_bounds__(256) void rbf_apply_kernel(RbfSets s, int zero_diag, const double* __restrict__ G, int K,
                                                        double* __restrict__ out) {
  __shared__ double smem[kTileDoubles];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long i0 = (long)blockIdx.x * kTile, irow0 = i0 + wv * kRowsTileWave;
  for (int c0 = 0; c0 < K; c0 += KC) {
    double acc[kRowsTileWave][KC];
#pragma unroll
    for (int r = 0; r < kRowsTileWave; ++r)
#pragma unroll
      for (int c = 0; c < KC; ++c) acc[r][c] = 0.0;
    rbf_for_tiles(s, i0, smem, [&](long j0) { rbf_terms<KC>(smem, irow0, j0 + lane, s.n, zero_diag != 0, G, K, c0, acc); });
#pragma unroll
    for (int r = 0; r < kRowsTileWave; ++r)
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const double v = wave_tree_sum(acc[r][c]);
        if (lane == 0 && irow0 + r < s.m && c0 + c < K) out[(irow0 + r) * K + c0 + c] = v;
      }
  }
}

// lp_degrees_kernel without W: the same two sums in the same order
__global__ __launch_bounds__(256) void rbf_degrees_kernel(RbfSets s, double* __restrict__ s_out, double* __restrict__ d_out) {
  __shared__ double smem[kTileDoubles];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long i0 = (long)blockIdx.x * kTile, irow0 = i0 + wv * kRowsTileWave;
  double sum[kRowsTileWave], dg[kRowsTileWave];
#pragma unroll
  for (int r = 0; r < kRowsTileWave; ++r) sum[r] = dg[r] = 0.0;
  rbf_for_tiles(s, i0, smem, [&](long j0) {
    const long j = j0 + lane;
    if (j >= s.n) return;
#pragma unroll
    for (int r = 0; r < kRowsTileWave; ++r) {
      const double w = smem[(wv * kRowsTileWave + r) * kWt + lane];
      sum[r] = sum[r] + w;
      dg[r] = dg[r] + (j == irow0 + r ? 0.0 : w);
    }
  });
#pragma unroll
  for (int r = 0; r < kRowsTileWave; ++r) {
    const double a = wave_tree_sum(sum[r]), b = wave_tree_sum(dg[r]);
    if (lane == 0 && irow0 + r < s.n) {
      s_out[irow0 + r] = a;
      d_out[irow0 + r] = b;
    }
  }
}

// s_i = sum over ALL j, d_i = the same sum with the diagonal term replaced by +0.0.  Lane l adds the columns j = l, l + 64, ... in
// ascending order from +0.0; then the lane tree.
__global__ __launch_bounds__(256) void lp_degrees_kernel(const double* __restrict__ W, long n, double* __restrict__ s_out,
                                                         double* __restrict__ d_out) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                                         // wave-uniform
  double s = 0.0, dg = 0.0;
  for (long j = lane; j < n; j += 64) {
    const double w = W[i * n + j];
    s = s + w;
    dg = dg + (j == i ? 0.0 : w);
  }
  s = wave_tree_sum(s);
  dg = wave_tree_sum(dg);
  if (lane == 0) {
    s_out[i] = s;
    d_out[i] = dg;
  }
}

// ---- propagation ----------------------------------------------------------------------------------------------------------------
struct LpArgs {
  const double* W;             // the stored route; NULL on the matrix-free one, which reads `pts`
  RbfSets pts;
  const double* scale;        // propagation: s [n]; spreading: d [n]
  const int32_t* labels;       // [n, T] class index of the task or -1
  const int32_t* task_col;     // [T + 1]
  long n;
  int T, K, spreading;
  double alpha, tol;
  int max_iter, step;          // step: the number of steps done before this launch
  const double* Fprev;         // [n, K] distributions before the step
  const double* Gprev;         // the operand of the product: Fprev (propagation) or Fprev / sqrt(d) by rows (spreading)
  double* Fnext;
  double* Gnext;               // spreading only
  double* partial;             // [blocks, T]
  int32_t* status;
  int32_t* n_iter;
  unsigned* running;
};

__device__ __forceinline__ double sqrt_degree(double d) { return d == 0.0 ? 1.0 : sqrt(d); }   // scipy's laplacian: an isolated node

// y_static of (row, task) at class c: the one-hot label, times 1 - alpha for spreading
__device__ __forceinline__ double y_static(const LpArgs& a, int label, int c) {
  return label == c ? (a.spreading ? 1.0 - a.alpha : 1.0) : 0.0;
}

// the tail shared by init and step: rowdelta [32][T] in LDS -> partial[block][t], rows in ascending order from +0.0
__device__ __forceinline__ void block_partials(const LpArgs& a, const double (*rowdelta)[kMaxTasks], long block) {
  __syncthreads();
  if ((int)threadIdx.x < a.T) {
    double p = 0.0;
    for (int r = 0; r < kRowsWg; ++r) p = p + rowdelta[r][threadIdx.x];
    a.partial[block * a.T + threadIdx.x] = p;
  }
}

// F0 = the one-hot labels; G0 = F0 / sqrt(d); the partials of sum |F0 - 0|
__global__ __launch_bounds__(256) void lp_init_kernel(LpArgs a) {
  __shared__ double rowdelta[kRowsWg][kMaxTasks];
  for (int e = threadIdx.x; e < kRowsWg * a.T; e += 256) {
    const int r = e / a.T, t = e - r * a.T;
    const long i = (long)blockIdx.x * kRowsWg + r;
    double delta = 0.0;
    if (i < a.n) {
      const int c0 = a.task_col[t], c1 = a.task_col[t + 1], label = a.labels[i * a.T + t];
      const double sd = a.spreading ? sqrt_degree(a.scale[i]) : 1.0;
      for (int c = c0; c < c1; ++c) {
        const double v = label == c - c0 ? 1.0 : 0.0;
        a.Fnext[i * a.K + c] = v;
        if (a.spreading) a.Gnext[i * a.K + c] = v / sd;
        delta = delta + v;
      }
    }
    rowdelta[r][t] = delta;
  }
  block_partials(a, rowdelta, (long)blockIdx.x);
}

// After `step` steps: a running task whose partials add up (workgroup order, from +0.0) to less than tol has converged with n_iter =
// step; otherwise at step == max_iter it stops with n_iter = max_iter (BaseLabelPropagation.fit's for / else).  running <- tasks left.
__global__ __launch_bounds__(64) void lp_decide_kernel(LpArgs a, int blocks) {
  __shared__ int left[kMaxTasks];
  const int t = threadIdx.x;
  if (t < a.T) {
    int st = a.status[t];
    if (st == KGCN_LP_RUNNING) {
      if (a.step >= a.max_iter) {
        st = KGCN_LP_MAX_ITER;
        a.n_iter[t] = a.max_iter;
      } else {
        double sum = 0.0;
        for (int b = 0; b < blocks; ++b) sum = sum + a.partial[(long)b * a.T + t];
        if (sum < a.tol) {
          st = KGCN_LP_CONVERGED;
          a.n_iter[t] = a.step;
        }
      }
      a.status[t] = st;
    }
    left[t] = st == KGCN_LP_RUNNING;
  }
  __syncthreads();
  if (t == 0) {
    unsigned c = 0;
    for (int q = 0; q < a.T; ++q) c += left[q];
    *a.running = c;
  }
}

// THE epilogue of a step, for one block of kRowsWg rows whose raw sums are in LDS: one (row, task) a thread -- scaling, clamp,
// |F' - F|, the copy of a frozen task -- and the block's partials.  Every thread of the workgroup calls it.
__device__ __forceinline__ void step_epilogue(const LpArgs& a, const double (*raw)[kMaxCols], double (*rowdelta)[kMaxTasks], long block,
                                              const int* frozen, const int* tcol) {
  const long n = a.n;
  const int K = a.K;
  for (int e = threadIdx.x; e < kRowsWg * a.T; e += 256) {
    const int r = e / a.T, t = e - r * a.T;
    const long i = block * kRowsWg + r;
    double delta = 0.0;
    if (i < n) {
      const int b0 = tcol[t], b1 = tcol[t + 1];
      const double* fp = a.Fprev + i * K;
      double* fn = a.Fnext + i * K;
      if (frozen[t]) {
        for (int c = b0; c < b1; ++c) {
          fn[c] = fp[c];
          if (a.spreading) a.Gnext[i * K + c] = a.Gprev[i * K + c];
        }
      } else {
        const int label = a.labels[i * a.T + t];
        if (a.spreading) {
          const double sd = sqrt_degree(a.scale[i]);
          for (int c = b0; c < b1; ++c) {
            const double v = a.alpha * (raw[r][c] / sd) + y_static(a, label, c - b0);
            delta = delta + fabs(v - fp[c]);
            fn[c] = v;
            a.Gnext[i * K + c] = v / sd;
          }
        } else {
          const double s = a.scale[i];
          double norm = 0.0;
          for (int c = b0; c < b1; ++c) norm = norm + raw[r][c] / s;
          if (norm == 0.0) norm = 1.0;
          for (int c = b0; c < b1; ++c) {
            const double v = label >= 0 ? y_static(a, label, c - b0) : (raw[r][c] / s) / norm;
            delta = delta + fabs(v - fp[c]);
            fn[c] = v;
          }
        }
      }
    }
    rowdelta[r][t] = delta;
  }
  block_partials(a, rowdelta, block);
}

// One step.  raw[r][c] = sum_j w_ij G_jc: lane l adds j = l, l + 64, ... ascending from +0.0, each term w * g rounded before it is
// added; then the lane tree.  w_ii counts as +0.0 for spreading.  KC columns of F are carried at a time.
template <int KC>
__global__ __launch_bounds__(256) void lp_step_kernel(LpArgs a) {
  __shared__ double raw[kRowsWg][kMaxCols];
  __shared__ double rowdelta[kRowsWg][kMaxTasks];
  __shared__ int frozen[kMaxTasks], tcol[kMaxTasks + 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < a.T) frozen[tid] = a.status[tid] != KGCN_LP_RUNNING;
  if (tid <= a.T) tcol[tid] = a.task_col[tid];
  __syncthreads();
  const long n = a.n, row0 = (long)blockIdx.x * kRowsWg + wv * kRowsWave;
  const int K = a.K;
  for (int c0 = 0; c0 < K; c0 += KC) {
    bool live = false;                                        // workgroup-uniform: a chunk of frozen tasks only is not multiplied
    for (int t = 0; t < a.T; ++t) live = live || (!frozen[t] && tcol[t] < c0 + KC && tcol[t + 1] > c0);
    if (!live) continue;
    double acc[kRowsWave][KC];
#pragma unroll
    for (int r = 0; r < kRowsWave; ++r)
#pragma unroll
      for (int c = 0; c < KC; ++c) acc[r][c] = 0.0;
    // The operands of column j + 64 are requested before those of column j are used: all 8 + KC loads of a lane are in flight
    // together and a column's arithmetic covers the next one's latency.  (Written as one load after another with the diagonal test
    // in between, the compiler waited for each of the 8 rows in turn.)  The column past the end is read as the last one, unused.
    const double* wrow[kRowsWave];
    long irow[kRowsWave];
#pragma unroll
    for (int r = 0; r < kRowsWave; ++r) {
      irow[r] = row0 + r < n ? row0 + r : n - 1;              // rows past the matrix repeat the last one and are not stored
      wrow[r] = a.W + irow[r] * n;
    }
    const double* gcol = a.Gprev + c0;
    double wn[kRowsWave], gn[KC];
    {
      const long j0 = lane < n ? lane : n - 1;
#pragma unroll
      for (int r = 0; r < kRowsWave; ++r) wn[r] = wrow[r][j0];
#pragma unroll
      for (int c = 0; c < KC; ++c) gn[c] = c0 + c < K ? gcol[j0 * K + c] : 0.0;
    }
    for (long j = lane; j < n; j += 64) {
      double w[kRowsWave], g[KC];
#pragma unroll
      for (int r = 0; r < kRowsWave; ++r) w[r] = wn[r];
#pragma unroll
      for (int c = 0; c < KC; ++c) g[c] = gn[c];
      const long jn = j + 64 < n ? j + 64 : n - 1;
#pragma unroll
      for (int r = 0; r < kRowsWave; ++r) wn[r] = wrow[r][jn];
#pragma unroll
      for (int c = 0; c < KC; ++c) gn[c] = c0 + c < K ? gcol[jn * K + c] : 0.0;
      if (a.spreading) {
#pragma unroll
        for (int r = 0; r < kRowsWave; ++r) w[r] = j == irow[r] ? 0.0 : w[r];
      }
#pragma unroll
      for (int r = 0; r < kRowsWave; ++r)
#pragma unroll
        for (int c = 0; c < KC; ++c) acc[r][c] = acc[r][c] + w[r] * g[c];
    }
#pragma unroll
    for (int r = 0; r < kRowsWave; ++r)
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const double v = wave_tree_sum(acc[r][c]);
        if (lane == 0 && c0 + c < K) raw[wv * kRowsWave + r][c0 + c] = v;
      }
  }
  __syncthreads();
  step_epilogue(a, raw, rowdelta, (long)blockIdx.x, frozen, tcol);
}

// The step without W: a workgroup owns 64 rows (two blocks of the convergence partials), a wave 16 of them; the tiles of w come
// from rbf_for_tiles, the terms from rbf_terms in lp_step_kernel's order, the rest is lp_step_kernel's.  LDS: the tile (under the
// panels it is built from, and later under rowdelta), raw [64][kMaxCols], frozen and tcol -- all of it dynamic: a kernel that is
// allowed the CU's full LDS can hold no static LDS beside it.
constexpr size_t kFreeStepLds = (size_t)(kTileDoubles + kTile * kMaxCols) * sizeof(double) + (2 * kMaxTasks + 2) * sizeof(int);
static_assert(kRowsWg * kMaxTasks <= kTileDoubles && kTile == 2 * kRowsWg, "rowdelta lies over the tile; a workgroup is two blocks");

template <int KC>
__global__ __launch_bounds__(256) void lp_free_step_kernel(LpArgs a) {
  extern __shared__ double lds[];
  int* frozen = reinterpret_cast<int*>(lds + kTileDoubles + kTile * kMaxCols);
  int* tcol = frozen + kMaxTasks;
  double* smem = lds;
  double(*raw)[kMaxCols] = reinterpret_cast<double(*)[kMaxCols]>(lds + kTileDoubles);
  double(*rowdelta)[kMaxTasks] = reinterpret_cast<double(*)[kMaxTasks]>(lds);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < a.T) frozen[tid] = a.status[tid] != KGCN_LP_RUNNING;
  if (tid <= a.T) tcol[tid] = a.task_col[tid];
  __syncthreads();
  const long i0 = (long)blockIdx.x * kTile, irow0 = i0 + wv * kRowsTileWave;
  const int K = a.K;
  for (int c0 = 0; c0 < K; c0 += KC) {
    bool live = false;                                        // workgroup-uniform, as in lp_step_kernel
    for (int t = 0; t < a.T; ++t) live = live || (!frozen[t] && tcol[t] < c0 + KC && tcol[t + 1] > c0);
    if (!live) continue;
    double acc[kRowsTileWave][KC];
#pragma unroll
    for (int r = 0; r < kRowsTileWave; ++r)
#pragma unroll
      for (int c = 0; c < KC; ++c) acc[r][c] = 0.0;
    rbf_for_tiles(a.pts, i0, smem,
                  [&](long j0) { rbf_terms<KC>(smem, irow0, j0 + lane, a.n, a.spreading != 0, a.Gprev, K, c0, acc); });
#pragma unroll
    for (int r = 0; r < kRowsTileWave; ++r)
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const double v = wave_tree_sum(acc[r][c]);
        if (lane == 0 && c0 + c < K) raw[wv * kRowsTileWave + r][c0 + c] = v;
      }
  }
  __syncthreads();
  const long blocks = (a.n + kRowsWg - 1) / kRowsWg;
  for (int h = 0; h < 2; ++h) {                                 // the second block of the last workgroup may not exist
    const long block = (long)blockIdx.x * 2 + h;
    if (block >= blocks) break;
    if (h) __syncthreads();                                     // the first block's partials have been read
    step_epilogue(a, raw + h * kRowsWg, rowdelta, block, frozen, tcol);
  }
}

// dist = F / (row sum over the task's columns, ascending from +0.0; 0 counts as 1)
__global__ __launch_bounds__(256) void lp_finish_kernel(const double* __restrict__ F, const int32_t* __restrict__ task_col, long n, int T,
                                                        int K, double* __restrict__ dist) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * T) return;
  const long i = e / T;
  const int t = (int)(e - i * T), c0 = task_col[t], c1 = task_col[t + 1];
  double norm = 0.0;
  for (int c = c0; c < c1; ++c) norm = norm + F[i * K + c];
  if (norm == 0.0) norm = 1.0;
  for (int c = c0; c < c1; ++c) dist[i * K + c] = F[i * K + c] / norm;
}

// ---- scores and selection ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double entr(double p) {           // scipy.special.entr
  if (p != p) return p;
  if (p > 0.0) return -p * log(p);
  return p == 0.0 ? 0.0 : -INFINITY;
}

// scores [5, m] of the candidate rows: KGCN_LP_SCORE_* (see the header for each formula and order)
__global__ __launch_bounds__(256) void lp_scores_kernel(const double* __restrict__ dist, const int32_t* __restrict__ task_col, long n,
                                                        int T, int K, const int32_t* __restrict__ cand, long m,
                                                        double* __restrict__ scores) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= m) return;
  const long row = cand[q];
  double E = NAN, lcq = NAN, msq = NAN, lca = NAN, msa = NAN;
  if (row >= 0 && row < n) {
    const double* p = dist + row * K;
    const int C0 = task_col[1] - task_col[0];
    bool same = true;
    double conf = 0.0, margins = 0.0;
    E = 0.0;
    for (int t = 0; t < T; ++t) {
      const int c0 = task_col[t], c1 = task_col[t + 1];
      same = same && c1 - c0 == C0;
      double sum = 0.0;
      for (int c = c0; c < c1; ++c) sum = sum + p[c];
      double e = 0.0, top = -INFINITY, second = -INFINITY;
      for (int c = c0; c < c1; ++c) {
        e = e + entr(p[c] / sum);
        if (p[c] > top) { second = top; top = p[c]; }
        else if (p[c] > second) second = p[c];
      }
      E = E + e;
      conf = conf + top;
      margins = margins + (c1 - c0 == 1 ? top : top - second);
    }
    lca = conf / (double)T;
    msa = margins;
    if (same) {
      double top = -INFINITY, second = -INFINITY;
      for (int c = 0; c < C0; ++c) {
        double mean = 0.0;
        for (int t = 0; t < T; ++t) mean = mean + p[task_col[t] + c];
        mean = mean / (double)T;
        if (mean > top) { second = top; top = mean; }
        else if (mean > second) second = mean;
      }
      lcq = 1.0 - top;
      if (C0 >= 2) msq = top - second;
    }
  }
  scores[KGCN_LP_SCORE_E * m + q] = E;
  scores[KGCN_LP_SCORE_LC_MEAN * m + q] = lcq;
  scores[KGCN_LP_SCORE_MS_MEAN * m + q] = msq;
  scores[KGCN_LP_SCORE_LC_TASKS * m + q] = lca;
  scores[KGCN_LP_SCORE_MS_TASKS * m + q] = msa;
}

struct SelArgs {
  const double* score;         // [m]
  const int32_t* cand;         // [m] rows
  int32_t* active;             // [n] or NULL: a candidate whose row has active == 0 takes no part
  long m, n;
  int k, largest;
  int32_t* out;                // [k] positions into cand, -1 where fewer take part
  int32_t* labels;             // teach (k == 1): labels[row, :] = truth[row, :], active[row] = 0, log[0] = position
  const int32_t* truth;
  int T;
  int32_t* log;
};

// a sorts before b in the stable ascending order with NaN last
__device__ __forceinline__ bool sorts_before(double va, long ia, double vb, long ib) {
  const bool na = va != va, nb = vb != vb;
  if (na != nb) return nb;
  if (!na && va != vb) return va < vb;
  return ia < ib;
}

// One workgroup.  Pass r finds the r-th entry from the end (largest) or from the start of that order among the candidates not yet
// taken; `largest` fills out from its end, so out reads as the order's last k entries.
__global__ __launch_bounds__(256) void lp_select_kernel(SelArgs a) {
  __shared__ double sv[256];
  __shared__ long si[256];
  __shared__ long taken[KGCN_LP_MAX_PICKS];
  __shared__ int count_s;
  const int tid = threadIdx.x;
  if (tid == 0) count_s = 0;
  for (int r = 0; r < a.k; ++r) {
    __syncthreads();
    double bv = 0.0;
    long bi = -1;
    for (long q = tid; q < a.m; q += 256) {
      const long row = a.cand[q];
      if (row < 0 || row >= a.n || (a.active && a.active[row] == 0)) continue;
      bool used = false;
      for (int u = 0; u < r; ++u) used = used || taken[u] == q;
      if (used) continue;
      const double v = a.score[q];
      if (bi < 0 || (a.largest ? sorts_before(bv, bi, v, q) : sorts_before(v, q, bv, bi))) { bv = v; bi = q; }
    }
    sv[tid] = bv;
    si[tid] = bi;
    __syncthreads();
    if (tid == 0) {
      for (int u = 0; u < 256; ++u) {
        if (si[u] < 0) continue;
        if (bi < 0 || (a.largest ? sorts_before(bv, bi, sv[u], si[u]) : sorts_before(sv[u], si[u], bv, bi))) { bv = sv[u]; bi = si[u]; }
      }
      taken[r] = bi;
      if (bi >= 0) count_s = r + 1;
    }
  }
  __syncthreads();
  const int found = count_s;
  if (tid < a.k) {
    int32_t v = -1;
    if (tid < found) v = (int32_t)(a.largest ? taken[found - 1 - tid] : taken[tid]);
    a.out[tid] = v;
  }
  if (a.truth && found >= 1) {                                 // k == 1: taken[0] is the pick
    const long row = a.cand[taken[0]];
    if (tid < a.T) a.labels[row * a.T + tid] = a.truth[row * a.T + tid];
    if (tid == 0) {
      if (a.active) a.active[row] = 0;
      if (a.log) a.log[0] = (int32_t)taken[0];
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
int check_shape(const char* who, int64_t n, int32_t T, int32_t K) {
  if (n < 1 || n > KGCN_LP_MAX_ROWS) return fail("%s: %lld rows outside 1..%d", who, (long long)n, KGCN_LP_MAX_ROWS);
  if (T < 1 || T > kMaxTasks || K < T || K > kMaxCols)
    return fail("%s: %d tasks (1..%d) over %d class columns (tasks..%d)", who, T, kMaxTasks, K, kMaxCols);
  return 0;
}

long step_blocks(int64_t n) { return (long)((n + kRowsWg - 1) / kRowsWg); }

struct Workspace {
  unsigned* running;                 // the running-task word
  double *F[2], *G[2], *partial;     // one run of doubles: 4 x [n, K], then [step blocks, T]
  size_t total;
};

Workspace carve(unsigned char* base, int64_t n, int32_t T, int32_t K) {
  Workspace o{};
  Taker t{base};
  o.running = t.take<unsigned>(1);
  const size_t head = t.off, nk = (size_t)n * K, doubles = 4 * nk + (size_t)step_blocks(n) * T;
  double* p = t.take<double>(doubles);
  o.total = head + doubles * sizeof(double) + 256;             // the run is counted as it is, not rounded up
  if (!p) return o;
  o.F[0] = p;
  o.F[1] = p + nk;
  o.G[0] = p + 2 * nk;
  o.G[1] = p + 3 * nk;
  o.partial = p + 4 * nk;
  return o;
}

// max_bytes: what the caller grants a stored n x n affinity matrix
int check_points(const char* who, int64_t n, int32_t d, const double* gamma, int64_t max_bytes = INT64_MAX) {
  if (n < 1 || n > KGCN_LP_MAX_ROWS || d < 1) return fail("%s: %lld points of %d attributes (1..%d points)", who, (long long)n, d, KGCN_LP_MAX_ROWS);
  if (n * n * 8 > max_bytes)
    return fail("%s: the %lld x %lld affinity matrix takes %lld bytes, over max_bytes = %lld; refused before any launch", who,
                (long long)n, (long long)n, (long long)(n * n * 8), (long long)max_bytes);
  if (!gamma || !(*gamma > 0.0) || !(*gamma < INFINITY)) return fail("%s: gamma must be positive and finite", who);
  return 0;
}

void launch_norms(const double* x, int64_t n, int32_t d, double* norms, hipStream_t s) {
  hipLaunchKernelGGL(lp_norms_kernel, dim3(blocks_of((long)n)), dim3(256), 0, s, x, (long)n, d, norms);
}

template <int KC>
int launch_free_step(const char* who, const LpArgs& a, hipStream_t s) {
  if (int rc = allow_full_lds<lp_free_step_kernel<KC>>(kFreeStepLds, who)) return rc;
  hipLaunchKernelGGL(lp_free_step_kernel<KC>, dim3((unsigned)((a.n + kTile - 1) / kTile)), dim3(256), kFreeStepLds, s, a);
  return 0;
}

// THE protocol of both propagation entry points: W != NULL sweeps the stored matrix, W == NULL rebuilds it from x (whose norms the
// start writes to `norms` and the later calls read there).
int lp_propagate_steps(const char* who, const double* W, const double* x, double* norms, int32_t d, const double* gamma,
                       const double* scale, int64_t n, const int32_t* labels, const int32_t* task_col, int32_t tasks, int32_t cols,
                       int32_t variant, const double* alpha, const double* tol, int32_t max_iter, int32_t first_step, int32_t steps,
                       int32_t* n_iter, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_shape(who, n, tasks, cols)) return rc;
  if (!W)
    if (int rc = check_points(who, n, d, gamma)) return rc;
  if (variant != KGCN_LP_PROPAGATION && variant != KGCN_LP_SPREADING) return fail("%s: variant %d", who, variant);
  if (variant == KGCN_LP_SPREADING && !(alpha && *alpha > 0.0 && *alpha < 1.0)) return fail("%s: alpha must lie in (0, 1)", who);
  if (!tol || !(*tol >= 0.0) || !(*tol < INFINITY)) return fail("%s: the tolerance must be finite and not negative", who);
  if (max_iter < 0 || first_step < 0 || steps < 0 || (int64_t)first_step + steps >= INT32_MAX)
    return fail("%s: max_iter %d, first_step %d, steps %d", who, max_iter, first_step, steps);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)carve(nullptr, n, tasks, cols).total)) return rc;
  if ((!W && (!x || !norms)) || !scale || !labels || !task_col || !n_iter || !status) return fail("%s: NULL operand", who);
  const Workspace ws = carve(aligned_base(workspace), n, tasks, cols);
  hipStream_t s = as_stream(stream);
  const long blocks = step_blocks(n);
  const bool spreading = variant == KGCN_LP_SPREADING;
  LpArgs a{};
  a.W = W;
  if (!W) a.pts = RbfSets{x, norms, (long)n, x, norms, (long)n, d, 1, *gamma};
  a.scale = scale, a.labels = labels, a.task_col = task_col;
  a.n = (long)n, a.T = tasks, a.K = cols, a.spreading = spreading ? 1 : 0;
  a.alpha = spreading ? *alpha : 0.0, a.tol = *tol, a.max_iter = max_iter;
  a.partial = ws.partial, a.status = status, a.n_iter = n_iter, a.running = ws.running;
  if (first_step == 0) {
    if (int rc = zero_async(who, status, (size_t)tasks * sizeof(int32_t), s)) return rc;
    if (int rc = zero_async(who, n_iter, (size_t)tasks * sizeof(int32_t), s)) return rc;
    if (!W) launch_norms(x, n, d, norms, s);
    a.Fnext = ws.F[0];
    a.Gnext = ws.G[0];
    hipLaunchKernelGGL(lp_init_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(lp_decide_kernel, dim3(1), dim3(64), 0, s, a, (int)blocks);
  }
  for (int k = first_step; k < first_step + steps; ++k) {
    a.step = k;
    a.Fprev = ws.F[k & 1];
    a.Gprev = spreading ? ws.G[k & 1] : ws.F[k & 1];
    a.Fnext = ws.F[(k + 1) & 1];
    a.Gnext = ws.G[(k + 1) & 1];
    if (W) {
      if (cols <= 4) hipLaunchKernelGGL(lp_step_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, a);
      else hipLaunchKernelGGL(lp_step_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    } else if (int rc = cols <= 4 ? launch_free_step<4>(who, a, s) : launch_free_step<8>(who, a, s)) {
      return rc;
    }
    a.step = k + 1;
    hipLaunchKernelGGL(lp_decide_kernel, dim3(1), dim3(64), 0, s, a, (int)blocks);
  }
  return check_launch(who);
}

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int kgcn_rbf_affinity_f64(const double* x, int64_t n, int32_t d, const double* gamma, int64_t max_bytes, double* W,
                                     double* norms, void* stream) {
  const char* who = "kgcn_rbf_affinity_f64";
  if (int rc = check_points(who, n, d, gamma, max_bytes)) return rc;
  if (!x || !W || !norms) return fail("%s: NULL operand", who);
  hipStream_t s = as_stream(stream);
  launch_norms(x, n, d, norms, s);
  const long nt = (long)((n + kTile - 1) / kTile);
  hipLaunchKernelGGL(lp_affinity_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, x, norms, (long)n, d, *gamma, W);
  return check_launch(who);
}

extern "C" int kgcn_lp_degrees_f64(const double* W, int64_t n, double* s_out, double* d_out, void* stream) {
  const char* who = "kgcn_lp_degrees_f64";
  if (n < 1 || n > KGCN_LP_MAX_ROWS) return fail("%s: %lld rows outside 1..%d", who, (long long)n, KGCN_LP_MAX_ROWS);
  if (!W || !s_out || !d_out) return fail("%s: NULL operand", who);
  hipLaunchKernelGGL(lp_degrees_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), W, (long)n, s_out, d_out);
  return check_launch(who);
}

extern "C" int64_t kgcn_lp_workspace_bytes(int64_t n, int32_t tasks, int32_t cols) {
  if (check_shape("kgcn_lp_workspace_bytes", n, tasks, cols)) return -1;
  return (int64_t)carve(nullptr, n, tasks, cols).total;
}

extern "C" int kgcn_lp_propagate_f64(const double* W, const double* scale, int64_t n, const int32_t* labels, const int32_t* task_col,
                                     int32_t tasks, int32_t cols, int32_t variant, const double* alpha, const double* tol, int32_t max_iter,
                                     int32_t first_step, int32_t steps, int32_t* n_iter, int32_t* status, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_lp_propagate_f64";
  if (!W) return fail("%s: NULL operand", who);
  return lp_propagate_steps(who, W, nullptr, nullptr, 0, nullptr, scale, n, labels, task_col, tasks, cols, variant, alpha, tol, max_iter,
                            first_step, steps, n_iter, status, workspace, workspace_bytes, stream);
}

extern "C" int kgcn_lp_propagate_free_f64(const double* x, int32_t d, const double* gamma, double* norms, const double* scale, int64_t n,
                                          const int32_t* labels, const int32_t* task_col, int32_t tasks, int32_t cols, int32_t variant,
                                          const double* alpha, const double* tol, int32_t max_iter, int32_t first_step, int32_t steps,
                                          int32_t* n_iter, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_lp_propagate_free_f64";
  if (!x || !norms) return fail("%s: NULL operand", who);
  return lp_propagate_steps(who, nullptr, x, norms, d, gamma, scale, n, labels, task_col, tasks, cols, variant, alpha, tol, max_iter,
                            first_step, steps, n_iter, status, workspace, workspace_bytes, stream);
}

extern "C" int kgcn_rbf_apply_f64(const double* xq, int64_t m, const double* xr, int64_t n, int32_t d, const double* gamma, const double* G,
                                  int32_t cols, int32_t same_set, int32_t zero_diagonal, double* out, double* norms_q, double* norms_r,
                                  void* stream) {
  const char* who = "kgcn_rbf_apply_f64";
  if (int rc = check_points(who, n, d, gamma)) return rc;
  if (m < 1 || m > ((int64_t)1 << 36)) return fail("%s: %lld queries", who, (long long)m);
  if (cols < 1 || cols > kMaxCols) return fail("%s: %d columns outside 1..%d", who, cols, kMaxCols);
  if (!xq || !xr || !G || !out || !norms_r || (!same_set && !norms_q)) return fail("%s: NULL operand", who);
  if (same_set ? (xq != xr || m != n) : zero_diagonal != 0)
    return fail("%s: same_set takes one point set as queries and references; zero_diagonal takes same_set", who);
  hipStream_t s = as_stream(stream);
  launch_norms(xr, n, d, norms_r, s);
  if (!same_set) launch_norms(xq, m, d, norms_q, s);
  const RbfSets sets{xq, same_set ? norms_r : norms_q, (long)m, xr, norms_r, (long)n, d, same_set ? 1 : 0, *gamma};
  const dim3 grid((unsigned)((m + kTile - 1) / kTile));
  if (cols <= 4) hipLaunchKernelGGL(rbf_apply_kernel<4>, grid, dim3(256), 0, s, sets, zero_diagonal ? 1 : 0, G, cols, out);
  else hipLaunchKernelGGL(rbf_apply_kernel<8>, grid, dim3(256), 0, s, sets, zero_diagonal ? 1 : 0, G, cols, out);
  return check_launch(who);
}

extern "C" int kgcn_rbf_degrees_f64(const double* x, int64_t n, int32_t d, const double* gamma, double* s_out, double* d_out, double* norms,
                                    void* stream) {
  const char* who = "kgcn_rbf_degrees_f64";
  if (int rc = check_points(who, n, d, gamma)) return rc;
  if (!x || !s_out || !d_out || !norms) return fail("%s: NULL operand", who);
  hipStream_t s = as_stream(stream);
  launch_norms(x, n, d, norms, s);
  const RbfSets sets{x, norms, (long)n, x, norms, (long)n, d, 1, *gamma};
  hipLaunchKernelGGL(rbf_degrees_kernel, dim3((unsigned)((n + kTile - 1) / kTile)), dim3(256), 0, s, sets, s_out, d_out);
  return check_launch(who);
}

extern "C" int kgcn_lp_finish_f64(int64_t n, const int32_t* task_col, int32_t tasks, int32_t cols, int32_t steps_done, double* dist,
                                  const void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_lp_finish_f64";
  if (int rc = check_shape(who, n, tasks, cols)) return rc;
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)carve(nullptr, n, tasks, cols).total)) return rc;
  if (!task_col || !dist || steps_done < 0) return fail("%s: NULL operand or %d steps", who, steps_done);
  const Workspace ws = carve(aligned_base(const_cast<void*>(workspace)), n, tasks, cols);   // read only
  hipLaunchKernelGGL(lp_finish_kernel, dim3(blocks_of((long)n * tasks)), dim3(256), 0, as_stream(stream), ws.F[steps_done & 1],
                     task_col, (long)n, tasks, cols, dist);
  return check_launch(who);
}

extern "C" int kgcn_lp_scores_f64(const double* dist, int64_t n, const int32_t* task_col, int32_t tasks, int32_t cols,
                                  const int32_t* cand, int64_t m, double* scores, void* stream) {
  const char* who = "kgcn_lp_scores_f64";
  if (int rc = check_shape(who, n, tasks, cols)) return rc;
  if (m < 0 || m > KGCN_LP_MAX_ROWS) return fail("%s: %lld candidates", who, (long long)m);
  if (m == 0) return 0;
  if (!dist || !task_col || !cand || !scores) return fail("%s: NULL operand", who);
  hipLaunchKernelGGL(lp_scores_kernel, dim3(blocks_of((long)m)), dim3(256), 0, as_stream(stream), dist, task_col, (long)n, tasks,
                     cols, cand, (long)m, scores);
  return check_launch(who);
}

extern "C" int kgcn_lp_select_f64(const double* score, const int32_t* cand, int64_t m, int64_t n, int32_t* active, int32_t k,
                                  int32_t largest, int32_t* out, int32_t* labels, const int32_t* truth, int32_t tasks, int32_t* log,
                                  void* stream) {
  const char* who = "kgcn_lp_select_f64";
  if (n < 1 || n > KGCN_LP_MAX_ROWS || m < 0 || m > KGCN_LP_MAX_ROWS) return fail("%s: %lld candidates of %lld rows", who, (long long)m, (long long)n);
  if (k < 1 || k > KGCN_LP_MAX_PICKS) return fail("%s: %d picks outside 1..%d", who, k, KGCN_LP_MAX_PICKS);
  if (!out || (m > 0 && (!score || !cand))) return fail("%s: NULL operand", who);
  if (truth && (k != 1 || !labels || tasks < 1 || tasks > kMaxTasks))
    return fail("%s: teaching takes the single pick (k = 1), the label matrix and 1..%d tasks", who, kMaxTasks);
  SelArgs a{score, cand, active, (long)m, (long)n, k, largest ? 1 : 0, out, labels, truth, tasks, log};
  hipLaunchKernelGGL(lp_select_kernel, dim3(1), dim3(256), 0, as_stream(stream), a);
  return check_launch(who);
}
