// Hash graph kernels for continuous node attributes (graph_kernel/graphkernel/hash_graph_kernel.py over
// auxiliarymethods/auxiliary_methods.py:23-36 of the reference; the driver is kgcn_amd/graph_kernel.py hash_graph_kernel): the fp64
// front end that turns attribute rows into integer buckets, the ranking of 64-bit pairs that turns buckets and (label, hash) pairs
// into dense colours, and the entry points that run R colourings of the same graphs through ONE launch sequence of the refinement,
// run and shortest-path kernels of graphkern.hip (graphkern.h).  fp64 and integers only, no float atomics: bitwise reproducible.
//
//   scale    hash_graph_kernel.py:38-40 (sklearn.preprocessing.scale) with a stated summation order, so that numpy can restate it
//            bit for bit: per column, rows are added one after another in ascending order inside chunks of 256 rows (one thread a
//            (chunk, column), the column the fast axis: a wave reads consecutive doubles), then one thread a column adds the chunk
//            sums in ascending chunk order.  mean = sum / rows; the same two stages over (x - mean) * (x - mean); std = sqrt(sum /
//            rows); scaled = (x - mean) / (std == 0 ? 1 : std).  Every sum starts from +0.0 and nothing is fused: the Makefile
//            builds this file with -ffp-contract=off (under the library's -ffp-contract=fast the backend fuses a product into
//            a sum whatever `#pragma clang fp contract(off)` says, and __dmul_rn / __dadd_rn are the plain operators).
//   buckets  auxiliary_methods.py:31: floor((x . v_r + b_r) / w), acc = 0, acc = acc + x_k * v_rk for k ascending (unfused).  A
//            workgroup stages its rows in LDS once (row stride d | 1 doubles: 32 lanes of a ds_read_b64 fall on 32 different bank
//            pairs) and every draw reads them there; lane = row, so a draw's bucket row is written coalesced.  A value that is not
//            finite or not below 2^62 in magnitude is counted (integer atomic) and written as 0: the caller refuses the count.
//   rank     auxiliary_methods.py:34 / wl_kernel.py:66-70 (np.unique(..., return_inverse=True)): dense ranks of (hi, lo) int64
//            pairs in ascending signed order by two stable 64-bit radix passes over the sign-flipped words, as kgcn_wl_rank_i32
//            ranks its keys.  A row marked as not existing sorts as (all ones, all ones) and gets -1; an existing row whose hi is
//            2^63 - 1 would sort among them and is counted in info[1] for the caller to refuse.
#include <math.h>

#include "graphkern.h"

namespace kgcn {
namespace {

constexpr int kChunkRows = 256;      // rows a first-stage thread adds: part of the stated summation order
constexpr int kLshMaxDim = KGCN_LSH_MAX_DIM;
constexpr u64 kSign = 1ull << 63;

// part [chunks, d]: the chunk sums of x (kSquares: of (x - mean)^2)
template <bool kSquares>
__global__ __launch_bounds__(256) void attr_chunk_sums_kernel(const double* __restrict__ x, const double* __restrict__ mean, long rows,
                                                              int d, long chunks, double* __restrict__ part) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= chunks * d) return;
  const long ch = idx / d, r0 = ch * kChunkRows, r1 = min(rows, r0 + kChunkRows);
  const int col = (int)(idx - ch * d);
  const double m = kSquares ? mean[col] : 0.0;
  double acc = 0.0;
  for (long r = r0; r < r1; ++r) {
    double v = x[r * d + col];
    if (kSquares) {
      const double dv = v - m;
      v = dv * dv;
    }
    acc = acc + v;
  }
  part[idx] = acc;
}

// out[col] = (sum over the chunks in ascending order) / rows, kSquares: its square root
template <bool kSquares>
__global__ __launch_bounds__(256) void attr_finish_kernel(const double* __restrict__ part, long rows, int d, long chunks,
                                                          double* __restrict__ out) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= d) return;
  double acc = 0.0;
  for (long ch = 0; ch < chunks; ++ch) acc = acc + part[ch * d + col];
  const double q = acc / (double)rows;
  out[col] = kSquares ? sqrt(q) : q;
}

__global__ __launch_bounds__(256) void attr_scale_kernel(const double* __restrict__ x, const double* __restrict__ mean,
                                                         const double* __restrict__ sd, long rows, int d, double* __restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * d) return;
  const int col = (int)(idx % d);
  const double s = sd[col];
  out[idx] = (x[idx] - mean[col]) / (s == 0.0 ? 1.0 : s);
}

__global__ __launch_bounds__(256) void lsh_buckets_kernel(const double* __restrict__ x, const double* __restrict__ v,
                                                          const double* __restrict__ b, double w, long rows, int d, int draws,
                                                          int rows_pb, long long* __restrict__ bucket, u64* __restrict__ errors) {
  extern __shared__ double xs[];                               // [rows_pb, ld]
  const int tid = threadIdx.x, ld = d | 1;
  const long r0 = (long)blockIdx.x * rows_pb;
  const int nr = (int)min((long)rows_pb, rows - r0);
  for (int i = tid; i < nr * d; i += 256) {                    // the rows of a workgroup are one contiguous piece of x
    const int rr = i / d;
    xs[rr * ld + (i - rr * d)] = x[r0 * d + i];
  }
  __syncthreads();
  const int row = tid % rows_pb, group = tid / rows_pb, groups = 256 / rows_pb;
  if (group >= groups || row >= nr) return;
  const double* xr = xs + row * ld;
  for (int r = group; r < draws; r += groups) {
    const double* vr = v + (long)r * d;
    double acc = 0.0;
    for (int k = 0; k < d; ++k) acc = acc + xr[k] * vr[k];
    const double z = (acc + b[r]) / w;
    long long q = 0;
    if (fabs(z) < 0x1p62) q = (long long)floor(z);             // false for NaN and the infinities too
    else atomicAdd(errors, 1ull);
    bucket[(long)r * rows + r0 + row] = q;
  }
}

// the sign-flipped words of the rows that exist, all ones for the others; info[1] counts existing rows that sort as missing ones
__global__ __launch_bounds__(256) void pair_keys_kernel(const long long* __restrict__ hi, const long long* __restrict__ lo,
                                                        const int32_t* __restrict__ mark, long n, u64* __restrict__ khi,
                                                        u64* __restrict__ klo, u64* __restrict__ info) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const bool exists = !mark || mark[p] >= 0;
  const u64 h = (u64)hi[p] ^ kSign;
  if (exists && h == ~0ull) atomicAdd(&info[1], 1ull);
  khi[p] = exists ? h : ~0ull;
  klo[p] = exists ? ((u64)lo[p] ^ kSign) : ~0ull;
}

struct PairArgs {
  const u64* hi_s;                   // high words in sorted order
  const u64* klo;                    // low words by row
  const uint32_t* order;             // rows in (hi, lo) order
  const int32_t* mark;

  __device__ __forceinline__ bool exists(uint32_t row) const { return !mark || mark[row] >= 0; }
  __device__ __forceinline__ bool same_as_prev(long p) const {
    return hi_s[p] == hi_s[p - 1] && klo[order[p]] == klo[order[p - 1]];
  }
};

struct PairLayout {
  u64 *khi, *klo;
  RankLayout rank;
  size_t total;
};
PairLayout pair_layout(unsigned char* base, size_t n) {
  PairLayout o{};
  Taker t{base};
  o.khi = t.take<u64>(n);
  o.klo = t.take<u64>(n);
  o.rank = rank_layout(t, n);
  o.total = t.off + 256;
  return o;
}

// one array: the chunk sums
size_t attr_scale_bytes(long chunks, int32_t d) { return al256((size_t)chunks * d * sizeof(double)) + 256; }

int check_attr(const char* who, int64_t rows, int32_t d) {
  if (rows < 1 || rows >= (int64_t)INT32_MAX) return fail("%s: %lld rows outside 1..2^31-2", who, (long long)rows);
  if (d < 1 || d > kLshMaxDim) return fail("%s: %d attributes a row outside 1..%d", who, d, kLshMaxDim);
  return 0;
}

inline long chunks_of(int64_t rows) { return (long)((rows + kChunkRows - 1) / kChunkRows); }

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int64_t kgcn_attr_scale_workspace_bytes(int64_t rows, int32_t d) {
  if (check_attr("kgcn_attr_scale_workspace_bytes", rows, d)) return -1;
  return (int64_t)attr_scale_bytes(chunks_of(rows), d);
}

extern "C" int kgcn_attr_scale_f64(const double* x, int64_t rows, int32_t d, double* scaled, double* mean, double* std_dev,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_attr_scale_f64";
  if (int rc = check_attr(who, rows, d)) return rc;
  if (!x || !scaled || !mean || !std_dev) return fail("%s: NULL operand", who);
  const long chunks = chunks_of(rows);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)attr_scale_bytes(chunks, d))) return rc;
  double* part = reinterpret_cast<double*>(aligned_base(workspace));
  hipStream_t s = as_stream(stream);
  const unsigned nb1 = blocks_of(chunks * d), nb2 = blocks_of(d);
  hipLaunchKernelGGL(attr_chunk_sums_kernel<false>, dim3(nb1), dim3(256), 0, s, x, (const double*)nullptr, (long)rows, d, chunks, part);
  hipLaunchKernelGGL(attr_finish_kernel<false>, dim3(nb2), dim3(256), 0, s, part, (long)rows, d, chunks, mean);
  hipLaunchKernelGGL(attr_chunk_sums_kernel<true>, dim3(nb1), dim3(256), 0, s, x, mean, (long)rows, d, chunks, part);
  hipLaunchKernelGGL(attr_finish_kernel<true>, dim3(nb2), dim3(256), 0, s, part, (long)rows, d, chunks, std_dev);
  hipLaunchKernelGGL(attr_scale_kernel, dim3(blocks_of((long)rows * d)), dim3(256), 0, s, x, mean, std_dev, (long)rows, d, scaled);
  return check_launch(who);
}

extern "C" int kgcn_lsh_buckets_f64(const double* scaled, int64_t rows, int32_t d, const double* v, const double* b, int32_t draws,
                                    const double* bin_width, int64_t* bucket, int64_t* errors, void* stream) {
  const char* who = "kgcn_lsh_buckets_f64";
  if (int rc = check_attr(who, rows, d)) return rc;
  if (draws < 1 || (int64_t)draws * rows >= (int64_t)INT32_MAX)
    return fail("%s: %d draws x %lld rows outside 1..2^31-2 buckets", who, draws, (long long)rows);
  if (!scaled || !v || !b || !bin_width || !bucket || !errors) return fail("%s: NULL operand", who);
  const double w = *bin_width;
  if (!(w > 0.0) || !isfinite(w)) return fail("%s: the bin width %g must be positive and finite", who, w);
  hipStream_t s = as_stream(stream);
  if (int rc = zero_async(who, errors, sizeof(int64_t), s)) return rc;
  const int ld = d | 1, rows_pb = 8192 / ld < 64 ? 8192 / ld : 64;   // at most 64 KB of LDS; kLshMaxDim keeps it >= 1
  const unsigned nb = (unsigned)((rows + rows_pb - 1) / rows_pb);
  hipLaunchKernelGGL(lsh_buckets_kernel, dim3(nb), dim3(256), (size_t)rows_pb * ld * sizeof(double), s, scaled, v, b, w, (long)rows, d,
                     draws, rows_pb, reinterpret_cast<long long*>(bucket), reinterpret_cast<u64*>(errors));
  return check_launch(who);
}

extern "C" int64_t kgcn_rank_pairs_workspace_bytes(int64_t n) {
  if (n < 0 || n >= (int64_t)INT32_MAX) return refuse_query("kgcn_rank_pairs_workspace_bytes: %lld pairs outside 0..2^31-2", (long long)n);
  return (int64_t)pair_layout(nullptr, (size_t)n).total;
}

extern "C" int kgcn_rank_pairs_i64(const int64_t* hi, const int64_t* lo, const int32_t* mark, int64_t n, int32_t* ranks, int64_t* info,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_rank_pairs_i64";
  if (n < 0 || n >= (int64_t)INT32_MAX) return fail("%s: %lld pairs outside 0..2^31-2", who, (long long)n);
  if (!info || (n > 0 && (!hi || !lo || !ranks))) return fail("%s: NULL operand", who);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)pair_layout(nullptr, (size_t)n).total)) return rc;
  hipStream_t s = as_stream(stream);
  if (int rc = zero_async(who, info, 2 * sizeof(int64_t), s)) return rc;
  if (n == 0) return 0;
  const PairLayout o = pair_layout(aligned_base(workspace), (size_t)n);
  hipLaunchKernelGGL(pair_keys_kernel, dim3(blocks_of((long)n)), dim3(256), 0, s, reinterpret_cast<const long long*>(hi),
                     reinterpret_cast<const long long*>(lo), mark, (long)n, o.khi, o.klo, reinterpret_cast<u64*>(info));
  if (int rc = rank_order(who, o.rank, o.khi, o.klo, (long)n, s)) return rc;
  const PairArgs a{o.rank.hi_s, o.klo, o.rank.idx2, mark};
  return rank_sorted(who, a, o.rank, ranks, reinterpret_cast<u64*>(info), (long)n, s);
}

// ---- R colourings of the same graphs through the kernels of graphkern.hip ---------------------------------------------------------
extern "C" int kgcn_wl_refine_copies_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, int32_t copies,
                                         uint64_t hash_mask, int32_t* sorted_nbr, uint64_t* key_hi, uint64_t* key_lo, void* stream) {
  return wl_refine_run("kgcn_wl_refine_copies_i32", a, num_nodes, colors, copies, hash_mask, sorted_nbr, key_hi, key_lo, stream);
}

extern "C" int64_t kgcn_wl_rank_copies_workspace_bytes(int64_t rows, int32_t copies) {
  if (rows < 0 || copies < 1 || rows * copies >= (int64_t)INT32_MAX)
    return refuse_query("kgcn_wl_rank_copies_workspace_bytes: %d copies x %lld rows outside 0..2^31-2", copies, (long long)rows);
  return kgcn_wl_rank_workspace_bytes(rows * copies);
}

extern "C" int kgcn_wl_rank_copies_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, int32_t copies,
                                       const int32_t* sorted_nbr, const uint64_t* key_hi, const uint64_t* key_lo, int32_t* new_colors,
                                       int64_t* info, void* workspace, int64_t workspace_bytes, void* stream) {
  return wl_rank_run("kgcn_wl_rank_copies_i32", a, num_nodes, colors, copies, sorted_nbr, key_hi, key_lo, new_colors, info, workspace,
                     workspace_bytes, stream);
}

extern "C" int64_t kgcn_graph_runs_copies_workspace_bytes(int32_t graphs, int32_t copies) {
  if (graphs < 0 || copies < 1 || (int64_t)graphs * copies >= (int64_t)INT32_MAX)
    return refuse_query("kgcn_graph_runs_copies_workspace_bytes: %d copies x %d graphs", copies, graphs);
  return kgcn_graph_runs_workspace_bytes(graphs * copies);
}

extern "C" int kgcn_wl_runs_copies_i32(const int32_t* colors, const int32_t* num_nodes, int32_t graphs, int32_t rows, int32_t copies,
                                       uint64_t column_offset, uint64_t column_stride, int64_t* run_ptr, uint64_t* run_col,
                                       int32_t* run_graph, int32_t* run_count, int64_t capacity, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  return wl_runs_run("kgcn_wl_runs_copies_i32", colors, num_nodes, graphs, rows, copies, column_offset, column_stride, run_ptr, run_col,
                     run_graph, run_count, capacity, workspace, workspace_bytes, stream);
}

extern "C" int kgcn_sp_features_copies_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* labels, int32_t copies,
                                           int32_t num_labels, int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph,
                                           int32_t* run_count, int64_t capacity, void* workspace, int64_t workspace_bytes, void* stream) {
  return sp_features_run("kgcn_sp_features_copies_i32", a, num_nodes, labels, copies, num_labels, run_ptr, run_col, run_graph, run_count,
                         capacity, workspace, workspace_bytes, stream);
}
