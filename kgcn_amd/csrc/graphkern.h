// What graphkern.hip (classical graph kernels) and hashkern.hip (hash graph kernels over them) share: the ranking of rows by
// two 64-bit words, and the launchers of the colour refinement, the colour runs and the shortest-path features.  The launchers live
// in graphkern.hip and take a number of COPIES: colours / labels [copies, T*M] over ONE stored batch, row c * T*M + p reading
// rowptr / cv of row p, sorted_nbr [copies, nnz], run slots [copies * T] (slot c * T + t).  copies == 1 is the plain kernel.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "workspace.h"

namespace kgcn {

typedef unsigned long long u64;

int wl_refine_run(const char* who, const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, int copies,
                  uint64_t hash_mask, int32_t* sorted_nbr, uint64_t* key_hi, uint64_t* key_lo, void* stream);
int wl_rank_run(const char* who, const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, int copies,
                const int32_t* sorted_nbr, const uint64_t* key_hi, const uint64_t* key_lo, int32_t* new_colors, int64_t* info,
                void* workspace, int64_t workspace_bytes, void* stream);
// column of a run = column_offset + copy * column_stride + colour
int wl_runs_run(const char* who, const int32_t* colors, const int32_t* num_nodes, int32_t graphs, int32_t rows, int copies,
                uint64_t column_offset, uint64_t column_stride, int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph,
                int32_t* run_count, int64_t capacity, void* workspace, int64_t workspace_bytes, void* stream);
// column of a run = copy << 32 | key; the breadth-first searches of a graph run once for all copies
int sp_features_run(const char* who, const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* labels, int copies,
                    int32_t num_labels, int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph, int32_t* run_count,
                    int64_t capacity, void* workspace, int64_t workspace_bytes, void* stream);
// copies >= 1 and copies * T * M rows that int32 positions index, or the reason
int check_copies(const char* who, const kgcn_csr_batch* a, int32_t copies);

namespace {

__global__ __launch_bounds__(256) void iota_kernel(uint32_t* __restrict__ idx, long n) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p < n) idx[p] = (uint32_t)p;
}

__global__ __launch_bounds__(256) void gather_u64_kernel(const u64* __restrict__ src, const uint32_t* __restrict__ idx,
                                                         u64* __restrict__ dst, long n) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p < n) dst[p] = src[idx[p]];
}

size_t sort_temp_bytes(size_t n) {
  size_t b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (const u64*)nullptr, (u64*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, 64u,
                                  (hipStream_t)0);                // const keys in, here and in every sort: one instantiation
  return b;
}
size_t scan_temp_bytes(size_t n) {
  size_t b = 0;
  (void)rocprim::inclusive_scan(nullptr, b, (int*)nullptr, (int*)nullptr, n, rocprim::plus<int>(), (hipStream_t)0);
  return b;
}

// ---- the ranking of n rows by two 64-bit words (kgcn_wl_rank_i32, kgcn_rank_pairs_i64) -------------------------------------------
// Two stable radix passes (low word, then high word) carry the row index; a row that exists and differs from its predecessor in
// that order opens a class; an inclusive scan of those flags is the dense rank.
struct RankLayout {
  uint32_t *idx0, *idx1, *idx2;      // idx2: the rows in (hi, lo) order
  u64 *lo_s, *hi_g, *hi_s;           // hi_s: the high words in that order
  int *flags, *pos;
  void* temp;
  size_t temp_bytes, total;
};
// carves behind whatever t has handed out already; total counts that too
RankLayout rank_layout(Taker& t, size_t n) {
  RankLayout o{};
  o.idx0 = t.take<uint32_t>(n);
  o.idx1 = t.take<uint32_t>(n);
  o.idx2 = t.take<uint32_t>(n);
  o.lo_s = t.take<u64>(n);
  o.hi_g = t.take<u64>(n);
  o.hi_s = t.take<u64>(n);
  o.flags = t.take<int>(n);
  o.pos = t.take<int>(n);
  const size_t a = n ? sort_temp_bytes(n) : 0, b = n ? scan_temp_bytes(n) : 0;
  o.temp_bytes = a > b ? a : b;
  o.temp = t.take<unsigned char>(o.temp_bytes);
  o.total = t.off + 256;
  return o;
}
RankLayout rank_layout(unsigned char* base, size_t n) {
  Taker t{base};
  return rank_layout(t, n);
}

// n > 0 rows in (hi, lo) order: leaves o.idx2 and o.hi_s
int rank_order(const char* who, const RankLayout& o, const u64* hi, const u64* lo, long n, hipStream_t s) {
  const unsigned nb = blocks_of(n);
  hipLaunchKernelGGL(iota_kernel, dim3(nb), dim3(256), 0, s, o.idx0, n);
  size_t temp = o.temp_bytes;
  if (rocprim::radix_sort_pairs(o.temp, temp, lo, o.lo_s, o.idx0, o.idx1, (size_t)n, 0u, 64u, s) != hipSuccess)
    return fail("%s: rocprim::radix_sort_pairs failed", who);
  hipLaunchKernelGGL(gather_u64_kernel, dim3(nb), dim3(256), 0, s, hi, o.idx1, o.hi_g, n);
  temp = o.temp_bytes;
  if (rocprim::radix_sort_pairs(o.temp, temp, (const u64*)o.hi_g, o.hi_s, o.idx1, o.idx2, (size_t)n, 0u, 64u, s) != hipSuccess)
    return fail("%s: rocprim::radix_sort_pairs failed", who);
  return 0;
}

// Args: `order` (the rows in sorted order) and two device functions, exists(row) and same_as_prev(p) for p > 0
template <typename Args>
__global__ __launch_bounds__(256) void rank_flag_kernel(Args a, int* __restrict__ flags, long n) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const bool eq_prev = p > 0 && a.same_as_prev(p);
  flags[p] = (a.exists(a.order[p]) && !eq_prev) ? 1 : 0;
}

template <typename Args>
__global__ __launch_bounds__(256) void rank_write_kernel(Args a, const int* __restrict__ pos, int32_t* __restrict__ out,
                                                         u64* __restrict__ info, long n) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t row = a.order[p];
  out[row] = a.exists(row) ? pos[p] - 1 : -1;
  if (p == n - 1) info[0] = (u64)pos[p];
}

// after rank_order: out[row] = dense rank of an existing row, -1 of the others; info[0] = classes
template <typename Args>
int rank_sorted(const char* who, const Args& a, const RankLayout& o, int32_t* out, u64* info, long n, hipStream_t s) {
  const unsigned nb = blocks_of(n);
  hipLaunchKernelGGL(rank_flag_kernel<Args>, dim3(nb), dim3(256), 0, s, a, o.flags, n);
  size_t temp = o.temp_bytes;
  if (rocprim::inclusive_scan(o.temp, temp, o.flags, o.pos, (size_t)n, rocprim::plus<int>(), s) != hipSuccess)
    return fail("%s: rocprim::inclusive_scan failed", who);
  hipLaunchKernelGGL(rank_write_kernel<Args>, dim3(nb), dim3(256), 0, s, a, o.pos, out, info, n);
  return check_launch(who);
}

}  // namespace
}  // namespace kgcn
