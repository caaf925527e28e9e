// What graphkern.hip (classical graph kernels) and hashkern.hip (hash graph kernels over them) share: the workspace carving, two
// helper kernels, and the launchers of the colour refinement, the colour runs and the shortest-path features.  The launchers live
// in graphkern.hip and take a number of COPIES: colours / labels [copies, T*M] over ONE stored batch, row c * T*M + p reading
// rowptr / cv of row p, sorted_nbr [copies, nnz], run slots [copies * T] (slot c * T + t).  copies == 1 is the plain kernel.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "kgcn_common.h"

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

__host__ __device__ __forceinline__ size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

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
  (void)rocprim::radix_sort_pairs(nullptr, b, (u64*)nullptr, (u64*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, 64u,
                                  (hipStream_t)0);
  return b;
}
size_t scan_temp_bytes(size_t n) {
  size_t b = 0;
  (void)rocprim::inclusive_scan(nullptr, b, (int*)nullptr, (int*)nullptr, n, rocprim::plus<int>(), (hipStream_t)0);
  return b;
}

struct Taker {
  unsigned char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += al256(count * sizeof(T));
    return p;
  }
};
unsigned char* aligned_base(void* ws) { return reinterpret_cast<unsigned char*>(al256(reinterpret_cast<size_t>(ws))); }

// the workspace of a ranking by two stable 64-bit radix passes over n rows (kgcn_wl_rank_i32, kgcn_rank_pairs_i64)
struct RankLayout {
  uint32_t *idx0, *idx1, *idx2;
  u64 *lo_s, *hi_g, *hi_s;
  int *flags, *pos;
  void* temp;
  size_t temp_bytes, total;
};
RankLayout rank_layout(unsigned char* base, size_t n) {
  RankLayout o{};
  Taker t{base};
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

}  // namespace
}  // namespace kgcn
