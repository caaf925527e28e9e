// The caller's workspace, one protocol for every file.  An op states its layout ONCE, in a layout function that carves with a
// Taker and is called twice: with a NULL base to size the workspace (the *_workspace_bytes query), with the caller's base to get
// the pointers (the entry point).  check_workspace refuses with one text, zero_async reports a failed memset.
//
// Two families share it:
//   * the sort-and-rank ops (graph and hash kernels, pair ranking, CV metrics, link prediction, SVM, label propagation, COO
//     packing) carve at 256 bytes from a base that is itself rounded up (aligned_base), so a layout's total carries 256 bytes of
//     slack and the caller may hand in any pointer;
//   * the ops of the training step (dense, fused GraphConv, stack, BN, SpMM, GAT, seq, conv1d, VAE, losses, ragged, pack, cpi-ig)
//     keep their packed sizes: they carve at 4 bytes (16 where a wider word follows) and use the caller's pointer as it is.  A
//     layout that holds anything accessed wider than 4 bytes states the base alignment it relies on, and check_workspace refuses
//     a base without it.
#pragma once

#include "kgcn_common.h"

namespace kgcn {

__host__ __device__ __forceinline__ size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }
inline unsigned char* aligned_base(void* ws) { return reinterpret_cast<unsigned char*>(al256(reinterpret_cast<size_t>(ws))); }

// every array starts on a multiple of `align` (a power of two) and ends on one; `off` is the total after the last take
struct Taker {
  unsigned char* base;
  size_t align = 256;
  size_t off = 0;
  explicit Taker(void* b, size_t a = 256) : base(static_cast<unsigned char*>(b)), align(a) {}
  size_t up(size_t x) const { return (x + align - 1) & ~(align - 1); }
  template <typename T>
  T* take(size_t count) {
    off = up(off);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off = up(off + count * sizeof(T));
    return p;
  }
};

// base_align: what the layout relies on for its widest access (1: nothing beyond what the element types of the caller imply)
inline int check_workspace(const char* who, const void* ws, int64_t have, int64_t need, int base_align = 1) {
  if (!ws || have < need) return fail("%s: workspace %lld < %lld bytes", who, (long long)have, (long long)need);
  if (reinterpret_cast<uintptr_t>(ws) % (uintptr_t)base_align) return fail("%s: workspace not %d-byte aligned", who, base_align);
  return 0;
}

// for the queries that are deliberate upper bounds: the layout of this shape has to fit what the query promised the caller
inline int check_layout_fits(const char* who, size_t layout_bytes, int64_t query_bytes) {
  if ((int64_t)layout_bytes > query_bytes)
    return fail("%s: layout of %lld bytes exceeds the %lld of its workspace query", who, (long long)layout_bytes, (long long)query_bytes);
  return 0;
}

inline int zero_async(const char* who, void* p, size_t bytes, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(p, 0, bytes, s);
  return e == hipSuccess ? 0 : fail("%s: hipMemsetAsync failed: %s", who, hipGetErrorString(e));
}

// a *_workspace_bytes query that refuses its shape: the reason goes to kgcn_last_error, the size is -1
template <typename... A>
int64_t refuse_query(const char* fmt, A... a) {
  fail(fmt, a...);
  return -1;
}

}  // namespace kgcn
