// The caller's workspace of the sort-and-rank ops (graph and hash kernels, pair ranking, CV metrics, link prediction, SVM, label
// propagation, COO packing): every array starts on a 256-byte boundary of a base that is itself rounded up to one, so a layout's
// total carries 256 bytes of slack and the caller may hand in any pointer.  A layout function carves with a Taker and is called
// twice: with a NULL base to size the workspace, with the aligned base to get the pointers.
#pragma once

#include "kgcn_common.h"

namespace kgcn {

__host__ __device__ __forceinline__ size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }
inline unsigned char* aligned_base(void* ws) { return reinterpret_cast<unsigned char*>(al256(reinterpret_cast<size_t>(ws))); }

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

inline int check_workspace(const char* who, const void* ws, int64_t have, int64_t need) {
  if (!ws || have < need) return fail("%s: workspace %lld < %lld bytes", who, (long long)have, (long long)need);
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
