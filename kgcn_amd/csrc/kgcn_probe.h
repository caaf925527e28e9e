// Cycle probe of the development builds (-DKGCN_PROBE; compiled out of the product library): a wave sums the cycles it spends
// between consecutive stamps per phase and writes the sums to a device buffer that a tool under tools/ hands in and reads back
// (phase_probe.py, pairs_probe.py, fwd_pairs_probe.py, gemm3_probe.py, gemmh_probe.py, gemmh_fwd_probe.py, gemmb_probe.py).
//   KP_BUFFER(name, setter)       the file's buffer pointer and the extern "C" entry point that sets it
//   KP_DECL(n)                    n phase sums, the clock starts
//   KP_STAMP(k)                   the cycles since the previous stamp belong to phase k
//   KP_FLUSH(buffer, slot, n)     lane 0 of the wave writes its sums to buffer[slot * n ..] (`lane` is the kernel's)
#pragma once

#include <hip/hip_runtime.h>

#ifdef KGCN_PROBE
namespace kgcn {
inline int probe_set(const void* symbol, void* buf) {
  long long* p = static_cast<long long*>(buf);
  return hipMemcpyToSymbol(symbol, &p, sizeof(p)) == hipSuccess ? 0 : 1;
}
}  // namespace kgcn
#define KP_BUFFER(name, setter)         \
  __device__ long long* name = nullptr; \
  extern "C" int setter(void* buf) { return kgcn::probe_set(&name, buf); }
#define KP_DECL(n) long long pt_[n] = {}; long long pc_ = __builtin_readcyclecounter();
#define KP_STAMP(k) { const long long n_ = __builtin_readcyclecounter(); pt_[k] += n_ - pc_; pc_ = n_; }
#define KP_FLUSH(buffer, slot, n) if (buffer && lane == 0) { for (int k_ = 0; k_ < n; ++k_) buffer[(long)(slot) * n + k_] = pt_[k_]; }
#else
#define KP_BUFFER(name, setter)
#define KP_DECL(n)
#define KP_STAMP(k)
#define KP_FLUSH(buffer, slot, n)
#endif
