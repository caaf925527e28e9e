// How a wave and a 256-thread workgroup sum: the small step under the two-stage reductions of kgcn_common.h, and the finish
// kernel of the task-column loss heads (cvloss.hip, regress.hip).  No float atomics: every sum here has ONE order.
#pragma once

#include <hip/hip_runtime.h>

namespace kgcn {

// Sum over the 64 lanes of a wave, every lane gets it: the xor butterfly 32, 16, .. 1 (floats; an int count in coopack.hip).
template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Sums of v[0..M) over a workgroup of exactly 256 threads, every thread gets them; red is M x 256 elements of LDS.
// THE ORDER IS THE CONTRACT: a halving tree 128, 64, .. 1 in which thread t < off adds element t + off to element t.  Every
// result of the library that passes through here keeps its bits only as long as that pairing stays.
// Barriers: after the write, after every level, and after the read -- so a second call on the same red is always safe.
template <typename V, int M>
__device__ __forceinline__ void block_sum(V (&v)[M], V (*red)[256]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < M; ++q) red[q][t] = v[q];
  __syncthreads();
#pragma unroll
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int q = 0; q < M; ++q) red[q][t] += red[q][t + off];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < M; ++q) v[q] = red[q][0];
  __syncthreads();
}

// One value; red is 256 elements.  The same tree with the same barriers, written out over a flat red and not forwarded to the
// form above: through the array form the compiler emits each level's add with its operands exchanged (the same sum, another
// instruction stream for every kernel that summed a scalar before the two forms met here).
template <typename V>
__device__ __forceinline__ V block_sum(V v, V* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const V s = red[0];
  __syncthreads();
  return s;
}

// Second kernel of a task-column loss head, one workgroup.  stats = S blocks of T per-task statistics (the first block: the
// per-task cost) | total [| mean]: adds the T costs (t ascending in thread-strided partials, one tree), writes the total and,
// with MEAN, total / (B T) behind it, and adds the batch's S T statistics and its total into accum [S T + 1] when there is one.
template <int S, bool MEAN>
__global__ __launch_bounds__(256) void task_loss_finish_kernel(float* __restrict__ stats, long B, int T, float* __restrict__ accum) {
  __shared__ float red[1][256];
  float c[1] = {0.f};
  for (int t = threadIdx.x; t < T; t += 256) c[0] += stats[t];
  block_sum(c, red);
  if (threadIdx.x == 0) {
    stats[S * T] = c[0];
    if constexpr (MEAN) stats[S * T + 1] = c[0] / ((float)B * (float)T);
  }
  if (accum) {
    for (int i = threadIdx.x; i < S * T; i += 256) accum[i] += stats[i];
    if (threadIdx.x == 0) accum[S * T] += c[0];
  }
}

}  // namespace kgcn
