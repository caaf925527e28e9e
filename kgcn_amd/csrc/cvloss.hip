// Loss head of the compound-protein interaction networks (sample_chem/compound-protein_interaction/multitask.py:53-86,
// singletask.py with T = 1): logits [B, 2, T], a two-way softmax per task under mask_label.
//
//   d        = z1 - z0                                       (logits[b, 1, t] - logits[b, 0, t])
//   ce       = softplus(z_other - z_label) = max(u, 0) + log1p(exp(-|u|)),  u = label ? -d : d     (finite at |z| = 80)
//   p1       = sigmoid(d), from e = exp(-|d|): d >= 0 ? 1 / (1 + e) : e / (1 + e)                  (prediction[b, t])
//   argmax   = d > 0 ? 1 : 0                                 (a tie goes to class 0, as tf.argmax)
//   dlogits  = mask ? (p1 - label) : 0 for class 1, its negation for class 0
//
// One workgroup per task sums its column over the rows in a fixed order (thread-strided partials, one tree): no float atomics.
// A one-workgroup kernel behind it adds the task costs (cost = sum_t each_cost[t]: a sum, not a mean) and, when the call carries
// an accumulator block, adds the batch's [each_cost | each_correct | each_count | cost] into it in place -- a captured step
// accumulates a whole epoch on the device and the host reads one block back (the reference sums on the host per batch,
// kgcn/core.py:269-271).  Counts are floats holding integers: exact up to 2^24 rows per accumulator.
#include "kgcn_common.h"

namespace kgcn {
namespace {

constexpr int kBlock = 256;

// sums of a, b, c over the workgroup, the same tree for every call
__device__ __forceinline__ void block_sum3(float& a, float& b, float& c, float (*red)[kBlock]) {
  const int t = threadIdx.x;
  red[0][t] = a;
  red[1][t] = b;
  red[2][t] = c;
  __syncthreads();
#pragma unroll
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if (t < off) {
      red[0][t] += red[0][t + off];
      red[1][t] += red[1][t + off];
      red[2][t] += red[2][t + off];
    }
    __syncthreads();
  }
  a = red[0][0];
  b = red[1][0];
  c = red[2][0];
}

// stats [3 T + 1] = each_cost [T] | each_correct [T] | each_count [T] | cost; this kernel writes the first 3 T
__global__ __launch_bounds__(kBlock) void softmax2_ce_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                            const float* __restrict__ mask_label, long B, int T,
                                                            float* __restrict__ dlogits, float* __restrict__ prediction,
                                                            float* __restrict__ stats) {
  __shared__ float red[3][kBlock];
  const int t = blockIdx.x;
  float cost = 0.f, correct = 0.f, count = 0.f;
  for (long b = threadIdx.x; b < B; b += kBlock) {
    const long i0 = b * 2 * T + t, i1 = i0 + T;
    const float d = logits[i1] - logits[i0];
    const bool pos = labels[b * T + t] != 0.f;
    const bool used = mask_label[b * T + t] != 0.f;
    const float e = expf(-fabsf(d));
    const float inv = 1.0f / (1.0f + e);
    const float p1 = d >= 0.f ? inv : e * inv;
    prediction[b * T + t] = p1;
    float g = 0.f;
    if (used) {
      const float u = pos ? -d : d;
      cost += fmaxf(u, 0.f) + log1pf(e);
      correct += ((d > 0.f) == pos) ? 1.f : 0.f;
      count += 1.f;
      g = p1 - (pos ? 1.f : 0.f);
    }
    dlogits[i1] = g;
    dlogits[i0] = -g;
  }
  block_sum3(cost, correct, count, red);
  if (threadIdx.x == 0) {
    stats[t] = cost;
    stats[T + t] = correct;
    stats[2 * T + t] = count;
  }
}

// cost = sum_t each_cost[t], t ascending in thread-strided partials and one tree; accum += stats
__global__ __launch_bounds__(kBlock) void softmax2_finish_kernel(float* __restrict__ stats, int T, float* __restrict__ accum) {
  __shared__ float red[3][kBlock];
  float c = 0.f, z0 = 0.f, z1 = 0.f;
  for (int t = threadIdx.x; t < T; t += kBlock) c += stats[t];
  block_sum3(c, z0, z1, red);
  if (threadIdx.x == 0) stats[3 * T] = c;
  if (accum) {
    for (int i = threadIdx.x; i < 3 * T; i += kBlock) accum[i] += stats[i];
    if (threadIdx.x == 0) accum[3 * T] += c;
  }
}

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int kgcn_multitask_softmax2_ce_f32(const float* logits, const float* labels, const float* mask_label, int64_t batch,
                                              int32_t tasks, float* dlogits, float* prediction, float* stats, float* accum,
                                              void* stream) {
  const char* who = "kgcn_multitask_softmax2_ce_f32";
  if (batch < 1 || batch > KGCN_SOFTMAX2_MAX_BATCH) return fail("%s: batch %lld outside 1..%d", who, (long long)batch, KGCN_SOFTMAX2_MAX_BATCH);
  if (tasks < 1 || tasks > KGCN_SOFTMAX2_MAX_TASKS) return fail("%s: %d tasks outside 1..%d", who, tasks, KGCN_SOFTMAX2_MAX_TASKS);
  if (!logits || !labels || !mask_label || !dlogits || !prediction || !stats) return fail("%s: NULL operand", who);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(softmax2_ce_kernel, dim3((unsigned)tasks), dim3(kBlock), 0, s, logits, labels, mask_label, (long)batch, tasks,
                     dlogits, prediction, stats);
  hipLaunchKernelGGL(softmax2_finish_kernel, dim3(1), dim3(kBlock), 0, s, stats, tasks, accum);
  return check_launch(who);
}
