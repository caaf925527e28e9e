// Loss head of the compound-protein interaction networks (sample_chem/compound-protein_interaction/multitask.py:53-86,
// singletask.py with T = 1): logits [B, 2, T], a two-way softmax per task under mask_label.
//
//   d        = z1 - z0                                       (logits[b, 1, t] - logits[b, 0, t])
//   ce       = softplus(z_other - z_label) = max(u, 0) + log1p(exp(-|u|)),  u = label ? -d : d     (finite at |z| = 80)
//   p1       = sigmoid(d), from e = exp(-|d|): d >= 0 ? 1 / (1 + e) : e / (1 + e)                  (prediction[b, t])
//   argmax   = d > 0 ? 1 : 0                                 (a tie goes to class 0, as tf.argmax)
//   dlogits  = mask ? (p1 - label) : 0 for class 1, its negation for class 0
//
// One workgroup per task sums its column over the rows in a fixed order (thread-strided partials, one block_sum): no float atomics.
// The finish kernel of block_reduce.h behind it, shared with the squared-error head of regress.hip, adds the task costs (cost = sum_t each_cost[t]: a sum, not a mean) and, when the call carries
// an accumulator block, adds the batch's [each_cost | each_correct | each_count | cost] into it in place -- a captured step
// accumulates a whole epoch on the device and the host reads one block back (the reference sums on the host per batch,
// kgcn/core.py:269-271).  Counts are floats holding integers: exact up to 2^24 rows per accumulator.
#include "block_reduce.h"
#include "kgcn_common.h"

namespace kgcn {
namespace {

constexpr int kBlock = 256;

// stats [3 T + 1] = each_cost [T] | each_correct [T] | each_count [T] | cost; this kernel writes the first 3 T
__global__ __launch_bounds__(kBlock) void softmax2_ce_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                            const float* __restrict__ mask_label, long B, int T,
                                                            float* __restrict__ dlogits, float* __restrict__ prediction,
                                                            float* __restrict__ stats) {
  __shared__ float red[3][kBlock];
  const int t = blockIdx.x;
  float v[3] = {0.f, 0.f, 0.f};                // cost, correct, count
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
      v[0] += fmaxf(u, 0.f) + log1pf(e);
      v[1] += ((d > 0.f) == pos) ? 1.f : 0.f;
      v[2] += 1.f;
      g = p1 - (pos ? 1.f : 0.f);
    }
    dlogits[i1] = g;
    dlogits[i0] = -g;
  }
  block_sum(v, red);
  if (threadIdx.x == 0) {
    stats[t] = v[0];
    stats[T + t] = v[1];
    stats[2 * T + t] = v[2];
  }
}

// the kernel behind it: task_loss_finish_kernel<3, false> (block_reduce.h)

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
  hipLaunchKernelGGL((task_loss_finish_kernel<3, false>), dim3(1), dim3(kBlock), 0, s, stats, (long)batch, (int)tasks, accum);
  return check_launch(who);
}
