// Regression head (example_model/model_multimodal_regression.py:92-101; gcn.py:204-208): the masked squared error with its
// gradient and per-task sums, and the sums behind r2 / mse / gmfe of an evaluated set.
//
//   loss      = mask_label (labels - pred)^2                     [B, T]
//   cost_sum  = sum loss            (metrics["error_sum"], :97, :100)
//   cost_opt  = cost_sum / (B T)    (reduce_mean over the PADDED batch, :96)
//   error_sum [T], count [T] = sum_b mask_label                  (per task; their totals are the file's metrics)
//   dpred     = d cost_sum / d pred = -2 mask_label (labels - pred)
//
// A task-column head, like the softmax2 head of cvloss.hip: one workgroup per task sums its column over the rows in a fixed
// order (thread-strided partials, one block_sum), the shared finish kernel of block_reduce.h behind it adds the tasks and, when
// the call carries an accumulator block [2 T + 1] = error_sum | count | cost_sum, adds the batch's values into it in place (an
// epoch is read back once).  No float atomics.
//
// kgcn_regression_sums_f64: per task over n rows, two passes in fp64 inside one workgroup (pass 1: n, sum y; pass 2 around the
// mean: sum (y - mean)^2, sum (y - p)^2, sum log(y / p) over the rows whose ratio is positive and finite, the count of the
// others), thread-strided partials and one tree: fixed order, no atomics.
#include "block_reduce.h"
#include "kgcn_common.h"

namespace kgcn {
namespace {

constexpr int kBlock = 256;

// stats [2 T + 3] = error_sum [T] | count [T] | cost_sum | cost_opt | spare; this kernel writes the first 2 T
__global__ __launch_bounds__(kBlock) void sqerr_kernel(const float* __restrict__ pred, const float* __restrict__ labels,
                                                      const float* __restrict__ mask_label, long B, int T,
                                                      float* __restrict__ dpred, float* __restrict__ stats) {
  __shared__ float red[2][kBlock];
  const int t = blockIdx.x;
  float v[2] = {0.f, 0.f};
  for (long b = threadIdx.x; b < B; b += kBlock) {
    const long i = b * T + t;
    const float m = mask_label[i];
    const float d = labels[i] - pred[i];
    // a row that does not count contributes exactly 0 to loss and gradient, whatever its prediction holds (0 * inf is NaN)
    const bool used = m != 0.f;
    v[0] += used ? m * d * d : 0.f;
    v[1] += m;
    dpred[i] = used ? -2.0f * m * d : 0.f;
  }
  block_sum(v, red);
  if (threadIdx.x == 0) {
    stats[t] = v[0];
    stats[T + t] = v[1];
  }
}

// the kernel behind it: task_loss_finish_kernel<2, true> (block_reduce.h)

// out [T, 6] = n | sum y | sum (y - mean)^2 | sum (y - p)^2 | sum log(y / p) | rows with y / p <= 0 or not finite
__global__ __launch_bounds__(kBlock) void regression_sums_kernel(const float* __restrict__ pred, long pred_ld,
                                                                const float* __restrict__ label, long label_ld,
                                                                const float* __restrict__ mask, long n, int T,
                                                                double* __restrict__ out) {
  __shared__ double red[4][kBlock];
  const int t = blockIdx.x;
  double a[2] = {0.0, 0.0};
  for (long i = threadIdx.x; i < n; i += kBlock) {
    if (mask && mask[i * T + t] == 0.f) continue;
    a[0] += 1.0;
    a[1] += (double)label[i * label_ld + t];
  }
  block_sum(a, red);
  const double mean = a[0] > 0.0 ? a[1] / a[0] : 0.0;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (long i = threadIdx.x; i < n; i += kBlock) {
    if (mask && mask[i * T + t] == 0.f) continue;
    const double y = (double)label[i * label_ld + t], p = (double)pred[i * pred_ld + t];
    v[0] += (y - mean) * (y - mean);
    v[1] += (y - p) * (y - p);
    const double q = y / p;
    if (q > 0.0 && q < __builtin_huge_val()) {
      v[2] += log(q);
    } else {
      v[3] += 1.0;
    }
  }
  block_sum(v, red);
  if (threadIdx.x == 0) {
    double* o = out + 6l * t;
    o[0] = a[0]; o[1] = a[1]; o[2] = v[0]; o[3] = v[1]; o[4] = v[2]; o[5] = v[3];
  }
}

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int kgcn_masked_sqerr_f32(const float* pred, const float* labels, const float* mask_label, int64_t batch, int32_t tasks,
                                     float* dpred, float* stats, float* accum, void* stream) {
  const char* who = "kgcn_masked_sqerr_f32";
  if (batch < 1 || batch > KGCN_SQERR_MAX_BATCH) return fail("%s: batch %lld outside 1..%d", who, (long long)batch, KGCN_SQERR_MAX_BATCH);
  if (tasks < 1 || tasks > KGCN_SQERR_MAX_TASKS) return fail("%s: %d tasks outside 1..%d", who, tasks, KGCN_SQERR_MAX_TASKS);
  if (!pred || !labels || !mask_label || !dpred || !stats) return fail("%s: NULL operand", who);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(sqerr_kernel, dim3((unsigned)tasks), dim3(kBlock), 0, s, pred, labels, mask_label, (long)batch, (int)tasks, dpred,
                     stats);
  hipLaunchKernelGGL((task_loss_finish_kernel<2, true>), dim3(1), dim3(kBlock), 0, s, stats, (long)batch, (int)tasks, accum);
  return check_launch(who);
}

extern "C" int kgcn_regression_sums_f64(const float* pred, int64_t pred_ld, const float* label, int64_t label_ld, const float* mask,
                                        int64_t n, int32_t tasks, double* sums, void* stream) {
  const char* who = "kgcn_regression_sums_f64";
  if (n < 1 || n > KGCN_REGRESSION_SUMS_MAX_ROWS) return fail("%s: %lld rows outside 1..2^31", who, (long long)n);
  if (tasks < 1 || tasks > KGCN_SQERR_MAX_TASKS) return fail("%s: %d tasks outside 1..%d", who, tasks, KGCN_SQERR_MAX_TASKS);
  if (!pred || !label || !sums) return fail("%s: NULL operand", who);
  if (pred_ld < tasks || label_ld < tasks) return fail("%s: row stride below %d tasks", who, tasks);
  hipLaunchKernelGGL(regression_sums_kernel, dim3((unsigned)tasks), dim3(kBlock), 0, as_stream(stream), pred, (long)pred_ld, label,
                     (long)label_ld, mask, (long)n, (int)tasks, sums);
  return check_launch(who);
}
