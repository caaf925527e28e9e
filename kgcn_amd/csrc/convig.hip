// Integrated gradients of the protein-sequence CNN (kgcn visualize on sample_protein/sequence/cnn.py; kgcn/visualization.py:187-260):
// the two sweeps over the K scaled copies of the model's FIRST layer, Conv1D(F, 4, same, relu) -> MaxPooling1D(4).
//
//   Copy k of protein c feeds alpha_k e_c, so its pre-activation is alpha_k P + b with P = conv(e_c) WITHOUT the bias, and because
//   p -> relu(fl(fl(alpha p) + b)) is non-decreasing for alpha >= 0 the window maximum commutes with it: with Pm = maxpool(P)
//   formed ONCE per protein (kgcn_conv1d_pool_fwd_f32, zero bias, KGCN_ACT_NONE),
//     expand   out[c K + k, t, f] = max(0, fl(fl(alpha_k Pm[c, t, f]) + b_f))                       conv1d_ig_expand_kernel
//   replaces K convolutions by K element-wise sweeps.  conv is linear, so the weighted sum over the copies of the input gradients
//   is conv^T of the weighted sum of the pre-activation gradients:
//     reduce   r[c, t, f] = sum_k w_k dout[c K + k, t, f] [out[c K + k, t, f] > 0]                  conv1d_ig_reduce_kernel
//   followed by ONE kgcn_conv1d_pool_bwd_f32 (KGCN_ACT_NONE, dout = r, the arg-max of the Pm pass) replaces K of them.
//
//   Arithmetic, fp32, nothing contracted (this file is built with -ffp-contract=off; numpy restates both kernels bit for bit):
//     expand   v = fl(fl(alpha_k * p) + b_f);  out = v > 0 ? v : +0
//     reduce   acc = +0;  for k = 0, 1, ..: if w_k != 0 and out_k > 0: acc = fl(acc + fl(w_k * dout_k))
//   A copy of weight 0 is neither read nor added: its loads are redirected to the first copy of non-zero weight and dropped by a
//   select (no branch between the loads of a batch).  No atomics, no workgroup-level sum: bitwise reproducible, and a protein's
//   rows do not depend on which other proteins the launch holds.
//
//   Both are bandwidth-bound streams over the n = T F contiguous floats of a (protein, copy) row.  A thread owns ONE group of 4
//   consecutive floats of that row (consecutive lanes, consecutive groups) and walks copies; the accesses are 16 bytes wide and
//   4-byte aligned -- F = 505 and n are no multiples of 4, so a row starts at any float -- which gfx950 serves as one dwordx4
//   access.  The last group of a row holds n mod 4 floats and is read and written float by float: nothing is touched past a row.
#include "kgcn_common.h"

namespace kgcn {

namespace {
constexpr int kThreads = 256;
constexpr int kExpandCopies = 8;       // copies a thread writes (grid.y walks the rest)
constexpr int kReduceBatch = 8;        // copies whose loads are in flight together

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef f32x4 f32x4u __attribute__((aligned(4)));      // 16 bytes wide, 4-byte aligned

// n floats at p: a whole group as one access, the ragged last group float by float
__device__ __forceinline__ f32x4 load_group(const float* p, int n) {
  if (n == 4) return *reinterpret_cast<const f32x4u*>(p);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < n; ++j) v[j] = p[j];
  return v;
}
__device__ __forceinline__ void store_group(float* p, int n, f32x4 v) {
  if (n == 4) {
    *reinterpret_cast<f32x4u*>(p) = v;
    return;
  }
  for (int j = 0; j < n; ++j) p[j] = v[j];
}

// thread = (protein c, group g of the row); blockIdx.y = chunk of kExpandCopies copies
__global__ __launch_bounds__(kThreads) void conv1d_ig_expand_kernel(const float* __restrict__ Pm, const float* __restrict__ alpha,
                                                                    const float* __restrict__ bias, float* __restrict__ out, long C,
                                                                    int K, long n, int F, long groups) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= C * groups) return;
  const long c = i / groups, i0 = (i - c * groups) * 4;
  const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
  const f32x4 p = load_group(Pm + c * n + i0, cnt);
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  int f = (int)(i0 % F);
  for (int j = 0; j < cnt; ++j) {
    b[j] = bias[f];
    f = f + 1 == F ? 0 : f + 1;
  }
  const int k0 = blockIdx.y * kExpandCopies, k1 = k0 + kExpandCopies < K ? k0 + kExpandCopies : K;
  for (int k = k0; k < k1; ++k) {
    const float a = alpha[k];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = a * p[j] + b[j];                  // two roundings: the file is built without contraction
      o[j] = v > 0.f ? v : 0.f;
    }
    store_group(out + (c * K + k) * n + i0, cnt, o);
  }
}

// thread = (protein c, group g of the row): the K copies in order
__global__ __launch_bounds__(kThreads) void conv1d_ig_reduce_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                                    const float* __restrict__ w, float* __restrict__ r, long C, int K,
                                                                    long n, long groups) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= C * groups) return;
  const long c = i / groups, i0 = (i - c * groups) * 4;
  const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int knz = 0;                                          // the first copy of non-zero weight: where a weight-0 copy's loads go
  while (knz < K && w[knz] == 0.f) ++knz;
  if (knz < K) {
    const float* dy = dout + c * K * n + i0;
    const float* y = out + c * K * n + i0;
    for (int k0 = 0; k0 < K; k0 += kReduceBatch) {
      float wk[kReduceBatch];
      f32x4 g[kReduceBatch], a[kReduceBatch];
#pragma unroll
      for (int u = 0; u < kReduceBatch; ++u) {          // the loads of a batch first, no branch between them
        const float wv = k0 + u < K ? w[k0 + u] : 0.f;
        const int k = wv != 0.f ? k0 + u : knz;
        wk[u] = wv;
        g[u] = load_group(dy + (long)k * n, cnt);
        a[u] = load_group(y + (long)k * n, cnt);
      }
#pragma unroll
      for (int u = 0; u < kReduceBatch; ++u) {          // ... then their terms, k ascending
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float t = acc[j] + wk[u] * g[u][j];
          acc[j] = (wk[u] != 0.f && a[u][j] > 0.f) ? t : acc[j];
        }
      }
    }
  }
  store_group(r + c * n + i0, cnt, acc);
}

int ig_check(const char* who, int64_t proteins, int32_t copies, int32_t positions, int32_t filters, long* groups, unsigned* grid) {
  if (proteins < 0) return fail("%s: %lld proteins", who, (long long)proteins);
  if (copies < 1 || copies > KGCN_CONV1D_IG_MAX_COPIES) return fail("%s: K = %d copies outside 1..%d", who, copies, KGCN_CONV1D_IG_MAX_COPIES);
  if (positions < 1 || positions > KGCN_CONV1D_MAX_LENGTH)
    return fail("%s: %d pooled positions outside 1..%d", who, positions, KGCN_CONV1D_MAX_LENGTH);
  if (filters < 1 || filters > KGCN_CONV1D_MAX_CHANNELS) return fail("%s: %d filters outside 1..%d", who, filters, KGCN_CONV1D_MAX_CHANNELS);
  if (proteins * (int64_t)copies >= (int64_t)INT32_MAX)
    return fail("%s: %lld proteins x %d copies: too many rows, pass fewer proteins", who, (long long)proteins, copies);
  *groups = ((long)positions * filters + 3) / 4;
  const int64_t blocks = (proteins * *groups + kThreads - 1) / kThreads;
  if (blocks >= (int64_t)INT32_MAX) return fail("%s: %lld workgroups exceed one launch's grid: pass fewer proteins", who, (long long)blocks);
  *grid = (unsigned)blocks;
  return 0;
}
}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int kgcn_ig_conv1d_expand_f32(const float* Pm, int64_t proteins, int32_t copies, int32_t positions, int32_t filters,
                                         const float* alpha, const float* bias, float* out, void* stream) {
  const char* who = "kgcn_ig_conv1d_expand_f32";
  long groups;
  unsigned grid;
  if (int rc = ig_check(who, proteins, copies, positions, filters, &groups, &grid)) return rc;
  if (proteins == 0) return 0;
  if (!Pm || !alpha || !bias || !out) return fail("%s: NULL operand", who);
  hipLaunchKernelGGL(conv1d_ig_expand_kernel, dim3(grid, (unsigned)((copies + kExpandCopies - 1) / kExpandCopies)), dim3(kThreads), 0,
                     as_stream(stream), Pm, alpha, bias, out, (long)proteins, (int)copies, (long)positions * filters, (int)filters, groups);
  return check_launch(who);
}

extern "C" int kgcn_ig_conv1d_reduce_f32(const float* dout, const float* out, int64_t proteins, int32_t copies, int32_t positions,
                                         int32_t filters, const float* w, float* r, void* stream) {
  const char* who = "kgcn_ig_conv1d_reduce_f32";
  long groups;
  unsigned grid;
  if (int rc = ig_check(who, proteins, copies, positions, filters, &groups, &grid)) return rc;
  if (proteins == 0) return 0;
  if (!dout || !out || !w || !r) return fail("%s: NULL operand", who);
  hipLaunchKernelGGL(conv1d_ig_reduce_kernel, dim3(grid), dim3(kThreads), 0, as_stream(stream), dout, out, w, r, (long)proteins,
                     (int)copies, (long)positions * filters, groups);
  return check_launch(who);
}
