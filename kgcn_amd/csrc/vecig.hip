// Integrated gradients over the per-graph vector of the vector-modality models (kgcn visualize on
// example_model/model_multimodal_vec.py / model_multimodal_regression.py; kgcn/visualization.py:187-260, kgcn/feed.py:201-206):
// the two sweeps over the scaled copies of the vector tower's FIRST layer, Dense(Dv -> H) + BatchNormalization + activation.
//
//   Clean copy k of compound c feeds alpha_k v_c, so its first-layer pre-activation is alpha_k (v_c W) + b: with P = v W formed
//   ONCE per compound by the caller,
//     expand   Y[c K + k, :] = act(bn(alpha_k P[c, :] + b))                                ig_copies_expand_kernel
//   replaces K GEMM rows of Dv products each by K element-wise rows.  The gradient with respect to the fed vector is linear in
//   the gradient of the pre-activation, d score / d v_k = dpre_k W^T, for clean and noisy copies alike, so
//     reduce   S[c, :] = scale (.) sum_k w_k dY[c K + k, :] (.) act'(Y[c K + k, :])          ig_copies_reduce_kernel
//   followed by ONE [C, H] x W^T product of the caller replaces K of them.
//
//   Arithmetic, fp32: pre = fma(alpha, P, b) (alpha = 1: P + b rounded once, the dense layer's own bias add), then the
//   GraphBatchNormalization apply pass of bn.hip word for word -- (pre - mean) * (1 / sqrt(var + eps)) * gamma + beta -- and
//   act_fwd: given the same P, a scale-1 copy IS the composed dense -> graph_bn layer, bit for bit.  The reduce sums k = 0, 1, ...
//   in that order in one register per element (acc = fma(w_k, dY act'(Y), acc)), skips a copy of weight 0 (a select: whatever
//   its rows hold never reaches the sum), and multiplies by `scale` once at the end.  No atomics, no workgroup-level sum: the
//   results are bitwise reproducible and a compound's rows do not depend on which other compounds the launch holds.
//
//   Both are bandwidth-bound sweeps: a thread owns ONE column group (4 floats, 16-byte accesses, when every row start is 16-byte
//   aligned; 1 float otherwise -- H and the row strides carry no alignment promise) and walks copies, so the per-column constants
//   are loaded and the square root is taken once per thread, not once per element; the lanes of a row read / write consecutive
//   addresses.  Y and dY are touched once.
#include "kgcn_common.h"

namespace kgcn {

namespace {
constexpr int kThreads = 256;
constexpr int kCopiesPerThread = 8;                   // expand: copies a thread writes
constexpr int kReduceUnroll = 16;                     // reduce: copies whose loads are in flight together

template <int V>
struct Vec {
  typedef float type __attribute__((ext_vector_type(V)));
};
template <>
struct Vec<1> {
  typedef float type;
};
template <int V>
__device__ __forceinline__ float& lane_of(typename Vec<V>::type& v, int j) {
  if constexpr (V == 1) {
    return v;
  } else {
    return reinterpret_cast<float*>(&v)[j];
  }
}

// block = (compound, chunk of rpp * kCopiesPerThread copies, block of up to 256 column groups); thread = (copy sub-index, group)
template <int V, bool BN>
__global__ __launch_bounds__(kThreads) void ig_copies_expand_kernel(const float* __restrict__ P, const float* __restrict__ alpha,
                                                                    const float* __restrict__ bias, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, const float* __restrict__ mean,
                                                                    const float* __restrict__ var, float eps, int act,
                                                                    float* __restrict__ Y, long y_ld, int K, int H, int gpb, int rpp,
                                                                    int kchunks, int cblocks) {
  typedef typename Vec<V>::type fv;
  long b = blockIdx.x;
  const int cb = (int)(b % cblocks);
  b /= cblocks;
  const int kc = (int)(b % kchunks);
  const long c = b / kchunks;
  const int ksub = (int)threadIdx.x / gpb;
  const int col = (cb * gpb + (int)threadIdx.x % gpb) * V;
  if (ksub >= rpp || col >= H) return;                // (H is a multiple of V on the vector route: a group is whole or absent)
  float p[V], bv[V], mu[V], rs[V], ga[V], be[V];
  fv pv = *reinterpret_cast<const fv*>(P + c * H + col);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    p[j] = lane_of<V>(pv, j);
    bv[j] = bias ? bias[col + j] : 0.f;
    if constexpr (BN) {
      mu[j] = mean[col + j];
      rs[j] = 1.0f / __builtin_sqrtf(var[col + j] + eps);
      ga[j] = gamma[col + j];
      be[j] = beta[col + j];
    }
  }
  const int k0 = kc * rpp * kCopiesPerThread + ksub;
#pragma unroll
  for (int i = 0; i < kCopiesPerThread; ++i) {
    const int k = k0 + i * rpp;
    if (k >= K) break;
    const float a = alpha[k];
    fv o;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float v = fmaf(a, p[j], bv[j]);
      if constexpr (BN) v = (v - mu[j]) * rs[j] * ga[j] + be[j];
      lane_of<V>(o, j) = act_fwd(v, act);
    }
    *reinterpret_cast<fv*>(Y + (c * K + k) * y_ld + col) = o;
  }
}

// thread = (compound, column group): the K copies in order
template <int V>
__global__ __launch_bounds__(kThreads) void ig_copies_reduce_kernel(const float* __restrict__ dY, long dy_ld, const float* __restrict__ Y,
                                                                    long y_ld, const float* __restrict__ w,
                                                                    const float* __restrict__ scale, int act, float* __restrict__ S,
                                                                    long C, int K, int H) {
  typedef typename Vec<V>::type fv;
  const int hv = H / V;
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= C * hv) return;
  const long c = i / hv;
  const int col = (int)(i - c * hv) * V;
  const float* dy = dY + c * K * dy_ld + col;
  const float* y = Y + c * K * y_ld + col;
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  for (int k0 = 0; k0 < K; k0 += kReduceUnroll) {
    float wk[kReduceUnroll];
    fv g[kReduceUnroll], a[kReduceUnroll];
    // The loads of kReduceUnroll copies first, WITHOUT a branch between them (a branch on every w[k] made each pair of loads
    // wait for the pair before it: one memory latency per copy).  A copy past the end repeats row K - 1 with weight 0.
#pragma unroll
    for (int u = 0; u < kReduceUnroll; ++u) {
      const int k = k0 + u < K ? k0 + u : K - 1;
      const float wv = w[k];
      wk[u] = k0 + u < K ? wv : 0.f;
      g[u] = *reinterpret_cast<const fv*>(dy + (long)k * dy_ld);
      a[u] = *reinterpret_cast<const fv*>(y + (long)k * y_ld);
    }
    // ... then their terms, in the order of k.  A copy of weight 0 is skipped by a select: whatever its rows hold (NaN
    // included) never reaches the sum, and the sum keeps its bits.
#pragma unroll
    for (int u = 0; u < kReduceUnroll; ++u) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float t = fmaf(wk[u], lane_of<V>(g[u], j) * act_dout(lane_of<V>(a[u], j), act), acc[j]);
        acc[j] = wk[u] != 0.f ? t : acc[j];
      }
    }
  }
  fv o;
#pragma unroll
  for (int j = 0; j < V; ++j) lane_of<V>(o, j) = scale ? acc[j] * scale[col + j] : acc[j];
  *reinterpret_cast<fv*>(S + c * H + col) = o;
}

int check_shape(const char* who, int64_t compounds, int32_t copies, int32_t width, int32_t act) {
  if (compounds < 0) return fail("%s: %lld compounds", who, (long long)compounds);
  if (width < 1 || width > KGCN_IG_COPIES_MAX_WIDTH) return fail("%s: H = %d outside 1..%d", who, width, KGCN_IG_COPIES_MAX_WIDTH);
  if (copies < 1 || copies > KGCN_IG_COPIES_MAX_COPIES) return fail("%s: K = %d copies outside 1..%d", who, copies, KGCN_IG_COPIES_MAX_COPIES);
  if (compounds * (int64_t)copies > KGCN_IG_COPIES_MAX_ROWS)
    return fail("%s: %lld compounds x %d copies exceed %lld rows: pass fewer compounds", who, (long long)compounds, copies,
                (long long)KGCN_IG_COPIES_MAX_ROWS);
  if (act != KGCN_ACT_NONE && act != KGCN_ACT_SIGMOID && act != KGCN_ACT_RELU && act != KGCN_ACT_TANH)
    return fail("%s: unknown activation code %d", who, act);
  return 0;
}

// every row of a [rows, H] block with row stride ld starts on a 16-byte boundary and holds whole 4-float groups
bool rows_vec4(const void* p, int64_t ld, int32_t H) { return aligned16(p) && (ld & 3) == 0 && (H & 3) == 0; }

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int kgcn_ig_copies_expand_f32(const float* P, int64_t compounds, int32_t copies, int32_t width, const float* alpha,
                                         const float* bias, const float* gamma, const float* beta, const float* mean, const float* var,
                                         float eps, int32_t act, float* Y, int64_t y_ld, void* stream) {
  const char* who = "kgcn_ig_copies_expand_f32";
  if (int rc = check_shape(who, compounds, copies, width, act)) return rc;
  if (y_ld < width) return fail("%s: row stride %lld below the row width %d", who, (long long)y_ld, width);
  const bool bn = gamma != nullptr;
  if ((beta != nullptr) != bn || (mean != nullptr) != bn || (var != nullptr) != bn)
    return fail("%s: gamma, beta, mean and var come together or not at all", who);
  if (compounds == 0) return 0;
  if (!P || !alpha || !Y) return fail("%s: NULL operand", who);
  const bool vec = rows_vec4(P, width, width) && rows_vec4(Y, y_ld, width);
  const int groups = vec ? width / 4 : width;
  const int gpb = groups < kThreads ? groups : kThreads;               // column groups a block covers
  const int rpp = kThreads / gpb;                                      // copies a block writes side by side
  const int cblocks = (groups + gpb - 1) / gpb;
  const int per = rpp * kCopiesPerThread;
  const int kchunks = (copies + per - 1) / per;
  const int64_t grid = compounds * kchunks * cblocks;
  if (grid >= INT32_MAX) return fail("%s: %lld workgroups exceed one launch's grid: pass fewer compounds", who, (long long)grid);
  hipStream_t s = as_stream(stream);
#define KGCN_EXPAND(V, BN)                                                                                                          \
  hipLaunchKernelGGL((ig_copies_expand_kernel<V, BN>), dim3((unsigned)grid), dim3(kThreads), 0, s, P, alpha, bias, gamma, beta, mean, \
                     var, eps, (int)act, Y, (long)y_ld, (int)copies, (int)width, gpb, rpp, kchunks, cblocks)
  if (vec && bn) KGCN_EXPAND(4, true);
  else if (vec) KGCN_EXPAND(4, false);
  else if (bn) KGCN_EXPAND(1, true);
  else KGCN_EXPAND(1, false);
#undef KGCN_EXPAND
  return check_launch(who);
}

extern "C" int kgcn_ig_copies_reduce_f32(const float* dY, int64_t dy_ld, const float* Y, int64_t y_ld, int64_t compounds, int32_t copies,
                                         int32_t width, const float* w, const float* scale, int32_t act, float* S, void* stream) {
  const char* who = "kgcn_ig_copies_reduce_f32";
  if (int rc = check_shape(who, compounds, copies, width, act)) return rc;
  if (dy_ld < width || y_ld < width)
    return fail("%s: row strides %lld / %lld below the row width %d", who, (long long)dy_ld, (long long)y_ld, width);
  if (compounds == 0) return 0;
  if (!dY || !Y || !w || !S) return fail("%s: NULL operand", who);
  const bool vec = rows_vec4(dY, dy_ld, width) && rows_vec4(Y, y_ld, width) && rows_vec4(S, width, width);
  const int64_t threads = compounds * (vec ? width / 4 : width);
  const int64_t grid = (threads + kThreads - 1) / kThreads;
  if (grid >= INT32_MAX) return fail("%s: %lld workgroups exceed one launch's grid: pass fewer compounds", who, (long long)grid);
  hipStream_t s = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(ig_copies_reduce_kernel<4>, dim3((unsigned)grid), dim3(kThreads), 0, s, dY, (long)dy_ld, Y, (long)y_ld, w, scale,
                       (int)act, S, (long)compounds, (int)copies, (int)width);
  else
    hipLaunchKernelGGL(ig_copies_reduce_kernel<1>, dim3((unsigned)grid), dim3(kThreads), 0, s, dY, (long)dy_ld, Y, (long)y_ld, w, scale,
                       (int)act, S, (long)compounds, (int)copies, (int)width);
  return check_launch(who);
}
