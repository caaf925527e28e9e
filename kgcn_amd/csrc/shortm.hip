// Dense + BatchNormalization (learning phase 0) + activation for SHORT batches: the vector towers of
// example_model/model_multimodal_vec.py:84-108 and model_multimodal_regression.py:84-90 at the samples' batch sizes.
//
//   pre = x W + b,   y = act(s (pre - mean) + beta),   s = gamma / sqrt(var + eps)        (gamma == NULL: y = act(pre))
//
// With at most a few hundred rows the whole batch fits one workgroup, so a workgroup owns a SLAB of kSlab output columns and
// EVERY row: the forward is one launch (x is re-read from cache by each slab owner, W is read once overall), and the backward is
// one launch in which the slab owner holds complete sums -- dW [K, slab], dbias, dgamma, dbeta -- with no partials and no second
// stage (the short-M twin of skinny.hip's narrow-N kernels).  dX sums over the slabs: a second launch of the forward's
// contraction with W read transposed, over the d pre the backward wrote.  Plain fp32 FMAs, every sum in one fixed order (a thread
// adds its terms ascending, one thread adds the row groups' partials ascending): no float atomics, two runs agree bit for bit.
// Scalar loads only: no alignment or multiple-of-4 requirement on K, N, the row strides or out_col (profeat is 70 wide,
// dragon 37).
#include "kgcn_common.h"

namespace kgcn {
namespace {

constexpr int kThreads = 256;
constexpr int kSlab = 16;                       // output columns of one workgroup
constexpr int kGroups = kThreads / kSlab;       // row groups: thread (r, c) owns rows r, r + 16, ... of column c
constexpr int kChunk = 32;                      // contraction steps staged in LDS at a time

struct BnArgs {
  const float* bias;
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* var;
  float eps;
  int act;
};

// out[b, j] = sum_t a[b, t] Wm(t, j) for all rows b < rows and the slab's columns j < width, t ascending.
//   TRANS = false: Wm(t, j) = w[t * w_ld + j]   (forward: t over K, j over N)
//   TRANS = true:  Wm(t, j) = w[j * w_ld + t]   (dX: t over N, j over K)
//   EPI: the bias / BN / activation epilogue, pre-activations to `stash` [rows, width] when given
template <int RT, bool TRANS, bool EPI>
__global__ __launch_bounds__(kThreads) void shortm_gemm_kernel(const float* __restrict__ a, long a_ld, int rows, int depth,
                                                               const float* __restrict__ w, int w_ld, int width, BnArgs bn,
                                                               float* __restrict__ out, long out_ld, float* __restrict__ stash) {
  __shared__ float As[RT * kGroups][kChunk + 1];
  __shared__ float Ws[kChunk][kSlab + 1];
  const int tid = threadIdx.x, r = tid / kSlab, c = tid % kSlab;
  const int j0 = blockIdx.x * kSlab;
  float acc[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) acc[i] = 0.f;
  for (int t0 = 0; t0 < depth; t0 += kChunk) {
    for (int idx = tid; idx < RT * kGroups * kChunk; idx += kThreads) {
      const int b = idx / kChunk, kk = idx % kChunk;
      As[b][kk] = (b < rows && t0 + kk < depth) ? a[(long)b * a_ld + t0 + kk] : 0.f;
    }
    for (int idx = tid; idx < kChunk * kSlab; idx += kThreads) {
      int kk, cc;
      if (TRANS) { cc = idx / kChunk; kk = idx % kChunk; } else { kk = idx / kSlab; cc = idx % kSlab; }
      const bool in = t0 + kk < depth && j0 + cc < width;
      const long at = TRANS ? (long)(j0 + cc) * w_ld + t0 + kk : (long)(t0 + kk) * w_ld + j0 + cc;
      Ws[kk][cc] = in ? w[at] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < kChunk; ++kk) {
      const float wv = Ws[kk][c];
#pragma unroll
      for (int i = 0; i < RT; ++i) acc[i] = fmaf(As[r + kGroups * i][kk], wv, acc[i]);
    }
    __syncthreads();
  }
  const int j = j0 + c;
  if (j >= width) return;
  float bj = 0.f, s = 1.f, m = 0.f, be = 0.f;
  if (EPI) {
    bj = bn.bias ? bn.bias[j] : 0.f;
    if (bn.gamma) {
      s = bn.gamma[j] / sqrtf(bn.var[j] + bn.eps);
      m = bn.mean[j];
      be = bn.beta[j];
    }
  }
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const int b = r + kGroups * i;
    if (b >= rows) continue;
    float v = acc[i];
    if (EPI) {
      v += bj;
      if (stash) stash[(long)b * width + j] = v;
      if (bn.gamma) v = fmaf(s, v - m, be);
      v = act_fwd(v, bn.act);
    }
    out[(long)b * out_ld + j] = v;
  }
}

// One launch: d pre [rows, N] (into LDS and, when asked, into `dpre` for the dX launch), dbias, dgamma, dbeta and dW [K, slab].
//   dz = dy act'(y);  dbeta = sum_b dz;  dgamma = sum_b dz (pre - mean) / sqrt(var + eps);  d pre = s dz;  dbias = sum_b d pre
//   dW[k, j] = sum_b x[b, k] d pre[b, j], b ascending
template <int RT>
__global__ __launch_bounds__(kThreads) void shortm_bwd_kernel(const float* __restrict__ x, long x_ld, int rows, int K, int N,
                                                              const float* __restrict__ y, long y_ld, const float* __restrict__ dy,
                                                              long dy_ld, const float* __restrict__ pre, BnArgs bn,
                                                              float* __restrict__ dw, float* __restrict__ dbias,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              float* __restrict__ dpre) {
  __shared__ float Dz[RT * kGroups][kSlab + 1];
  __shared__ float Xs[RT * kGroups][kChunk + 1];
  __shared__ float red[2][kGroups][kSlab];
  const int tid = threadIdx.x, r = tid / kSlab, c = tid % kSlab;
  const int j0 = blockIdx.x * kSlab, j = j0 + c;
  const bool col = j < N;
  float s = 1.f, rstd = 0.f, m = 0.f;
  if (col && bn.gamma) {
    rstd = 1.0f / sqrtf(bn.var[j] + bn.eps);
    s = bn.gamma[j] * rstd;
    m = bn.mean[j];
  }
  float sb = 0.f, sg = 0.f;
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const int b = r + kGroups * i;
    float dp = 0.f;
    if (col && b < rows) {
      const float dz = dy[(long)b * dy_ld + j] * act_dout(y[(long)b * y_ld + j], bn.act);
      sb += dz;
      if (bn.gamma) sg = fmaf(dz, (pre[(long)b * N + j] - m) * rstd, sg);
      dp = dz * s;
      if (dpre) dpre[(long)b * N + j] = dp;
    }
    Dz[b][c] = dp;
  }
  red[0][r][c] = sb;
  red[1][r][c] = sg;
  __syncthreads();
  if (r == 0 && col) {
    float tb = 0.f, tg = 0.f;
#pragma unroll
    for (int q = 0; q < kGroups; ++q) {
      tb += red[0][q][c];
      tg += red[1][q][c];
    }
    if (dbias) dbias[j] = s * tb;
    if (dbeta) dbeta[j] = tb;
    if (dgamma) dgamma[j] = tg;
  }
  if (!dw) return;
  // here thread (r, c) owns the contraction steps k0 + r and k0 + r + 16 of column c
  for (int k0 = 0; k0 < K; k0 += kChunk) {
    for (int idx = tid; idx < RT * kGroups * kChunk; idx += kThreads) {
      const int b = idx / kChunk, kk = idx % kChunk;
      Xs[b][kk] = (b < rows && k0 + kk < K) ? x[(long)b * x_ld + k0 + kk] : 0.f;
    }
    __syncthreads();
    float a0 = 0.f, a1 = 0.f;
    for (int b = 0; b < rows; ++b) {
      const float d = Dz[b][c];
      a0 = fmaf(Xs[b][r], d, a0);
      a1 = fmaf(Xs[b][r + kGroups], d, a1);
    }
    if (col) {
      if (k0 + r < K) dw[(long)(k0 + r) * N + j] = a0;
      if (k0 + r + kGroups < K) dw[(long)(k0 + r + kGroups) * N + j] = a1;
    }
    __syncthreads();
  }
}

// y[b, 0:n] = act(x[b, 0:n]) between two strided column blocks (tanh of a read-out into its place in a concatenation)
__global__ __launch_bounds__(kThreads) void act_cols_fwd_kernel(const float* __restrict__ x, long x_ld, long total, int n, int act,
                                                                float* __restrict__ y, long y_ld) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long)gridDim.x * kThreads) {
    const long b = i / n;
    const int j = (int)(i % n);
    y[b * y_ld + j] = act_fwd(x[b * x_ld + j], act);
  }
}
__global__ __launch_bounds__(kThreads) void act_cols_bwd_kernel(const float* __restrict__ y, long y_ld, const float* __restrict__ g,
                                                                long g_ld, long total, int n, int act, float* __restrict__ dx,
                                                                long dx_ld) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long)gridDim.x * kThreads) {
    const long b = i / n;
    const int j = (int)(i % n);
    dx[b * dx_ld + j] = g[b * g_ld + j] * act_dout(y[b * y_ld + j], act);
  }
}

bool shape_ok(int64_t rows, int64_t k, int64_t n) {
  return rows >= 1 && rows <= KGCN_DENSE_BN_SHORT_MAX_ROWS && k >= 1 && k <= KGCN_DENSE_BN_SHORT_MAX_K && n >= 1 &&
         n <= KGCN_DENSE_BN_SHORT_MAX_N;
}
int check_shape(const char* who, int64_t rows, int64_t k, int64_t n) {
  if (!shape_ok(rows, k, n))
    return fail("%s: %lld rows, %lld -> %lld outside 1..%d rows, 1..%d inputs, 1..%d outputs", who, (long long)rows, (long long)k,
                (long long)n, KGCN_DENSE_BN_SHORT_MAX_ROWS, KGCN_DENSE_BN_SHORT_MAX_K, KGCN_DENSE_BN_SHORT_MAX_N);
  return 0;
}
int check_act(const char* who, int act) {
  if (act != KGCN_ACT_NONE && act != KGCN_ACT_SIGMOID && act != KGCN_ACT_RELU && act != KGCN_ACT_TANH)
    return fail("%s: unknown activation code %d", who, act);
  return 0;
}

// rows per thread: 4 (up to 64 rows), 8 (128), 16 (256)
#define KGCN_SHORTM_BY_ROWS(rows, CALL) \
  do {                                  \
    if ((rows) <= 4 * kGroups) {        \
      CALL(4);                          \
    } else if ((rows) <= 8 * kGroups) { \
      CALL(8);                          \
    } else {                            \
      CALL(16);                         \
    }                                   \
  } while (0)

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int kgcn_dense_bn_short_supported(int64_t rows, int64_t k, int64_t n) { return shape_ok(rows, k, n) ? 1 : 0; }

extern "C" int kgcn_dense_bn_short_fwd_f32(const float* x, int64_t x_ld, int64_t rows, int32_t k, const float* w, const float* bias,
                                           int32_t n, const float* gamma, const float* beta, const float* mean, const float* var,
                                           float eps, int32_t act, float* y, int64_t y_ld, float* pre, void* stream) {
  const char* who = "kgcn_dense_bn_short_fwd_f32";
  if (int rc = check_shape(who, rows, k, n)) return rc;
  if (int rc = check_act(who, act)) return rc;
  if (!x || !w || !y) return fail("%s: NULL operand", who);
  if (gamma && (!beta || !mean || !var)) return fail("%s: gamma without beta / moving mean / moving variance", who);
  if (!gamma && (beta || mean || var)) return fail("%s: beta / moving statistics without gamma", who);
  if (gamma && !(eps > 0.f)) return fail("%s: eps must be positive, got %g", who, (double)eps);
  if (x_ld < k || y_ld < n) return fail("%s: row stride below the row width (x_ld %lld < %d or y_ld %lld < %d)", who,
                                        (long long)x_ld, k, (long long)y_ld, n);
  const BnArgs bn{bias, gamma, beta, mean, var, eps, act};
  const dim3 grid((unsigned)((n + kSlab - 1) / kSlab));
#define CALL(RT)                                                                                                              \
  hipLaunchKernelGGL((shortm_gemm_kernel<RT, false, true>), grid, dim3(kThreads), 0, as_stream(stream), x, (long)x_ld, (int)rows, \
                     (int)k, w, (int)n, (int)n, bn, y, (long)y_ld, pre)
  KGCN_SHORTM_BY_ROWS(rows, CALL);
#undef CALL
  return check_launch(who);
}

extern "C" int kgcn_dense_bn_short_bwd_f32(const float* x, int64_t x_ld, int64_t rows, int32_t k, int32_t n, const float* y,
                                           int64_t y_ld, const float* dy, int64_t dy_ld, const float* pre, const float* gamma,
                                           const float* mean, const float* var, float eps, int32_t act, float* dw, float* dbias,
                                           float* dgamma, float* dbeta, float* dpre, void* stream) {
  const char* who = "kgcn_dense_bn_short_bwd_f32";
  if (int rc = check_shape(who, rows, k, n)) return rc;
  if (int rc = check_act(who, act)) return rc;
  if (!y || !dy) return fail("%s: NULL operand", who);
  if (dw && !x) return fail("%s: dW needs x", who);
  if (gamma && (!pre || !mean || !var)) return fail("%s: gamma without the stashed pre-activations / moving statistics", who);
  if (!gamma && (dgamma || dbeta)) return fail("%s: dgamma / dbeta without gamma", who);
  if (gamma && !(eps > 0.f)) return fail("%s: eps must be positive, got %g", who, (double)eps);
  if (!dw && !dbias && !dgamma && !dbeta && !dpre) return fail("%s: no output requested", who);
  if ((x && x_ld < k) || y_ld < n || dy_ld < n) return fail("%s: row stride below the row width", who);
  const BnArgs bn{nullptr, gamma, nullptr, mean, var, eps, act};
  const dim3 grid((unsigned)((n + kSlab - 1) / kSlab));
#define CALL(RT)                                                                                                                  \
  hipLaunchKernelGGL((shortm_bwd_kernel<RT>), grid, dim3(kThreads), 0, as_stream(stream), x, (long)x_ld, (int)rows, (int)k, (int)n, y, \
                     (long)y_ld, dy, (long)dy_ld, pre, bn, dw, dbias, dgamma, dbeta, dpre)
  KGCN_SHORTM_BY_ROWS(rows, CALL);
#undef CALL
  return check_launch(who);
}

extern "C" int kgcn_dense_bn_short_dx_f32(const float* dpre, int64_t rows, int32_t n, const float* w, int32_t k, float* dx,
                                          int64_t dx_ld, void* stream) {
  const char* who = "kgcn_dense_bn_short_dx_f32";
  if (int rc = check_shape(who, rows, k, n)) return rc;
  if (!dpre || !w || !dx) return fail("%s: NULL operand", who);
  if (dx_ld < k) return fail("%s: dx_ld %lld below the row width %d", who, (long long)dx_ld, k);
  const BnArgs bn{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, KGCN_ACT_NONE};
  const dim3 grid((unsigned)((k + kSlab - 1) / kSlab));
#define CALL(RT)                                                                                                                \
  hipLaunchKernelGGL((shortm_gemm_kernel<RT, true, false>), grid, dim3(kThreads), 0, as_stream(stream), dpre, (long)n, (int)rows, \
                     (int)n, w, (int)n, (int)k, bn, dx, (long)dx_ld, (float*)nullptr)
  KGCN_SHORTM_BY_ROWS(rows, CALL);
#undef CALL
  return check_launch(who);
}

static int check_cols(const char* who, int64_t rows, int32_t n, int32_t act) {
  if (rows < 1 || n < 1 || rows * (int64_t)n >= (int64_t)INT32_MAX) return fail("%s: %lld x %d elements outside 1..2^31", who, (long long)rows, n);
  return check_act(who, act);
}

extern "C" int kgcn_act_cols_fwd_f32(const float* x, int64_t x_ld, int64_t rows, int32_t n, int32_t act, float* y, int64_t y_ld,
                                     void* stream) {
  const char* who = "kgcn_act_cols_fwd_f32";
  if (int rc = check_cols(who, rows, n, act)) return rc;
  if (!x || !y) return fail("%s: NULL operand", who);
  if (x_ld < n || y_ld < n) return fail("%s: row stride below the row width %d", who, n);
  const long total = (long)rows * n;
  const unsigned blocks = (unsigned)((total + kThreads - 1) / kThreads < 1024 ? (total + kThreads - 1) / kThreads : 1024);
  hipLaunchKernelGGL(act_cols_fwd_kernel, dim3(blocks), dim3(kThreads), 0, as_stream(stream), x, (long)x_ld, total, (int)n, (int)act, y,
                     (long)y_ld);
  return check_launch(who);
}

extern "C" int kgcn_act_cols_bwd_f32(const float* y, int64_t y_ld, const float* g, int64_t g_ld, int64_t rows, int32_t n, int32_t act,
                                     float* dx, int64_t dx_ld, void* stream) {
  const char* who = "kgcn_act_cols_bwd_f32";
  if (int rc = check_cols(who, rows, n, act)) return rc;
  if (!y || !g || !dx) return fail("%s: NULL operand", who);
  if (y_ld < n || g_ld < n || dx_ld < n) return fail("%s: row stride below the row width %d", who, n);
  const long total = (long)rows * n;
  const unsigned blocks = (unsigned)((total + kThreads - 1) / kThreads < 1024 ? (total + kThreads - 1) / kThreads : 1024);
  hipLaunchKernelGGL(act_cols_bwd_kernel, dim3(blocks), dim3(kThreads), 0, as_stream(stream), y, (long)y_ld, g, (long)g_ld, total,
                     (int)n, (int)act, dx, (long)dx_ld);
  return check_launch(who);
}
