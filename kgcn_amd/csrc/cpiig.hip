// Integrated gradients of the compound-protein interaction multitask network (kgcn visualize on
// sample_chem/compound-protein_interaction/multitask.py:35-51; kgcn/visualization.py:187-286 and :442-574) for MANY compounds
// and ALL tasks: the sweep over the scaled copies.
//
//   The network is GraphConv(Wd) -> sigmoid -> sum over the node rows -> Dense(2 T), and task t's prediction is
//   sigmoid(h . u_t + e_t).  Copy k feeds a_k X and c_k v, so its pre-activation is Z_k = alpha_k P + gamma_k Q with
//   alpha_k = a_k c_k, gamma_k = c_k and P = sum_ch A_ch X W_ch, Q = sum_ch rowsum(A_ch) (x) b_ch formed ONCE per compound by
//   the caller.  Everything the K forwards and the K T backwards need is element-wise in (P, Q):
//     score pass       S[c, k, j]  = sum_n sigmoid(Z_k[n, j])                     cpi_ig_colsum_kernel, n in order
//                      p[c, k, t]  = sigmoid(S[c, k, :] . u_t + e_t)              cpi_ig_score_kernel, one wave per (c, k)
//     accumulate pass  G^A[c, t, n, j] = u_t[j] sum_k wA_k p(1 - p)[c, k, t] H_k(1 - H_k)[n, j]   (and G^B with wB)
//                      cpi_ig_accum_kernel: one element (n, j) per lane, k in order, ONE sigmoid per k; d = H(1 - H) is shared
//                      by the tasks, the coefficients w_k p(1 - p) of kCoefSteps copies sit in LDS, u_t[j] multiplies once at
//                      the end.  A lane carries kTaskCap tasks (2 kTaskCap sums with G^B); further tasks take further passes
//                      (blocks), each of which runs the sigmoids again.
//   P and Q of one compound (2 N Wd floats, 205 KB at N = 50, Wd = 512) do not fit LDS: the score pass streams them once per
//   block of kStepBlock copies (they stay in L2), the accumulate pass holds its element in two registers.
//
//   sigmoid(z) and sigmoid(z) sigmoid(-z) come from e = exp(-|z|) in (0, 1]: r = 1 / (1 + e), H = r or e r, H(1 - H) = e r r.
//   Nothing overflows and nothing cancels, whatever |z| (e underflows to 0 around |z| = 104: H(1 - H) = 0, as it should be).
//   p(1 - p) is formed the same way by the score kernel and handed on in the workspace, not recomputed as p - p p.
//   Every sum runs in one fixed order, there are no atomics, and no block works on more than one compound: the outputs are
//   bitwise reproducible and do not depend on which compounds share a launch.
#include "block_reduce.h"
#include "workspace.h"

namespace kgcn {

namespace {
constexpr int kTaskCap = KGCN_CPIIG_TASKS_PER_PASS;   // tasks a lane accumulates in one pass
constexpr int kStepBlock = 8;                         // copies per block of the column-sum kernel
constexpr int kCoefSteps = 128;                       // copies whose coefficients are staged in LDS at a time

struct Sig {
  float h, d;                                         // sigmoid(z) and sigmoid(z) (1 - sigmoid(z))
};

__device__ __forceinline__ Sig stable_sigmoid(float z) {
  const float e = expf(-fabsf(z));
  const float r = 1.0f / (1.0f + e);
  Sig s;
  s.h = z >= 0.f ? r : e * r;
  s.d = e * r * r;
  return s;
}

__device__ __forceinline__ float pre_activation(float alpha, float p, float gamma, float q) { return fmaf(alpha, p, gamma * q); }

// S[c, k, j] = sum_n sigmoid(alpha_k P[c, n, j] + gamma_k Q[c, n, j]): block = (compound, kStepBlock copies, 256 columns)
__global__ __launch_bounds__(256) void cpi_ig_colsum_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                            const float* __restrict__ alpha, const float* __restrict__ gamma,
                                                            float* __restrict__ S, int N, int Wd, int K, int jblocks, int kblocks) {
  long b = blockIdx.x;
  const int jb = (int)(b % jblocks);
  b /= jblocks;
  const int kb = (int)(b % kblocks);
  const long c = b / kblocks;
  const int j = jb * 256 + (int)threadIdx.x;
  const int k0 = kb * kStepBlock;
  if (j >= Wd) return;
  float al[kStepBlock], ga[kStepBlock], acc[kStepBlock];
#pragma unroll
  for (int kk = 0; kk < kStepBlock; ++kk) {
    const int k = min(k0 + kk, K - 1);                // a copy past the end repeats the last one; its sum is not stored
    al[kk] = alpha[k];
    ga[kk] = gamma[k];
    acc[kk] = 0.f;
  }
  const float* p = P + c * N * Wd + j;
  const float* q = Q + c * N * Wd + j;
  for (int n = 0; n < N; ++n) {
    const float pv = p[(long)n * Wd], qv = q[(long)n * Wd];
#pragma unroll
    for (int kk = 0; kk < kStepBlock; ++kk) acc[kk] += stable_sigmoid(pre_activation(al[kk], pv, ga[kk], qv)).h;
  }
#pragma unroll
  for (int kk = 0; kk < kStepBlock; ++kk)
    if (k0 + kk < K) S[(c * K + k0 + kk) * Wd + j] = acc[kk];
}

// p[ck, t] = sigmoid(S[ck, :] . u_t + e_t), pq[ck, t] = p (1 - p): one wave per (compound, copy), lane-strided columns in
// order, then the butterfly
__global__ __launch_bounds__(256) void cpi_ig_score_kernel(const float* __restrict__ S, const float* __restrict__ u,
                                                           const float* __restrict__ e, float* __restrict__ p,
                                                           float* __restrict__ pq, long CK, int Wd, int T) {
  const int lane = threadIdx.x & 63;
  const long ck = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ck >= CK) return;                               // whole waves leave
  const float* s = S + ck * Wd;
  for (int t = 0; t < T; ++t) {
    const float* ut = u + (long)t * Wd;
    float part = 0.f;
    for (int j = lane; j < Wd; j += 64) part += s[j] * ut[j];
    part = wave_sum(part);
    if (lane == 0) {
      const Sig y = stable_sigmoid(part + e[t]);
      p[ck * T + t] = y.h;
      pq[ck * T + t] = y.d;
    }
  }
}

// G^A[c, t, n, j] = u_t[j] sum_k wA_k pq[c, k, t] d_k[n, j] (G^B with wB): block = (compound, pass of kTaskCap tasks, 256 elements)
template <bool HASB>
__global__ __launch_bounds__(256) void cpi_ig_accum_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                           const float* __restrict__ alpha, const float* __restrict__ gamma,
                                                           const float* __restrict__ wA, const float* __restrict__ wB,
                                                           const float* __restrict__ pq, const float* __restrict__ u,
                                                           float* __restrict__ GA, float* __restrict__ GB, int N, int Wd, int K,
                                                           int T, int eblocks, int passes) {
  __shared__ float cfA[kCoefSteps * kTaskCap];
  __shared__ float cfB[HASB ? kCoefSteps * kTaskCap : 1];
  __shared__ float sal[kCoefSteps], sga[kCoefSteps];
  const int tid = threadIdx.x;
  long b = blockIdx.x;
  const int eb = (int)(b % eblocks);
  b /= eblocks;
  const int pass = (int)(b % passes);
  const long c = b / passes;
  const int t0 = pass * kTaskCap;
  const int nt = min(kTaskCap, T - t0);
  const long NW = (long)N * Wd;
  const long el = (long)eb * 256 + tid;
  const bool live = el < NW;
  const float pv = live ? P[c * NW + el] : 0.f, qv = live ? Q[c * NW + el] : 0.f;
  float accA[kTaskCap], accB[kTaskCap];
#pragma unroll
  for (int tt = 0; tt < kTaskCap; ++tt) accA[tt] = accB[tt] = 0.f;

  for (int k0 = 0; k0 < K; k0 += kCoefSteps) {
    const int kc = min(kCoefSteps, K - k0);
    __syncthreads();                                  // the readers of the previous chunk are done
    for (int i = tid; i < kc * kTaskCap; i += 256) {
      const int kl = i / kTaskCap, tt = i % kTaskCap;
      const float v = tt < nt ? pq[(c * K + k0 + kl) * T + t0 + tt] : 0.f;
      cfA[i] = wA[k0 + kl] * v;
      if (HASB) cfB[i] = wB[k0 + kl] * v;
    }
    for (int i = tid; i < kc; i += 256) {
      sal[i] = alpha[k0 + i];
      sga[i] = gamma[k0 + i];
    }
    __syncthreads();
    for (int kl = 0; kl < kc; ++kl) {
      const float d = stable_sigmoid(pre_activation(sal[kl], pv, sga[kl], qv)).d;
#pragma unroll
      for (int tt = 0; tt < kTaskCap; ++tt) {
        accA[tt] = fmaf(cfA[kl * kTaskCap + tt], d, accA[tt]);
        if (HASB) accB[tt] = fmaf(cfB[kl * kTaskCap + tt], d, accB[tt]);
      }
    }
  }
  if (!live) return;
  const int j = (int)(el % Wd);
#pragma unroll
  for (int tt = 0; tt < kTaskCap; ++tt) {
    if (tt < nt) {
      const float ut = u[(long)(t0 + tt) * Wd + j];
      const long o = (c * T + t0 + tt) * NW + el;
      GA[o] = accA[tt] * ut;
      if (HASB) GB[o] = accB[tt] * ut;
    }
  }
}

// the column sums S [C, K, Wd] | p (1 - p) [C, K, T]
struct IgWorkspace { float *S, *pq; size_t bytes; };
IgWorkspace ig_layout(void* base, int64_t CK, int32_t width, int32_t tasks) {
  Taker t(base, 4);
  IgWorkspace w;
  w.S = t.take<float>((size_t)CK * width);
  w.pq = t.take<float>((size_t)CK * tasks);
  w.bytes = t.off;
  return w;
}

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int64_t kgcn_cpi_ig_workspace_bytes(int32_t compounds, int32_t width, int32_t tasks, int32_t steps) {
  if (compounds <= 0 || width <= 0 || tasks <= 0 || steps <= 0) return 0;
  return (int64_t)ig_layout(nullptr, (int64_t)compounds * steps, width, tasks).bytes;
}

extern "C" int kgcn_cpi_ig_f32(const float* P, const float* Q, int32_t compounds, int32_t nodes, int32_t width, const float* u,
                               const float* e, int32_t tasks, const float* alpha, const float* gamma, const float* wA,
                               const float* wB, int32_t steps, float* p, float* GA, float* GB, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_cpi_ig_f32";
  if (compounds < 0) return fail("%s: %d compounds", who, compounds);
  if (nodes < 1 || width < 1 || tasks < 1) return fail("%s: N = %d, Wd = %d, T = %d: each must be >= 1", who, nodes, width, tasks);
  if (steps < 2) return fail("%s: %d copies, at least 2 (start and end)", who, steps);
  if (compounds == 0) return 0;
  if (!P || !Q || !u || !e || !alpha || !gamma || !wA || !p || !GA) return fail("%s: NULL operand", who);
  if ((wB == nullptr) != (GB == nullptr)) return fail("%s: wB and GB go together", who);
  const int64_t CK = (int64_t)compounds * steps;
  const IgWorkspace ws = ig_layout(workspace, CK, width, tasks);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)ws.bytes)) return rc;
  const int64_t NW = (int64_t)nodes * width;
  const int jblocks = (width + 255) / 256, kblocks = (steps + kStepBlock - 1) / kStepBlock;
  const int passes = (tasks + kTaskCap - 1) / kTaskCap;
  const int64_t eblocks = (NW + 255) / 256;
  const int64_t grid_a = (int64_t)compounds * kblocks * jblocks, grid_b = (CK + 3) / 4, grid_c = (int64_t)compounds * passes * eblocks;
  if (grid_a >= INT32_MAX || grid_b >= INT32_MAX || grid_c >= INT32_MAX || eblocks >= INT32_MAX)
    return fail("%s: %d compounds of %d x %d with %d copies exceed one launch's grid: pass fewer compounds", who, compounds, nodes,
                width, steps);
  float *S = ws.S, *pq = ws.pq;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(cpi_ig_colsum_kernel, dim3((unsigned)grid_a), dim3(256), 0, s, P, Q, alpha, gamma, S, nodes, width, steps, jblocks,
                     kblocks);
  if (int rc = check_launch("cpi_ig_colsum_kernel")) return rc;
  hipLaunchKernelGGL(cpi_ig_score_kernel, dim3((unsigned)grid_b), dim3(256), 0, s, S, u, e, p, pq, (long)CK, width, tasks);
  if (int rc = check_launch("cpi_ig_score_kernel")) return rc;
  if (wB)
    hipLaunchKernelGGL(cpi_ig_accum_kernel<true>, dim3((unsigned)grid_c), dim3(256), 0, s, P, Q, alpha, gamma, wA, wB, pq, u, GA, GB,
                       nodes, width, steps, tasks, (int)eblocks, passes);
  else
    hipLaunchKernelGGL(cpi_ig_accum_kernel<false>, dim3((unsigned)grid_c), dim3(256), 0, s, P, Q, alpha, gamma, wA, wB, pq, u, GA, GB,
                       nodes, width, steps, tasks, (int)eblocks, passes);
  return check_launch("cpi_ig_accum_kernel");
}
