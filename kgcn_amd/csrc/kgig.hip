// Integrated gradients of the link-prediction model (kgcn visualize on sample_kg/network_prediction/model_py/gcn.py:
// cal_feature_IG_for_kg / KnowledgeGraphVisualizer of kgcn/visualization.py:289-439) for MANY targets over ONE graph.
//
//   The network is relu(A (relu(A (E W1 + b1)) W2 + b2)) and the embedded layer E is scaled by alpha_k.  Layer 1 is affine in
//   alpha: Z1_k = alpha_k G1 + r (x) b1 with P = E W1, G1 = A P, r = row sums of A, so its relu mask is recomputed from one row
//   of G1.  The layer-2 output H2_k [K, N, C] does not depend on the target: the caller stashes it once.  A target (an edge
//   score s = h[a] . h[b], or the ranking cost of s1 = h[a] . h[b] against s2 = h[a'] . h[b']) seeds at most four rows of dH2,
//   each "seed row s gets coef * h[partner]"; everything downstream is linear in the seeds, so every (seed, partner) entry is
//   carried on its own and a == b or shared nodes need no special case:
//     dZ2[s]     = coef_k H2_k[partner] (.) [H2_k[s] > 0]                          coef = 1, or +-pair_dcost(s1_k, s2_k)
//     v_(s,k)    = dZ2[s] W2^T                                                     [<= 4 K rows, 128] x [128, 128]: fp32 MFMA
//     U[i]      += w_k A[s, i] v_(s,k) (.) [alpha_k G1[i] + r[i] b1 > 0]           every entry of row s of A, k in order
//     node_ig[j] = sum_i A[i, j] <U[i], P[j]>                                      = sum_d E[j, d] dE[j, d], what the dump reads
//   A^T and W1 do not depend on k, so the sum over k sits inside: no per-target [N, C] tensor is formed unless the caller
//   asks for U (the full [N, De] attribution is E (.) ((A^T U) W1^T) from the existing ops).
//
//   One persistent workgroup (4 waves) per target, grid-stride over the targets; it owns the target's output rows.  LDS: W2
//   (64 KiB, once per workgroup), the 128-row operand / product block (the product overwrites the operand: wave j owns seed
//   j's 32 rows of both), four U rows and the target's node_ig row [N] -- the last bounds N (KGCN_KGIG_MAX_NODES).  Steps
//   beyond 32 run as further chunks of 32 in order.  The (seed, i) pairs are taken in a fixed order (seed, then CSR order),
//   four at a time: wave w forms the U row of pair q + w, then the four rows are scattered one after the other, the entries
//   of row i of A spread over the 256 threads -- columns within a CSR row are distinct (the caller checks it), so no two
//   threads meet on a node_ig slot.  No float atomics anywhere: results are bitwise reproducible.
#include "block_reduce.h"
#include "kgcn_common.h"

namespace kgcn {

namespace {
constexpr int kC = KGCN_KGIG_WIDTH;      // layer width
constexpr int kSteps = 32;               // steps per chunk: 4 seeds x 32 steps = the 128 rows of one product
constexpr int kLdv = kC + 1;             // operand / product row stride
constexpr float kLogEps = 1.0e-10f;

struct Args {
  const int32_t* indptr;
  const int32_t* indices;
  const float* values;
  const float* g1;
  const float* rowsum;
  const float* b1;
  const float* w2;
  const float* h2;
  const float* p;
  const float* scales;
  const float* weights;
  const int32_t* targets;
  float* node_ig;
  float* score;
  float* u;
  int N, K, T, mode;
};

__host__ __device__ constexpr size_t lds_floats(int N) {
  return (size_t)kC * kC + (size_t)4 * kSteps * kLdv + 4 * kC + kSteps + 8 + (size_t)N;
}

// d cost / d s1 of -log(sigmoid(s1 - s2) + 1e-10) = -y (1 - y) / (y + 1e-10) (linkpred.hip, KGCN_LP_GCN), with 1 - y formed as
// sigmoid(s2 - s1) instead of by cancellation: the attribution sums this factor over the steps, saturated ones included
__device__ __forceinline__ float gcn_dcost(float x1, float x2) {
  const float x = x1 - x2;
  const float y = 1.0f / (1.0f + expf(-x)), q = 1.0f / (1.0f + expf(x));
  return -(y * q) / (y + kLogEps);
}

__global__ __launch_bounds__(256) void kg_ig_kernel(Args a) {
  extern __shared__ float lds[];
  float* w2t = lds;                           // [d][c ^ ((d & 1) << 5)] = W2[c][d]: the B operand, halves of odd rows swapped
  float* vb = w2t + kC * kC;                  // [4 seeds x kSteps][kLdv]: dZ2 rows, then v rows
  float* ub = vb + 4 * kSteps * kLdv;         // [4][kC]: the U rows of four pairs
  float* cf = ub + 4 * kC;                    // [kSteps] the upstream coefficient of the chunk's steps
  int* meta = reinterpret_cast<int*>(cf + kSteps);    // [8]: node i of the four pairs (-1: none)
  float* nig = reinterpret_cast<float*>(meta + 8);    // [N]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, hi = lane >> 5;
  const int N = a.N, K = a.K;

  for (int i = tid; i < kC * kC; i += 256) {
    const int c = i >> 7, d = i & (kC - 1);
    w2t[d * kC + (c ^ ((d & 1) << 5))] = a.w2[i];
  }
  for (int i = tid; i < N; i += 256) nig[i] = 0.f;
  __syncthreads();

  for (long t = blockIdx.x; t < a.T; t += gridDim.x) {
    const int ta = a.targets[t * 4 + 0], tb = a.targets[t * 4 + 1];
    const int tc = a.mode == KGCN_KGIG_LOSS ? a.targets[t * 4 + 2] : 0, td = a.mode == KGCN_KGIG_LOSS ? a.targets[t * 4 + 3] : 0;
    const int nseed = a.mode == KGCN_KGIG_LOSS ? 4 : 2;
    // ids are checked by the caller; a bad one must still not read or write out of bounds: such a target gives zeros
    const bool ok = (unsigned)ta < (unsigned)N && (unsigned)tb < (unsigned)N && (unsigned)tc < (unsigned)N && (unsigned)td < (unsigned)N;
    const int seed[4] = {ta, tb, tc, td};
    int beg[4], cum[5];
    cum[0] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = ok && j < nseed;
      beg[j] = live ? a.indptr[seed[j]] : 0;
      cum[j + 1] = cum[j] + (live ? a.indptr[seed[j] + 1] - beg[j] : 0);
    }
    const int npairs = cum[4];

    for (int k0 = 0; k0 < K; k0 += kSteps) {
      const int kc = min(kSteps, K - k0);
      // ---- the scores of the chunk's steps, read off the stash: one wave per step ------------------------------------------
      for (int kl = wv; kl < kc; kl += 4) {
        float s1 = 0.f, s2 = 0.f;
        if (ok) {
          const float* h = a.h2 + (long)(k0 + kl) * N * kC;
          s1 = h[(long)ta * kC + lane] * h[(long)tb * kC + lane] + h[(long)ta * kC + lane + 64] * h[(long)tb * kC + lane + 64];
          if (a.mode == KGCN_KGIG_LOSS)
            s2 = h[(long)tc * kC + lane] * h[(long)td * kC + lane] + h[(long)tc * kC + lane + 64] * h[(long)td * kC + lane + 64];
        }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        if (lane == 0) {
          cf[kl] = a.mode == KGCN_KGIG_LOSS ? gcn_dcost(s1, s2) : 1.0f;
          a.score[t * K + k0 + kl] = s1 - s2;
        }
      }
      __syncthreads();
      // ---- dZ2 rows: row j * 32 + kl = coef H2_k[partner_j] (.) [H2_k[seed_j] > 0] ----------------------------------------
      for (int i = tid; i < 4 * kSteps * kC; i += 256) {
        const int row = i >> 7, d = i & (kC - 1), j = row >> 5, kl = row & (kSteps - 1);
        float v = 0.f;
        if (ok && j < nseed && kl < kc) {
          const float* h = a.h2 + (long)(k0 + kl) * N * kC;
          const float coef = j >= 2 ? -cf[kl] : cf[kl];
          const int sj = j == 0 ? ta : j == 1 ? tb : j == 2 ? tc : td, pj = j == 0 ? tb : j == 1 ? ta : j == 2 ? td : tc;
          v = h[(long)sj * kC + d] > 0.f ? coef * h[(long)pj * kC + d] : 0.f;
        }
        vb[row * kLdv + d] = v;
      }
      __syncthreads();
      // ---- v = dZ2 W2^T: wave j owns seed j's 32 rows and overwrites them ---------------------------------------------------
      if (wv < nseed) {
        f32x16 acc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
        const float* xa = vb + (wv * 32 + li) * kLdv + hi;
        const float* wb = w2t + hi * kC;
#pragma unroll 4
        for (int s = 0; s < kC / 2; ++s) {
          const float av = xa[2 * s];
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wb[2 * s * kC + ((cb * 32 + li) ^ (hi << 5))], acc[cb], 0, 0, 0);
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            vb[(wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi) * kLdv + cb * 32 + li] = acc[cb][r];
      }
      __syncthreads();
      // ---- the (seed, i) pairs in order, four at a time --------------------------------------------------------------------
      for (int q0 = 0; q0 < npairs; q0 += 4) {
        const int q = q0 + wv;
        if (q < npairs) {
          const int j = q < cum[1] ? 0 : q < cum[2] ? 1 : q < cum[3] ? 2 : 3;
          const int bj = j == 0 ? beg[0] : j == 1 ? beg[1] : j == 2 ? beg[2] : beg[3];
          const int cj = j == 0 ? cum[0] : j == 1 ? cum[1] : j == 2 ? cum[2] : cum[3];
          const int e = bj + q - cj;
          int i = a.indices[e];
          const float av = a.values[e];
          const bool in = (unsigned)i < (unsigned)N;
          i = in ? i : 0;
          const float ga = a.g1[(long)i * kC + lane], gb = a.g1[(long)i * kC + lane + 64];
          const float rs = a.rowsum[i];
          const float ba = __fmul_rn(rs, a.b1[lane]), bb = __fmul_rn(rs, a.b1[lane + 64]);
          const float* vr = vb + j * 32 * kLdv;
          float ua = 0.f, ub2 = 0.f;
          for (int kl = 0; kl < kc; ++kl) {
            const float al = a.scales[k0 + kl], wk = a.weights[k0 + kl];
            // the pre-activation exactly as the caller formed it for the stash: a product, a product, a sum (no fma)
            const float za = __fadd_rn(__fmul_rn(al, ga), ba), zb = __fadd_rn(__fmul_rn(al, gb), bb);
            if (za > 0.f) ua += wk * vr[kl * kLdv + lane];
            if (zb > 0.f) ub2 += wk * vr[kl * kLdv + lane + 64];
          }
          if (lane == 0) meta[wv] = in ? i : -1;
          ub[wv * kC + lane] = in ? av * ua : 0.f;
          ub[wv * kC + lane + 64] = in ? av * ub2 : 0.f;
        }
        __syncthreads();
        const int nq = min(4, npairs - q0);
        for (int w = 0; w < nq; ++w) {
          const int i = meta[w];
          if (i >= 0) {
            const float* ur = ub + w * kC;
            if (a.u && tid < kC) a.u[(t * N + i) * kC + tid] += ur[tid];     // this thread alone ever touches the element
            const int rb = a.indptr[i], re = a.indptr[i + 1];
            for (int e = rb + tid; e < re; e += 256) {
              const int jn = a.indices[e];
              if ((unsigned)jn >= (unsigned)N) continue;
              const f32x4* pr = reinterpret_cast<const f32x4*>(a.p + (long)jn * kC);
              float dot = 0.f;
#pragma unroll 8
              for (int c4 = 0; c4 < kC / 4; ++c4) {
                const f32x4 pv = pr[c4];
                dot += ur[4 * c4] * pv[0];
                dot += ur[4 * c4 + 1] * pv[1];
                dot += ur[4 * c4 + 2] * pv[2];
                dot += ur[4 * c4 + 3] * pv[3];
              }
              nig[jn] += a.values[e] * dot;
            }
          }
          __syncthreads();
        }
      }
    }
    for (int i = tid; i < N; i += 256) {
      a.node_ig[t * N + i] = nig[i];
      nig[i] = 0.f;
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int kgcn_kg_ig_f32(const int32_t* indptr, const int32_t* indices, const float* values, int64_t nnz, int32_t nodes,
                              int32_t width, const float* g1, const float* rowsum, const float* b1, const float* w2,
                              const float* h2, const float* p, const float* scales, const float* weights, int32_t steps,
                              const int32_t* targets, int32_t num_targets, int32_t mode, int32_t groups, float* node_ig,
                              float* score, float* u, void* stream) {
  const char* who = "kgcn_kg_ig_f32";
  if (width != KGCN_KGIG_WIDTH) return fail("%s: layer width %d, the kernel is built for %d", who, width, KGCN_KGIG_WIDTH);
  if (nodes < 1 || nodes > KGCN_KGIG_MAX_NODES) return fail("%s: %d nodes outside 1..%d", who, nodes, KGCN_KGIG_MAX_NODES);
  if (steps < 1 || steps > KGCN_KGIG_MAX_STEPS) return fail("%s: %d steps outside 1..%d", who, steps, KGCN_KGIG_MAX_STEPS);
  if (mode != KGCN_KGIG_SCORE && mode != KGCN_KGIG_LOSS) return fail("%s: unknown mode %d", who, mode);
  if (num_targets < 0) return fail("%s: %d targets", who, num_targets);
  if (nnz < 0 || nnz >= (int64_t)INT32_MAX) return fail("%s: %lld adjacency entries", who, (long long)nnz);
  if (groups < 0 || groups > 65535) return fail("%s: %d workgroups", who, groups);
  if (num_targets == 0) return 0;
  if (!indptr || (nnz > 0 && (!indices || !values)) || !g1 || !rowsum || !b1 || !w2 || !h2 || !p || !scales || !weights || !targets ||
      !node_ig || !score)
    return fail("%s: NULL operand", who);
  if (!aligned16(p)) return fail("%s: p must be 16-byte aligned", who);
  const size_t lds = lds_floats(nodes) * 4;
  if (int rc = allow_full_lds<kg_ig_kernel>(lds, who)) return rc;
  int grid = groups > 0 ? groups : KGCN_KGIG_GROUPS;
  if (grid > num_targets) grid = num_targets;
  Args a{indptr, indices, values, g1, rowsum, b1, w2, h2, p, scales, weights, targets, node_ig, score, u, nodes, steps, num_targets, mode};
  hipLaunchKernelGGL(kg_ig_kernel, dim3((unsigned)grid), dim3(256), lds, as_stream(stream), a);
  return check_launch("kg_ig_kernel");
}
