// Knowledge-graph link prediction of sample_kg/network_prediction (model_py/{gcn,distmult,ip}.py): the label-batch feed
// with its negative resampling, the pairwise ranking loss, and its gradient without float atomics.
//
//   feed     window j = step mod (M / L) of the row-permuted label list [M, 6] (step read on the DEVICE, so a replayed
//            hipGraph advances it); col 3 := col 0, col 5 := all_label[u] with u drawn bias-free from Philox4x64-10 with
//            key (seed, 0) and counter (row, step, round, 0) -- Lemire's multiply-shift on the 64-bit words in order,
//            rejecting a word whose low product half is below 2^64 mod K (kgcn/feed.py:56-59).  The assembled rows are written.
//   score    s1 = sum_d h[c0] h[c2] w[c1], s2 = sum_d h[c3] h[c5] w[c4] (w = 1 for gcn / ip), one wave per row, fixed-order
//            butterfly.  gcn: cost = -log(sigmoid(s1 - s2) + 1e-10); distmult: cost = -log(1 / (1 + exp(s2 - s1 + 0.1)) +
//            1e-10); ip: the distmult cost on the batch-wide sums S1 = sum_i s1_i, S2 = sum_i s2_i (ip.py:46-47 reduce_sum
//            without an axis).  One workgroup adds the rows in a fixed order: cost_opt = mean, cost_sum, correct = sum [s1 > s2].
//            Where exp(s2 - s1 + 0.1) overflows fp32, TF's gradient out^2 e is 0 * inf = NaN: here it is 0 (the cost is
//            -log(1e-10) either way) -- the one deliberate deviation.
//   backward row i with upstream a_i = d objective / d s1_i (= -d objective / d s2_i) adds a_i h2 w to h0, a_i h0 w to h2,
//            -a_i h5 w' to h3 and -a_i h3 w' to h5.  Store-and-sum: the (row, role) entries are keyed by their node and
//            stably sorted (rocprim LSD radix sort = stable counting sorts, 8 B an entry), so every node's list is in list
//            order.  A wave per chunk of kChunk sorted entries regathers the partner rows and accumulates; a list that lies
//            inside one chunk is written to dH at once, a list that crosses chunks leaves per-chunk partials that a per-node
//            pass adds in chunk order; that pass also writes the zero rows.  Every dH row is written exactly once: no memset,
//            no atomics, bitwise reproducible.  d w[r] (distmult): per-workgroup partials in LDS (each lane owns its columns),
//            fixed-order second stage (deferrable: kgcn_reduce_defer).
#include <rocprim/device/device_radix_sort.hpp>

#include "block_reduce.h"
#include "workspace.h"
#include "philox.h"

namespace kgcn {

namespace {
constexpr int kChunk = 16;           // sorted entries per wave of the sum pass (longer lists are split and re-added in order):
                                     // each entry is a chain of dependent loads, so a wave's time grows with its entries
constexpr int kDwGroups = 256;       // workgroups (= partials) of the relation-vector gradient
constexpr float kLogEps = 1.0e-10f;
constexpr float kGamma = 0.1f;

__device__ __forceinline__ uint64_t read_step(const int64_t* step) { return step ? (uint64_t)*step : 0ull; }

// u in [0, K) for row `row` of step `step`: no modulo bias (rejection of the 2^64 mod K lowest product halves)
__device__ __forceinline__ uint32_t draw_index(uint64_t seed, uint64_t step, uint64_t row, uint32_t K) {
  const uint64_t k = K;
  const uint64_t t = (0ull - k) % k;
  for (uint64_t r = 0;; ++r) {
    const Philox4 p = philox4x64_10(row, step, r, 0, seed);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (p.v[q] * k >= t) return (uint32_t)__umul64hi(p.v[q], k);
  }
}

struct FwdArgs {
  const float* h;
  const float* w;
  const int32_t* labels;
  const int32_t* perm;
  const int32_t* neg;
  const int64_t* step;
  int32_t* rows;
  float* s1;
  float* s2;
  long nwin;
  uint64_t seed;
  int D, L, K;
};

__global__ __launch_bounds__(256) void lp_score_kernel(FwdArgs a) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.L) return;
  const uint64_t st = read_step(a.step);
  const long j = (long)(st % (uint64_t)a.nwin);
  const long src0 = j * a.L + i;
  const long src = a.perm ? (long)a.perm[src0] : src0;
  int c[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) c[q] = a.labels[src * 6 + q];
  c[3] = c[0];
  c[5] = a.neg[draw_index(a.seed, st, (uint64_t)i, (uint32_t)a.K)];
  if (lane < 6) {
    int v = c[0];
#pragma unroll
    for (int q = 1; q < 6; ++q) v = lane == q ? c[q] : v;
    a.rows[i * 6 + lane] = v;
  }
  const float* h0 = a.h + (long)c[0] * a.D;
  const float* h2 = a.h + (long)c[2] * a.D;
  const float* h3 = a.h + (long)c[3] * a.D;
  const float* h5 = a.h + (long)c[5] * a.D;
  float p1 = 0.f, p2 = 0.f;
  if (a.w) {
    const float* w1 = a.w + (long)c[1] * a.D;
    const float* w4 = a.w + (long)c[4] * a.D;
    for (int d = lane; d < a.D; d += 64) {
      p1 += h0[d] * h2[d] * w1[d];
      p2 += h3[d] * h5[d] * w4[d];
    }
  } else {
    for (int d = lane; d < a.D; d += 64) {
      p1 += h0[d] * h2[d];
      p2 += h3[d] * h5[d];
    }
  }
  p1 = wave_sum(p1);
  p2 = wave_sum(p2);
  if (lane == 0) {
    a.s1[i] = p1;
    a.s2[i] = p2;
  }
}

// cost of one (s1, s2) pair and d cost / d s1 (d cost / d s2 is its negative), as TF differentiates the graph
__device__ __forceinline__ float pair_cost(float x1, float x2, int mode) {
  if (mode == KGCN_LP_GCN) {
    const float y = 1.0f / (1.0f + expf(-(x1 - x2)));
    return -logf(y + kLogEps);
  }
  const float out = 1.0f / (1.0f + expf(x2 - x1 + kGamma));
  return -logf(out + kLogEps);
}
__device__ __forceinline__ float pair_dcost(float x1, float x2, int mode) {
  if (mode == KGCN_LP_GCN) {                      // -(sigmoid' = y (1 - y)) / (y + 1e-10), y -> 0 gives 0 / 1e-10 = 0
    const float y = 1.0f / (1.0f + expf(-(x1 - x2)));
    return -(y * (1.0f - y)) / (y + kLogEps);
  }
  const float e = expf(x2 - x1 + kGamma);
  if (isinf(e)) return 0.f;                       // the defined limit (TF: 0 * inf = NaN)
  const float out = 1.0f / (1.0f + e);
  return -(out * out * e) / (out + kLogEps);      // d cost / d score = out^2 e / (out + 1e-10), d score / d s1 = -1
}

// sums: cost_opt, cost_sum, correct_count, S1, S2 (the last two: ip only)
__global__ __launch_bounds__(256) void lp_cost_kernel(const float* __restrict__ s1, const float* __restrict__ s2, int L, int mode,
                                                      float* __restrict__ sums) {
  __shared__ float red[2][256];
  const int t = threadIdx.x;
  float a[2] = {0.f, 0.f};
  for (int i = t; i < L; i += 256) {
    const float x1 = s1[i], x2 = s2[i];
    if (mode == KGCN_LP_IP) {
      a[0] += x1;
      a[1] += x2;
    } else {
      a[0] += pair_cost(x1, x2, mode);
      a[1] += x1 > x2 ? 1.f : 0.f;
    }
  }
  block_sum(a, red);
  if (t == 0) {
    if (mode == KGCN_LP_IP) {
      const float S1 = a[0], S2 = a[1], c = pair_cost(S1, S2, mode);
      sums[0] = c;
      sums[1] = c;
      sums[2] = S1 > S2 ? 1.f : 0.f;
      sums[3] = S1;
      sums[4] = S2;
    } else {
      sums[0] = a[0] / (float)L;
      sums[1] = a[0];
      sums[2] = a[1];
      sums[3] = 0.f;
      sums[4] = 0.f;
    }
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------
// role k of an entry 4 i + k: the label column it sits in, its partner column, the relation column, the sign of a_i
__device__ __forceinline__ int role_col(int k) { return k == 0 ? 0 : k == 1 ? 2 : k == 2 ? 3 : 5; }
__device__ __forceinline__ int partner_col(int k) { return k == 0 ? 2 : k == 1 ? 0 : k == 2 ? 5 : 3; }

__global__ __launch_bounds__(256) void lp_keys_kernel(const int32_t* __restrict__ rows, const float* __restrict__ s1,
                                                      const float* __restrict__ s2, const float* __restrict__ sums, int L,
                                                      int mode, const float* g_opt, const float* g_sum,
                                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                      float* __restrict__ up) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= L) return;
  const float go = g_opt ? *g_opt : 0.f, gs = g_sum ? *g_sum : 0.f;
  float ai;
  if (mode == KGCN_LP_IP)                        // one scalar cost: cost_opt = cost_sum = cost
    ai = (go + gs) * pair_dcost(sums[3], sums[4], mode);
  else
    ai = (go / (float)L + gs) * pair_dcost(s1[i], s2[i], mode);
  up[i] = ai;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    keys[4 * i + k] = (uint32_t)rows[i * 6 + role_col(k)];
    vals[4 * i + k] = (uint32_t)(4 * i + k);
  }
}

// start[n] = first sorted position of node n, start[N] = E
__global__ __launch_bounds__(256) void lp_start_kernel(const uint32_t* __restrict__ keys, long E, long N, int32_t* __restrict__ start) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p > E) return;
  const long prev = p > 0 ? (long)keys[p - 1] : -1;
  const long cur = p < E ? (long)keys[p] : N;
  for (long n = prev + 1; n <= cur; ++n) start[n] = (int32_t)p;
}

struct SumArgs {
  const float* h;
  const float* w;
  const int32_t* rows;
  const float* up;
  const uint32_t* keys;
  const uint32_t* vals;
  const int32_t* start;
  float* dh;
  float* part;          // [chunks, 2, D]: slot 0 = the list that begins at the chunk's first entry, slot 1 = the one that ends it
  long E, nchunks;
  int D;
};

constexpr int kMaxCols = KGCN_LP_MAX_DIM / 64;

__global__ __launch_bounds__(256) void lp_chunk_sum_kernel(SumArgs a) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.nchunks) return;
  const long p0 = c * kChunk, p1 = min(a.E, p0 + kChunk);
  float acc[kMaxCols];
#pragma unroll
  for (int s = 0; s < kMaxCols; ++s) acc[s] = 0.f;
  long seg0 = p0;
  for (long p = p0; p < p1; ++p) {
    const uint32_t n = a.keys[p], e = a.vals[p];
    const int i = (int)(e >> 2), k = (int)(e & 3);
    const float f = k < 2 ? a.up[i] : -a.up[i];
    const float* hq = a.h + (long)a.rows[i * 6 + partner_col(k)] * a.D;
    const float* wr = a.w ? a.w + (long)a.rows[i * 6 + (k < 2 ? 1 : 4)] * a.D : nullptr;
#pragma unroll
    for (int s = 0; s < kMaxCols; ++s) {
      const int d = lane + 64 * s;
      if (d < a.D) acc[s] += wr ? f * hq[d] * wr[d] : f * hq[d];
    }
    if (p + 1 == p1 || a.keys[p + 1] != n) {    // the end of node n's run inside this chunk
      const long ns = a.start[n], ne = a.start[n + 1];
      float* dst;
      if (ns >= p0 && ne <= p1) dst = a.dh + (long)n * a.D;                 // the whole list: final
      else dst = a.part + (c * 2 + (seg0 == p0 ? 0 : 1)) * a.D;             // a piece of a list that crosses chunks
#pragma unroll
      for (int s = 0; s < kMaxCols; ++s) {
        const int d = lane + 64 * s;
        if (d < a.D) dst[d] = acc[s];
        acc[s] = 0.f;
      }
      seg0 = p + 1;
    }
  }
}

// per node: zero row (no entries), or the chunk partials of a list that crosses chunks added in chunk order
__global__ __launch_bounds__(256) void lp_node_sum_kernel(const int32_t* __restrict__ start, const float* __restrict__ part,
                                                          long N, int D, float* __restrict__ dh) {
  const int lane = threadIdx.x & 63;
  const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const long ns = start[n], ne = start[n + 1];
  float* dst = dh + n * D;
  if (ns == ne) {
    for (int d = lane; d < D; d += 64) dst[d] = 0.f;
    return;
  }
  const long cs = ns / kChunk, ce = (ne - 1) / kChunk;
  if (cs == ce) return;                          // written by the chunk pass
#pragma unroll
  for (int s = 0; s < kMaxCols; ++s) {
    const int d = lane + 64 * s;
    if (d >= D) break;
    float acc = part[(cs * 2 + (ns > cs * kChunk ? 1 : 0)) * D + d];
    for (long c = cs + 1; c <= ce; ++c) acc += part[(c * 2) * D + d];
    dst[d] = acc;
  }
}

// d w partials: workgroup g (one wave) owns rows [g RB, (g + 1) RB) and an [R, D] LDS slab, lane l the columns l + 64 s
__global__ __launch_bounds__(64) void lp_dw_kernel(const float* __restrict__ h, const int32_t* __restrict__ rows,
                                                   const float* __restrict__ up, int L, int D, int R, int rb,
                                                   float* __restrict__ part) {
  extern __shared__ float slab[];
  const int lane = threadIdx.x;
  for (int q = lane; q < R * D; q += 64) slab[q] = 0.f;
  __syncthreads();
  const int i0 = blockIdx.x * rb, i1 = min(L, i0 + rb);
  for (int i = i0; i < i1; ++i) {
    const float ai = up[i];
    const int* c = rows + (long)i * 6;
    const float* h0 = h + (long)c[0] * D;
    const float* h2 = h + (long)c[2] * D;
    const float* h3 = h + (long)c[3] * D;
    const float* h5 = h + (long)c[5] * D;
    float* w1 = slab + c[1] * D;
    float* w4 = slab + c[4] * D;
    for (int d = lane; d < D; d += 64) {
      w1[d] += ai * h0[d] * h2[d];
      w4[d] -= ai * h3[d] * h5[d];
    }
  }
  __syncthreads();
  float* out = part + (long)blockIdx.x * R * D;
  for (int q = lane; q < R * D; q += 64) out[q] = slab[q];
}

int dw_groups(int L) { return L < kDwGroups ? (L > 0 ? L : 1) : kDwGroups; }

struct Layout {
  uint32_t *keys_in, *keys_out, *vals_in, *vals_out;
  int32_t* start;
  float *up, *part, *dwpart;
  void* temp;
  size_t temp_bytes, total;
};

unsigned key_bits(long n) {
  unsigned b = 1;
  while ((1l << b) < n + 1) ++b;
  return b;
}

size_t sort_temp_bytes(long E, unsigned bits) {
  size_t b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                  (size_t)E, 0u, bits, (hipStream_t)0);
  return b;
}

Layout layout(unsigned char* base, long N, int D, int R, int L) {
  Layout o{};
  const long E = 4l * L, nch = (E + kChunk - 1) / kChunk;
  Taker t{base};
  o.keys_in = t.take<uint32_t>((size_t)E);
  o.keys_out = t.take<uint32_t>((size_t)E);
  o.vals_in = t.take<uint32_t>((size_t)E);
  o.vals_out = t.take<uint32_t>((size_t)E);
  o.start = t.take<int32_t>((size_t)N + 1);
  o.up = t.take<float>((size_t)L);
  o.part = t.take<float>((size_t)nch * 2 * D);
  o.dwpart = t.take<float>(R > 0 ? (size_t)dw_groups(L) * R * D : 0);
  o.temp_bytes = sort_temp_bytes(E, key_bits(N));
  o.temp = t.take<unsigned char>(o.temp_bytes);
  o.total = t.off + 256;
  return o;
}

int check_shape(const char* who, int64_t nodes, int32_t dim, int32_t relations, int32_t mode, int32_t batch) {
  if (mode != KGCN_LP_GCN && mode != KGCN_LP_DISTMULT && mode != KGCN_LP_IP) return fail("%s: unknown mode %d", who, mode);
  if (nodes <= 0 || nodes >= (int64_t)INT32_MAX) return fail("%s: node count %lld out of range", who, (long long)nodes);
  if (dim <= 0 || dim > KGCN_LP_MAX_DIM) return fail("%s: dim %d outside 1..%d", who, dim, KGCN_LP_MAX_DIM);
  if (batch <= 0 || batch > KGCN_LP_MAX_BATCH) return fail("%s: label batch %d outside 1..%d", who, batch, KGCN_LP_MAX_BATCH);
  if (mode == KGCN_LP_DISTMULT && (relations <= 0 || (int64_t)relations * dim > KGCN_LP_MAX_REL_FLOATS))
    return fail("%s: %d relations x dim %d exceeds %d floats", who, relations, dim, KGCN_LP_MAX_REL_FLOATS);
  return 0;
}

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int64_t kgcn_linkpred_workspace_bytes(int64_t nodes, int32_t dim, int32_t relations, int32_t mode, int32_t batch) {
  if (check_shape("kgcn_linkpred_workspace_bytes", nodes, dim, relations, mode, batch)) return -1;
  return (int64_t)layout(nullptr, nodes, dim, mode == KGCN_LP_DISTMULT ? relations : 0, batch).total;
}

extern "C" int kgcn_linkpred_fwd_f32(const float* h, int64_t nodes, int32_t dim, const float* w, int32_t relations, int32_t mode,
                                     const int32_t* labels, const int32_t* perm, int64_t num_labels, int32_t batch,
                                     const int32_t* negatives, int32_t num_negatives, uint64_t seed, const int64_t* step,
                                     int32_t* rows, float* s1, float* s2, float* sums, void* stream) {
  if (int rc = check_shape("kgcn_linkpred_fwd_f32", nodes, dim, relations, mode, batch)) return rc;
  if (num_labels < batch) return fail("kgcn_linkpred_fwd_f32: %lld labels < one batch of %d", (long long)num_labels, batch);
  if (num_negatives <= 0) return fail("kgcn_linkpred_fwd_f32: empty negative table");
  if (!h || !labels || !negatives || !rows || !s1 || !s2 || !sums || (mode == KGCN_LP_DISTMULT && !w))
    return fail("kgcn_linkpred_fwd_f32: NULL operand");
  hipStream_t s = as_stream(stream);
  FwdArgs a{h, mode == KGCN_LP_DISTMULT ? w : nullptr, labels, perm, negatives, step, rows, s1, s2,
            (long)(num_labels / batch), seed, dim, batch, num_negatives};
  hipLaunchKernelGGL(lp_score_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(lp_cost_kernel, dim3(1), dim3(256), 0, s, s1, s2, batch, mode, sums);
  return check_launch("kgcn_linkpred_fwd_f32");
}

extern "C" int kgcn_linkpred_bwd_f32(const float* h, int64_t nodes, int32_t dim, const float* w, int32_t relations, int32_t mode,
                                     const int32_t* rows, const float* s1, const float* s2, const float* sums, int32_t batch,
                                     const float* g_opt, const float* g_sum, float* dh, float* dw, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  if (int rc = check_shape("kgcn_linkpred_bwd_f32", nodes, dim, relations, mode, batch)) return rc;
  const bool dm = mode == KGCN_LP_DISTMULT;
  if (!h || !rows || !s1 || !s2 || !sums || !dh || (dm && (!w || !dw))) return fail("kgcn_linkpred_bwd_f32: NULL operand");
  const int R = dm ? relations : 0;
  if (int rc = check_workspace("kgcn_linkpred_bwd_f32", workspace, workspace_bytes, (int64_t)layout(nullptr, nodes, dim, R, batch).total))
    return rc;
  hipStream_t s = as_stream(stream);
  const Layout o = layout(aligned_base(workspace), nodes, dim, R, batch);
  const long E = 4l * batch, nch = (E + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(lp_keys_kernel, dim3(blocks_of(batch)), dim3(256), 0, s, rows, s1, s2, sums, batch, mode,
                     g_opt, g_sum, o.keys_in, o.vals_in, o.up);
  size_t temp = o.temp_bytes;
  if (rocprim::radix_sort_pairs(o.temp, temp, o.keys_in, o.keys_out, o.vals_in, o.vals_out, (size_t)E, 0u, key_bits(nodes), s) !=
      hipSuccess)
    return fail("kgcn_linkpred_bwd_f32: rocprim::radix_sort_pairs failed");
  hipLaunchKernelGGL(lp_start_kernel, dim3(blocks_of(E + 1)), dim3(256), 0, s, o.keys_out, E, (long)nodes, o.start);
  SumArgs sa{h, dm ? w : nullptr, rows, o.up, o.keys_out, o.vals_out, o.start, dh, o.part, E, nch, dim};
  hipLaunchKernelGGL(lp_chunk_sum_kernel, dim3((unsigned)((nch + 3) / 4)), dim3(256), 0, s, sa);
  hipLaunchKernelGGL(lp_node_sum_kernel, dim3((unsigned)((nodes + 3) / 4)), dim3(256), 0, s, o.start, o.part, (long)nodes, dim, dh);
  if (dm) {
    const int G = dw_groups(batch), rb = (batch + G - 1) / G;
    hipLaunchKernelGGL(lp_dw_kernel, dim3((unsigned)G), dim3(64), (size_t)R * dim * 4, s, h, rows, o.up, batch, dim, R, rb,
                       o.dwpart);
    if (int rc = check_launch("kgcn_linkpred_bwd_f32")) return rc;
    return reduce_or_defer(o.dwpart, G, (long)R * dim, dw, s);
  }
  return check_launch("kgcn_linkpred_bwd_f32");
}
