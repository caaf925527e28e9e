// Graph VAE of example_model/model_vae.py: counter-based normal noise, the reparameterisation with its KL term, and the
// reconstruction loss of the decoded [B, C, N, N] adjacency logits without ever writing them.
//
//   noise   Philox4x64-10 (Random123; the generator numpy ships as np.random.Philox) with key (seed, 0) and counter
//           (block index, step, 0, 0): one call gives four 64-bit words = four N(0, 1) values by Box-Muller in f32.  The step
//           is read on the DEVICE through a pointer, so a replayed hipGraph draws fresh noise every step (kgcn_amd binds it
//           to the optimiser's step counter: the noise of step t is a pure function of (seed, t)).
//   sample  mean = clip(m, -100, 100), std = clip(sqrt(softplus(s)), -5, 5) (model_vae.py:89-96),
//           z[b, n, :] = mean_b + std_b * eps[b, n, :] for all N rows (:169-175),
//           kl[b] = N * sum_k (1 + 2 log(std + 1e-10) - mean^2 - std) (:178-180; the loss is -1/2 mean_b kl[b], :181).
//           The backward regenerates eps from (seed, step) instead of storing it.
//   recon   per graph, per channel c: L = (Y_c * w_c) Y_c^T, cost += TF's stable sigmoid CE against the dense label matrix
//           of the packed CSR (:224-228); the channel-max of L and of the labels give correct_exist (:244-251); the node
//           feature CE (:217-221).  The backward recomputes L, forms H = G + G^T with G = (sigmoid(L) - A) s_b and
//           dY_c = (H Y_c) * w_c, dw_c = 1/2 sum_i Y_c[i] * (H Y_c)[i] (per-workgroup partials, deferrable second stage).
// One workgroup owns one graph at a time and keeps Y_c and the N x N label / gradient matrix in LDS; L is evaluated in
// 4 x 4 register tiles of the upper triangle only (L is symmetric), in fp32 with fused multiply-adds.
#include "block_reduce.h"
#include "workspace.h"
#include "philox.h"

namespace kgcn {

namespace {
// box_muller: philox.h
__device__ __forceinline__ float normal_at(uint64_t seed, uint64_t step, long e) {
  const Philox4 p = philox4x64_10((uint64_t)(e >> 2), step, seed);
  const int q = (int)(e & 3);
  float n0, n1;
  box_muller(q < 2 ? p.v[0] : p.v[2], q < 2 ? p.v[1] : p.v[3], n0, n1);
  return (q & 1) ? n1 : n0;
}

__device__ __forceinline__ uint64_t read_step(const int64_t* step) { return step ? (uint64_t)*step : 0ull; }

__global__ __launch_bounds__(256) void philox_raw_kernel(uint64_t seed, const int64_t* step, long nblocks, uint64_t* out) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= nblocks) return;
  const Philox4 p = philox4x64_10((uint64_t)j, read_step(step), seed);
#pragma unroll
  for (int q = 0; q < 4; ++q) out[4 * j + q] = p.v[q];
}

__global__ __launch_bounds__(256) void normal_fill_kernel(uint64_t seed, const int64_t* step, long n, float* out) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (4 * j >= n) return;
  const Philox4 p = philox4x64_10((uint64_t)j, read_step(step), seed);
  float v[4];
  box_muller(p.v[0], p.v[1], v[0], v[1]);
  box_muller(p.v[2], p.v[3], v[2], v[3]);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (4 * j + q < n) out[4 * j + q] = v[q];
}

// ---- reparameterisation ------------------------------------------------------------------------------------------
constexpr float kKlEps = 1.0e-10f;

__device__ __forceinline__ float softplus_f(float s) { return fmaxf(s, 0.f) + log1pf(expf(-fabsf(s))); }

__global__ __launch_bounds__(256) void vae_sample_fwd_kernel(const float* __restrict__ m_pre, const float* __restrict__ s_pre,
                                                             int N, int D, int ld, const float* __restrict__ eps,
                                                             uint64_t seed, const int64_t* step, float* __restrict__ z,
                                                             float* __restrict__ kl) {
  __shared__ float mean_s[64], std_s[64], red[64];
  const int b = blockIdx.x, t = threadIdx.x;
  if (t < 64) {
    float term = 0.f;
    if (t < D) {
      const float m = fminf(fmaxf(m_pre[(long)b * ld + t], -100.f), 100.f);
      const float sd = fminf(fmaxf(sqrtf(softplus_f(s_pre[(long)b * ld + t])), -5.f), 5.f);
      mean_s[t] = m;
      std_s[t] = sd;
      term = 1.f + 2.f * logf(sd + kKlEps) - m * m - sd;
    }
    red[t] = term;
  }
  __syncthreads();
  // fixed-order tree over the 64 columns, levels 32 .. 1 with the pairing of block_sum (block_reduce.h); kept in place: red is
  // 64 floats here, block_sum's tree wants 256
  for (int w = 32; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0 && kl) kl[b] = (float)N * red[0];
  const uint64_t st = eps ? 0ull : read_step(step);
  const long base = (long)b * N * D;
  for (int e = t; e < N * D; e += 256) {
    const int k = e % D;
    const float ep = eps ? eps[base + e] : normal_at(seed, st, base + e);
    z[base + e] = mean_s[k] + std_s[k] * ep;
  }
}

// the gradients of z from its consumers (the node decoder and every link decoder: one z output each, summed here in order)
constexpr int kMaxDz = KGCN_VAE_MAX_CHANNELS + 1;
struct DzList { const float* p[kMaxDz]; int n; };

// dz and eps are summed over the node rows by four groups of 64 threads (fixed split, fixed order of the 4 partials)
__global__ __launch_bounds__(256) void vae_sample_bwd_kernel(const float* __restrict__ m_pre, const float* __restrict__ s_pre,
                                                             int N, int D, int ld, const float* __restrict__ eps,
                                                             uint64_t seed, const int64_t* step, DzList dz,
                                                             const float* __restrict__ dkl, float* __restrict__ dm,
                                                             float* __restrict__ ds) {
  __shared__ float sz[4][64], sze[4][64];
  const int b = blockIdx.x, t = threadIdx.x, k = t & 63, g = t >> 6;
  const long base = (long)b * N * D;
  const uint64_t st = eps ? 0ull : read_step(step);
  float a = 0.f, ae = 0.f;
  if (k < D)
    for (int n = g; n < N; n += 4) {
      const long e = base + (long)n * D + k;
      const float ep = eps ? eps[e] : normal_at(seed, st, e);
      float g = dz.p[0][e];
      for (int i = 1; i < dz.n; ++i) g += dz.p[i][e];
      a += g;
      ae = __builtin_fmaf(g, ep, ae);
    }
  sz[g][k] = a;
  sze[g][k] = ae;
  __syncthreads();
  if (t < D) {
    const float gz = (sz[0][t] + sz[1][t]) + (sz[2][t] + sz[3][t]);
    const float gze = (sze[0][t] + sze[1][t]) + (sze[2][t] + sze[3][t]);
    const float mraw = m_pre[(long)b * ld + t], sraw = s_pre[(long)b * ld + t];
    const float m = fminf(fmaxf(mraw, -100.f), 100.f);
    const float sp = softplus_f(sraw);
    const float sq = sqrtf(sp);
    const float sd = fminf(fmaxf(sq, -5.f), 5.f);
    const float gk = dkl ? dkl[b] : 0.f;
    // d kl / d mean = -2 N mean, d kl / d std = N (2 / (std + 1e-10) - 1)
    const float gmean = gz + gk * (-2.f * (float)N * m);
    const float gstd = gze + gk * ((float)N * (2.f / (sd + kKlEps) - 1.f));
    // tf.clip_by_value's gradient passes where min <= x <= max (equality included); sqrt: 0.5 / y; softplus: sigmoid(s)
    const float gsq = (sq >= -5.f && sq <= 5.f) ? gstd : 0.f;
    const float gsp = gsq * 0.5f / sq;
    const float sig = 1.f / (1.f + expf(-sraw));
    dm[(long)b * ld + t] = (mraw >= -100.f && mraw <= 100.f) ? gmean : 0.f;
    ds[(long)b * ld + t] = gsp * sig;
  }
}

// ---- reconstruction loss ------------------------------------------------------------------------------------------
struct ReconArgs {
  const int32_t* rowptr[KGCN_VAE_MAX_CHANNELS];
  const int32_t* cv[KGCN_VAE_MAX_CHANNELS];
  const float* y[KGCN_VAE_MAX_CHANNELS];
  const float* w[KGCN_VAE_MAX_CHANNELS];
  float* dy[KGCN_VAE_MAX_CHANNELS];
  int skip_pad[KGCN_VAE_MAX_CHANNELS];      // row_pad == 4 containers: drop the (KGCN_PAD_COL, 0) padding entries
  int B, C, N, D, F;
  int NP, D4;                               // N, D rounded up to multiples of 4 (register tile / float4 width)
};

__device__ __forceinline__ float sig_ce(float l, float a) { return fmaxf(l, 0.f) - l * a + log1pf(expf(-fabsf(l))); }
__device__ __forceinline__ float sigmoid_f(float l) { return 1.f / (1.f + expf(-l)); }

// tile u of the upper triangle (I <= J) of a T4 x T4 tile grid, row-major
__device__ __forceinline__ void upper_tile(int u, int T4, int& I, int& J) {
  I = 0;
  while (u >= T4 - I) {
    u -= T4 - I;
    ++I;
  }
  J = I + u;
}

// Y_c[b] -> ys [NP][D4 + 4] (zero padding rows / columns); w_c -> ws [D4] (zero padding)
__device__ __forceinline__ void stage_y(const ReconArgs& a, int c, int b, float* ys, float* ws) {
  const int yld = a.D4 + 4;
  const float* yb = a.y[c] + (long)b * a.N * a.D;
  for (int e = threadIdx.x; e < a.NP * a.D4; e += 256) {
    const int i = e / a.D4, k = e - i * a.D4;
    ys[i * yld + k] = (i < a.N && k < a.D) ? yb[i * a.D + k] : 0.f;
  }
  for (int k = threadIdx.x; k < a.D4; k += 256) ws[k] = k < a.D ? a.w[c][k] : 0.f;
}

// dense label matrix of (b, c) in LDS: zeros, then one thread per row writes its entries in CSR order (a repeated column:
// the last entry wins, deterministically); entries outside [0, N) are ignored
__device__ __forceinline__ void stage_labels(const ReconArgs& a, int c, int b, float* A, int ald) {
  for (int e = threadIdx.x; e < a.NP * ald; e += 256) A[e] = 0.f;
  __syncthreads();
  for (int i = threadIdx.x; i < a.N; i += 256) {
    const int r = b * a.N + i;
    const int e0 = a.rowptr[c][r], e1 = a.rowptr[c][r + 1];
    for (int e = e0; e < e1; ++e) {
      const int col = a.cv[c][2 * e];
      const float v = __int_as_float(a.cv[c][2 * e + 1]);
      if (a.skip_pad[c] && col == KGCN_PAD_COL && v == 0.f) continue;
      if (col >= 0 && col < a.N) A[i * ald + col] = v;
    }
  }
}

// 4 x 4 tile of L = (Y * w) Y^T: rows 4I.., columns 4J..
__device__ __forceinline__ void l_tile(const float* ys, const float* ws, int yld, int D4, int I, int J, float (&acc)[4][4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.f;
  const float* ra = ys + 4 * I * yld;
  const float* rb = ys + 4 * J * yld;
  for (int k = 0; k < D4; k += 4) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + k);
    f32x4 av[4], bv[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      av[p] = *reinterpret_cast<const f32x4*>(ra + p * yld + k) * wv;
      bv[p] = *reinterpret_cast<const f32x4*>(rb + p * yld + k);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float s = acc[p][q];
        s = __builtin_fmaf(av[p].x, bv[q].x, s);
        s = __builtin_fmaf(av[p].y, bv[q].y, s);
        s = __builtin_fmaf(av[p].z, bv[q].z, s);
        s = __builtin_fmaf(av[p].w, bv[q].w, s);
        acc[p][q] = s;
      }
  }
}

// P tile = H[rows 4I..] Y[:, cols 4K..]; writes dY = P * w (valid rows / columns) and leaves 1/2 y * p in pv
__device__ __forceinline__ void p_tile(const ReconArgs& a, const float* ys, const float* H, int yld, int ald, int I, int K,
                                       float* __restrict__ dyb, float (&pv)[4][4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) pv[p][q] = 0.f;
  for (int j = 0; j < a.N; ++j) {
    const f32x4 yv = *reinterpret_cast<const f32x4*>(ys + j * yld + 4 * K);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float h = H[(4 * I + p) * ald + j];
      pv[p][0] = __builtin_fmaf(h, yv.x, pv[p][0]);
      pv[p][1] = __builtin_fmaf(h, yv.y, pv[p][1]);
      pv[p][2] = __builtin_fmaf(h, yv.z, pv[p][2]);
      pv[p][3] = __builtin_fmaf(h, yv.w, pv[p][3]);
    }
  }
  const float* ws = ys + (size_t)a.NP * yld + (size_t)a.NP * ald;     // w follows ys and H (recon_lds_floats)
  const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + 4 * K);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = 4 * I + p;
    const f32x4 yv = *reinterpret_cast<const f32x4*>(ys + i * yld + 4 * K);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = 4 * K + q;
      if (i < a.N && k < a.D) dyb[i * a.D + k] = pv[p][q] * wv[q];
      pv[p][q] *= 0.5f * yv[q];
    }
  }
}

__host__ __device__ inline size_t recon_lds_floats(int NP, int D4, bool bwd, int C) {
  const size_t ys = (size_t)NP * (D4 + 4), A = (size_t)NP * (NP + 1);
  return ys + A + 64 + 256 + (bwd ? (size_t)C * 64 : (size_t)NP * NP / 4);   // + w + reduction + (dw sums | flags)
}

// per graph: per_graph[0][b] = feature cost, [1][b] = link cost (mean over C, N, N), [2][b] = mean of correct_exist
__global__ __launch_bounds__(256) void vae_recon_fwd_kernel(ReconArgs a, const float* __restrict__ xf,
                                                            const float* __restrict__ tf, float* __restrict__ per_graph) {
  extern __shared__ float sm[];
  const int yld = a.D4 + 4, ald = a.NP + 1, T4 = a.NP / 4;
  float* ys = sm;
  float* A = ys + (size_t)a.NP * yld;
  float* ws = A + (size_t)a.NP * ald;
  float* red = ws + 64;
  unsigned char* flags = reinterpret_cast<unsigned char*>(red + 256);   // bit 0: some channel has L > 0, bit 1: label > 0.5
  const int ntiles = T4 * (T4 + 1) / 2;
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();
    for (int e = threadIdx.x; e < a.NP * a.NP; e += 256) flags[e] = 0;
    float link = 0.f;
    for (int c = 0; c < a.C; ++c) {
      __syncthreads();
      stage_y(a, c, b, ys, ws);
      stage_labels(a, c, b, A, ald);
      __syncthreads();
      for (int u = threadIdx.x; u < ntiles; u += 256) {
        int I, J;
        upper_tile(u, T4, I, J);
        float acc[4][4];
        l_tile(ys, ws, yld, a.D4, I, J, acc);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int i = 4 * I + p, j = 4 * J + q;
            if (i >= a.N || j >= a.N || (I == J && p > q)) continue;
            const float l = acc[p][q];
            const float aij = A[i * ald + j];
            unsigned char fl = (l > 0.f ? 1 : 0) | (aij > 0.5f ? 2 : 0);
            link += sig_ce(l, aij);
            flags[i * a.NP + j] |= fl;
            if (i != j) {
              const float aji = A[j * ald + i];
              link += sig_ce(l, aji);
              flags[j * a.NP + i] |= (unsigned char)((l > 0.f ? 1 : 0) | (aji > 0.5f ? 2 : 0));
            }
          }
      }
    }
    __syncthreads();
    float hits = 0.f;
    for (int e = threadIdx.x; e < a.N * a.N; e += 256) {
      const int i = e / a.N, j = e - i * a.N;
      const unsigned char fl = flags[i * a.NP + j];
      hits += ((fl & 1) != 0) == ((fl & 2) != 0) ? 1.f : 0.f;
    }
    float feat = 0.f;
    const long fb = (long)b * a.N * a.F;
    for (int e = threadIdx.x; e < a.N * a.F; e += 256) feat += sig_ce(xf[fb + e], tf[fb + e]);
    const float nn = (float)a.N * (float)a.N;
    const float link_sum = block_sum(link, red);
    const float hit_sum = block_sum(hits, red);
    const float feat_sum = block_sum(feat, red);
    if (threadIdx.x == 0) {
      per_graph[b] = feat_sum / ((float)a.N * (float)a.F);
      per_graph[a.B + b] = link_sum / ((float)a.C * nn);
      per_graph[2 * a.B + b] = hit_sum / nn;
    }
  }
}

// sums[0] = cost_opt = mean_b cost_b - 1/2 mean_b kl_b, sums[1] = cost_sum = mean_b cost_b, sums[2] = correct_count
// (cost_b = mask_b (feature_b + link_b); every mean over the PADDED batch); one block, fixed order
__global__ __launch_bounds__(256) void vae_recon_finish_kernel(const float* __restrict__ per_graph, const float* __restrict__ mask,
                                                               const float* __restrict__ kl, int B, float* __restrict__ sums) {
  __shared__ float red[256];
  float cs = 0.f, ks = 0.f, cc = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float m = mask ? mask[b] : 1.f;
    cs += m * (per_graph[b] + per_graph[B + b]);
    cc += m * per_graph[2 * B + b];
    if (kl) ks += kl[b];
  }
  const float c_tot = block_sum(cs, red);
  const float k_tot = block_sum(ks, red);
  const float h_tot = block_sum(cc, red);
  if (threadIdx.x == 0) {
    const float cost_sum = c_tot / (float)B;
    sums[0] = cost_sum - 0.5f * (k_tot / (float)B);
    sums[1] = cost_sum;
    sums[2] = h_tot;
  }
}

__global__ __launch_bounds__(256) void vae_recon_bwd_kernel(ReconArgs a, const float* __restrict__ xf,
                                                            const float* __restrict__ tf, const float* __restrict__ mask,
                                                            const float* __restrict__ g_opt, const float* __restrict__ g_sum,
                                                            float* __restrict__ dxf, float* __restrict__ dkl,
                                                            float* __restrict__ part_dw) {
  extern __shared__ float sm[];
  const int yld = a.D4 + 4, ald = a.NP + 1, T4 = a.NP / 4;
  float* ys = sm;
  float* H = ys + (size_t)a.NP * yld;
  float* ws = H + (size_t)a.NP * ald;
  float* red = ws + 64;
  float* dws = red + 256;                  // [C][64]: this workgroup's dw partial; column k owned by thread k
  const int ntiles = T4 * (T4 + 1) / 2;
  const int ptiles = T4 * (a.D4 / 4);
  for (int e = threadIdx.x; e < a.C * 64; e += 256) dws[e] = 0.f;
  const float go = g_opt ? *g_opt : 0.f, gs = g_sum ? *g_sum : 0.f;
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const float mb = mask ? mask[b] : 1.f;
    const float gb = mb * (go + gs) / (float)a.B;            // d (cost_opt, cost_sum) / d cost_b
    const float s_link = gb / ((float)a.C * (float)a.N * (float)a.N);
    if (threadIdx.x == 0 && dkl) dkl[b] = -0.5f * go / (float)a.B;
    for (int c = 0; c < a.C; ++c) {
      __syncthreads();
      stage_y(a, c, b, ys, ws);
      stage_labels(a, c, b, H, ald);
      __syncthreads();
      // H = G + G^T in place of the labels, G = (sigmoid(L) - A) s_link
      for (int u = threadIdx.x; u < ntiles; u += 256) {
        int I, J;
        upper_tile(u, T4, I, J);
        float acc[4][4];
        l_tile(ys, ws, yld, a.D4, I, J, acc);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int i = 4 * I + p, j = 4 * J + q;
            if (i >= a.N || j >= a.N || (I == J && p > q)) continue;
            const float sg = sigmoid_f(acc[p][q]);
            const float h = ((sg - H[i * ald + j]) + (sg - H[j * ald + i])) * s_link;
            H[i * ald + j] = h;
            H[j * ald + i] = h;
          }
      }
      __syncthreads();
      // P = H Y in 4 x 4 tiles (rows 4I.., columns 4K..; at most 32 x 16 = 512 tiles: two per thread); dY = P * w; the
      // products 1/2 y * p stay in registers until every thread has finished reading Y, then go to the dw column sums
      float pv[2][4][4];
      int ti[2] = {-1, -1}, tk[2] = {-1, -1};
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int u = threadIdx.x + 256 * r;
        if (u < ptiles) {
          ti[r] = u / (a.D4 / 4);
          tk[r] = u - ti[r] * (a.D4 / 4);
          p_tile(a, ys, H, yld, ald, ti[r], tk[r], a.dy[c] + (long)b * a.N * a.D, pv[r]);
        }
      }
      __syncthreads();                        // every read of ys / H is done: ys now receives 1/2 y * p
#pragma unroll
      for (int r = 0; r < 2; ++r)
        if (ti[r] >= 0)
#pragma unroll
          for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) ys[(4 * ti[r] + p) * yld + 4 * tk[r] + q] = pv[r][p][q];
      __syncthreads();
      if ((int)threadIdx.x < a.D) {         // rows >= N hold 0 (y = 0 there): summing all NP rows in order is exact
        float sacc = 0.f;
        for (int i = 0; i < a.N; ++i) sacc += ys[i * yld + threadIdx.x];
        dws[c * 64 + threadIdx.x] += sacc;
      }
    }
    // node-feature CE: d cost_b / d logit = (sigmoid(x) - t) / (N F)
    const float s_feat = gb / ((float)a.N * (float)a.F);
    const long fb = (long)b * a.N * a.F;
    for (int e = threadIdx.x; e < a.N * a.F; e += 256) dxf[fb + e] = (sigmoid_f(xf[fb + e]) - tf[fb + e]) * s_feat;
  }
  __syncthreads();
  if (part_dw)
    for (int e = threadIdx.x; e < a.C * a.D; e += 256) {
      const int c = e / a.D, k = e - c * a.D;
      part_dw[((long)c * gridDim.x + blockIdx.x) * a.D + k] = dws[c * 64 + k];
    }
}

int recon_args(const kgcn_csr_batch* adj_ch, int C, const float* const* y, const float* const* w, int d, int f, const char* who,
               ReconArgs& a) {
  if (!adj_ch) return fail("%s: adjacency descriptors are NULL", who);
  if (C < 1 || C > KGCN_VAE_MAX_CHANNELS) return fail("%s: %d channels (1..%d supported)", who, C, KGCN_VAE_MAX_CHANNELS);
  if (d < 1 || d > KGCN_VAE_MAX_DIM) return fail("%s: decoder width %d (1..%d supported)", who, d, KGCN_VAE_MAX_DIM);
  if (f < 1) return fail("%s: feature width %d", who, f);
  if (!y || !w) return fail("%s: NULL decoder operands", who);
  const int B = adj_ch[0].num_graphs, N = adj_ch[0].rows;
  if (N < 1 || N > KGCN_VAE_MAX_NODES) return fail("%s: %d nodes per graph (1..%d supported)", who, N, KGCN_VAE_MAX_NODES);
  a = ReconArgs{};
  for (int c = 0; c < C; ++c) {
    if (int rc = validate_csr(&adj_ch[c], who, true)) return rc;
    if (adj_ch[c].num_graphs != B || adj_ch[c].rows != N || adj_ch[c].cols != N)
      return fail("%s: channel %d is %d graphs of %d x %d, channel 0 %d graphs of %d x %d", who, c, adj_ch[c].num_graphs,
                  adj_ch[c].rows, adj_ch[c].cols, B, N, N);
    if (!y[c] || !w[c]) return fail("%s: NULL Y / w of channel %d", who, c);
    a.rowptr[c] = adj_ch[c].rowptr;
    a.cv[c] = adj_ch[c].cv;
    a.y[c] = y[c];
    a.w[c] = w[c];
    a.skip_pad[c] = adj_ch[c].row_pad == 4;
  }
  a.B = B;
  a.C = C;
  a.N = N;
  a.D = d;
  a.F = f;
  a.NP = (N + 3) / 4 * 4;
  a.D4 = (d + 3) / 4 * 4;
  return 0;
}

int recon_bwd_grid(int B) { return B < 1024 ? B : 1024; }

// d w partials: per channel one array [grid, d] of `n` floats, channel after channel from `part` (the kernel indexes them as one)
struct ReconWorkspace { int grid; size_t n; float* part; size_t bytes; };
ReconWorkspace recon_layout(void* base, int32_t B, int32_t C, int32_t d) {
  Taker t(base, 4);
  ReconWorkspace w{recon_bwd_grid(B), 0, nullptr, 0};
  w.n = (size_t)w.grid * d;
  w.part = t.take<float>((size_t)C * w.n);
  w.bytes = t.off;
  return w;
}
}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int kgcn_philox4x64_raw(uint64_t seed, const int64_t* step, int64_t num_blocks, uint64_t* out, void* stream) {
  if (num_blocks < 0) return fail("kgcn_philox4x64_raw: negative count");
  if (num_blocks == 0) return 0;
  if (!out) return fail("kgcn_philox4x64_raw: NULL output");
  hipLaunchKernelGGL(philox_raw_kernel, dim3((unsigned)((num_blocks + 255) / 256)), dim3(256), 0, as_stream(stream), seed, step,
                     (long)num_blocks, out);
  return check_launch("philox_raw_kernel");
}

extern "C" int kgcn_normal_f32(uint64_t seed, const int64_t* step, int64_t n, float* out, void* stream) {
  if (n < 0) return fail("kgcn_normal_f32: negative count");
  if (n == 0) return 0;
  if (!out) return fail("kgcn_normal_f32: NULL output");
  const int64_t blocks = (n + 3) / 4;
  hipLaunchKernelGGL(normal_fill_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, as_stream(stream), seed, step,
                     (long)n, out);
  return check_launch("normal_fill_kernel");
}

static int sample_shape(int32_t B, int32_t N, int32_t d, int32_t ld, const char* who) {
  if (B < 0 || N < 1 || d < 1) return fail("%s: bad shape (%d graphs, %d nodes, width %d)", who, B, N, d);
  if (ld < d) return fail("%s: row stride %d < width %d", who, ld, d);
  if (d > KGCN_VAE_MAX_DIM) return fail("%s: latent width %d (at most %d supported)", who, d, KGCN_VAE_MAX_DIM);
  if ((int64_t)N * d >= (int64_t)INT32_MAX) return fail("%s: N * d exceeds int32", who);
  return 0;
}

extern "C" int kgcn_vae_sample_fwd_f32(const float* m_pre, const float* s_pre, int32_t num_graphs, int32_t n_nodes, int32_t d,
                                       int32_t ld, const float* eps, uint64_t seed, const int64_t* step, float* z, float* kl,
                                       void* stream) {
  if (int rc = sample_shape(num_graphs, n_nodes, d, ld, "kgcn_vae_sample_fwd_f32")) return rc;
  if (num_graphs == 0) return 0;
  if (!m_pre || !s_pre || !z) return fail("kgcn_vae_sample_fwd_f32: NULL operand");
  hipLaunchKernelGGL(vae_sample_fwd_kernel, dim3(num_graphs), dim3(256), 0, as_stream(stream), m_pre, s_pre, n_nodes, d, ld,
                     eps, seed, step, z, kl);
  return check_launch("vae_sample_fwd_kernel");
}

extern "C" int kgcn_vae_sample_bwd_f32(const float* m_pre, const float* s_pre, int32_t num_graphs, int32_t n_nodes, int32_t d,
                                       int32_t ld, const float* eps, uint64_t seed, const int64_t* step, const float* const* dz,
                                       int32_t num_dz, const float* dkl, float* dm_pre, float* ds_pre, void* stream) {
  if (int rc = sample_shape(num_graphs, n_nodes, d, ld, "kgcn_vae_sample_bwd_f32")) return rc;
  if (num_dz < 1 || num_dz > kMaxDz) return fail("kgcn_vae_sample_bwd_f32: %d gradients of z (1..%d)", num_dz, kMaxDz);
  if (num_graphs == 0) return 0;
  if (!m_pre || !s_pre || !dz || !dm_pre || !ds_pre) return fail("kgcn_vae_sample_bwd_f32: NULL operand");
  DzList dl{};
  for (int i = 0; i < num_dz; ++i) {
    if (!dz[i]) return fail("kgcn_vae_sample_bwd_f32: gradient %d of z is NULL", i);
    dl.p[i] = dz[i];
  }
  dl.n = num_dz;
  hipLaunchKernelGGL(vae_sample_bwd_kernel, dim3(num_graphs), dim3(256), 0, as_stream(stream), m_pre, s_pre, n_nodes, d, ld,
                     eps, seed, step, dl, dkl, dm_pre, ds_pre);
  return check_launch("vae_sample_bwd_kernel");
}

extern "C" int64_t kgcn_vae_recon_workspace_bytes(int32_t num_graphs, int32_t num_channels, int32_t d) {
  if (num_graphs <= 0 || num_channels <= 0 || d <= 0) return 0;
  return (int64_t)recon_layout(nullptr, num_graphs, num_channels, d).bytes;
}

extern "C" int kgcn_vae_recon_fwd_f32(const kgcn_csr_batch* adj_ch, int32_t num_channels, const float* const* y,
                                      const float* const* w, int32_t d, const float* feat_logits, const float* feat_target,
                                      int32_t f, const float* mask, const float* kl, float* per_graph, float* sums,
                                      void* stream) {
  const char* who = "kgcn_vae_recon_fwd_f32";
  ReconArgs a;
  if (int rc = recon_args(adj_ch, num_channels, y, w, d, f, who, a)) return rc;
  if (!feat_logits || !feat_target || !per_graph || !sums) return fail("%s: NULL operand", who);
  if (a.B == 0) return fail("%s: empty batch", who);
  hipStream_t s = as_stream(stream);
  if (int rc = allow_full_lds<vae_recon_fwd_kernel>(0, who)) return rc;
  const size_t lds = recon_lds_floats(a.NP, a.D4, false, a.C) * 4;
  hipLaunchKernelGGL(vae_recon_fwd_kernel, dim3(a.B), dim3(256), lds, s, a, feat_logits, feat_target, per_graph);
  if (int rc = check_launch("vae_recon_fwd_kernel")) return rc;
  hipLaunchKernelGGL(vae_recon_finish_kernel, dim3(1), dim3(256), 0, s, per_graph, mask, kl, a.B, sums);
  return check_launch("vae_recon_finish_kernel");
}

extern "C" int kgcn_vae_recon_bwd_f32(const kgcn_csr_batch* adj_ch, int32_t num_channels, const float* const* y,
                                      const float* const* w, int32_t d, const float* feat_logits, const float* feat_target,
                                      int32_t f, const float* mask, const float* g_opt, const float* g_sum, float* const* dy,
                                      float* const* dw, float* dfeat, float* dkl, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  const char* who = "kgcn_vae_recon_bwd_f32";
  ReconArgs a;
  if (int rc = recon_args(adj_ch, num_channels, y, w, d, f, who, a)) return rc;
  if (!feat_logits || !feat_target || !dy || !dfeat) return fail("%s: NULL operand", who);
  if (a.B == 0) return fail("%s: empty batch", who);
  for (int c = 0; c < a.C; ++c) {
    if (!dy[c]) return fail("%s: NULL dY of channel %d", who, c);
    a.dy[c] = dy[c];
  }
  const ReconWorkspace ws = recon_layout(dw ? workspace : nullptr, a.B, a.C, d);
  const int grid = ws.grid;
  if (dw)
    if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)ws.bytes)) return rc;
  hipStream_t s = as_stream(stream);
  if (int rc = allow_full_lds<vae_recon_bwd_kernel>(0, who)) return rc;
  float* part = ws.part;
  const size_t lds = recon_lds_floats(a.NP, a.D4, true, a.C) * 4;
  hipLaunchKernelGGL(vae_recon_bwd_kernel, dim3(grid), dim3(256), lds, s, a, feat_logits, feat_target, mask, g_opt, g_sum, dfeat,
                     dkl, part);
  if (int rc = check_launch("vae_recon_bwd_kernel")) return rc;
  if (dw)
    for (int c = 0; c < a.C; ++c)
      if (dw[c])
        if (int rc = reduce_or_defer(part + c * ws.n, grid, d, dw[c], s)) return rc;
  return 0;
}
